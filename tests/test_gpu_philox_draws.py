"""The Philox mode's env draws against an independent restatement (oracle/philox.py).

Every other test of rng="philox" is relative to the GPU's own output (fused == split launches,
replays from the handle's own exports).  Here every draw is regenerated on the CPU from (seed,
global env index, episode, index) alone -- the task scales, the per-pair bump parameters, the
reset permutation and the random policy's actions -- and compared with what each device copy
of the draw produced: a wrong key mix, counter purpose, bit field, word routing or a stuck
episode counter fails here even if every kernel shares the mistake.  tests/test_philox_kat.py
checks the restatement itself on the CPU (hand-derived vectors, float32 exactness).

Tolerances.  scale and center are float32 values of the specification (test_philox_kat.py:
test_bump_decode_exact_in_float32) and compare bit for bit.  a2 = log2(e) sqrt(-2 ln 0.05) / spread
is formed on the device as float32 constant * v_rcp_f32(spread): the constant rounds within 2^-24,
the reciprocal is within 1 ulp (2^-23), the product rounds within 2^-24 -- 2^-22 relative against
the float64 value.  The 14-bit width index recovered from a2 must equal the oracle's: the width
grid's relative step is >= 3 * 2^-14 / 6 = 2^-15, far above 2^-22, so the recovery is unique.
"""
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from marl_sap_amd.components import EpisodeBatch  # noqa: E402
from marl_sap_amd.envs import AssignEnvBatch  # noqa: E402
from oracle import oracle as ora  # noqa: E402
from oracle import philox as px  # noqa: E402
from oracle.check import PHILOX_ATOL, PHILOX_RTOL, bump_table_from_params, replay_and_compare  # noqa: E402

DEV = torch.device("cuda", 0)
A2_RTOL = 2.0 ** -22
A2_NUM = np.log2(np.e) * np.sqrt(-2.0 * np.log(0.05))  # a2 * spread
TALLY = {"pairs": 0, "perms": 0, "actions": 0, "a2_dev": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _tally():
    yield
    print(f"\nphilox draws compared with the oracle: {TALLY}")


def new_batch(env):
    return EpisodeBatch(env.scheme, {"agents": env.n}, env.num_envs, env.T + 1, preprocess=env.preprocess,
                        device=DEV, time_major=True)


def genvs(env):
    return px.global_envs(env.env_index_base, env.num_envs)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def check_params(env, episode, batch=None):
    """export_bump_params() of every pair of every env == the oracle's; with `batch`, whose row 0
    the reset of this episode wrote, also that row's obs / beta (the row writer's own copies of
    the draw, float32 bump values) against the C oracle's reset row on the oracle's table.
    Returns (that float64 table, the exported parameters)."""
    n, m, T = env.n, env.m, env.T
    p = env.export_bump_params().cpu().numpy()
    assert p.dtype == np.float32 and p.shape == (env.num_envs, n, m, 3)
    active, scale, center, spread, u14, a2 = px.bump_params(env.seed_value, genvs(env), episode, n, m, T,
                                                            dense=env.benefits == "dense")
    bad = np.argwhere(bits(p[..., 0]) != bits(scale))
    assert bad.size == 0, f"scale: {len(bad)} pairs differ, first (env, i, j) {bad[0]}: " \
                          f"{p[..., 0][tuple(bad[0])]} vs {scale[tuple(bad[0])]}"
    bad = np.argwhere(bits(p[..., 1]) != bits(center))
    assert bad.size == 0, f"center: {len(bad)} pairs differ, first (env, i, j) {bad[0]}: " \
                          f"{p[..., 1][tuple(bad[0])]!r} vs {center[tuple(bad[0])]!r}"
    got_a2 = p[..., 2].astype(np.float64)
    got_u14 = np.rint((A2_NUM / got_a2 - 3.0) / 3.0 * 16384.0).astype(np.int64)
    bad = np.argwhere(got_u14 != u14)
    assert bad.size == 0, f"width index: {len(bad)} pairs differ, first (env, i, j) {bad[0]}: " \
                          f"{got_u14[tuple(bad[0])]} vs {u14[tuple(bad[0])]}"
    dev = float((np.abs(got_a2 - a2) / a2).max())
    TALLY["pairs"] += active.size
    TALLY["a2_dev"] = max(TALLY["a2_dev"], dev)
    print(f"params {n}x{m} T={T} E={env.num_envs} episode {episode}: {active.size} pairs, "
          f"largest a2 deviation {dev:.4g} = {dev * 2 ** 22:.3f} * 2^-22 (running: {TALLY})")
    assert dev <= A2_RTOL, f"a2 deviates {dev:.4g} > 2^-22 relative (the width indices match)"
    # the float64 table of the ORACLE's scale and center and the exported a2 (the oracle's, above)
    table = bump_table_from_params(np.stack([scale, center, got_a2], axis=-1), T)
    if batch is not None:
        for e in range(env.num_envs):
            o = ora.OracleMockEnv(n, m, T, env.L, env.lambda_, sat_prox_mat=table[e], mt=ora.MT(0))
            o.reset()
            for k, want in (("obs", o._obs), ("beta", o.beta)):
                np.testing.assert_allclose(batch[k][e, 0].cpu().numpy(), want.astype(np.float32), rtol=PHILOX_RTOL,
                                           atol=PHILOX_ATOL, err_msg=f"{k} row 0 of env {e}")
    return table, p


def check_perm(env, episode, batch, export=True):
    want = px.reset_perm(env.seed_value, genvs(env), episode, env.n, env.m)
    row0 = batch["prev_assigns"][:, 0].reshape(env.num_envs, env.n).cpu().numpy()
    np.testing.assert_array_equal(row0, want, err_msg=f"prev_assigns row 0, episode {episode}")
    if export:  # the handle's copy holds the permutation until the first step
        np.testing.assert_array_equal(env.export_prev_assigns().cpu().numpy(), want,
                                      err_msg=f"export_prev_assigns, episode {episode}")
    TALLY["perms"] += len(want)
    return want


def make_agent(env, seed=9):
    from marl_sap_amd.action_selectors.classic_selectors import EpsilonGreedyActionSelector
    from marl_sap_amd.modules.agents import RNNFusedAgent
    torch.manual_seed(seed)
    agent = RNNFusedAgent(env.m * (env.L + 1), SimpleNamespace(hidden_dim=64, use_rnn=True, m=env.m)).to(DEV)
    sel = EpsilonGreedyActionSelector(SimpleNamespace(epsilon_start=0.2, epsilon_finish=0.2, epsilon_anneal_time=1,
                                                      evaluation_epsilon=0.0, seed=4))
    return agent, sel


def fused_episode(env, batch, agent, sel, steps=None):
    """reset + the first `steps` steps (default: the whole episode) in one launch (asg_reset_rollout)"""
    assert env.can_step_select() and env.fused_reset_ok
    steps = env.T if steps is None else steps
    h = torch.zeros((env.num_envs * env.n, 64), device=DEV)
    with torch.no_grad():
        eps, seed, c, st, _ = sel.fused_params(0, False, DEV, calls=steps)
        env.rollout(batch, 0, steps, agent, h, eps, seed, c, st, select_first=True, select_last=False, reset=True)
    env.sync()


# ---- parameters ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,T,L,E,kw", [
    (64, 64, 20, 3, 5, {}),                                 # the SQ64 instance's shape
    (5, 6, 20, 3, 4, {}),                                   # m % 4 != 0: a call's four words straddle rows
    (3, 9, 20, 2, 4, {}),
    (16, 16, 20, 3, 4, {}),
    (256, 256, 5, 1, 2, {"benefits": "dense"}),             # every pair active
    (4, 8, 1, 3, 3, {}),                                    # T = 1: the coarsest center grid that is still < T
    (4, 8, 255, 3, 3, {}),                                  # q = 16: the last T of the one-multiply center
    (4, 8, 256, 3, 3, {}),                                  # q = 15: the shifted center
    (4, 8, 300, 3, 3, {}),
    (64, 64, 20, 3, 4, {"env_index_base": 2 ** 32 - 2}),    # the key's high-word mix, across the carry
    (16, 16, 20, 3, 3, {"seed": (0x9E3779B9 << 32) | 77}),  # the seed's high word
    (5, 6, 7, 3, 3, {"seed": 2 ** 63 + 5, "env_index_base": 2 ** 33 + 1}),
])
def test_bump_params_equal_oracle(n, m, T, L, E, kw):
    kw = dict({"seed": 11}, **kw)
    env = AssignEnvBatch(n, m, T, L, 0.5, num_envs=E, device=DEV, **kw)
    b = new_batch(env)
    env.reset(b, 0)
    env.sync()
    check_params(env, 0, b)
    check_perm(env, 0, b)
    env.close()


def test_two_shards_draw_their_own_parameters():
    """Shards [0, 3) and [3, 6) of one global range: each draws its global envs' parameters, not the
    first shard's again."""
    n, m, T = 16, 16, 20
    a = AssignEnvBatch(n, m, T, 3, 0.5, seed=5, num_envs=3, device=DEV)
    c = AssignEnvBatch(n, m, T, 3, 0.5, seed=5, num_envs=3, env_index_base=3, device=DEV)
    for env in (a, c):
        b = new_batch(env)
        env.reset(b, 0)
        env.sync()
        check_params(env, 0, b)
        check_perm(env, 0, b)
    assert not torch.equal(a.export_bump_params(), c.export_bump_params())
    a.close()
    c.close()


# ---- the episode counter ------------------------------------------------------------------------
def test_episode_counter_over_every_kind_of_reset():
    """One handle at 64 x 64: reset x 3, random_rollout(reset=True), a fused reset-rollout --
    parameters and permutation are those of episodes 0, 1, 2, 3, 4."""
    n = m = 64
    T, L, E = 4, 3, 3
    env = AssignEnvBatch(n, m, T, L, 0.5, seed=21, num_envs=E, env_index_base=40, device=DEV)
    agent, sel = make_agent(env)
    perms = []
    for ep in range(3):
        b = new_batch(env)
        env.reset(b, 0)
        env.sync()
        check_params(env, ep, b)
        perms.append(check_perm(env, ep, b))
    b = new_batch(env)
    env.random_rollout(b, 0, T, reset=True)
    env.sync()
    check_params(env, 3, b)
    perms.append(check_perm(env, 3, b, export=False))
    b = new_batch(env)
    fused_episode(env, b, agent, sel)
    check_params(env, 4, b)
    perms.append(check_perm(env, 4, b, export=False))
    for i in range(5):
        for j in range(i + 1, 5):
            assert not np.array_equal(perms[i], perms[j]), (i, j)
    env.close()


# ---- the reset permutation on every copy of the draw --------------------------------------------
@pytest.mark.parametrize("n,m", [(5, 9), (64, 64)])
def test_perm_reset_kernel(n, m):
    env = AssignEnvBatch(n, m, 6, 3, 0.5, seed=31, num_envs=5, env_index_base=17, device=DEV)
    for ep in range(2):
        b = new_batch(env)
        env.reset(b, 0)
        env.sync()
        check_perm(env, ep, b)
    env.close()


@pytest.mark.parametrize("n,m", [(5, 9), (64, 64)])
def test_perm_random_rollout(n, m):
    env = AssignEnvBatch(n, m, 6, 3, 0.5, seed=32, num_envs=5, env_index_base=17, device=DEV)
    for ep in range(2):
        b = new_batch(env)
        env.random_rollout(b, 0, 6, reset=True)
        env.sync()
        check_perm(env, ep, b, export=False)
    env.close()


@pytest.mark.parametrize("n,m,T,steps", [
    (20, 25, 4, 4),   # the wave path, ragged shape
    (32, 32, 4, 4),   # the wave path, whole tiles
    (96, 128, 3, 3),  # the wave path, m > 64: two draws per lane
    (64, 64, 4, 4),   # the pair path: four agent passes
    (64, 64, 4, 1),   # the single-pass 64 x 64 instance (reset + one step: one wave per env)
])
def test_perm_fused_reset_rollout(n, m, T, steps):
    env = AssignEnvBatch(n, m, T, 3, 0.5, seed=33, num_envs=5, env_index_base=17, device=DEV)
    agent, sel = make_agent(env)
    for ep in range(2):
        b = new_batch(env)
        fused_episode(env, b, agent, sel, steps)
        check_perm(env, ep, b, export=False)
    env.close()


def test_perm_real_power_env(golden):
    """real_reset_kernel's copy: the power variant at its smallest fixture shape, Philox draws (no
    injected assignments), two episodes."""
    from marl_sap_amd.envs import RealPowerAssignEnvBatch
    d = golden("real_variants")
    cases = [c for c in range(int(d["n_cases"])) if str(d[f"v{c}_kind"]) == "power"]
    c = min(cases, key=lambda c: int(d[f"v{c}_spec"][0]) * int(d[f"v{c}_spec"][1]))
    n, m, T, L, N, M = (int(x) for x in d[f"v{c}_spec"])
    E, seed, base = 4, (3 << 32) | 11, 2 ** 32 - 1
    env = RealPowerAssignEnvBatch(1, n, m, T, N, M, L, float(d[f"v{c}_lambda"]), sat_prox_mat=d[f"v{c}_table"],
                                  graphs=[None] * T, task_prios=d[f"v{c}_prios"], num_envs=E, seed=seed,
                                  env_index_base=base, device=DEV)
    b = EpisodeBatch(env.scheme, {"agents": n}, E, T + 1, preprocess=env.preprocess, device=DEV, time_major=True)
    for ep in range(2):
        env.reset(b, 0)
        env.sync()
        want = px.reset_perm(seed, px.global_envs(base, E), ep, n, m)
        np.testing.assert_array_equal(b["prev_assigns"][:, 0].cpu().numpy().astype(np.int64), want, err_msg=str(ep))
        TALLY["perms"] += E
    env.close()


# ---- the random policy's actions ----------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(5, 6), (16, 16)])
def test_random_actions_equal_oracle(n, m):
    T, E = 7, 3
    a = AssignEnvBatch(n, m, T, 3, 0.5, seed=41, num_envs=E, env_index_base=6, device=DEV)
    f = AssignEnvBatch(n, m, T, 3, 0.5, seed=41, num_envs=E, env_index_base=6, device=DEV)
    for ep in range(2):
        want = px.random_actions(41, genvs(a), ep, n, m, T)
        ba, bf = new_batch(a), new_batch(f)
        a.reset(ba, 0)
        for t in range(T):
            a.random_actions(ba, t)
            a.sync()
            np.testing.assert_array_equal(ba["actions"][:, t, :, 0].cpu().numpy(), want[:, t], err_msg=f"step {t}")
            a.step(ba, t)
        f.random_rollout(bf, 0, T, reset=True)
        f.sync()
        np.testing.assert_array_equal(bf["actions"][:, :T, :, 0].cpu().numpy(), want, err_msg=f"episode {ep}")
        TALLY["actions"] += 2 * want.size
    a.close()
    f.close()


# ---- a shard with a non-zero base, end to end ---------------------------------------------------
def test_fused_episode_nonzero_base_vs_oracle_draws():
    """A fused 64 x 64 episode at env_index_base = 1000 replayed on the C oracle from the ORACLE's
    scale, center and permutation (and the exported a2, shown above to be the oracle's within
    2^-22): pins the rollout kernel's own env_base, not only the export kernel's."""
    n = m = 64
    T, L, E = 4, 3, 5
    env = AssignEnvBatch(n, m, T, L, 0.5, seed=51, num_envs=E, env_index_base=1000, device=DEV)
    agent, sel = make_agent(env)
    b = new_batch(env)
    fused_episode(env, b, agent, sel)
    table, _ = check_params(env, 0)
    prev0 = check_perm(env, 0, b, export=False)
    td = {k: v.cpu().numpy() for k, v in b.data.transition_data.items()}
    replay_and_compare(n, m, T, L, 0.5, table, prev0, td, env.get_returns().cpu().numpy(), philox=True)
    # and not the draws of base 0
    assert not np.array_equal(prev0, px.reset_perm(51, px.global_envs(0, E), 0, n, m))
    env.close()
