"""The rollout tile's action-only rows (obs block 0 = onehot(a), actions_onehot, avail_actions)
on a POISONED batch.  The bit-identity tests of test_gpu_fused_rollout.py run on freshly zeroed
batches, where a one-hot or block-0 element the kernel never writes is a zero and passes; a
re-mapped store can fail exactly that way, or the opposite way by writing a neighbour.  Here the
batch is allocated once (reuse_batch), every transition field's storage is filled with the byte
0xA5 before each episode -- in the fused run and in the split-launch run alike -- and the fields
are compared as raw bytes: whatever one schedule writes the other must write, and what neither
writes stays poison in both.  No tolerances: everything is byte equality."""
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from marl_sap_amd.controllers import REGISTRY as MAC  # noqa: E402
from marl_sap_amd.runners import REGISTRY as RUN  # noqa: E402

DEV = torch.device("cuda", 0)
POISON = 0xA5


class _Logger:
    def log_stat(self, *a, **k):
        pass


def _poison(batch):
    """every transition field's whole storage = POISON bytes"""
    for v in batch.data.transition_data.values():
        torch.empty(0, dtype=torch.uint8, device=v.device).set_(v.untyped_storage()).fill_(POISON)
    torch.cuda.synchronize()


def _raw(v):
    """a field (or a slice of one) as its bytes, on the host (bool fields are re-typed before any
    copy: an element-wise bool copy may normalise the poison byte to 1)"""
    v = v.detach()
    if v.dtype == torch.bool:
        v = v.view(torch.uint8)
    return v.cpu().contiguous().view(torch.uint8)


def _is_poison(v):
    return bool((_raw(v) == POISON).all())


def _table(n, m, T, seed=None, large=False):
    """large: two tasks x 40, two x 5000 and a per-agent multiplier from {1, 1, 30} (zeros kept):
    observation rows below 16 and up to 1.5e6 in one 32-agent tile -- fc1's retry"""
    # the large table's seed: one at which tile 0 of every shape used here mixes both kinds of rows
    r = np.random.RandomState((5 if large else 0) if seed is None else seed)
    t = r.rand(n, m, T) * (r.rand(n, m, 1) > 0.6) * r.choice([1.0, 10.0], size=(1, m, 1))
    if large:
        task = np.ones(m)
        task[r.permutation(m)[:4]] = [40.0, 40.0, 5000.0, 5000.0]
        t = t * task[None, :, None] * r.choice([1.0, 1.0, 30.0], size=(n, 1, 1))
    return t


def _check_large(obs_bytes, n, m, T, L):
    """the raw obs field [E, T + 1, n, 4 m (L + 1)] of an injected_large run: the retry ran next to
    rows that keep the first scale, and the lookahead blocks are float32(table) -- stored once,
    from the first attempt"""
    look = obs_bytes.view(torch.float32)[..., m:].numpy()
    assert look.max() >= 16.0
    rowmax = look[0, 0, :32].max(-1)
    assert (rowmax >= 16.0).any() and (rowmax < 16.0).any()
    table = _table(n, m, T, large=True)
    want = np.zeros((T + 1, n, L, m), dtype=np.float32)
    for t in range(T + 1):
        for l in range(min(L, T - t)):
            want[t, :, l, :] = table[:, :, t + l].astype(np.float32)
    assert np.array_equal(look, np.broadcast_to(want.reshape(T + 1, n, L * m), look.shape))


def _episodes(n, m, T, L, E, fused, use_rnn=True, benefits="bump", rng="philox", selector="epsilon_greedy",
              eps=0.2, episodes=2):
    """`episodes` episodes of the runner on one poisoned, reused batch: per episode the fields'
    bytes, the returns and the hidden state.  selector "sap": the Q-output schedule (step_q)."""
    env_args = dict(n=n, m=m, T=T, L=L, lambda_=0.5, bids_as_actions=False, seed=7, benefits=benefits)
    if benefits in ("injected", "injected_large"):
        env_args["sat_prox_mat"] = _table(n, m, T, large=benefits == "injected_large")
        env_args["benefits"] = "injected"
    sap = selector == "sap"
    args = SimpleNamespace(
        batch_size_run=E, env="mock_constellation_env", env_args=env_args, env_rng=rng, env_quirks=(),
        runner_protocol="episode", test_nepisode=1, runner_log_interval=10 ** 12, n=n, m=m, T=T, hidden_dim=64,
        use_rnn=use_rnn, obs_last_action=False, obs_agent_id=False, agent_output_type="q", action_selector=selector,
        agent="rnn" if sap else "rnn_fused", mac="basic_mac", seed=3, epsilon_start=eps, epsilon_finish=eps,
        epsilon_anneal_time=1, evaluation_epsilon=0.0, fused_rollout=fused, reuse_batch=True)
    np.random.seed(3)
    runner = RUN["gpu"](args, _Logger())
    env = runner.get_env()
    torch.manual_seed(1234)
    mac = MAC["basic_mac"](env.scheme, {"agents": n}, args)
    mac.to(DEV)
    runner.setup(env.scheme, {"agents": n}, env.preprocess, mac)
    runner.reset(env_reset=False)  # allocates the one batch every episode overwrites
    with torch.no_grad():
        if sap:
            st = np.random.get_state()
            assert mac.fused_mode(env, runner.batch) == ("step_q" if fused else None)
            np.random.set_state(st)
        else:
            assert mac.fused_step_ok(env, runner.batch) == bool(fused)
    out = []
    for _ in range(episodes):
        _poison(runner.batch)
        batch = runner.run(test_mode=False)
        assert batch is runner.batch
        out.append(({k: _raw(v) for k, v in batch.data.transition_data.items()},
                    _raw(runner.last_returns), _raw(mac.hidden_states),
                    _is_poison(batch.data.transition_data["actions_onehot"][:, T])))
    env.close()
    return out


def _same(a, b):
    assert len(a) == len(b)
    for (fa, reta, ha, _), (fb, retb, hb, _) in zip(a, b):
        assert fa.keys() == fb.keys()
        for k in fa:
            assert torch.equal(fa[k], fb[k]), k
        assert torch.equal(reta, retb)
        assert torch.equal(ha, hb)


@pytest.mark.parametrize("n,m,T,L,E,use_rnn", [
    (64, 64, 4, 3, 5, True),    # the SQ = 64 instance: both tiles, both halves of each new lane mapping
    (64, 64, 4, 1, 5, False),   # the SQ = 64 instance with the Linear agent
    (32, 32, 4, 3, 5, True),    # the smallest run-time-shape !GEN instance: one tile, one chunk
    (96, 128, 3, 3, 3, True),   # three tiles; a one-hot row is exactly one instruction
    (20, 25, 4, 3, 5, True),    # the untouched ragged path
])
def test_poisoned_episodes_fused_equal_split(n, m, T, L, E, use_rnn):
    split = _episodes(n, m, T, L, E, fused=False, use_rnn=use_rnn)
    # rows never written: actions_onehot row T is still poison after a full episode
    assert all(ep[3] for ep in split)
    for mode in ("always", "step"):
        fused = _episodes(n, m, T, L, E, fused=mode, use_rnn=use_rnn)
        _same(fused, split)
        assert all(ep[3] for ep in fused), mode


@pytest.mark.parametrize("benefits,rng,selector", [
    ("injected", "philox", "epsilon_greedy"),  # the injected float64 table (TAB = 1)
    ("bump", "mt19937", "epsilon_greedy"),     # MT19937 draws: the compact table (TAB = 2)
    ("bump", "philox", "sap"),                 # the Q-output schedule (asg_step_forward + SAP selector)
])
def test_poisoned_episodes_other_64x64_instances(benefits, rng, selector):
    kw = dict(n=64, m=64, T=4, L=3, E=5, benefits=benefits, rng=rng, selector=selector)
    split = _episodes(fused=False, **kw)
    assert all(ep[3] for ep in split)
    for mode in ((True,) if selector == "sap" else ("always", "step")):
        fused = _episodes(fused=mode, **kw)
        _same(fused, split)
        assert all(ep[3] for ep in fused), mode


@pytest.mark.parametrize("selector", ["epsilon_greedy", "sap"])
def test_poisoned_episodes_large_table_three_envs(selector):
    """The injected table with rows from below 16 to 1.5e6 (fc1 re-runs for part of each tile), three
    envs, on the poisoned batch: epsilon-greedy and the Q-output schedule."""
    kw = dict(n=64, m=64, T=4, L=3, E=3, benefits="injected_large", selector=selector)
    split = _episodes(fused=False, **kw)
    assert all(ep[3] for ep in split)
    for mode in ((True,) if selector == "sap" else ("always", "step")):
        fused = _episodes(fused=mode, **kw)
        _same(fused, split)
        assert all(ep[3] for ep in fused), mode
        for ep in fused:
            _check_large(ep[0]["obs"], 64, 64, 4, 3)


def test_poisoned_chunk_inside_an_episode():
    """Steps 1..2 of T = 4 as one launch (select_first false, select_last true) into a batch
    poisoned just before it: the rows it writes equal the one-launch episode's, every row below
    its first and above its last still holds the poison, in every field."""
    from marl_sap_amd.envs import AssignEnvBatch
    from marl_sap_amd.components import EpisodeBatch
    from marl_sap_amd.modules.agents import RNNFusedAgent
    from marl_sap_amd.action_selectors.classic_selectors import EpsilonGreedyActionSelector
    n, m, T, L, E = 64, 64, 4, 3, 5

    def run(chunked):
        env = AssignEnvBatch(n, m, T, L, 0.5, seed=3, num_envs=E, device=DEV)
        b = EpisodeBatch(env.scheme, {"agents": n}, E, T + 1, preprocess=env.preprocess, device=DEV, time_major=True)
        torch.manual_seed(9)
        agent = RNNFusedAgent(m * (L + 1), SimpleNamespace(hidden_dim=64, use_rnn=True, m=m)).to(DEV)
        sel = EpsilonGreedyActionSelector(SimpleNamespace(epsilon_start=0.2, epsilon_finish=0.2,
                                                          epsilon_anneal_time=1, evaluation_epsilon=0.0, seed=4))
        _poison(b)
        env.reset(b, 0)
        h = agent.init_hidden().unsqueeze(0).expand(E, n, -1)
        with torch.no_grad():
            if not chunked:
                eps, seed, c, st, _ = sel.fused_params(0, False, DEV, calls=T)
                env.rollout(b, 0, T, agent, h, eps, seed, c, st, select_first=True, select_last=False)
            else:
                # step 0 (rows 0 and 1), then the poison again: the chunk reads only its first
                # transition's actions (row 1) from the batch
                eps, seed, c, st, _ = sel.fused_params(0, False, DEV, calls=2)
                h = env.rollout(b, 0, 1, agent, h, eps, seed, c, st, select_first=True, select_last=True)
                env.sync()
                a1 = b["actions"][:, 1].clone()
                _poison(b)
                b["actions"][:, 1] = a1
                torch.cuda.synchronize()
                eps, seed, c, st, _ = sel.fused_params(0, False, DEV, calls=2)
                env.rollout(b, 1, 2, agent, h, eps, seed, c, st, select_first=False, select_last=True)
        env.sync()
        out = {k: (v.view(torch.uint8) if v.dtype == torch.bool else v).detach().cpu().clone()
               for k, v in b.data.transition_data.items()}
        env.close()
        return out

    one, chunk = run(False), run(True)
    # the rows transitions 1, 2 and the selections on rows 2, 3 write: per-transition fields at
    # the transition's row, pre-transition fields at the row after it; actions row 1 was the input
    at_t = {"rewards", "terminated", "actions_onehot"}
    assert one.keys() == chunk.keys() and at_t <= one.keys()
    for k in one:
        lo, hi = (1, 2) if k in at_t else (2, 3)
        if k == "actions":
            lo = 1
        for t in range(T + 1):
            if lo <= t <= hi:
                assert torch.equal(_raw(chunk[k][:, t]), _raw(one[k][:, t])), (k, t)
            else:
                assert _is_poison(chunk[k][:, t]), (k, t)
