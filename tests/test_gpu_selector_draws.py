"""Every selector's Philox draw against the numpy restatement (oracle/philox.py).

The other selector tests check a statistic of the noise or the kernel's own output.  Here each
draw is regenerated on the CPU from (seed, global env, call counter, index) alone: the SAP and
bids exploration noise, the filtered selectors' tie uniforms, Gaussian noise and soft map, and the
standalone epsilon-greedy selection.  A wrong key or counter word, a local env index, cos and sin
exchanged, the counter words exchanged, a shifted register row or two families on one stream all
leave the moments intact and fail here.  tests/test_selector_draws_host.py checks the restatement
itself on the CPU.

Tolerances.  What is built on integers or one float32 operation compares exactly (tie noise,
soft map, epsilon-greedy actions).  The Gaussians go through the hardware's __logf / __cosf /
__sinf and a float32 2 pi u2: TOL_Z bounds |z - z64| of one standard normal against the float64
restatement.  It is four times the largest deviation measured by
test_bids_noise_bit_observable on MI355X (|z| <= 5.77 and the error grows with the radius), and
must stay at or below 2^-14: a wrong key, counter, word or decode moves a draw by O(1).
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from marl_sap_amd import _lib  # noqa: E402
from marl_sap_amd.action_selectors.filtered_selectors import filtered_benefit_matrix  # noqa: E402
from marl_sap_amd.envs import AssignEnvBatch  # noqa: E402
from oracle import oracle as ora  # noqa: E402
from oracle import philox as px  # noqa: E402

DEV = torch.device("cuda", 0)
# largest |z - z64| over the 51,826 draws of test_bids_noise_bit_observable on MI355X (at |z| = 1.2;
# the largest |z| among them 4.26)
Z_ERR_MEASURED = 1.31e-6
TOL_Z = 4 * Z_ERR_MEASURED
assert TOL_Z <= 2.0 ** -14

SEED_HI = 0xC3A5C85C97CB3127  # bit 63 set
SEED_LO = 5
# (envs, global env base, seed, call counter): bases across the 2^32 carry and above 2^33
RUNS = [(5, 2 ** 32 - 2, SEED_HI, 7), (3, 0, SEED_LO, 1), (4, 17, SEED_HI, 1), (3, 2 ** 33 + 1, SEED_LO, 7)]
TALLY = {"draws": 0, "z_err": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _tally():
    yield
    print(f"\nbit-observable bids draws: {TALLY['draws']}, largest |z - z64| = {TALLY['z_err']:.4g} "
          f"= 2^-14 * {TALLY['z_err'] * 2 ** 14:.4f} (TOL_Z = {TOL_Z:.4g})")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _bids(q, base, row_sm, col_sm, std, seed, counter):
    """asg_bids_select of a handle holding the global envs base .. base + E - 1: the bids [E, n, m]."""
    E, n, m = q.shape
    env = AssignEnvBatch(n, m, 5, 3, 0.5, bids_as_actions=True, seed=7, num_envs=E, env_index_base=base, device=DEV)
    out = torch.full((E, n, m), float("nan"), dtype=torch.float32, device=DEV)
    env.bids_select(q, out, row_sm, col_sm, std, seed, counter)
    env.sync()
    env.close()
    return out.cpu().numpy()


def _sap_noisy(q, eps, seed, counter, base):
    """asg_sap_noise: the matrix the SAP selector solves (q any strides)."""
    B, n, m = q.shape
    out = torch.full((B, n, m), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().asg_sap_noise(_p(q), _lib.i64arr(q.stride()), B, n, m, float(eps), seed, counter, base,
                                        _p(out), None, _lib.stream_ptr(DEV)))
    return out.cpu().numpy()


def _sap_select(q, eps, seed, counter, base):
    B, n, m = q.shape
    out = torch.full((B, n), -2.0, dtype=torch.float32, device=DEV)
    st = torch.full((B,), -99, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().asg_sap_select(_p(q), _lib.i64arr(q.stride()), B, n, m, float(eps), seed, counter, base,
                                         _p(out), _p(st), None, _lib.stream_ptr(DEV)))
    return out.cpu().numpy(), st.cpu().numpy()


def _strided(q):
    """The same values behind a view whose task stride is 2 and whose rows are padded."""
    E, n, m = q.shape
    wide = torch.zeros((E, n + 1, 2 * m + 2), dtype=q.dtype, device=q.device)
    view = wide[:, :n, 1:2 * m + 1:2]
    view.copy_(q)
    assert not view.is_contiguous() and torch.equal(view, q)
    return view


# ---- bids noise ------------------------------------------------------------------------------
@pytest.mark.parametrize("std", [1.0, 0.25])
@pytest.mark.parametrize("n,m,run", [(64, 64, 0), (33, 41, 2), (1, 7, 3)])
def test_bids_noise_bit_observable(n, m, run, std):
    """Zero logits, no softmax, std a power of two: the bids are std z exactly as the kernel formed
    z.  Every element against std * bids_noise within std * TOL_Z; this case measures TOL_Z."""
    E, base, seed, counter = RUNS[run]
    out = _bids(torch.zeros((E, n, m), device=DEV), base, 0, 0, std, seed, counter)
    z64 = px.bids_noise(seed, px.global_envs(base, E), counter, n, m)
    err = np.abs(out.astype(np.float64) / std - z64)
    TALLY["draws"] += err.size
    TALLY["z_err"] = max(TALLY["z_err"], float(err.max()))
    print(f"\nbids noise ({n}, {m}) std {std}: largest |z - z64| = {err.max():.4g} at |z64| = "
          f"{abs(z64.ravel()[err.argmax()]):.3f}, largest |z64| = {np.abs(z64).max():.3f}")
    bad = np.argwhere(err > TOL_Z)
    assert bad.size == 0, f"{len(bad)} of {err.size} draws differ, first (env, row, task) {bad[0]}: " \
                          f"{out[tuple(bad[0])] / std} vs {z64[tuple(bad[0])]}"


def _softmax64(q):
    x = np.exp(q - q.max(axis=-1, keepdims=True))
    x = x / x.sum(axis=-1, keepdims=True)
    y = np.exp(x - x.max(axis=1, keepdims=True))
    return y / y.sum(axis=1, keepdims=True)


@pytest.mark.parametrize("n,m,run", [(20, 25, 1), (64, 64, 0)])
def test_bids_noise_on_a_policy(n, m, run):
    """Logits 3 randn through both softmaxes, std 0.3: the bids are softmax64 + 0.3 z64 within the
    softmax tolerance of tests/test_gpu_bids.py (rtol 2e-6, atol 1e-8) plus 0.3 TOL_Z.  The noise
    the kernel added, noisy - (the std 0 call of the same logits), is 0.3 z64 within 0.3 TOL_Z and
    the float32 roundings of the product and the sum (an ulp of the bid).  No element can be asked
    to agree bit for bit between the two calls: 0.3 TOL_Z alone is a hundred times the ulp of a
    softmax value, so the noise never provably rounds away."""
    E, base, seed, counter = RUNS[run]
    std = 0.3
    rng = np.random.RandomState(n * 100 + m)
    q = (3.0 * rng.standard_normal((E, n, m))).astype(np.float32)
    noisy = _bids(_dev(q), base, 1, 1, std, seed, counter)
    clean = _bids(_dev(q), base, 1, 1, 0.0, seed, counter)
    z64 = px.bids_noise(seed, px.global_envs(base, E), counter, n, m)
    mean = _softmax64(q.astype(np.float64))
    err = np.abs(noisy - (mean + std * z64))
    tol = 2e-6 * np.abs(mean) + 1e-8 + std * TOL_Z
    print(f"\nbids policy ({n}, {m}): largest error / tolerance = {(err / tol).max():.4g}")
    assert (err <= tol).all(), np.argwhere(err > tol)[0]
    assert np.allclose(clean, mean, rtol=2e-6, atol=1e-8)
    added = noisy.astype(np.float64) - clean.astype(np.float64)
    budget = std * TOL_Z + _ulp32(noisy)
    err = np.abs(added - std * z64)
    print(f"bids policy ({n}, {m}): largest (noisy - clean - 0.3 z64) / budget = {(err / budget).max():.4g}")
    assert (err <= budget).all(), np.argwhere(err > budget)[0]


# ---- SAP noise -------------------------------------------------------------------------------
def _sap_expect(q, eps, seed, counter, base):
    """(restated noisy matrix float64, per-element tolerance): std64 TOL_Z, the float32 summation
    bound of the mean std64 |z| n m 2^-24, and one float32 ulp of the entry."""
    E, n, m = q.shape
    z64 = px.sap_noise(seed, px.global_envs(base, E), counter, n, m)
    sd = px.sap_std(q, eps)[:, None, None]
    want = q.astype(np.float64) + sd * z64
    tol = sd * TOL_Z + sd * np.abs(z64) * (n * m) * 2.0 ** -24 + _ulp32(want)
    return want, tol


@pytest.mark.parametrize("scale", [1.0, 1e-3])
@pytest.mark.parametrize("eps", [0.05, 0.5])
@pytest.mark.parametrize("n,m,run", [(64, 64, 0), (20, 25, 2), (33, 41, 3)])
def test_sap_noise_vs_restatement(n, m, run, eps, scale):
    """asg_sap_noise == Q + (mean|Q| eps 2) z64, element by element; a strided view of the same Q
    gives the same bits.  asg_sap_noise always runs the guarded staging (sap_stage<false>), at
    (64, 64) contiguous too: this test says nothing about the selector's dense-64 staging, which
    only test_sap_selection_is_scipy_on_the_restated_matrix observes (through its actions)."""
    E, base, seed, counter = RUNS[run]
    rng = np.random.RandomState(n + m + int(eps * 100))
    q = (scale * rng.standard_normal((E, n, m))).astype(np.float32)
    qd = _dev(q)
    got = _sap_noisy(qd, eps, seed, counter, base)
    want, tol = _sap_expect(q, eps, seed, counter, base)
    err = np.abs(got - want)
    print(f"\nSAP noise ({n}, {m}) eps {eps} scale {scale}: largest error / tolerance = {(err / tol).max():.4g}")
    assert (err <= tol).all(), np.argwhere(err > tol)[0]
    assert np.array_equal(_sap_noisy(_strided(qd), eps, seed, counter, base), got)


def test_sap_selection_is_scipy_on_the_restated_matrix():
    """64 x 64 at eps 0.5: asg_sap_select (contiguous Q: the dense-64 staging; a strided view: the
    guarded one) picks scipy's assignment of the RESTATED noisy matrix.  An env is left out when
    its restated optimum is not unique within twice the element tolerance: the best assignment
    that avoids one of the optimum's pairs (one more LSA per pair) comes within twice the env's
    largest element tolerance.  At most 10 % of the envs may be left out."""
    n = m = 64
    E, base, seed, counter = RUNS[0]
    eps = 0.5
    q = np.random.RandomState(64).standard_normal((E, n, m)).astype(np.float32)
    want, tol = _sap_expect(q, eps, seed, counter, base)
    qd = _dev(q)
    acts, st = _sap_select(qd, eps, seed, counter, base)
    acts_s, st_s = _sap_select(_strided(qd), eps, seed, counter, base)
    assert (st == 0).all() and (st_s == 0).all()
    left_out = 0
    for e in range(E):
        rows, cols = ora.lsa(want[e], maximize=True)
        best = want[e][rows, cols].sum()
        gap = np.inf
        for i in range(n):
            x = want[e].copy()
            x[i, cols[i]] = -1e30
            r2, c2 = ora.lsa(x, maximize=True)
            gap = min(gap, best - x[r2, c2].sum())
        print(f"\nenv {e}: gap to the next assignment {gap:.4g}, twice the element tolerance {2 * tol[e].max():.4g}")
        if gap <= 2 * tol[e].max():
            left_out += 1
            continue
        assert np.array_equal(acts[e], cols.astype(np.float32)), e
        assert np.array_equal(acts_s[e], cols.astype(np.float32)), e
    assert left_out <= 0.1 * E, left_out


# ---- filtered selectors ----------------------------------------------------------------------
def _random_topm(rng, B, n, m, M):
    return np.stack([[rng.permutation(m)[:M] for _ in range(n)] for _ in range(B)]).astype(np.int64)


@pytest.mark.parametrize("zero_base", [False, True])
@pytest.mark.parametrize("m,run", [(7, 1), (200, 0), (450, 3)])
def test_filtered_tie_noise_bit_exact(m, run, zero_base):
    """asg_filtered_benefits without Gaussian noise: off the top M every entry is
    float32(base) + float32(u * float32(1e-8)) in float32 arithmetic, on the top M the Q value."""
    n, M = 16, 5
    E, base, seed, counter = RUNS[run]
    rng = np.random.RandomState(m)
    q = (1e-3 * rng.standard_normal((E, n, M + 1))).astype(np.float32)
    if zero_base:
        q[..., M] = 0.0
    topm = _random_topm(rng, E, n, m, M)
    got = filtered_benefit_matrix(_dev(q), _dev(topm), m, seed=seed, counter=counter, env_base=base).cpu().numpy()
    u = px.filtered_tie_u(seed, px.global_envs(base, E), counter, n, m)
    want = q[..., M:M + 1] + u * np.float32(1e-8)
    assert want.dtype == np.float32
    bi, ii = np.indices((E, n))
    want[bi[..., None], ii[..., None], topm] = q[..., :M]
    np.testing.assert_array_equal(got, want)
    if zero_base:
        assert np.unique(got).size > 0.9 * (m - M)  # the noise itself, not a constant


@pytest.mark.parametrize("n,m,run", [(5, 7, 2), (20, 450, 0)])
def test_filtered_gauss_vs_restatement(n, m, run):
    """eps 0.4: noisy - clean (the eps 0 call of the same counter) == sd z64 with sd =
    filtered_std(clean, eps), within sd TOL_Z, an ulp of sd times |z| (the order of the float64
    sum) and an ulp of the entry."""
    M, eps = 5, 0.4
    E, base, seed, counter = RUNS[run]
    rng = np.random.RandomState(n * m)
    q = _dev(rng.standard_normal((E, n, M + 1)).astype(np.float32))
    topm = _dev(_random_topm(rng, E, n, m, M))
    kw = dict(seed=seed, counter=counter, env_base=base)
    clean = filtered_benefit_matrix(q, topm, m, **kw).cpu().numpy()
    noisy = filtered_benefit_matrix(q, topm, m, gauss_epsilon=eps, **kw).cpu().numpy()
    sd = px.filtered_std(clean, eps)
    z64 = px.filtered_gauss(seed, px.global_envs(base, E), counter, n, m)
    sd64 = sd.astype(np.float64)[:, None, None]
    err = np.abs(noisy.astype(np.float64) - clean.astype(np.float64) - sd64 * z64)
    tol = sd64 * TOL_Z + _ulp32(sd)[:, None, None] * np.abs(z64) + _ulp32(noisy)
    print(f"\nfiltered Gaussian ({n}, {m}): largest error / tolerance = {(err / tol).max():.4g}")
    assert (sd > 0).all() and (err <= tol).all(), np.argwhere(err > tol)[0]


@pytest.mark.parametrize("m,run", [(50, 2), (450, 0)])
def test_filtered_soft_map_exact(m, run):
    B, n, M = 4, 32, 5
    _, base, seed, counter = RUNS[run]
    rng = np.random.RandomState(m)
    topm = _random_topm(rng, B, n, m, M)
    picked = rng.randint(0, M, size=(B, n)).astype(np.int64)
    picked.ravel()[rng.permutation(B * n)[: B * n // 2]] = M
    out = torch.full((B, n), -1, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    picked_d, topm_d = _dev(picked), _dev(topm)
    _lib.check(_lib.lib().asg_filtered_soft_map(_p(picked_d), _p(topm_d), B, n, m, M, seed, counter, base,
                                                _p(out), _p(status), _lib.stream_ptr(DEV)))
    got = out.cpu().numpy()
    assert int(status.item()) == 0
    target = px.filtered_soft_target(seed, px.global_envs(base, B), counter, n, m, M, topm)
    bi, ii = np.indices((B, n))
    want = np.where(picked == M, target, topm[bi, ii, np.minimum(picked, M - 1)])
    np.testing.assert_array_equal(got, want)


# ---- standalone epsilon-greedy ---------------------------------------------------------------
def _eps_greedy_avail(rng, explore, m, hi0):
    """avail [R, m] whose rows cycle through four kinds, separately among the exploring and the
    other rows, so every kind explores: 0 a single task at j >= hi0, 1 about half of the tasks
    j >= hi0 and none below, 2 a single task anywhere, 3 about half of all tasks.  Returns
    (avail, kind [R])."""
    R = explore.size
    avail = np.zeros((R, m), bool)
    kind = np.zeros(R, np.int64)
    for mask in (explore, ~explore):
        kind[mask] = np.arange(int(mask.sum())) % 4
    for r in range(R):
        lo = hi0 if kind[r] < 2 else 0
        if kind[r] in (1, 3):
            avail[r, lo:] = rng.uniform(size=m - lo) < 0.5
        avail[r, lo + rng.randint(0, m - lo)] = True
    return avail, kind


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("m", [7, 64, 130, 450, 1100])
def test_epsilon_greedy_actions_exact(m, strided):
    """asg_epsilon_greedy (masked argmax) and asg_filtered_epsilon_greedy (unmasked argmax) at eps
    0.3: every row's action is the restated one.  env_index_base 2^30 with n = 4 puts the global
    rows at 2^32 and above (high counter word 1), 2^30 - 1 on both sides of the carry.  Which rows
    explore depends on (seed, global row, counter) alone, so the availability is laid out around
    them (_eps_greedy_avail): among the exploring rows some hold a single task and some about
    half of the tasks of the row's LAST 64-task chunk only (j >= hi0), so their pick needs the
    count carried over every earlier chunk; at m = 1100 that is j >= 1024, which the kernel reads
    again from `avail` (chunks >= 16) -- with the contiguous and the strided layout."""
    B, n, eps = 6, 4, 0.3
    hi0 = 64 * ((m - 1) // 64)
    rng = np.random.RandomState(m)
    q = rng.standard_normal((B, n, m)).astype(np.float32)
    assert all(np.unique(r).size == m for r in q.reshape(-1, m))  # tie-free
    qd = _dev(q)
    for fn, masked in (("asg_epsilon_greedy", True), ("asg_filtered_epsilon_greedy", False)):
        for base, seed, counter in ((2 ** 30, SEED_HI, 1), (2 ** 30 - 1, SEED_LO, 7)):
            grows = np.arange(B * n, dtype=np.uint64) + np.uint64(base * n)
            explore = px.eps_greedy_draws(seed, grows, counter, eps, 1)[0]
            assert explore.sum() >= 4 and (~explore).sum() >= 4, explore.sum()
            rows, kind = _eps_greedy_avail(rng, explore, m, hi0)
            avail = rows.reshape(B, n, m)
            assert (rows.sum(1) >= 1).all() and (rows.sum(1) == 1).sum() >= B * n // 3
            av = _dev(avail)
            if strided:
                wide = torch.zeros((B, n, 2 * m + 1), dtype=torch.bool, device=DEV)
                av = wide[:, :, 1::2]
                av.copy_(_dev(avail))
                assert av.stride(2) == 2 and av.shape == (B, n, m)
            greedy = (np.where(avail, q, -np.inf) if masked else q).argmax(-1).ravel()
            out = torch.full((B, n), -1, dtype=torch.int64, device=DEV)
            status = torch.zeros(1, dtype=torch.int32, device=DEV)
            _lib.check(getattr(_lib.lib(), fn)(_p(qd), _lib.i64arr(qd.stride()), _p(av), _lib.i64arr(av.stride()), B,
                                               n, m, eps, seed, counter, base, _p(out), _lib.i64arr(out.stride()),
                                               _p(status), _lib.stream_ptr(DEV)))
            got = out.cpu().numpy().ravel()
            assert int(status.item()) == 0
            want = px.eps_greedy_actions(seed, base * n, counter, eps, rows, greedy)
            # the exploring rows confined to the last chunk pick there: both kinds are exercised
            for k in (0, 1):
                assert (explore & (kind == k)).any() and (want[explore & (kind == k)] >= hi0).all()
            np.testing.assert_array_equal(got, want, err_msg=f"{fn} base {base}")


# ---- shards ----------------------------------------------------------------------------------
def test_shards_draw_their_global_envs():
    """Envs [2, 5) held by a handle / call with base + 2 draw the restated noise of those global
    envs (base 2^32 - 2: the shard starts on the carry)."""
    E, base, seed, counter = RUNS[0]
    g = px.global_envs(base + 2, E - 2)
    n = m = 16
    out = _bids(torch.zeros((E - 2, n, m), device=DEV), base + 2, 0, 0, 1.0, seed, counter)
    assert (np.abs(out - px.bids_noise(seed, g, counter, n, m)) <= TOL_Z).all()
    # SAP: the full call's envs 2.. and the shard's call agree bit for bit and with the restatement
    q = np.random.RandomState(1).standard_normal((E, n, m)).astype(np.float32)
    full = _sap_noisy(_dev(q), 0.5, seed, counter, base)
    part = _sap_noisy(_dev(q[2:]), 0.5, seed, counter, base + 2)
    assert np.array_equal(full[2:], part)
    want, tol = _sap_expect(q[2:], 0.5, seed, counter, base + 2)
    assert (np.abs(part - want) <= tol).all()
    # filtered Gaussian
    M, eps = 5, 0.4
    rng = np.random.RandomState(2)
    qf = _dev(rng.standard_normal((E - 2, n, M + 1)).astype(np.float32))
    topm = _dev(_random_topm(rng, E - 2, n, m, M))
    kw = dict(seed=seed, counter=counter, env_base=base + 2)
    clean = filtered_benefit_matrix(qf, topm, m, **kw).cpu().numpy()
    noisy = filtered_benefit_matrix(qf, topm, m, gauss_epsilon=eps, **kw).cpu().numpy()
    sd = px.filtered_std(clean, eps)
    z64 = px.filtered_gauss(seed, g, counter, n, m)
    sd64 = sd.astype(np.float64)[:, None, None]
    err = np.abs(noisy.astype(np.float64) - clean.astype(np.float64) - sd64 * z64)
    assert (err <= sd64 * TOL_Z + _ulp32(sd)[:, None, None] * np.abs(z64) + _ulp32(noisy)).all()
