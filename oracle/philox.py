"""numpy restatement of the product's counter-based draws (TEST INFRASTRUCTURE ONLY).

Philox4x32-10 (Salmon et al., SC'11) exactly as marl_sap_amd/csrc/asg_device.h
`philox4x32_10` computes it, and the epsilon-greedy selection draw built on it
(asg_agent.hip `select_finish`, asg_select.hip): the row's counter is
(global row lo, global row hi, kCtrSelect, call counter) under the selector key
(k0, k1) = (seed lo, seed hi ^ 0x5bd1e995); the row explores when
(x >> 8) * 2^-24 < epsilon and then takes the target-th available task,
target = (y * count) >> 32.  The reference draws these from torch's CPU generator
(classic_selectors.py:45-52), which no GPU kernel can reproduce; this restatement lets
a test predict every exploring row of a GPU rollout and check the rest against a
greedy argmax of the PyTorch RNNAgent.

The env draws of the Philox mode (rng="philox") are restated here as well, from their
specification and in integer / exact-rational arithmetic, so a GPU test can regenerate
every draw from (seed, global env index, episode, index) alone:

  key        k0 = lo32(seed) ^ (hi32(g) * 0x85EBCA6B mod 2^32), k1 = hi32(seed) ^ lo32(g)
             for the global env g = env_index_base + e (as a uint64)
  counter    (index, second, purpose, episode); episode = resets of the handle so far
  purposes   1 task scale, 4 reset permutation, 5 random action, 9 bump parameters
             (6 is the selector's, above)

The selectors' own draws use the same env key with the selector's seed and call counter in
place of the env's seed and episode (PURPOSES below is the whole table):

  7  SAP noise       counter (task j, row >> 2, 7, call): normal k of the call -> row 4 (row >> 2) + k;
                     std = mean|Q| eps 2 per env (sap_stage.h)
  10 bids noise      the same layout (asg_sap.hip, bids_select_kernel)
  11 filtered tie    counter (j >> 2, agent i, 11, call): word j & 3, u = (w >> 8) 2^-24 (float32)
  12 filtered Gauss  flat element x = i m + j: counter (x >> 2, x >> 34, 12, call), normal x & 3;
                     std = float32(float32(mean|mat| eps) 2) per env
  13 filtered soft   counter (agent i, 0, 13, call): target = (x (m - M)) >> 32 among the tasks
                     outside the agent's top M, ascending

The four normals of one call are Box-Muller's: u1 = ((w >> 8) + 1) 2^-24 from words x and z,
u2 = (w >> 8) 2^-24 from words y and w, r = sqrt(-2 ln u1), then r cos(2 pi u2), r sin(2 pi u2)
for (x, y) and for (z, w).  They are evaluated in float64 here; the device uses float32
intrinsics, so a test compares them within a measured tolerance.

Nothing under marl_sap_amd/ imports this module.
"""
import math
from fractions import Fraction

import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
# every draw family: (purpose word = counter word 2, the key it draws under)
PURPOSES = {
    "task_scale": (1, "env"),
    "reset_perm": (4, "env"),
    "random_action": (5, "env"),
    "select": (6, "selector"),
    "sap_noise": (7, "env"),
    "bump_params": (9, "env"),
    "bids_noise": (10, "env"),
    "filtered_tie": (11, "env"),
    "filtered_gauss": (12, "env"),
    "filtered_soft": (13, "env"),
}
K_CTR_SCALE = PURPOSES["task_scale"][0]
K_CTR_PERM = PURPOSES["reset_perm"][0]
K_CTR_ACTION = PURPOSES["random_action"][0]
K_CTR_SELECT = PURPOSES["select"][0]
K_CTR_SAP_NOISE = PURPOSES["sap_noise"][0]
K_CTR_PAIR4 = PURPOSES["bump_params"][0]
K_CTR_BIDS_NOISE = PURPOSES["bids_noise"][0]
K_CTR_FILT_TIE = PURPOSES["filtered_tie"][0]
K_CTR_FILT_GAUSS = PURPOSES["filtered_gauss"][0]
K_CTR_FILT_SOFT = PURPOSES["filtered_soft"][0]
KEY_MIX = 0x85EBCA6B


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised Philox4x32-10 over uint32 arrays (counters and keys broadcast); returns
    (x, y, z, w) as uint64 arrays holding 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) & _MASK for v in (c0, c1, c2, c3))
    k0, k1 = (np.asarray(v, dtype=np.uint64) & _MASK for v in (k0, k1))
    for _ in range(10):
        p0 = _M0 * c0
        p1 = _M1 * c2
        hi0, lo0 = p0 >> _S32, p0 & _MASK
        hi1, lo1 = p1 >> _S32, p1 & _MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + _W0) & _MASK
        k1 = (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def select_keys(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, ((seed >> 32) ^ 0x5BD1E995) & 0xFFFFFFFF


def eps_greedy_draws(seed, global_rows, counter, epsilon, n_avail):
    """(explore mask, target index among the available tasks) of the fused / standalone
    epsilon-greedy selection for the given global (env, agent) rows at one call counter."""
    rows = np.asarray(global_rows, dtype=np.uint64)
    k0, k1 = select_keys(seed)
    x, y, _, _ = philox4x32_10(rows & _MASK, rows >> np.uint64(32), K_CTR_SELECT, counter, k0, k1)
    u = (x >> np.uint64(8)).astype(np.float32) * np.float32(5.9604644775390625e-08)
    explore = u < np.float32(epsilon) if epsilon > 0 else np.zeros(rows.shape, bool)
    target = ((y * np.asarray(n_avail, dtype=np.uint64)) >> np.uint64(32)).astype(np.int64)
    return explore, target


def eps_greedy_actions(seed, row_base, counter, epsilon, avail, greedy):
    """int64 [R]: the actions of the epsilon-greedy selection over R consecutive global rows
    row_base, row_base + 1, ... (row = global env * n + agent).  avail [R, m] bool, greedy [R] =
    the rows' non-exploring choice.  An exploring row with an available task takes the target-th
    available task in index order, target = (y * n_avail) >> 32 with n_avail counted on that row."""
    avail = np.asarray(avail, dtype=bool)
    R = avail.shape[0]
    rows = np.arange(R, dtype=np.uint64) + np.uint64(int(row_base))
    n_avail = avail.sum(axis=1)
    explore, target = eps_greedy_draws(seed, rows, counter, epsilon, n_avail)
    rank = np.cumsum(avail, axis=1)  # 1-based rank of each available task among the row's available ones
    pick = np.argmax(avail & (rank == (target + 1)[:, None]), axis=1)
    return np.where(explore & (n_avail > 0), pick, np.asarray(greedy, dtype=np.int64)).astype(np.int64)


# ---- the env draws -------------------------------------------------------------------------
def global_envs(env_index_base, num_envs):
    """The global env indices env_index_base + e of a handle's envs, as Python integers."""
    return [int(env_index_base) + e for e in range(int(num_envs))]


def env_key(seed, global_env):
    """(k0, k1) of one global env (Python integers)."""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    g = int(global_env) & 0xFFFFFFFFFFFFFFFF  # the int64 index reinterpreted as a uint64
    k0 = (s & 0xFFFFFFFF) ^ (((g >> 32) * KEY_MIX) & 0xFFFFFFFF)
    k1 = (s >> 32) ^ (g & 0xFFFFFFFF)
    return k0, k1


def _keys(seed, genvs, extra_dims):
    ks = [env_key(seed, g) for g in np.atleast_1d(np.asarray(genvs, dtype=object)).tolist()]
    shape = (len(ks),) + (1,) * extra_dims
    return (np.array([k[0] for k in ks], dtype=np.uint64).reshape(shape),
            np.array([k[1] for k in ks], dtype=np.uint64).reshape(shape))


def env_words(seed, genvs, index, second, purpose, episode):
    """The four words of counter (index, second, purpose, episode) for every given global env:
    uint64 arrays [E, *index.shape] (index and second broadcast against each other)."""
    index, second = np.broadcast_arrays(np.asarray(index, dtype=np.uint64), np.asarray(second, dtype=np.uint64))
    k0, k1 = _keys(seed, genvs, index.ndim)
    return philox4x32_10(index[None], second[None], int(purpose), int(episode), k0, k1)


def task_scales(seed, genvs, episode, m):
    """float64 [E, m]: 10 where word x of counter (j, 0, 1, episode) has both low bits set, else 1."""
    x = env_words(seed, genvs, np.arange(m), 0, K_CTR_SCALE, episode)[0]
    return np.where((x & np.uint64(3)) == np.uint64(3), 10.0, 1.0)


def center_grid_exponent(T):
    """q: the center lies on the 2^-q grid, q = 24 - bit_length(T)."""
    q = 24 - int(T).bit_length()
    if T < 1 or q < 0:
        raise ValueError("T must be in [1, 2^24)")
    return q


def decode_word_exact(w, T, wmin=3, wmax=6):
    """One pair's (active, center, spread, u14) from its 32-bit word, center and spread as
    exact rationals (fractions.Fraction)."""
    w = int(w) & 0xFFFFFFFF
    q = center_grid_exponent(T)
    u16, u14 = w >> 16, (w >> 2) & 0x3FFF
    center = Fraction((u16 * int(T) * 2 ** q) // 2 ** 16, 2 ** q)
    spread = Fraction(wmin) + (Fraction(wmax) - Fraction(wmin)) * Fraction(u14, 2 ** 14)
    return (w & 3) == 3, center, spread, u14


_LN005 = np.log(0.05)
_LOG2E = np.log2(np.e)


def a2_from_spread(spread):
    """log2(e) / (2 sigma_2), sigma_2 = sqrt(spread^2 / -8 / ln 0.05), in float64."""
    spread = np.asarray(spread, dtype=np.float64)
    return _LOG2E / (2.0 * np.sqrt(spread * spread / -8.0 / _LN005))


def decode_words(w, T, wmin=3, wmax=6):
    """Vectorised decode_word_exact: (active bool, center f64, spread f64, u14 i64); the float64
    values are the exact rationals (one correctly rounded division of two integers below 2^53,
    whose quotient is representable whenever the widths are dyadic)."""
    w = np.asarray(w, dtype=np.uint64) & _MASK
    q = center_grid_exponent(T)
    u16 = w >> np.uint64(16)
    u14 = (w >> np.uint64(2)) & np.uint64(0x3FFF)
    idx = (u16 * np.uint64(int(T)) * np.uint64(2 ** q)) >> np.uint64(16)  # < T 2^q <= 2^24
    center = idx.astype(np.float64) / float(2 ** q)
    lo, hi = Fraction(wmin), Fraction(wmax)
    den = math.lcm(lo.denominator, hi.denominator)
    lo_n, span_n = int(lo * den), int((hi - lo) * den)
    num = np.int64(lo_n * 2 ** 14) + np.int64(span_n) * u14.astype(np.int64)
    spread = num.astype(np.float64) / float(den * 2 ** 14)
    return (w & np.uint64(3)) == np.uint64(3), center, spread, u14.astype(np.int64)


def pair_words(seed, genvs, episode, n, m):
    """uint64 [E, n, m]: pair p = i m + j takes word p & 3 of counter (p >> 2, 0, 9, episode)."""
    npairs = n * m
    calls = np.arange((npairs + 3) // 4)
    words = np.stack(env_words(seed, genvs, calls, 0, K_CTR_PAIR4, episode), axis=-1)  # [E, calls, 4]
    return words.reshape(words.shape[0], -1)[:, :npairs].reshape(-1, n, m)


def bump_params(seed, genvs, episode, n, m, T, wmin=3, wmax=6, dense=False):
    """Per env the bump parameters of every pair, each [E, n, m]:
    (active bool, scale f64, center f64, spread f64, u14 i64, a2 f64)."""
    active, center, spread, u14 = decode_words(pair_words(seed, genvs, episode, n, m), T, wmin, wmax)
    if dense:
        active = np.ones_like(active)
    scale = np.where(active, task_scales(seed, genvs, episode, m)[:, None, :], 0.0)
    return active, scale, center, spread, u14, a2_from_spread(spread)


def reset_perm(seed, genvs, episode, n, m):
    """int64 [E, n]: the first n of the Fisher-Yates permutation of arange(m) drawn from the top:
    for i = m - 1 .. 1, jj = (x (i + 1)) >> 32 with x of counter (i, 0, 4, episode); swap i, jj."""
    i = np.arange(m, dtype=np.uint64)
    x = env_words(seed, genvs, i, 0, K_CTR_PERM, episode)[0]
    jj = ((x * (i + np.uint64(1))[None]) >> _S32).astype(np.int64)
    E = x.shape[0]
    perm = np.tile(np.arange(m, dtype=np.int64), (E, 1))
    rows = np.arange(E)
    for k in range(m - 1, 0, -1):
        j = jj[:, k]
        a, b = perm[rows, k].copy(), perm[rows, j].copy()
        perm[rows, k], perm[rows, j] = b, a
    return perm[:, :n]


def random_actions(seed, genvs, episode, n, m, T):
    """int64 [E, T, n]: agent i at step k takes (x m) >> 32 with x of counter (i, k, 5, episode)."""
    x = env_words(seed, genvs, np.arange(n)[None, :], np.arange(T)[:, None], K_CTR_ACTION, episode)[0]
    return ((x * np.uint64(m)) >> _S32).astype(np.int64)


# ---- the selectors' draws ------------------------------------------------------------------
_2M24 = 2.0 ** -24


def normal_quads(words):
    """float64 [..., 4]: the four Box-Muller normals of Philox calls whose words are (x, y, z, w)
    (arrays of one shape): u1 = ((w >> 8) + 1) 2^-24 in (0, 1] from x and z, u2 = (w >> 8) 2^-24 in
    [0, 1) from y and w (24-bit integers: exact), then sqrt(-2 ln u1) times cos / sin of 2 pi u2."""
    x, y, z, w = (np.asarray(v, dtype=np.uint64) & _MASK for v in words)
    s8, one = np.uint64(8), np.uint64(1)
    u1 = np.stack([((x >> s8) + one), ((z >> s8) + one)], axis=-1).astype(np.float64) * _2M24
    u2 = np.stack([y >> s8, w >> s8], axis=-1).astype(np.float64) * _2M24
    r = np.sqrt(-2.0 * np.log(u1))
    t = 2.0 * np.pi * u2
    out = np.stack([r * np.cos(t), r * np.sin(t)], axis=-1)  # [..., pair (x y | z w), cos | sin]
    return out.reshape(out.shape[:-2] + (4,))


def _column_noise(seed, genvs, counter, n, m, purpose):
    """float64 [E, n, m]: counter (task j, row >> 2, purpose, counter), normal k -> row 4 (row >> 2) + k."""
    n4 = (n + 3) // 4
    z = normal_quads(env_words(seed, genvs, np.arange(m)[None, :], np.arange(n4)[:, None], purpose, counter))
    return np.moveaxis(z, -1, 2).reshape(z.shape[0], 4 * n4, m)[:, :n]  # [E, n4, m, 4] -> [E, n4, 4, m]


def sap_noise(seed, genvs, counter, n, m):
    """float64 [E, n, m]: the standard normals of the SAP selector's exploration noise."""
    return _column_noise(seed, genvs, counter, n, m, K_CTR_SAP_NOISE)


def bids_noise(seed, genvs, counter, n, m):
    """float64 [E, n, m]: the standard normals of the bids noise."""
    return _column_noise(seed, genvs, counter, n, m, K_CTR_BIDS_NOISE)


def sap_std(q, eps):
    """float64 [E]: the SAP noise's standard deviation mean|Q| eps 2 of each env, q [E, n, m]."""
    return np.abs(np.asarray(q, dtype=np.float64)).mean(axis=(1, 2)) * float(eps) * 2.0


def _flat_calls(seed, genvs, counter, second, count, purpose):
    """The words of calls 0 .. ceil(count / 4) - 1, one element per word: uint64 [E, *second.shape, count]."""
    calls = np.arange((count + 3) // 4, dtype=np.uint64)
    second = np.asarray(second, dtype=np.uint64)
    w = np.stack(env_words(seed, genvs, calls, second[..., None], purpose, counter), axis=-1)
    return w.reshape(w.shape[:-2] + (-1,))[..., :count]


def filtered_tie_u(seed, genvs, counter, n, m):
    """float32 [E, n, m]: the tie uniforms: word j & 3 of counter (j >> 2, agent i, 11, counter),
    u = (w >> 8) 2^-24."""
    w = _flat_calls(seed, genvs, counter, np.arange(n), m, K_CTR_FILT_TIE)
    return (w >> np.uint64(8)).astype(np.float32) * np.float32(_2M24)


def filtered_gauss(seed, genvs, counter, n, m):
    """float64 [E, n, m]: the standard normals of the filtered SAP selector's exploration noise:
    flat element x = i m + j takes normal x & 3 of counter (x >> 2, x >> 34, 12, counter)."""
    nm = n * m
    calls = np.arange((nm + 3) // 4, dtype=np.uint64)
    z = normal_quads(env_words(seed, genvs, calls & _MASK, calls >> _S32, K_CTR_FILT_GAUSS, counter))
    return z.reshape(z.shape[0], -1)[:, :nm].reshape(-1, n, m)


def filtered_std(mat, eps):
    """float32 [E]: per env the float64 mean of |mat| over its n m entries, rounded to float32,
    then (mean * eps) * 2 in float32."""
    mean = np.abs(np.asarray(mat, dtype=np.float64)).mean(axis=(1, 2)).astype(np.float32)
    return (mean * np.float32(eps)) * np.float32(2.0)


def filtered_soft_target(seed, genvs, counter, n, m, M, topm):
    """int64 [E, n]: the task a row picked at index M maps to: the target-th task in ascending
    order outside the agent's top M (topm [E, n, M]), target = (x (m - M)) >> 32 with x of counter
    (agent i, 0, 13, counter)."""
    x = env_words(seed, genvs, np.arange(n), 0, K_CTR_FILT_SOFT, counter)[0]
    target = ((x * np.uint64(m - M)) >> _S32).astype(np.int64)
    # s_k - k tasks outside the top M lie below the k-th smallest top task s_k, so the target-th
    # outside task has exactly those s_k with s_k - k <= target below it
    s = np.sort(np.asarray(topm, dtype=np.int64), axis=-1)
    below = ((s - np.arange(M)) <= target[..., None]).sum(axis=-1)
    return target + below
