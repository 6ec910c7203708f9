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
             (6 is the selector's, above; 7 / 10 the SAP / bids noise, not restated)

Nothing under marl_sap_amd/ imports this module.
"""
import math
from fractions import Fraction

import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
K_CTR_SCALE = 1
K_CTR_PERM = 4
K_CTR_ACTION = 5
K_CTR_SELECT = 6
K_CTR_PAIR4 = 9
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
