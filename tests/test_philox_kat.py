"""The numpy Philox restatement used by the GPU action checks (oracle/philox.py) against
the published Philox4x32-10 known-answer vectors (Random123 kat_vectors), so a wrong
checker cannot agree with a wrong kernel."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import philox as px
from oracle.philox import eps_greedy_draws, philox4x32_10

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_philox_known_answers():
    for ctr, key, want in KAT:
        got = philox4x32_10(*ctr, *key)
        assert tuple(int(v) for v in got) == want


def test_philox_vectorised_matches_scalar():
    rows = np.arange(1000, dtype=np.uint64) * np.uint64(7919) + np.uint64(2 ** 33)
    x, y, z, w = philox4x32_10(rows & np.uint64(0xFFFFFFFF), rows >> np.uint64(32), 6, 17, 0x1234, 0x5678)
    for i in (0, 1, 500, 999):
        r = int(rows[i])
        s = philox4x32_10(r & 0xFFFFFFFF, r >> 32, 6, 17, 0x1234, 0x5678)
        assert (int(x[i]), int(y[i]), int(z[i]), int(w[i])) == tuple(int(v) for v in s)


def test_eps_greedy_draw_rates():
    rows = np.arange(200000)
    explore, target = eps_greedy_draws(12345, rows, 3, 0.05, 64)
    assert abs(explore.mean() - 0.05) < 0.003
    assert target.min() >= 0 and target.max() < 64
    assert abs(np.bincount(target, minlength=64).std() / (len(rows) / 64)) < 0.05
    assert not eps_greedy_draws(12345, rows, 3, 0.0, 64)[0].any()


# ---- the env draws (oracle/philox.py: key, task scale, bump parameters, permutation, actions) ----
SEED = 0xDEADBEEF12345678  # lo32 = 0x12345678, hi32 = 0xDEADBEEF


def test_env_key_hand_vectors():
    """k0 = lo32(seed) ^ (hi32(g) * 0x85EBCA6B mod 2^32), k1 = hi32(seed) ^ lo32(g), by hand:
      g = 0:        hi32 = 0, lo32 = 0          -> (0x12345678, 0xDEADBEEF)
      g = 5:        hi32 = 0, lo32 = 5          -> k1 = 0xDEADBEEF ^ 5 = 0xDEADBEEA
      g = 2^32 - 1: hi32 = 0, lo32 = 0xFFFFFFFF -> k1 = ~0xDEADBEEF = 0x21524110
      g = 2^32:     hi32 = 1, lo32 = 0          -> k0 = 0x12345678 ^ 0x85EBCA6B = 0x97DF9C13
                    (12^85 = 97, 34^EB = DF, 56^CA = 9C, 78^6B = 13)
      g = 2^32 + 1: hi32 = 1, lo32 = 1          -> (0x97DF9C13, 0xDEADBEEE)
      g = 2^33:     hi32 = 2: 2 * 0x85EBCA6B = 0x10BD794D6 -> mod 2^32 = 0x0BD794D6 (the product wraps),
                    k0 = 0x12345678 ^ 0x0BD794D6 = 0x19E3C2AE (12^0B = 19, 34^D7 = E3, 56^94 = C2, 78^D6 = AE)
      g = -1 (int64) = 2^64 - 1: hi32 = lo32 = 0xFFFFFFFF; 0xFFFFFFFF * M mod 2^32 = -M = 0x7A143595,
                    k0 = 0x12345678 ^ 0x7A143595 = 0x682063ED, k1 = 0x21524110"""
    want = {0: (0x12345678, 0xDEADBEEF), 5: (0x12345678, 0xDEADBEEA), 2 ** 32 - 1: (0x12345678, 0x21524110),
            2 ** 32: (0x97DF9C13, 0xDEADBEEF), 2 ** 32 + 1: (0x97DF9C13, 0xDEADBEEE),
            2 ** 33: (0x19E3C2AE, 0xDEADBEEF), -1: (0x682063ED, 0x21524110)}
    for g, k in want.items():
        assert px.env_key(SEED, g) == k, hex(g)
    # the vectorised path keys each env with the same pair
    gs = list(want)
    x = px.env_words(SEED, gs, np.arange(3), 0, 9, 2)
    for e, g in enumerate(gs):
        for i in range(3):
            s = philox4x32_10(i, 0, 9, 2, *want[g])
            assert tuple(int(v[e, i]) for v in x) == tuple(int(v) for v in s)


def test_bump_decode_hand_vectors():
    """active = (w & 3) == 3, u16 = w >> 16, u14 = (w >> 2) & 0x3fff, q = 24 - bit_length(T),
    center = floor(u16 T 2^q / 2^16) 2^-q, spread = 3 + 3 u14 / 2^14.
    T = 20: bit_length 5, q = 19 >= 16, so u16 T 2^q / 2^16 = u16 T 2^3 is an integer (no floor):
      w = 0xFFFFFFFF: u16 = 65535, center = 65535 * 20 / 65536 = 20 - 20/65536 = 19.99969482421875;
                      u14 = 16383, spread = 3 + 3 * 16383/16384 = 6 - 3/16384 = 5.99981689453125
      w = 0x00000003: u16 = 0, u14 = 0: center 0, spread 3, active
      w = 0x80000000: u16 = 32768: center = 32768 * 20 / 65536 = 10; low bits 00: inactive
    T = 300: bit_length 9, q = 15 < 16: the grid index is floor(u16 * 300 / 2).  300 is even, so
    nothing is dropped here:
      w = 0xABCD0007: u16 = 0xABCD = 43981, index = 43981 * 150 = 6597150,
                      center = 6597150 / 32768 = 201 + 10782/32768 = 201.32904052734375;
                      u14 = 7 >> 2 = 1, spread = 3 + 3/16384 = 3.00018310546875; low bits 11: active
    T = 301 (same q = 15, odd T): the floor drops a half:
      w = 0xABCD0007: 43981 * 301 = 13238281, / 2 = 6619140.5 -> index 6619140,
                      center = 6619140 / 32768 = 202 + 4/32768 = 202.0001220703125
                      (the unfloored 13238281 / 65536 = 202.00013732910156...)"""
    cases = [(0xFFFFFFFF, 20, True, 19.99969482421875, 5.99981689453125, 16383),
             (0x00000003, 20, True, 0.0, 3.0, 0),
             (0x80000000, 20, False, 10.0, 3.0, 0),
             (0xABCD0007, 300, True, 201.32904052734375, 3.00018310546875, 1),
             (0xABCD0007, 301, True, 202.0001220703125, 3.00018310546875, 1)]
    for w, T, active, center, spread, u14 in cases:
        a, c, s, u = px.decode_word_exact(w, T)
        assert (a, u) == (active, u14), hex(w)
        assert c == Fraction(center) and s == Fraction(spread), (hex(w), T, float(c), float(s))
        av, cv, sv, uv = px.decode_words(np.array([w]), T)
        assert (bool(av[0]), int(uv[0])) == (active, u14)
        assert cv[0] == center and sv[0] == spread
    assert Fraction(13238281, 65536) > Fraction(202.0001220703125)  # a bit was dropped at T = 301
    # a2 = log2(e) / (2 sqrt(spread^2 / -8 / ln 0.05)) = log2(e) sqrt(-2 ln 0.05) / spread
    a2 = px.a2_from_spread(np.array([3.0, 6.0]))
    np.testing.assert_allclose(a2, np.log2(np.e) * np.sqrt(-2 * np.log(0.05)) / np.array([3.0, 6.0]), rtol=1e-15)
    # other widths (the __init__ draw's U(5, 8)) are arguments
    assert px.decode_word_exact(0xFFFFFFFF, 20, 5, 8)[2] == Fraction(8) - Fraction(3, 16384)
    assert px.decode_words(np.array([3]), 20, 5, 8)[2][0] == 5.0


T_SET = [1, 2, 16, 20, 100, 255, 256, 300, 1000]


@pytest.mark.parametrize("T", T_SET)
def test_bump_decode_exact_in_float32(T):
    """Over 120,000 random words per T (1.08e6 in all), plus the extreme fields: center and spread
    are float32 values, center < T, and t - center is exact in float32 for t = 0 and t = T - 1 --
    so the device's float32 parameters can be compared bit for bit."""
    r = np.random.RandomState(1000 + T)
    w = r.randint(0, 2 ** 32, size=120000, dtype=np.uint64)
    w[:4] = [0, 0xFFFFFFFF, 0xFFFF0000, 0x0000FFFF]
    active, center, spread, u14 = px.decode_words(w, T)
    assert np.array_equal(center.astype(np.float32).astype(np.float64), center)
    assert np.array_equal(spread.astype(np.float32).astype(np.float64), spread)
    assert center.min() >= 0.0 and center.max() < T
    assert spread.min() >= 3.0 and spread.max() < 6.0
    c32 = center.astype(np.float32)
    for t in (0, T - 1):
        d32 = np.float32(t) - c32
        assert d32.dtype == np.float32
        assert np.array_equal(d32.astype(np.float64), float(t) - center), t
    # the vectorised decode is the exact-rational one
    for i in list(range(4)) + list(r.randint(0, len(w), size=200)):
        a, c, s, u = px.decode_word_exact(int(w[i]), T)
        assert (a, u) == (bool(active[i]), int(u14[i]))
        assert c == Fraction(float(center[i])) and s == Fraction(float(spread[i]))


def test_env_draw_distributions():
    """The oracle alone follows the distributions of the specification.  Bounds are five standard
    deviations of the statistic under the specification (the draws are deterministic: this either
    passes always or never)."""
    n = m = 64
    T, E = 20, 64
    g = px.global_envs(0, E)
    active, scale, center, spread, u14, a2 = px.bump_params(11, g, 0, n, m, T)
    N = active.size
    assert abs(active.mean() - 0.25) < 5 * np.sqrt(0.25 * 0.75 / N)
    assert abs(center.mean() - T / 2) < 5 * T / np.sqrt(12 * N)
    assert 3.0 <= spread.min() and spread.max() < 6.0 and spread.max() - spread.min() > 2.99
    assert abs(spread.mean() - 4.5) < 5 * 3 / np.sqrt(12 * N)
    assert set(np.unique(scale)) == {0.0, 1.0, 10.0} and np.array_equal(scale > 0, active)
    ts = px.task_scales(11, px.global_envs(0, 512), 0, m)
    assert set(np.unique(ts)) == {1.0, 10.0}
    assert abs((ts == 10.0).mean() - 0.25) < 5 * np.sqrt(0.25 * 0.75 / ts.size)
    # an active pair carries its task's scale
    assert np.array_equal(scale, active * ts[:E, None, :])
    # dense: every pair active, the same centers and widths
    d = px.bump_params(11, g[:2], 0, n, m, T, dense=True)
    assert d[0].all() and np.array_equal(d[1], np.broadcast_to(ts[:2, None, :], d[1].shape))
    assert np.array_equal(d[2], center[:2]) and np.array_equal(d[4], u14[:2])

    E, n, m = 4096, 5, 16
    g = px.global_envs(7, E)
    full = px.reset_perm(3, g, 1, m, m)
    assert np.array_equal(np.sort(full, axis=1), np.tile(np.arange(m), (E, 1)))
    assert np.array_equal(px.reset_perm(3, g, 1, n, m), full[:, :n])
    for col in (0, n - 1, m - 1):  # chi-square, 15 degrees of freedom: P(> 50) ~ 1e-5
        cnt = np.bincount(full[:, col], minlength=m)
        assert ((cnt - E / m) ** 2 / (E / m)).sum() < 50.0, col

    acts = px.random_actions(3, px.global_envs(0, 64), 0, 16, m, 20)
    assert acts.shape == (64, 20, 16) and acts.min() == 0 and acts.max() == m - 1
    cnt = np.bincount(acts.ravel(), minlength=m)
    assert ((cnt - acts.size / m) ** 2 / (acts.size / m)).sum() < 50.0


def test_env_draws_depend_on_every_key_part():
    """Changing any one of seed low word, seed high word, global env index, episode or counter
    purpose changes every draw."""
    n, m, T = 5, 6, 7
    base = dict(seed=SEED, g=[9], episode=3)
    variants = [dict(base, seed=SEED ^ 1), dict(base, seed=SEED ^ (1 << 32)), dict(base, g=[10]),
                dict(base, g=[9 + 2 ** 32]), dict(base, episode=4)]

    def draws(seed, g, episode):
        p = px.bump_params(seed, g, episode, n, m, T)
        return [px.task_scales(seed, g, episode, 64), p[2], p[4], px.reset_perm(seed, g, episode, 64, 64),
                px.random_actions(seed, g, episode, n, 1000, T)]

    ref = draws(**base)
    for v in variants:
        for a, b in zip(ref, draws(**v)):
            assert not np.array_equal(a, b), v
    words = {p: px.env_words(SEED, [9], np.arange(8), 0, p, 3)[0] for p in (1, 2, 3, 4, 5, 6, 8, 9)}
    keys = list(words)
    for i, p in enumerate(keys):
        for q in keys[i + 1:]:
            assert not np.array_equal(words[p], words[q]), (p, q)
    # the purposes the draws use
    assert np.array_equal(px.pair_words(SEED, [9], 3, 2, 4)[0].ravel(),
                          np.stack(px.env_words(SEED, [9], np.arange(2), 0, 9, 3), -1).ravel())
    assert np.array_equal(px.task_scales(SEED, [9], 3, 8)[0] == 10.0, (words[1][0] & np.uint64(3)) == np.uint64(3))


def test_pair_words_straddle_rows():
    """m % 4 != 0: a call's four words serve pairs of two rows (p = i m + j, word p & 3 of call p >> 2)."""
    n, m = 3, 9
    pw = px.pair_words(5, [0, 1], 2, n, m)
    for e in (0, 1):
        for i in range(n):
            for j in range(m):
                p = i * m + j
                k0, k1 = px.env_key(5, e)
                assert int(pw[e, i, j]) == int(philox4x32_10(p >> 2, 0, 9, 2, k0, k1)[p & 3])
