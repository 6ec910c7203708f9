"""The restatement of the selectors' Philox draws (oracle/philox.py) checked on the CPU, so a
wrong checker cannot agree with a wrong kernel in tests/test_gpu_selector_draws.py: the
Box-Muller decode on the published Philox known-answer outputs, one hand-laid-out element per
draw family, the purpose table (also against the kernels' own enum), the moments and
cross-correlations of the three Gaussian families, and the two index maps (soft map, epsilon-greedy)
against brute-force loops."""
import math
import os
import re

import numpy as np
import pytest

from oracle import philox as px
from oracle.philox import philox4x32_10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "marl_sap_amd", "csrc")
SEED = 0xDEADBEEF12345678  # lo32 = 0x12345678, hi32 = 0xDEADBEEF
# global env 2^32 + 1 under SEED (tests/test_philox_kat.py::test_env_key_hand_vectors)
G, KEY = 2 ** 32 + 1, (0x97DF9C13, 0xDEADBEEE)


def test_normal_quads_hand_vectors():
    """The three published Philox4x32-10 outputs (tests/test_philox_kat.py KAT), decoded by hand:
    a = (x >> 8) + 1, b = y >> 8, c = (z >> 8) + 1, d = w >> 8 (drop the low byte, add one to the
    radius words), u = integer / 2^24, ra = sqrt(-2 log(a / 2^24)), rb = sqrt(-2 log(c / 2^24)):

      (6627E8D5, E169C58D, BC57AC4C, 9B00DBD8): a = 0x6627E9 = 6694889, b = 0xE169C5 = 14772677,
          c = 0xBC57AD = 12343213, d = 0x9B00DB = 10158299
          ra = math.sqrt(-2 * math.log(6694889 / 2**24)) = 1.3554905945860984
          rb = math.sqrt(-2 * math.log(12343213 / 2**24)) = 0.7834735708583972
          ra * math.cos(2 * math.pi * 14772677 / 2**24) =  0.9911374751458971
          ra * math.sin(2 * math.pi * 14772677 / 2**24) = -0.9246627803544332
          rb * math.cos(2 * math.pi * 10158299 / 2**24) = -0.6176090549848544
          rb * math.sin(2 * math.pi * 10158299 / 2**24) = -0.4820683472644963
      (408F276D, 41C83B0E, A20BC7C6, 6D5451FD): a = 0x408F28 = 4230952, b = 0x41C83B = 4311099,
          c = 0xA20BC8 = 10619848, d = 0x6D5451 = 7165009
          ra = 1.6598763499951268, rb = 0.9563441560241266
          normals -0.07258075259421823, 1.6582887359039744, -0.8576777618271872, 0.42306382689684746
      (D16CFE09, 94FDCCEB, 5001E420, 24126EA1): a = 0xD16CFF = 13724927, b = 0x94FDCC = 9764300,
          c = 0x5001E5 = 5243365, d = 0x24126E = 2364014
          ra = 0.6337319730838077, rb = 1.5251611768435778
          normals -0.5514679117504742, -0.31224886872215757, 0.9654673558991425, 1.1806732825146868"""
    cases = [
        ((0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8), (6694889, 14772677, 12343213, 10158299),
         (0.9911374751458971, -0.9246627803544332, -0.6176090549848544, -0.4820683472644963)),
        ((0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD), (4230952, 4311099, 10619848, 7165009),
         (-0.07258075259421823, 1.6582887359039744, -0.8576777618271872, 0.42306382689684746)),
        ((0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1), (13724927, 9764300, 5243365, 2364014),
         (-0.5514679117504742, -0.31224886872215757, 0.9654673558991425, 1.1806732825146868)),
    ]
    for words, (a, b, c, d), literal in cases:
        ra = math.sqrt(-2 * math.log(a / 2 ** 24))
        rb = math.sqrt(-2 * math.log(c / 2 ** 24))
        want = [ra * math.cos(2 * math.pi * b / 2 ** 24), ra * math.sin(2 * math.pi * b / 2 ** 24),
                rb * math.cos(2 * math.pi * d / 2 ** 24), rb * math.sin(2 * math.pi * d / 2 ** 24)]
        got = px.normal_quads([np.array([v]) for v in words])
        assert got.shape == (1, 4) and got.dtype == np.float64
        for k in range(4):
            assert abs(got[0, k] - want[k]) <= 1e-15, (hex(words[0]), k, got[0, k], want[k])
            assert abs(want[k] - literal[k]) <= 1e-15, (hex(words[0]), k)
    # the radius word 0xFFFFFFxx gives u1 = 1 exactly (z = 0, never log(0)); 0x000000xx gives 2^-24
    edge = px.normal_quads([np.array([0xFFFFFFFF, 0x000000FF])] + [np.array([0, 0])] * 3)
    assert edge[0, 0] == 0.0 and edge[0, 1] == 0.0
    assert abs(edge[1, 0] - math.sqrt(2 * 24 * math.log(2))) <= 1e-15  # the largest radius, 5.768


def _quad(c0, c1, purpose, counter):
    return [np.array([int(v)]) for v in philox4x32_10(c0, c1, purpose, counter, *KEY)]


def test_layout_hand_vectors():
    """One element per family with (c0, c1, purpose, counter, key) laid out by hand, global env
    2^32 + 1 under SEED (key (0x97DF9C13, 0xDEADBEEE)), call counter 7:
      SAP / bids noise, row 35 of task 3:  35 = 4 * 8 + 3 -> counter (3, 8, 7 | 10, 7), normal 3
                                           (the sin member of the (z, w) pair)
      filtered Gaussian, flat element 37 of a 5 x 9 matrix (agent 4, task 1): 37 = 4 * 9 + 1 ->
                                           counter (9, 0, 12, 7), normal 1 (the sin of (x, y))
      filtered tie, task 6 of agent 2:     6 = 4 * 1 + 2 -> counter (1, 2, 11, 7), word 2 (z)
      filtered soft map, agent 3:          counter (3, 0, 13, 7), word 0 (x)"""
    assert px.env_key(SEED, G) == KEY
    others = [0, G, 5]
    sap = px.sap_noise(SEED, others, 7, 40, 9)
    assert sap.shape == (3, 40, 9) and sap[1, 35, 3] == px.normal_quads(_quad(3, 8, 7, 7))[0, 3]
    bids = px.bids_noise(SEED, others, 7, 40, 9)
    assert bids[1, 35, 3] == px.normal_quads(_quad(3, 8, 10, 7))[0, 3]
    assert bids[1, 35, 3] != sap[1, 35, 3]
    gauss = px.filtered_gauss(SEED, others, 7, 5, 9)
    assert gauss.shape == (3, 5, 9) and gauss[1, 4, 1] == px.normal_quads(_quad(9, 0, 12, 7))[0, 1]
    tie = px.filtered_tie_u(SEED, others, 7, 4, 9)
    z = int(_quad(1, 2, 11, 7)[2][0])
    assert tie.shape == (3, 4, 9) and tie.dtype == np.float32
    assert tie[1, 2, 6] == np.float32((z >> 8) / 2.0 ** 24)
    x = int(_quad(3, 0, 13, 7)[0][0])
    m, M = 50, 5
    topm = np.tile(np.arange(m - M, m), (3, 6, 1))  # the top M are the last tasks: target-th outside = target
    assert px.filtered_soft_target(SEED, others, 7, 6, m, M, topm)[1, 3] == (x * (m - M)) >> 32
    # the std formulas on a matrix whose mean|.| is exact: mean 1.5, eps 0.25 -> 0.75
    mat = np.array([[[1.0, -2.0], [1.5, -1.5]]], dtype=np.float32)
    assert px.sap_std(mat, 0.25)[0] == 0.75 and px.sap_std(mat, 0.25).dtype == np.float64
    fs = px.filtered_std(mat, 0.25)
    assert fs[0] == np.float32(0.75) and fs.dtype == np.float32
    # float32 steps: mean = float32(0.1) (not 0.1), then two float32 products
    m01 = np.float32(0.1)
    assert px.filtered_std(np.full((1, 3, 5), 0.1), 0.3)[0] == (m01 * np.float32(0.3)) * np.float32(2.0)


def _kernel_purposes():
    """Every `kCtrName = value` of the kernels' sources, per file."""
    found = {}
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name), encoding="utf-8") as f:
            for ident, value in re.findall(r"\bkCtr(\w+)\s*=\s*(\d+)u?\b", f.read()):
                found.setdefault(name, {})[ident] = int(value)
    return found


def test_purpose_table_is_disjoint_and_is_the_kernels():
    """No two draw families under the env key share a purpose word (two that did would read the
    same Philox words for one seed, global env and counter), here and in the kernels: every
    kCtr enumerator lives in the one enum of asg_device.h, with distinct values, and each family
    restated here carries the kernels' value."""
    env = [p for p, key in px.PURPOSES.values() if key == "env"]
    assert len(set(env)) == len(env), sorted(env)
    allp = [p for p, _ in px.PURPOSES.values()]
    assert len(set(allp)) == len(allp)
    found = _kernel_purposes()
    assert list(found) == ["asg_device.h"], f"purpose words defined outside asg_device.h: {sorted(found)}"
    dev = found["asg_device.h"]
    assert len(set(dev.values())) == len(dev), dev
    names = {"task_scale": "Scale", "reset_perm": "Perm", "random_action": "Action", "select": "Select",
             "sap_noise": "SapNoise", "bump_params": "Pair4", "bids_noise": "BidsNoise", "filtered_tie": "FiltTie",
             "filtered_gauss": "FiltGauss", "filtered_soft": "FiltSoft"}
    assert set(names) == set(px.PURPOSES)
    for family, ident in names.items():
        assert dev[ident] == px.PURPOSES[family][0], family
    # equal counters under one key: the filtered Gaussian words are not the bump parameters', the
    # soft map's word not the bids noise's
    calls = np.arange(16)
    for a, b in [(px.K_CTR_FILT_GAUSS, px.K_CTR_PAIR4), (px.K_CTR_FILT_SOFT, px.K_CTR_BIDS_NOISE),
                 (px.K_CTR_FILT_TIE, px.K_CTR_SAP_NOISE)]:
        wa, wb = px.env_words(SEED, [G], calls, 0, a, 3), px.env_words(SEED, [G], calls, 0, b, 3)
        assert not any(np.array_equal(x, y) for x, y in zip(wa, wb)), (a, b)


def _corr(a, b):
    a, b = a.ravel(), b.ravel()
    assert a.size == b.size and a.size >= 200_000
    return abs(float(np.corrcoef(a, b)[0, 1])), 4.0 / math.sqrt(a.size)


@pytest.mark.parametrize("family", ["sap_noise", "bids_noise", "filtered_gauss"])
def test_gaussian_families_moments_and_independence(family):
    """100 consecutive global envs (across the 2^32 carry) of a 64 x 64 matrix: 409,600 draws, so
    every statistic below has N >= 2e5 samples.  |mean| < 4 / sqrt(N), |var - 1| < 0.02, and
    |corr| < 4 / sqrt(N pairs) between the cos and sin members of a pair, rows r and r + 4 (the
    next call of the column families), tasks j and j + 1, envs g and g + 1.  The draws are
    deterministic: this passes always or never."""
    n = m = 64
    g = px.global_envs(2 ** 32 - 50, 100)
    z = getattr(px, family)(SEED, g, 7, n, m)
    N = z.size
    assert N >= 200_000 and z.shape == (100, n, m)
    assert abs(z.mean()) < 4.0 / math.sqrt(N), z.mean()
    assert abs(z.var() - 1.0) < 0.02, z.var()
    assert np.abs(z).max() <= math.sqrt(2 * 24 * math.log(2))
    if family == "filtered_gauss":  # normal x & 3 of the flat element x
        q = z.reshape(100, -1, 4)
    else:                           # normal row & 3
        q = np.moveaxis(z.reshape(100, n // 4, 4, m), 2, -1)
    pairs = {"cos-sin": (q[..., [0, 2]], q[..., [1, 3]]), "rows r, r+4": (z[:, :-4], z[:, 4:]),
             "tasks j, j+1": (z[:, :, :-1], z[:, :, 1:]), "envs g, g+1": (z[:-1], z[1:]),
             "pair (x,y) with (z,w)": (q[..., :2], q[..., 2:])}
    for name, (a, b) in pairs.items():
        c, bound = _corr(a, b)
        assert c < bound, (family, name, c, bound)


def test_gaussian_families_are_different_streams():
    g = px.global_envs(3, 2)
    a, b, c = (f(SEED, g, 7, 8, 8) for f in (px.sap_noise, px.bids_noise, px.filtered_gauss))
    assert not np.isin(a, b).any() and not np.isin(a, c).any() and not np.isin(b, c).any()
    assert not np.isin(px.sap_noise(SEED, g, 8, 8, 8), a).any()       # another call counter
    assert not np.isin(px.sap_noise(SEED ^ 1, g, 7, 8, 8), a).any()   # another seed


def test_filtered_tie_u_is_uniform_on_the_24_bit_grid():
    u = px.filtered_tie_u(SEED, px.global_envs(0, 8), 1, 16, 450)
    assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
    assert np.array_equal(u * np.float32(2.0 ** 24), np.rint(u * np.float32(2.0 ** 24)))
    N = u.size
    assert abs(float(u.astype(np.float64).mean()) - 0.5) < 4.0 / math.sqrt(12 * N)
    c = float(np.corrcoef(u[:, :, :-1].ravel(), u[:, :, 1:].ravel())[0, 1])
    assert abs(c) < 4.0 / math.sqrt(N)


@pytest.mark.parametrize("m,M", [(7, 5), (50, 5), (450, 5), (12, 11), (64, 1)])
def test_filtered_soft_target_vs_sorted_complement(m, M):
    rng = np.random.RandomState(m * 100 + M)
    E, n = 6, 9
    topm = np.stack([[rng.permutation(m)[:M] for _ in range(n)] for _ in range(E)])
    topm[0, 0] = np.arange(M)              # the top M are the first tasks
    topm[0, 1] = np.arange(m - M, m)[::-1]  # ... the last tasks, descending
    g = px.global_envs(2 ** 32 - 2, E)
    got = px.filtered_soft_target(SEED, g, 4, n, m, M, topm)
    assert got.shape == (E, n) and got.dtype == np.int64
    seen = set()
    for e in range(E):
        k0, k1 = px.env_key(SEED, g[e])
        for i in range(n):
            x = int(philox4x32_10(i, 0, 13, 4, k0, k1)[0])
            outside = sorted(set(range(m)) - set(topm[e, i].tolist()))
            target = (x * (m - M)) >> 32
            assert got[e, i] == outside[target], (e, i)
            seen.add(target)
    assert m - M == 1 or len(seen) > 1


@pytest.mark.parametrize("m", [1, 7, 64, 130, 1100])
def test_eps_greedy_actions_vs_loop(m):
    rng = np.random.RandomState(m)
    R, eps, counter, row_base = 400, 0.3, 5, 2 ** 32 - 200
    avail = rng.uniform(size=(R, m)) < 0.5
    avail[np.arange(R), rng.randint(0, m, size=R)] = True  # at least one task per row
    single = np.arange(0, R, 5)                             # rows with exactly one available task
    avail[single] = False
    avail[single, rng.randint(0, m, size=single.size)] = True
    greedy = rng.randint(0, m, size=R)
    got = px.eps_greedy_actions(SEED, row_base, counter, eps, avail, greedy)
    assert got.shape == (R,) and got.dtype == np.int64
    k0, k1 = px.select_keys(SEED)
    explored = 0
    for r in range(R):
        grow = row_base + r
        x, y, _, _ = (int(v) for v in philox4x32_10(grow & 0xFFFFFFFF, grow >> 32, 6, counter, k0, k1))
        want = int(greedy[r])
        if (x >> 8) / 2.0 ** 24 < float(np.float32(eps)):
            tasks = [j for j in range(m) if avail[r, j]]
            want = tasks[(y * len(tasks)) >> 32]
            explored += 1
        assert got[r] == want, r
    assert 0.2 * R < explored < 0.4 * R
    assert (avail.sum(1) == 1).sum() >= single.size
    # epsilon 0 explores nowhere; a row without an available task keeps its greedy choice
    assert np.array_equal(px.eps_greedy_actions(SEED, row_base, counter, 0.0, avail, greedy), greedy)
    none = np.zeros((R, m), bool)
    assert np.array_equal(px.eps_greedy_actions(SEED, row_base, counter, 1.0, none, greedy), greedy)
