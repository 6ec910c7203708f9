"""Case table and input generators for the LSA solver instances (tests/test_gpu_lsa_instances.py,
and their preconditions in tests/test_lsa_instance_cases_host.py).  Everything here runs on the
CPU; a case's arrays and oracle answers are built once, cached and read-only.

One wave-level solver (csrc/lsa_wave.h lsa_solve_wave<CPL>, and its register twin in
csrc/lsa_reg64.h) is stamped out behind three dispatchers; asg_lsa_instance / asg_haa_instance /
asg_bids_instance say which instance a shape runs on (cpl | storage << 8).  The table below has a
row per reachable instance of each dispatcher:

  role "main"   the smallest near-square shape the instance's storage allows with the working
                columns inside the CPL band (LDS rows: the largest row count the 48 KiB budget
                leaves at that width; global rows have no upper budget, so the two narrow bands
                are square and the two wide ones keep the row count small for the suite's time --
                the square 130 x 520 problem stands for them)
  role "edge"   the same instance with the working columns on an edge of its band (65, 128, 129,
                256, 257, 512, 513, 1024), where the storage class allows it
  role "tr"     a transposed twin, nr0 > nc0 with nr0 > 64 (multi-chunk emission)
  role "reg"    the register kernels (at most 64 working columns)

Families (all seeded, all exactly representable in the case's dtype -- asserted):
  binade   per working column a base of 1.0 or 0.5, entries base + k (base 2^-23), k in 0..7.  Two
           binades make the reduced costs odd multiples of 2^-24 next to 1, where float32 keys are
           2^-23 apart: keys collide while the float64 values differ.
  near64   (float64) 1 + a_j 2^-30 + k 2^-40, a_j in 0..4095 per column, k in 0..7: every float32
           key is shared by many columns, with equal float64 values only where a_j and k agree.
  int3     integers 0..2 (exact ties everywhere).
  corr     a shared column profile plus a small per-row term (the SAP selectors' Q-values).
The old `near32` family of test_gpu_parity.py (1 + k 2^-23 in float32) is kept as `near32` for the
host test that records why `binade` replaces it: every reduced cost of it stays a multiple of
2^-23 near 1, so its float32 keys never collide on unequal float64 values.

Contention: wide problems are trivial for scipy's scan (one step per row) unless the rows fight
for columns.  A contended case keeps the family on k = min(nr, nc) "good" working columns at random
positions over all slots and makes every other column expensive (binade: 3 + k 2^-21; near64,
int3: + 4; corr: + 8), so every row's path runs through assigned columns.  With `low` the first
half of the good columns are the working columns 0, 1, ...: they sit at the END of scipy's
`remaining`, are the ones its swap-with-last moves, and win ties among unassigned columns, so a
problem of a dozen rows (float64 in LDS at CPL 16 has no more) still depends on that bookkeeping.

HAA cases put the same structure into beta_hat = beta - lambda_ (beta > 1e-12).  A positive
beta_hat cannot show it: the selector maximizes, so the preferred entries are the large ones, whose
float32 keys are the coarse ones.  With 0 < beta < lambda_ the working matrix -beta_hat = lambda_ -
beta is positive, formed in float64 from a float32 beta of a finer binade: with s = lambda_ / 0.5
(lambda_ = 0.5 or 0.25), a column's beta is s (0.25 - k 2^-26) or s (0.125 - k 2^-27), k in 0..7,
so the working entries s (0.25 + k 2^-26) and s (0.375 + k 2^-27) are half and quarter float32
steps apart.  max(2, n / 8) columns have beta = 0.0: the mask leaves them at beta_hat = 0, the
BEST value of the matrix (without the mask they would be the worst), and the rows fight for them.
Contended cases make every column beyond the first n dear (beta = s (2^-20 + k 2^-43), beta_hat
next to -lambda_).  Four entries per problem are 1e-13 (below the mask: beta_hat = 1e-13), and
prev_assigns is drawn from the zero and good columns, so rows also share unpenalised columns
(beta_hat = beta > 0 there, or T_trans = 0 with a custom matrix).  Bids cases hand the env -W for
a contended binade W (the step maximizes).
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import oracle as ora

F32, F64 = np.float32, np.float64
REG, LDS, GLOBAL = 0, 1, 2
LDS_BUDGET = 48 * 1024
BAND_EDGES = (65, 128, 129, 256, 257, 512, 513, 1024)

Case = namedtuple("Case", "kind dtype nr nc family contended role B seed opts")


def _c(kind, dtype, nr, nc, family, contended=True, role="main", B=16, seed=0, **opts):
    return Case(kind, dtype, nr, nc, family, contended, role, B, seed, tuple(sorted(opts.items())))


def case_id(c):
    return f"{c.kind}-{np.dtype(c.dtype).name}-{c.nr}x{c.nc}-{c.family}{'-c' if c.contended else ''}-{c.role}"


def instance_of(c):
    """(cpl, storage) restated from the dispatch rules (the host test compares this with the
    library's queries over the whole table)."""
    k, K = min(c.nr, c.nc), max(c.nr, c.nc)
    cpl = 1 if K <= 64 else 2 if K <= 128 else 4 if K <= 256 else 8 if K <= 512 else 16
    if c.kind == "bids":
        return (1, REG) if K <= 64 else (cpl, LDS)
    elem = 4 if (c.kind == "haa" or c.dtype == F32) else 8
    if elem == 4 and K <= 64:
        return 1, REG
    return cpl, LDS if (elem * k * K + 15) // 16 * 16 <= LDS_BUDGET else GLOBAL


LSA_CASES = [
    # ---- float32: the register kernel
    _c("lsa", F32, 40, 64, "binade", role="reg", B=32, seed=1),
    _c("lsa", F32, 64, 64, "binade", False, role="reg", B=32),
    _c("lsa", F32, 64, 40, "binade", role="reg", B=32, seed=1),
    # ---- float32, LDS
    _c("lsa", F32, 90, 128, "binade"),
    _c("lsa", F32, 60, 65, "binade", False, role="edge"),
    _c("lsa", F32, 96, 128, "corr", False, role="edge"),
    _c("lsa", F32, 128, 90, "binade", role="tr"),
    _c("lsa", F32, 47, 256, "binade"),
    _c("lsa", F32, 90, 129, "int3", role="edge"),
    _c("lsa", F32, 48, 256, "binade", role="edge"),
    _c("lsa", F32, 30, 400, "binade"),
    _c("lsa", F32, 47, 257, "binade", role="edge"),
    _c("lsa", F32, 24, 512, "int3", role="edge"),
    _c("lsa", F32, 17, 700, "binade"),
    _c("lsa", F32, 23, 513, "binade", role="edge"),
    _c("lsa", F32, 12, 1024, "int3", role="edge"),
    # ---- float32, global
    _c("lsa", F32, 111, 111, "binade", False),
    _c("lsa", F32, 97, 128, "int3", role="edge"),
    _c("lsa", F32, 130, 130, "binade", False),
    _c("lsa", F32, 129, 129, "corr", False, role="edge"),
    _c("lsa", F32, 49, 256, "binade", role="edge"),
    _c("lsa", F32, 200, 70, "binade", role="tr"),
    _c("lsa", F32, 50, 300, "binade"),
    _c("lsa", F32, 48, 257, "int3", role="edge"),
    _c("lsa", F32, 25, 512, "binade", role="edge"),
    _c("lsa", F32, 130, 520, "binade"),
    _c("lsa", F32, 24, 513, "binade", role="edge"),
    _c("lsa", F32, 13, 1024, "int3", role="edge"),
    _c("lsa", F32, 24, 1000, "binade", role="edge"),
    _c("lsa", F32, 1000, 24, "binade", role="tr"),
    # ---- float64, LDS (CPL 1 included: float64 has no register kernel)
    _c("lsa", F64, 40, 64, "near64", B=32),
    _c("lsa", F64, 64, 64, "binade", False, role="edge", B=32),
    _c("lsa", F64, 64, 40, "near64", role="tr", B=32),
    _c("lsa", F64, 60, 100, "near64"),
    _c("lsa", F64, 60, 65, "binade", False, role="edge", seed=2),
    _c("lsa", F64, 48, 128, "binade", role="edge"),
    _c("lsa", F64, 100, 60, "near64", role="tr"),
    _c("lsa", F64, 70, 80, "binade", False, role="status"),  # more than 64 rows in float64 LDS
    _c("lsa", F64, 30, 200, "near64"),
    _c("lsa", F64, 47, 129, "binade", role="edge"),
    _c("lsa", F64, 24, 256, "int3", role="edge"),
    _c("lsa", F64, 15, 400, "near64"),
    _c("lsa", F64, 23, 257, "binade", role="edge"),
    _c("lsa", F64, 12, 512, "int3", role="edge"),
    _c("lsa", F64, 8, 700, "near64"),
    _c("lsa", F64, 11, 513, "int3", role="edge", low=True),
    _c("lsa", F64, 6, 1024, "near64", role="edge"),
    # ---- float64, global
    _c("lsa", F64, 80, 100, "near64"),
    _c("lsa", F64, 79, 79, "binade", False, role="main"),
    _c("lsa", F64, 49, 128, "corr", False, role="edge"),
    _c("lsa", F64, 40, 200, "near64"),
    _c("lsa", F64, 48, 129, "binade", role="edge"),
    _c("lsa", F64, 25, 256, "int3", role="edge"),
    _c("lsa", F64, 200, 70, "near64", role="tr"),
    _c("lsa", F64, 20, 400, "near64"),
    _c("lsa", F64, 24, 257, "binade", role="edge"),
    _c("lsa", F64, 13, 512, "int3", role="edge"),
    _c("lsa", F64, 130, 520, "near64"),
    _c("lsa", F64, 13, 513, "near64", role="edge"),
    _c("lsa", F64, 7, 1024, "int3", role="edge"),
    _c("lsa", F64, 24, 1000, "near64", role="edge"),
    _c("lsa", F64, 1000, 24, "near64", role="tr"),
]

# lam: lambda_; ttrans: a random 0/1 T_trans; strided: beta a non-contiguous view, prev strided
HAA_CASES = [
    _c("haa", F32, 40, 64, "binade", role="reg", lam=0.25),
    _c("haa", F32, 16, 24, "binade", role="reg", seed=4, lam=0.5, ttrans=True),
    _c("haa", F32, 90, 128, "binade", lam=0.25),
    _c("haa", F32, 60, 65, "binade", False, role="edge", lam=0.5),
    _c("haa", F32, 96, 128, "binade", role="edge", lam=0.5),
    _c("haa", F32, 47, 256, "binade", lam=0.5),
    _c("haa", F32, 90, 129, "binade", role="edge", lam=0.25),
    _c("haa", F32, 48, 256, "binade", role="edge", lam=0.25),
    _c("haa", F32, 30, 400, "binade", lam=0.25, ttrans=True),
    _c("haa", F32, 47, 257, "binade", role="edge", lam=0.5),
    _c("haa", F32, 24, 512, "binade", role="edge", lam=0.25),
    _c("haa", F32, 17, 700, "binade", lam=0.5, strided=True),
    _c("haa", F32, 23, 513, "binade", role="edge", lam=0.25),
    _c("haa", F32, 12, 1024, "binade", role="edge", lam=0.5),
    _c("haa", F32, 111, 111, "binade", False, lam=0.25),
    _c("haa", F32, 97, 128, "binade", role="edge", lam=0.5),
    _c("haa", F32, 60, 220, "binade", lam=0.5, ttrans=True),
    _c("haa", F32, 100, 129, "binade", role="edge", lam=0.25),
    _c("haa", F32, 49, 256, "binade", role="edge", lam=0.5),
    _c("haa", F32, 40, 400, "binade", lam=0.25, strided=True),
    _c("haa", F32, 48, 257, "binade", role="edge", lam=0.25),
    _c("haa", F32, 25, 512, "binade", role="edge", lam=0.5),
    _c("haa", F32, 30, 700, "binade", lam=0.25),
    _c("haa", F32, 24, 513, "binade", role="edge", lam=0.5),
    _c("haa", F32, 13, 1024, "binade", role="edge", lam=0.25),
]

BIDS_CASES = [
    _c("bids", F32, 40, 64, "binade", role="reg", B=8),
    _c("bids", F32, 90, 128, "binade", B=8),
    _c("bids", F32, 60, 65, "binade", False, role="edge", B=8),
    _c("bids", F32, 128, 128, "binade", False, role="edge", B=8),
    _c("bids", F32, 40, 200, "binade", B=8),
    _c("bids", F32, 90, 129, "binade", role="edge", B=8),
    _c("bids", F32, 64, 256, "binade", role="edge", B=8),
    _c("bids", F32, 30, 400, "binade", B=8),
    _c("bids", F32, 60, 257, "binade", role="edge", B=8),
    _c("bids", F32, 32, 512, "binade", role="edge", B=8),
    _c("bids", F32, 16, 700, "binade", B=8),
    _c("bids", F32, 31, 513, "binade", role="edge", B=8),
    _c("bids", F32, 16, 1024, "binade", role="edge", B=8),
]

ALL_CASES = LSA_CASES + HAA_CASES + BIDS_CASES


# ------------------------------------------------------------------------------ generators
def _rng(c):
    return np.random.RandomState((c.nr * 1009 + c.nc * 31 + c.seed * 7919 + len(c.kind) + 8 * (c.dtype == F64))
                                 % (2 ** 31))


def family_matrix(rng, family, B, k, K, dtype):
    """[B, k, K] float64 working matrices (k <= K) of a family, exact in `dtype`."""
    if family == "binade":
        base = rng.choice([1.0, 0.5], size=(B, 1, K))
        W = base + rng.randint(0, 8, size=(B, k, K)) * (base * 2.0 ** -23)
    elif family == "near64":
        assert dtype == F64
        W = 1.0 + rng.randint(0, 4096, size=(B, 1, K)) * 2.0 ** -30 + rng.randint(0, 8, size=(B, k, K)) * 2.0 ** -40
    elif family == "near32":
        W = 1.0 + rng.randint(0, 8, size=(B, k, K)) * 2.0 ** -23
    elif family == "int3":
        W = rng.randint(0, 3, size=(B, k, K)).astype(np.float64)
    elif family == "corr":
        W = (rng.normal(size=(B, 1, K)) + 0.05 * rng.normal(size=(B, k, K))).astype(dtype).astype(np.float64)
    else:
        raise ValueError(family)
    return W


def good_columns(rng, B, k, K, low=False):
    """[B, K] bool: k columns per problem at random positions over all slots; `low`: the first
    ceil(k / 2) columns among them."""
    good = np.zeros((B, K), dtype=bool)
    h = (k + 1) // 2 if low else 0
    good[:, :h] = True
    for b in range(B):
        good[b, h + rng.choice(K - h, size=k - h, replace=False)] = True
    return good


def contend(rng, W, family, dtype, low=False):
    """Keep the family on k good columns; every other column is expensive for every row."""
    B, k, K = W.shape
    bad = np.broadcast_to(~good_columns(rng, B, k, K, low)[:, None, :], W.shape)
    if family == "binade":
        W = np.where(bad, 3.0 + rng.randint(0, 8, size=W.shape) * 2.0 ** -21, W)
    elif family in ("near64", "int3"):
        W = np.where(bad, W + 4.0, W)
    else:
        W = np.where(bad, W + 8.0, W).astype(dtype).astype(np.float64)
    return W


def _exact(W, dtype):
    W = np.ascontiguousarray(W.astype(dtype))
    return W


@functools.lru_cache(maxsize=None)
def working(c):
    """The case's [B, k, K] working matrices in float64 (what scipy solves when minimizing)."""
    rng = _rng(c)
    k, K = min(c.nr, c.nc), max(c.nr, c.nc)
    W = family_matrix(rng, c.family, c.B, k, K, c.dtype)
    if c.contended:
        W = contend(rng, W, c.family, c.dtype, bool(dict(c.opts).get("low")))
    assert np.array_equal(W.astype(c.dtype).astype(np.float64), W), case_id(c)
    W.setflags(write=False)
    return W


@functools.lru_cache(maxsize=None)
def matrix(c):
    """An LSA case's cost matrices [B, nr, nc] in its dtype (minimize is the designed sense); a bids
    case's bids [B, n, m] float32 (= -working: the step maximizes)."""
    W = working(c)
    if c.kind == "bids":
        W = -W
    C = W.transpose(0, 2, 1) if c.nr > c.nc else W
    C = np.ascontiguousarray(C.astype(c.dtype))
    assert np.array_equal(C.astype(np.float64), W.transpose(0, 2, 1) if c.nr > c.nc else W)
    C.setflags(write=False)
    return C


HaaInputs = namedtuple("HaaInputs", "beta prev lam T_trans")


@functools.lru_cache(maxsize=None)
def haa_inputs(c):
    """beta [B, n, m] float32, prev [B, n] int64, lambda_, T_trans ([m, m] float64 of 0/1, or None)."""
    opts = dict(c.opts)
    lam = opts["lam"]
    s = lam / 0.5
    rng = _rng(c)
    B, n, m = c.B, c.nr, c.nc
    z = max(2, n // 8)
    cls = rng.randint(0, 2, size=(B, 1, m))
    kk = rng.randint(0, 8, size=(B, n, m))
    beta = s * np.where(cls == 0, 0.25 - kk * 2.0 ** -26, 0.125 - kk * 2.0 ** -27)
    prev = np.empty((B, n), dtype=np.int64)
    for b in range(B):
        cols = rng.permutation(m)
        zero, good = cols[:z], cols[z:n] if c.contended else cols[z:]
        beta[b][:, zero] = 0.0
        if c.contended:
            dear = cols[n:]
            beta[b][:, dear] = s * (2.0 ** -20 + rng.randint(0, 8, size=(n, dear.size)) * 2.0 ** -43)
        beta[b, rng.randint(0, n, size=4), rng.randint(0, m, size=4)] = 1e-13
        prev[b] = rng.choice(np.concatenate([zero, good]), size=n)
    beta32 = beta.astype(F32)
    big = beta > 1e-12
    assert np.array_equal(beta32[big].astype(np.float64), beta[big])
    assert (beta32 >= 0).all() and (beta32[big] < lam).all() and big.any(axis=(1, 2)).all()
    T_trans = (rng.uniform(size=(m, m)) > 0.3).astype(np.float64) if opts.get("ttrans") else None
    for a in (beta32, prev) + ((T_trans,) if T_trans is not None else ()):
        a.setflags(write=False)
    return HaaInputs(beta32, prev, lam, T_trans)


@functools.lru_cache(maxsize=None)
def haa_beta_hat(c):
    """oracle.beta_hat of the case, [B, n, m] float64 (the selector maximizes it)."""
    x = haa_inputs(c)
    out = np.stack([ora.beta_hat(x.beta[b].astype(np.float64), x.prev[b], x.lam, x.T_trans) for b in range(c.B)])
    out.setflags(write=False)
    return out


def problem(c, b, maximize=False):
    """(C, maximize) of problem b as scipy would be handed it: LSA cases minimize `matrix`, or
    maximize its negation (the same working matrix); HAA maximizes beta_hat; bids maximize."""
    if c.kind == "haa":
        return haa_beta_hat(c)[b], True
    if c.kind == "bids":
        return matrix(c)[b].astype(np.float64), True
    C = matrix(c)[b].astype(np.float64)
    return (-C, True) if maximize else (C, False)


@functools.lru_cache(maxsize=None)
def oracle_answers(c, negate=False, maximize=False):
    """oracle.lsa over the batch -> (rows [B, k], cols [B, k]) for (+-matrix, maximize)."""
    if c.kind == "haa":
        mats, maximize = haa_beta_hat(c), True
    else:
        mats = matrix(c).astype(np.float64)
        mats = -mats if negate else mats
        maximize = True if c.kind == "bids" else maximize
    ans = [ora.lsa(mats[b], maximize=maximize) for b in range(c.B)]
    rows, cols = np.stack([a[0] for a in ans]), np.stack([a[1] for a in ans])
    rows.setflags(write=False)
    cols.setflags(write=False)
    return rows, cols


def checked_problems(c):
    """Problems the numpy model is run on: two per case, one where a solve takes over a second."""
    return (0,) if min(c.nr, c.nc) >= 100 and max(c.nr, c.nc) >= 500 else (0, 1)


# ------------------------------------------------------------------------------ status batches
# one LDS and one global case per dtype, CPL >= 2 and more than 64 rows (the -1 fill loops)
STATUS_CASES = [next(c for c in LSA_CASES if (c.dtype, c.nr, c.nc) == key)
                for key in ((F32, 90, 128), (F32, 111, 111), (F64, 70, 80), (F64, 80, 100))]
INVALID, INFEASIBLE = -4, -5


@functools.lru_cache(maxsize=None)
def status_batch(c, maximize):
    """(C [8, nr, nc] in the case's dtype, expected status [8]): good problems of the case with
    scipy's error inputs mixed in.  Minimize: 1 a NaN, 2 a -inf, 4 a row of +inf (infeasible), 6 one
    +inf on the entry the row's good answer uses (stays feasible).  Maximize: the negated batch,
    and 3 a +inf (invalid under maximize) on top."""
    C = matrix(c)[:8].astype(np.float64)
    want = np.zeros(8, dtype=np.int32)
    r6 = 3
    j6 = int(oracle_answers(c)[1][6][r6])
    C[1, 3, 5] = np.nan
    C[2, 0, 1] = -np.inf
    C[4, 2, :] = np.inf
    C[6, r6, j6] = np.inf
    want[[1, 2]] = INVALID
    want[4] = INFEASIBLE
    if maximize:
        C = -C
        C[3, c.nr - 1, c.nc - 1] = np.inf
        want[3] = INVALID
    out = C.astype(c.dtype)
    out.setflags(write=False)
    want.setflags(write=False)
    return out, want
