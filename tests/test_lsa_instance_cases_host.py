"""Preconditions of tests/test_gpu_lsa_instances.py, proved on the CPU: the case table
(tests/lsa_instance_cases.py) reaches every solver instance the three dispatchers can launch, and
every case's inputs drive scipy's scan through the selection paths the case is there for.

The reachable instances are enumerated from the library's own host queries (asg_lsa_instance,
asg_haa_instance, asg_bids_instance -- the functions the launchers switch on) over a grid of legal
shapes, not written out by hand.  The selection paths are counted by an instrumented numpy
restatement of scipy's algorithm (tests/lsa_scan_model.py), which must agree with
scipy.optimize.linear_sum_assignment and with the C oracle on every problem it is run on.

Class conditions (conditions on the inputs; seeds were chosen so that they hold):
  contended   the scan takes more steps than rows in every checked problem
  binade      at least one step of each class: single, tie_unassigned, tie_assigned, exact64
  near64      at least one exact64 step and one tie_assigned step
  int3        at least one tie_unassigned and one tie_assigned step
  corr        at least one tie_assigned step (continuous values tie only at zero reduced cost,
              between assigned columns; float64 corr values also collide in float32)
  wide        with more than 64 working columns, each required tie class has a step whose
              candidates lie in more than one 64-column slot
"""
import numpy as np
import pytest

from oracle import oracle as ora
from tests import lsa_instance_cases as lc
from tests import lsa_scan_model as sm

scipy_lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment

GRID = (1, 2, 3, 5, 8, 12, 16, 24, 32, 40, 47, 48, 49, 56, 63, 64, 65, 80, 96, 97, 100, 111, 127, 128, 129, 160, 200,
        255, 256, 257, 300, 400, 511, 512, 513, 700, 1000, 1023, 1024)
REQUIRED = {"binade": ("single", "tie_unassigned", "tie_assigned", "exact64"), "near64": ("exact64", "tie_assigned"),
            "int3": ("tie_unassigned", "tie_assigned"), "corr": ("tie_assigned",)}


@pytest.fixture(scope="module")
def L():
    from marl_sap_amd import build, _lib
    build.build()
    return _lib.lib()


def _query(L, c):
    from marl_sap_amd import _lib
    if c.kind == "lsa":
        return L.asg_lsa_instance(_lib.ASG_F32 if c.dtype == lc.F32 else _lib.ASG_F64, c.nr, c.nc)
    return (L.asg_haa_instance if c.kind == "haa" else L.asg_bids_instance)(c.nr, c.nc)


def test_table_shapes_classify_as_stated(L):
    for c in lc.ALL_CASES:
        cpl, storage = lc.instance_of(c)
        assert _query(L, c) == cpl | storage << 8, lc.case_id(c)
        assert 8 <= c.B <= 32


def test_table_covers_every_reachable_instance(L):
    from marl_sap_amd import _lib
    reach = {"lsa32": set(), "lsa64": set(), "haa": set(), "bids": set()}
    for nr in GRID:
        for nc in GRID:
            reach["lsa32"].add(L.asg_lsa_instance(_lib.ASG_F32, nr, nc))
            reach["lsa64"].add(L.asg_lsa_instance(_lib.ASG_F64, nr, nc))
            if nr <= nc:
                reach["haa"].add(L.asg_haa_instance(nr, nc))
                if nr * nc <= 16384:
                    reach["bids"].add(L.asg_bids_instance(nr, nc))
    assert all(min(v) >= 0 for v in reach.values())
    # what the dispatch rules allow: 1 register + 8 wave instances for float32 (LDS and global at
    # CPL 2..16), 5 LDS + 4 global for float64, 1 + 8 for HAA, 1 + 4 for the bids
    assert [len(reach[k]) for k in ("lsa32", "lsa64", "haa", "bids")] == [9, 9, 9, 5]
    have = {k: set() for k in reach}
    for c in lc.ALL_CASES:
        have[{"lsa": "lsa32" if c.dtype == lc.F32 else "lsa64"}.get(c.kind, c.kind)].add(_query(L, c))
    assert have == reach
    # every wave instance has a main row and a row on an edge of its column band; transposed
    # twins of more than 64 rows in LDS and global per dtype; a 130-row CPL 16 problem per dtype
    for key in reach:
        for inst in reach[key]:
            if inst & 0xff == 1:
                continue
            rows = [c for c in lc.ALL_CASES
                    if {"lsa": "lsa32" if c.dtype == lc.F32 else "lsa64"}.get(c.kind, c.kind) == key
                    and _query(L, c) == inst]
            assert any(c.role == "main" for c in rows), (key, hex(inst))
            assert any(max(c.nr, c.nc) in lc.BAND_EDGES for c in rows), (key, hex(inst))
    for dtype in (lc.F32, lc.F64):
        for storage in (lc.LDS, lc.GLOBAL):
            assert any(c.dtype == dtype and c.nr > c.nc and c.nr > 64 and lc.instance_of(c)[1] == storage
                       for c in lc.LSA_CASES), (dtype, storage)
        assert any(c.dtype == dtype and min(c.nr, c.nc) >= 130 and lc.instance_of(c)[0] == 16 for c in lc.LSA_CASES)


def test_rejected_shapes_return_the_error(L):
    from marl_sap_amd import _lib
    E = _lib.ASG_E_INVALID_ARG
    assert L.asg_lsa_instance(5, 4, 4) == E                      # not a float dtype
    assert L.asg_lsa_instance(_lib.ASG_F32, 1025, 4) == L.asg_lsa_instance(_lib.ASG_F64, 4, 1025) == E
    assert L.asg_lsa_instance(_lib.ASG_F32, 0, 4) == L.asg_lsa_instance(_lib.ASG_F32, 4, -1) == E
    assert L.asg_haa_instance(9, 8) == L.asg_haa_instance(4, 1025) == L.asg_haa_instance(0, 4) == E
    assert L.asg_bids_instance(9, 8) == L.asg_bids_instance(128, 129) == L.asg_bids_instance(17, 1024) == E
    assert L.asg_bids_instance(128, 128) == 2 | _lib.ASG_LSA_LDS << 8   # the documented maximum


_counts = {}


def _model(c):
    """Model, scipy and the oracle on the case's checked problems -> summed step-class counts."""
    if c not in _counts:
        total, per_problem = sm.new_counts(), []
        for b in lc.checked_problems(c):
            C, maximize = lc.problem(c, b)
            row, col, cnt = sm.solve(C, maximize)
            r1, c1 = scipy_lsa(C, maximize=maximize)
            r2, c2 = ora.lsa(C, maximize=maximize)
            assert np.array_equal(row, r1) and np.array_equal(col, c1), (lc.case_id(c), b, "model vs scipy")
            assert np.array_equal(r1, r2) and np.array_equal(c1, c2), (lc.case_id(c), b, "scipy vs oracle")
            per_problem.append(cnt)
            total = sm.add_counts(total, cnt)
        _counts[c] = (total, per_problem)
    return _counts[c]


@pytest.mark.parametrize("c", lc.ALL_CASES, ids=lc.case_id)
def test_case_agrees_on_the_cpu_and_meets_its_class_conditions(c):
    total, per_problem = _model(c)
    # the answers the GPU tests compare with are the oracle's over the whole batch: scipy agrees
    if c.kind == "lsa":
        for negate, maximize in ((False, False), (True, True), (False, True)):
            rows, cols = lc.oracle_answers(c, negate, maximize)
            for b in lc.checked_problems(c):
                C = lc.matrix(c)[b].astype(np.float64)
                r1, c1 = scipy_lsa(-C if negate else C, maximize=maximize)
                assert np.array_equal(rows[b], r1) and np.array_equal(cols[b], c1), (b, negate, maximize)
        if c.nr > c.nc:
            assert np.array_equal(lc.oracle_answers(c)[0], lc.oracle_answers(c, True, True)[0])
        assert np.array_equal(lc.oracle_answers(c)[1], lc.oracle_answers(c, True, True)[1])
    if c.contended:
        for cnt in per_problem:
            assert cnt["steps"] > cnt["rows"], cnt
    wide = max(c.nr, c.nc) > 64
    for cls in REQUIRED[c.family]:
        assert total[cls] >= 1, (cls, total)
        if wide and cls != "single":
            assert total["x_" + cls] >= 1, ("x_" + cls, total)


def test_old_near32_family_never_reaches_the_exact_float64_path():
    """test_gpu_parity.py's `near32` (float32, 1 + k 2^-23, 40 x 64) was described as the case whose
    float32 keys collide on unequal float64 values.  They never do: every reduced cost of it stays a
    multiple of 2^-23 next to 1, so tied keys are exactly equal values.  The `binade` family at
    the same shape does reach that path (the register-kernel rows of the table)."""
    rng = np.random.RandomState(31 * (256 + 40 + 64) + len("near32"))  # the parity test's batch
    C = (1.0 + rng.randint(0, 8, size=(256, 40, 64)) * 2.0 ** -23).astype(np.float32)
    total = sm.new_counts()
    for b in range(4):
        for maximize in (False, True):
            row, col, cnt = sm.solve(C[b].astype(np.float64), maximize)
            assert np.array_equal(col, scipy_lsa(C[b].astype(np.float64), maximize=maximize)[1])
            total = sm.add_counts(total, cnt)
    assert total["exact64"] == 0 and total["tie_unassigned"] + total["tie_assigned"] > 0
    binade = next(c for c in lc.LSA_CASES if (c.dtype, c.nr, c.nc) == (lc.F32, 40, 64))
    assert _model(binade)[0]["exact64"] > 0


@pytest.mark.parametrize("c", lc.STATUS_CASES, ids=lc.case_id)
@pytest.mark.parametrize("maximize", [False, True])
def test_status_batches_raise_scipys_errors(c, maximize):
    C, want = lc.status_batch(c, maximize)
    msg = {lc.INVALID: "matrix contains invalid numeric entries", lc.INFEASIBLE: "cost matrix is infeasible"}
    assert sorted(set(want.tolist())) == [lc.INFEASIBLE, lc.INVALID, 0]
    for b in range(len(want)):
        Cb = C[b].astype(np.float64)
        if want[b] == 0:
            r1, c1 = scipy_lsa(Cb, maximize=maximize)
            r2, c2 = ora.lsa(Cb, maximize=maximize)
            assert np.array_equal(c1, c2) and np.array_equal(r1, r2), b
        else:
            for solver in (scipy_lsa, ora.lsa):
                with pytest.raises(ValueError, match=msg[int(want[b])]):
                    solver(Cb, maximize=maximize)
    # the single infinite entry sits on the good answer's own entry and changes it
    good = lc.oracle_answers(c, maximize, maximize)[1][6]
    assert np.isinf(C[6]).sum() == 1 and not np.array_equal(ora.lsa(C[6].astype(np.float64), maximize=maximize)[1], good)
