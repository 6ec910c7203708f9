"""An instrumented numpy restatement of scipy's linear_sum_assignment, for
the LSA instance cases (tests/lsa_instance_cases.py): besides the assignment it says which
selection path of the wave solvers (csrc/lsa_wave.h, csrc/lsa_reg64.h) every scan step takes.

The solvers pick a step's column from the float32-rounded path costs of the remaining columns
(the keys) and look at the float64 values only when several columns share the minimum key.  A
step is therefore of exactly one class:

  single          one column holds the minimum key
  tie_unassigned  several do, their float64 values are all equal, and at least one of them is
                  unassigned (scipy's scan ends on the LAST such position of `remaining`)
  tie_assigned    several do, all equal, all assigned (scipy keeps the FIRST position)
  exact64         several do and their float64 values differ: the exact float64 minimum decides
                  (exact64_tie counts those where several columns hold that exact minimum too)

and each class but the first has a cross-slot count (x_...): the columns sharing the minimum key
lie in more than one 64-column slot, i.e. in more than one register of a lane.

Everything is float64 with scipy's operation order, ((minv + c) - u) - v, one rounding each.
"""
import numpy as np

SLOT = 64
CLASSES = ("single", "tie_unassigned", "tie_assigned", "exact64")


def new_counts():
    c = {"steps": 0, "exact64_tie": 0, "rows": 0}
    for k in CLASSES:
        c[k] = 0
        if k != "single":
            c["x_" + k] = 0
    return c


def add_counts(a, b):
    return {k: a[k] + b[k] for k in a}


def scan(W, counts=None):
    """scipy's solve on the working matrix W [nr <= nc] float64 -> col4row; adds to `counts`."""
    W = np.asarray(W, dtype=np.float64)
    nr, nc = W.shape
    assert nr <= nc
    counts = new_counts() if counts is None else counts
    counts["rows"] += nr
    u, v = np.zeros(nr), np.zeros(nc)
    col4row = np.full(nr, -1, dtype=np.int64)
    row4col = np.full(nc, -1, dtype=np.int64)
    path = np.full(nc, -1, dtype=np.int64)
    for cur in range(nr):
        spc = np.full(nc, np.inf)
        rem = np.arange(nc - 1, -1, -1)  # remaining[it] = nc - it - 1
        nrem = nc
        SR = np.zeros(nr, dtype=bool)
        SC = np.zeros(nc, dtype=bool)
        minv, i, sink = 0.0, cur, -1
        while sink == -1:
            SR[i] = True
            js = rem[:nrem]
            r = ((minv + W[i, js]) - u[i]) - v[js]
            upd = r < spc[js]
            spc[js[upd]] = r[upd]
            path[js[upd]] = i
            s = spc[js]
            low = s.min()
            if low == np.inf:
                raise ValueError("cost matrix is infeasible")
            free = row4col[js] == -1
            # the solvers' view of the step
            with np.errstate(over="ignore"):
                key = s.astype(np.float32)
            cm = key == key.min()
            counts["steps"] += 1
            if cm.sum() == 1:
                cls = "single"
            elif (s[cm] == s[cm][0]).all():
                cls = "tie_unassigned" if free[cm].any() else "tie_assigned"
            else:
                cls = "exact64"
                counts["exact64_tie"] += int((s == low).sum() > 1)
            counts[cls] += 1
            if cls != "single" and np.unique(js[cm] // SLOT).size > 1:
                counts["x_" + cls] += 1
            # scipy's sequential scan: a later position replaces the choice when its cost is lower,
            # or equal and its column unassigned
            eq = s == low
            un = np.flatnonzero(eq & free)
            it = un[-1] if un.size else np.flatnonzero(eq)[0]
            minv = low
            j = js[it]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            SC[j] = True
            nrem -= 1
            rem[it] = rem[nrem]
        u[cur] += minv
        for r_ in np.flatnonzero(SR):
            if r_ != cur:
                u[r_] += minv - spc[col4row[r_]]
        v[SC] -= minv - spc[SC]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    return col4row


def solve(C, maximize=False):
    """linear_sum_assignment(C, maximize) -> (row_ind, col_ind, counts), scipy's errors included."""
    C = np.asarray(C, dtype=np.float64)
    W = C.T if C.shape[0] > C.shape[1] else C
    W = -W if maximize else W
    if np.isnan(W).any() or (W == -np.inf).any():
        raise ValueError("matrix contains invalid numeric entries")
    counts = new_counts()
    col4row = scan(np.ascontiguousarray(W), counts)
    if C.shape[0] > C.shape[1]:
        order = np.argsort(col4row)
        return col4row[order], order, counts
    return np.arange(C.shape[0]), col4row, counts
