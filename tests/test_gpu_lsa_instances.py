"""Every LSA solver instance on inputs that reach its tie paths (the table and generators of
tests/lsa_instance_cases.py; tests/test_lsa_instance_cases_host.py proves on the CPU that the table
covers every instance the three dispatchers can launch and that each case drives scipy's scan
through the selection paths it is there for).

Every comparison is exact array equality with the scipy-exact oracle: asg_lsa_batched over the
table (both senses, transposed shapes with row_out, NULL outputs through the raw ABI, a strided
transposed view read in place), the status paths above 64 rows and CPL 1, asg_haa_select over its
instances (against the oracle and against asg_beta_hat + asg_lsa_batched), and the mock env's
bids_assign_kernel above 64 tasks up to the documented maximum of 128 x 128.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU, but never run there
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from marl_sap_amd import _lib  # noqa: E402
from marl_sap_amd.action_selectors.lsa import linear_sum_assignment_batched  # noqa: E402
from marl_sap_amd.action_selectors.non_rl_selectors import haa_select_batched  # noqa: E402
from marl_sap_amd.components import EpisodeBatch  # noqa: E402
from marl_sap_amd.envs import AssignEnvBatch  # noqa: E402
from oracle import oracle as ora  # noqa: E402
from tests import lsa_instance_cases as lc  # noqa: E402

DEV = torch.device("cuda", 0)


def _dev(a):
    return torch.as_tensor(np.array(a), device=DEV)  # a copy: the cases' arrays are read-only


def _copy(a):
    return None if a is None else np.array(a)


def _raw_lsa(C, maximize, want_row=True, want_status=True):
    """asg_lsa_batched through the raw ABI; outputs prefilled with -7 so unwritten entries show."""
    B, nr, nc = C.shape
    k = min(nr, nc)
    row = torch.full((B, k), -7, dtype=torch.int64, device=DEV)
    col = torch.full((B, k), -7, dtype=torch.int64, device=DEV)
    status = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().asg_lsa_batched(
        ctypes.c_void_p(C.data_ptr()), _lib.dtype_code(C.dtype), _lib.i64arr(C.stride()), B, nr, nc, int(maximize),
        ctypes.c_void_p(row.data_ptr()) if want_row else None, ctypes.c_void_p(col.data_ptr()),
        ctypes.c_void_p(status.data_ptr()) if want_status else None, _lib.stream_ptr(DEV)))
    torch.cuda.synchronize()
    return row.cpu().numpy(), col.cpu().numpy(), status.cpu().numpy()


# ------------------------------------------------------------------------------ asg_lsa_batched
@pytest.mark.parametrize("c", lc.LSA_CASES, ids=lc.case_id)
def test_lsa_batched_every_instance_vs_oracle(c):
    C = _dev(lc.matrix(c))
    # the designed sense, the same working matrix through the maximize sign flip, and the other sense
    for negate, maximize in ((False, False), (True, True), (False, True)):
        want_row, want_col = lc.oracle_answers(c, negate, maximize)
        row, col, status = _raw_lsa(-C if negate else C, maximize)
        assert (status == 0).all()
        np.testing.assert_array_equal(col, want_col, err_msg=f"col negate={negate} maximize={maximize}")
        np.testing.assert_array_equal(row, want_row, err_msg=f"row negate={negate} maximize={maximize}")
    # row_out = NULL and status_out = NULL: the other outputs are the same, the absent ones untouched
    want_row, want_col = lc.oracle_answers(c)
    row, col, status = _raw_lsa(C, False, want_row=False)
    np.testing.assert_array_equal(col, want_col)
    assert (row == -7).all() and (status == 0).all()
    row, col, status = _raw_lsa(C, False, want_status=False)
    np.testing.assert_array_equal(col, want_col)
    np.testing.assert_array_equal(row, want_row)
    assert (status == -7).all()


@pytest.mark.parametrize("c", [c for c in lc.LSA_CASES if (c.nr, c.nc) in ((50, 300), (20, 400), (200, 70))
                               and lc.instance_of(c)[1] == lc.GLOBAL], ids=lc.case_id)
def test_lsa_global_path_reads_a_strided_transposed_view_in_place(c):
    """GlobalCost with its transpose flag and both strides: the case's matrices sit transposed
    inside a larger buffer, so the view handed over has the case's shape, a row stride of 1 and a
    padded column stride.  Storage is decided by the shape alone: still the global instance."""
    M = lc.matrix(c)
    big = torch.zeros((c.B, c.nc + 3, c.nr + 5), dtype=_dev(M[:1]).dtype, device=DEV)
    big[:, 2:2 + c.nc, 4:4 + c.nr] = _dev(M).transpose(1, 2)
    view = big[:, 2:2 + c.nc, 4:4 + c.nr].transpose(1, 2)
    assert tuple(view.shape) == M.shape and not view.is_contiguous() and view.stride(1) == 1
    for maximize in (False, True):
        want_row, want_col = lc.oracle_answers(c, False, maximize)
        row, col = linear_sum_assignment_batched(view, maximize=maximize)
        np.testing.assert_array_equal(col.cpu().numpy(), want_col)
        np.testing.assert_array_equal(row.cpu().numpy(), want_row)
    row, col, status = _raw_lsa(view, False)
    np.testing.assert_array_equal(col, lc.oracle_answers(c)[1])
    np.testing.assert_array_equal(row, lc.oracle_answers(c)[0])


@pytest.mark.parametrize("c", lc.STATUS_CASES, ids=lc.case_id)
@pytest.mark.parametrize("maximize", [False, True])
def test_lsa_status_above_64_rows(c, maximize):
    """scipy's errors per problem at CPL >= 2 with more than 64 outputs per problem: failed problems
    are -1 in every output, their neighbours are the good answers, and a single infinite entry
    that stays feasible is solved like scipy solves it."""
    Ch, want = lc.status_batch(c, maximize)
    assert min(c.nr, c.nc) > 64 and lc.instance_of(c)[0] >= 2
    row, col, status = _raw_lsa(_dev(Ch), maximize)
    np.testing.assert_array_equal(status, want)
    good_row, good_col = lc.oracle_answers(c, maximize, maximize)
    for b in range(len(want)):
        if want[b] != 0:
            assert (row[b] == -1).all() and (col[b] == -1).all(), b
        elif b == 6:
            r0, c0 = ora.lsa(Ch[b].astype(np.float64), maximize=maximize)
            np.testing.assert_array_equal(col[b], c0)
            np.testing.assert_array_equal(row[b], r0)
        else:
            np.testing.assert_array_equal(col[b], good_col[b], err_msg=str(b))
            np.testing.assert_array_equal(row[b], good_row[b], err_msg=str(b))
    with pytest.raises(ValueError, match="invalid numeric entries"):
        linear_sum_assignment_batched(_dev(Ch[:4]), maximize=maximize)
    with pytest.raises(ValueError, match="infeasible"):
        linear_sum_assignment_batched(_dev(Ch[4:5]), maximize=maximize)


# ------------------------------------------------------------------------------ asg_haa_select
@pytest.mark.parametrize("c", lc.HAA_CASES, ids=lc.case_id)
def test_haa_select_every_instance_vs_oracle(c):
    x = lc.haa_inputs(c)
    opts = dict(c.opts)
    B, n, m = x.beta.shape
    if opts.get("strided"):  # beta a non-contiguous view of a padded buffer, prev every second column
        big = torch.zeros((B, n + 2, 2 * m + 1), dtype=torch.float32, device=DEV)
        beta = big[:, 1:1 + n, 1:1 + 2 * m:2]
        beta.copy_(_dev(x.beta))
        pbig = torch.zeros((B, 2 * n), dtype=torch.int64, device=DEV)
        prev = pbig[:, ::2]
        prev.copy_(_dev(x.prev))
        assert not beta.is_contiguous() and not prev.is_contiguous()
    else:
        beta, prev = _dev(x.beta), _dev(x.prev)
    out, status = haa_select_batched(beta, prev, x.lam, _copy(x.T_trans), return_status=True)
    assert (status == 0).all()
    _, want = lc.oracle_answers(c)
    np.testing.assert_array_equal(out.cpu().numpy(), want.astype(np.float32))
    # the same through asg_beta_hat + asg_lsa_batched: beta_hat bit for bit the oracle's, same answer
    env = AssignEnvBatch(n, m, 2, 1, x.lam, T_trans=_copy(x.T_trans), num_envs=1, device=DEV)
    bh = env.beta_hat(beta, prev)
    np.testing.assert_array_equal(bh.cpu().numpy(), lc.haa_beta_hat(c))
    _, col = linear_sum_assignment_batched(bh, maximize=True)
    np.testing.assert_array_equal(col.cpu().numpy(), want)
    env.close()


@pytest.mark.parametrize("c", [c for c in lc.HAA_CASES if c.role == "main" and max(c.nr, c.nc) > 64], ids=lc.case_id)
def test_haa_infinite_beta_is_invalid_on_the_wave_instances(c):
    x = lc.haa_inputs(c)
    beta = _dev(x.beta).clone()
    beta[1, c.nr - 1, c.nc - 1] = float("inf")
    out, status = haa_select_batched(beta, _dev(x.prev), x.lam, _copy(x.T_trans), return_status=True)
    want_status = np.zeros(c.B, dtype=np.int32)
    want_status[1] = lc.INVALID
    np.testing.assert_array_equal(status.cpu().numpy(), want_status)
    want = lc.oracle_answers(c)[1].astype(np.float32).copy()
    want[1] = -1.0
    np.testing.assert_array_equal(out.cpu().numpy(), want)


# ------------------------------------------------------------------------------ mock env, bids
@pytest.mark.parametrize("c", lc.BIDS_CASES, ids=lc.case_id)
def test_bids_step_solves_the_row_on_every_instance(c):
    """bids_assign_kernel<CPL>: a bids row written directly (no asg_bids_select tag) is solved by
    the step itself; the next row's prev_assigns are LSA(bids, maximize)[1].  128 x 128 is the
    documented maximum of a bids_as_actions env."""
    n, m, E, T = c.nr, c.nc, c.B, 2
    env = AssignEnvBatch(n, m, T, 1, 0.5, bids_as_actions=True, seed=5, num_envs=E, device=DEV)
    batch = EpisodeBatch(env.scheme, {"agents": n}, E, T + 1, preprocess=env.preprocess, device=DEV,
                         time_major=True)
    env.reset(batch, 0)
    bids = _dev(lc.matrix(c))
    batch["actions"][:, 0].copy_(bids)
    env.step(batch, 0)
    env.sync()
    assert torch.equal(batch["actions"][:, 0], bids)
    np.testing.assert_array_equal(batch["prev_assigns"][:, 1].cpu().numpy(), lc.oracle_answers(c)[1])
    env.close()
