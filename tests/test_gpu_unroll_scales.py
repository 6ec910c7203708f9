"""The learner's unroll kernels (asg_rnn_agent_unroll / _backward, asg_mlp_agent_unroll / _ids /
_backward) outside default-init scales, per row class, against float64: the cases, references and
tolerances of tests/unroll_scale_cases.py (their preconditions, and a CPU model showing that a
correct kernel has room: tests/test_unroll_scale_cases_host.py).

The ABI entries are called directly, as modules/unroll.py calls them, on output buffers the
test owns: each has 64 extra rows and is pre-filled with a NaN payload no result can equal; after
the launch the tail must be untouched and no live element may still hold the pattern.

Forward planes (gru: the five saved planes, h_all and q; mlp / ids: x1, h, q) are checked per group,
teacher-forced; the kernel-owned backward outputs (dgi, dgh_n, dx1, dh0; dh, dx1) per group from the
forward kernel's own planes, every row divided by its gradient scale; groups whose float64 reference
is identically zero (masked rows, saturated gates) must be exactly zero, and the Linear agent's dh
is where(h > 0, dh_q, 0) bit for bit.  Rows are independent bit for bit under a permutation of envs
and of agents within envs, and the public paths (RNNFusedAgent.unroll, ACCritic.rows under autograd)
give the bits of the direct calls, parameter gradients included.

Found by these tests and fixed with them: fc1, the Linear agent's middle layer, fc2 and the GRU's
gh_n started their accumulators from the bias, so every MFMA rounded at the bias's magnitude (the
figures: DESIGN.md).  The bias is now added after the products.
"""
import ctypes
import functools
from types import SimpleNamespace

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from marl_sap_amd import _lib  # noqa: E402
from marl_sap_amd.modules.agents import RNNFusedAgent  # noqa: E402
from marl_sap_amd.modules.critics.ac import ACCritic  # noqa: E402
from tests import unroll_scale_cases as C  # noqa: E402

DEV = torch.device("cuda", 0)
H = C.HID
PATTERN = 0x7FC5A5A5  # a quiet NaN with a payload: no result has these bits
TAIL = 64
ALL = C.CASES + C.H0_VARIANTS
TRAINED = [("gru", C.SHAPES[0], "trained"), ("mlp", C.SHAPES[0], "trained"), ("ids", C.SHAPES[0], "trained")]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _buf(rows, width):
    t = torch.empty((rows + TAIL, width), dtype=torch.float32, device=DEV)
    t.view(torch.int32).fill_(PATTERN)
    return t


def _live(name, t, rows):
    """the canaries of one output buffer; returns its live rows"""
    bits = t.view(torch.int32)
    assert bool((bits[rows:] == PATTERN).all()), name + ": written past its last row"
    assert not bool((bits[:rows] == PATTERN).any()), name + ": live elements left unwritten"
    return t[:rows]


def _strides(x):
    return _lib.i64arr([x.stride(1), x.stride(0), x.stride(2)])


def _weights(c):
    return [c.sd[k].to(DEV).contiguous() for k in C.names(c.kind)]


def gru_forward(c, x, h0, hs, ws, save=True):
    """asg_rnn_agent_unroll on owned buffers: q [T1, R, m], h_all [T1, R, 64], save [5, T1, R, 64]"""
    T1, B, n, K, m = c.shape
    N = T1 * c.R
    q, h_all, sv = _buf(N, m), _buf(N, H), (_buf(5 * N, H) if save else None)
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib().asg_rnn_agent_unroll(
            _p(x), _strides(x), T1, B, n, K, _p(h0), hs, *[_p(w) for w in ws], H, m, 1, _p(q), _p(h_all), _p(sv),
            _lib.stream_ptr(DEV)))
    torch.cuda.synchronize()
    q, h_all = _live("q", q, N).view(T1, c.R, m), _live("h_all", h_all, N).view(T1, c.R, H)
    return q, h_all, (_live("save", sv, 5 * N).view(5, T1, c.R, H) if save else None)


def gru_backward(c, dh_q, dh_last, sv, h_all, h0, hs, ws, want_dh0=True):
    """asg_rnn_agent_unroll_backward on owned buffers: dgi [T1, R, 192], dgh_n, dx1 [T1, R, 64], dh0"""
    T1, m = c.T1, c.m
    N = T1 * c.R
    dgi, dghn, dx1, dh0 = _buf(N, 3 * H), _buf(N, H), _buf(N, H), (_buf(c.R, H) if want_dh0 else None)
    assert dh_q.is_contiguous() and sv.is_contiguous() and h_all.is_contiguous()
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib().asg_rnn_agent_unroll_backward(
            _p(dh_q), _p(dh_last), _p(sv), _p(h_all), _p(h0), hs, _p(ws[1]), _p(ws[2]), T1, c.R, H, m, 1, _p(dgi),
            _p(dghn), _p(dx1), _p(dh0), _lib.stream_ptr(DEV)))
    torch.cuda.synchronize()
    return (_live("dgi", dgi, N).view(T1, c.R, 3 * H), _live("dgh_n", dghn, N).view(T1, c.R, H),
            _live("dx1", dx1, N).view(T1, c.R, H), _live("dh0", dh0, c.R) if want_dh0 else None)


def mlp_forward(c, x, ws, save=True):
    T1, B, n, K, m = c.shape
    N = T1 * c.R
    q, h_all, x1 = _buf(N, m), _buf(N, H), (_buf(N, H) if save else None)
    fn = _lib.lib().asg_mlp_agent_unroll_ids if c.kind == "ids" else _lib.lib().asg_mlp_agent_unroll
    with torch.cuda.device(DEV):
        _lib.check(fn(_p(x), _strides(x), T1, B, n, K, *[_p(w) for w in ws], H, m, _p(q), _p(h_all), _p(x1),
                      _lib.stream_ptr(DEV)))
    torch.cuda.synchronize()
    return (_live("q", q, N).view(T1, c.R, m), _live("h_all", h_all, N).view(T1, c.R, H),
            _live("x1", x1, N).view(T1, c.R, H) if save else None)


def mlp_backward(c, dh_q, h_all, x1, ws):
    N = c.T1 * c.R
    dh, dx1 = _buf(N, H), _buf(N, H)
    assert dh_q.is_contiguous() and h_all.is_contiguous() and x1.is_contiguous()
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib().asg_mlp_agent_unroll_backward(_p(dh_q), _p(h_all), _p(x1), _p(ws[1]), N, H, _p(dh),
                                                            _p(dx1), _lib.stream_ptr(DEV)))
    torch.cuda.synchronize()
    return _live("dh", dh, N).view(c.T1, c.R, H), _live("dx1", dx1, N).view(c.T1, c.R, H)


def _perm(c):
    """envs permuted, and (not for the critic, whose rows carry their agent id) agents within envs"""
    g = torch.Generator().manual_seed(2024)
    rows = []
    for b in torch.randperm(c.B, generator=g).tolist():
        ag = torch.arange(c.n) if c.kind == "ids" else torch.randperm(c.n, generator=g)
        rows.append(b * c.n + ag)
    return torch.cat(rows)


def _x_dev(c, perm):
    if perm is None:
        x = c.x.to(DEV)
        assert x.stride() == c.x.stride()  # the case's storage order
        return x
    T1, B, n, K, _ = c.shape
    return C.x_rows(c)[:, perm].contiguous().to(DEV).view(T1, B, n, K).transpose(0, 1)


@functools.lru_cache(maxsize=None)
def _run(args, permuted=False, dh_last=True):
    """Forward and backward of one case through the ABI: every output on the CPU as [T1, R, ..]
    (dh0: [1, R, 64]), rows in the case's order."""
    c = C.case(*args)
    perm = _perm(c) if permuted else None
    idx = torch.arange(c.R) if perm is None else perm
    inv = torch.empty_like(idx)
    inv[idx] = torch.arange(c.R)
    x, ws = _x_dev(c, perm), _weights(c)
    dh_q = c.dh_q[:, idx].contiguous().to(DEV)
    if c.kind == "gru":
        if c.h0 is None:
            h0, hs = None, 0
        elif c.h0.shape[0] == 1:
            h0, hs = c.h0.to(DEV), 0
        else:
            h0, hs = c.h0[idx].contiguous().to(DEV), H
        q, h_all, sv = gru_forward(c, x, h0, hs, ws)
        dl = c.dh_last[idx].contiguous().to(DEV) if dh_last else None
        dgi, dghn, dx1, dh0 = gru_backward(c, dh_q, dl, sv, h_all, h0, hs, ws)
        out = dict(x1=sv[0], r=sv[1], z=sv[2], n=sv[3], gh_n=sv[4], h=h_all, q=q, dgi=dgi, dgh_n=dghn, dx1=dx1,
                   dh0=dh0.unsqueeze(0))
    else:
        q, h_all, x1 = mlp_forward(c, x, ws)
        dh, dx1 = mlp_backward(c, dh_q, h_all, x1, ws)
        out = dict(x1=x1, h=h_all, q=q, dh=dh, dx1=dx1)
    return {k: v.cpu()[:, inv].contiguous() for k, v in out.items()}


def _tag(args):
    kind, shape, regime = args[:3]
    return f"{kind} {shape[3]}x{shape[4]} {regime}" + "".join(" h0=" + s for s in args[3:])


@pytest.mark.parametrize("args", ALL, ids=_tag)
def test_forward_planes_per_group(args):
    c = C.case(*args)
    out = _run(args)
    h_prev = C.h_prev_of(c, out["h"]) if c.kind == "gru" else None
    rows, bad = C.forward_report(c, out, h_prev)
    print(C.format_rows(_tag(args), rows))
    assert not bad, (_tag(args), bad)


@pytest.mark.parametrize("args", ALL, ids=_tag)
def test_backward_outputs_per_group(args):
    c = C.case(*args)
    out = _run(args)
    h_prev = C.h_prev_of(c, out["h"]) if c.kind == "gru" else None
    rows, bad = C.backward_report(c, out, out, h_prev)
    print(C.format_rows(_tag(args), rows))
    assert not bad, (_tag(args), bad)
    if c.kind != "gru":
        want = torch.where(out["h"] > 0, c.dh_q, torch.zeros(()))
        assert torch.equal(out["dh"].view(torch.int32), want.view(torch.int32))
    if args == ("gru", C.SHAPES[1], "trained"):  # saturated gates: a group of exact zeros with D > 0
        assert any(tol == 0.0 for _, _, _, _, tol in rows)


def test_backward_without_dh_last():
    args = ("gru", C.SHAPES[0], "trained")
    c = C.case(*args)
    out = _run(args, dh_last=False)
    h_prev = C.h_prev_of(c, out["h"])
    rows, bad = C.backward_report(c, out, out, h_prev, dh_last=None)
    print(C.format_rows(_tag(args) + " dh_last=NULL", rows))
    assert not bad, bad
    assert not torch.equal(out["dh0"], _run(args)["dh0"])


def test_forward_without_save_gives_the_same_bits():
    args = ("gru", C.SHAPES[1], "trained")
    c = C.case(*args)
    q, h_all, sv = gru_forward(c, _x_dev(c, None), c.h0.to(DEV), H, _weights(c), save=False)
    assert sv is None
    assert torch.equal(q.cpu(), _run(args)["q"]) and torch.equal(h_all.cpu(), _run(args)["h"])


@pytest.mark.parametrize("args", ALL, ids=_tag)
def test_rows_are_independent_bit_for_bit(args):
    """Envs, and agents within envs, permuted in x, h0 and the gradients: every forward and
    backward output row has the same bits at its new place, whatever rows share its tile."""
    out, outp = _run(args), _run(args, permuted=True)
    assert set(out) == set(outp)
    for k in out:
        assert torch.equal(out[k], outp[k]), (k, (out[k] - outp[k]).abs().max().item())


def _loss_weights(c):
    g = torch.Generator().manual_seed(77)
    return (torch.randn((c.B, c.T1, c.n, c.m), generator=g).to(DEV), torch.randn((c.R, H), generator=g).to(DEV))


@pytest.mark.parametrize("args", TRAINED, ids=_tag)
def test_public_path_gives_the_bits_of_the_direct_calls(args):
    """RNNFusedAgent.unroll / ACCritic.rows under autograd against the direct ABI calls on the
    same inputs: q, h_last and the parameter gradients assembled from the kernels' outputs the
    way the autograd functions assemble them."""
    c = C.case(*args)
    T1, B, n, K, m = c.shape
    N = T1 * c.R
    x = _x_dev(c, None)
    wq, wh = _loss_weights(c)
    dQ = wq.permute(1, 0, 2, 3).reshape(N, m).contiguous()
    xf = x.permute(1, 0, 2, 3).reshape(N, K)
    if c.kind == "ids":
        net = ACCritic({"obs": {"vshape": K}}, SimpleNamespace(m=m, n=n, hidden_dim=H, env_args={"bids_as_actions": True}))
        net = net.to(DEV)
        net.load_state_dict(c.sd)
        q = net.rows({"obs": x})
        (q * wq.permute(1, 0, 2, 3).reshape(T1, c.R, m)).sum().backward()
        h_last = None
    else:
        net = RNNFusedAgent(K, SimpleNamespace(hidden_dim=H, use_rnn=c.kind == "gru", m=m,
                                               fused_linear_unroll=True)).to(DEV)
        net.load_state_dict(c.sd)
        h0 = c.h0.to(DEV).requires_grad_(True) if c.kind == "gru" else None
        q, h_last = net.unroll(x, h0)
        ((q * wq).sum() + (h_last * wh).sum()).backward()
        q = q.permute(1, 0, 2, 3).reshape(T1, c.R, m)
    got = {k: v.grad for k, v in net.named_parameters()}
    ws = [net.state_dict()[k].detach().contiguous() for k in C.names(c.kind)]
    nm = C.names(c.kind)
    if c.kind == "gru":
        h0k = h0.detach()
        qd, h_all, sv = gru_forward(c, x, h0k, H, ws)
        dgi, dghn, dx1, dh0 = gru_backward(c, dQ @ ws[3], wh, sv, h_all, h0k, H, ws)
        dgi, dx1, hf = dgi.reshape(N, 3 * H), dx1.reshape(N, H), h_all.reshape(N, H)
        dgh = torch.cat([dgi[:, :2 * H], dghn.reshape(N, H)], dim=1)
        h_prev = torch.cat([h0k, hf[:N - c.R]], dim=0)
        want = dict(zip(nm, (dx1.t() @ xf, dgi.t() @ sv[0].reshape(N, H), dgh.t() @ h_prev, dQ.t() @ hf, dx1.sum(0),
                             dgi.sum(0), dgh.sum(0), dQ.sum(0))))
        assert torch.equal(h0.grad, dh0)
    else:
        qd, h_all, x1 = mlp_forward(c, x, ws)
        dh_q = dQ @ ws[2]
        if c.kind == "mlp":
            dh_q[N - c.R:] += wh
        dh, dx1 = mlp_backward(c, dh_q, h_all, x1, ws)
        dh, dx1 = dh.reshape(N, H), dx1.reshape(N, H)
        dW1 = dx1.t() @ xf
        if c.kind == "ids":
            dW1 = torch.cat([dW1, dx1.view(T1, B, n, H).sum((0, 1)).t()], dim=1)
        want = dict(zip(nm, (dW1, dh.t() @ x1.reshape(N, H), dQ.t() @ h_all.reshape(N, H), dx1.sum(0), dh.sum(0),
                             dQ.sum(0))))
    assert torch.equal(q.detach(), qd)
    if h_last is not None:
        assert torch.equal(h_last.detach(), h_all[T1 - 1])
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), (k, (got[k] - want[k]).abs().max().item())
    # and the direct calls of this test are the checked ones: same bits as the case's run
    assert torch.equal(qd.cpu(), _run(args)["q"])
