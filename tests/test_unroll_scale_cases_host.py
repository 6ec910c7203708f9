"""The preconditions of tests/test_gpu_unroll_scales.py, on the CPU: the references of
tests/unroll_scale_cases.py are the modules (forward) and their autograd (backward) in float64, the
generated cases hold what the GPU tests rely on, and the tolerances leave a correct kernel room --
a float32 numpy model of the kernels' accumulation (exact products summed four at a time, one
rounding per MFMA, the bias added after the products, one accumulator per gate in the backward
pass) stays within err / tol <= 0.6 of every one of them."""
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from marl_sap_amd.modules.agents import RNNAgent  # noqa: E402
from marl_sap_amd.modules.unroll import gru_param_grads, mlp_param_grads  # noqa: E402
from tests import unroll_scale_cases as C  # noqa: E402
from tests.cont_ppo_ref import RefCritic  # noqa: E402

H = C.HID
F32, F64 = np.float32, np.float64


def _close(got, want, rel=1e-12):
    assert got.shape == want.shape
    scale = max(want.abs().max().item(), 1e-300)
    assert (got - want).abs().max().item() <= rel * scale, ((got - want).abs().max().item(), scale)


def _module(c, dtype=torch.float64):
    if c.kind == "ids":
        net = RefCritic(obs=c.K, n=c.n, n_out=c.m)
    else:
        net = RNNAgent(c.K, SimpleNamespace(hidden_dim=H, use_rnn=c.kind == "gru", m=c.m))
    net = net.to(dtype)
    net.load_state_dict({k: v.to(dtype) for k, v in c.sd.items()})
    return net


def _module_forward(c, net, h0=None):
    """(q [T1, R, m], h_last) of the module: the agent looped over t, the critic on the batch"""
    x = c.x.double()
    if c.kind == "ids":
        return net(x).permute(1, 0, 2, 3).reshape(c.T1, c.R, c.m), None
    h = C.h0_rows(c).double() if h0 is None else h0
    qs = []
    for t in range(c.T1):
        q, h = net(x[:, t].reshape(c.R, c.K), h)
        qs.append(q)
    return torch.stack(qs), h


FWD = [("gru", C.SHAPES[0], "trained"), ("gru", C.SHAPES[1], "outlier"), ("mlp", C.SHAPES[0], "small"),
       ("mlp", C.SHAPES[1], "trained"), ("ids", C.SHAPES[0], "trained")] + C.H0_VARIANTS


@pytest.mark.parametrize("args", FWD, ids=str)
def test_references_are_the_modules_in_float64(args):
    c = C.case(*args)
    q, h_last = _module_forward(c, _module(c))
    if c.kind == "gru":
        p, _ = C.gru_chain(c, torch.float64)
        _close(p["h"][-1], h_last.detach())
    else:
        p = C.forward_reference(c, torch.float64)
    _close(p["q"], q.detach())


# the order of the shipped functions' results: the modules' parameter order
PARAMS = {"gru": ("fc1.weight", "fc1.bias", "rnn.weight_ih", "rnn.weight_hh", "rnn.bias_ih", "rnn.bias_hh",
                  "fc2.weight", "fc2.bias"),
          "mlp": ("fc1.weight", "fc1.bias", "rnn.weight", "rnn.bias", "fc2.weight", "fc2.bias"),
          "ids": ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias")}


@pytest.mark.parametrize("args", FWD, ids=str)
def test_backward_references_are_float64_autograd(args):
    """gru_bptt / mlp_bwd assembled into parameter gradients by the functions the autograd wrappers
    call (modules/unroll.py: gru_param_grads, mlp_param_grads), against autograd of the module."""
    c = C.case(*args)
    g = torch.Generator().manual_seed(11)
    wq = torch.randn((c.T1, c.R, c.m), generator=g, dtype=torch.float64)
    wh = torch.randn((c.R, H), generator=g, dtype=torch.float64)
    net = _module(c)
    h0 = C.h0_rows(c).double().clone().requires_grad_(True) if c.kind == "gru" else None
    q, h_last = _module_forward(c, net, h0)
    loss = (q * wq).sum() + ((h_last * wh).sum() if c.kind != "ids" else 0.0)
    loss.backward()
    want = {k: v.grad for k, v in net.named_parameters()}
    N = c.T1 * c.R
    nm = C.names(c.kind)
    W2 = c.sd[nm[3 if c.kind == "gru" else 2]].double()
    dQ = wq.reshape(N, c.m)
    dh_q = (dQ @ W2).view(c.T1, c.R, H)
    x = c.x.double()
    if c.kind == "gru":
        p, h_prev = C.gru_chain(c, torch.float64)
        b = C.gru_bptt(p, h_prev, dh_q, wh, c.sd["rnn.weight_ih"], c.sd["rnn.weight_hh"], torch.float64)
        got = gru_param_grads(x, h_prev[0], p["x1"], p["h"], b["dgi"].reshape(N, 3 * H), b["dgh_n"].reshape(N, H),
                              b["dx1"].reshape(N, H), dQ)
        _close(b["dh0"], h0.grad, 1e-11)
    else:
        p = C.forward_reference(c, torch.float64)
        dh_q = dh_q.clone()
        if c.kind == "mlp":
            dh_q[-1] += wh
        b = C.mlp_bwd(dh_q, p["h"], p["x1"], c.sd[nm[1]], torch.float64)
        got = mlp_param_grads(x, p["x1"], p["h"], b["dh"].reshape(N, H), b["dx1"].reshape(N, H), dQ, c.kind == "ids")
    assert len(got) == len(PARAMS[c.kind])
    got = dict(zip(PARAMS[c.kind], got))
    assert set(got) == set(want)
    for k in want:
        _close(got[k], want[k], 1e-11)


def test_case_layout_and_groups():
    assert len(C.CASES) == 19 and len(set(C.CASES)) == 19
    cls, dcls = C.row_classes(C.R), C.d_classes(C.R)
    assert (dcls[:64] == 0).all()
    for xc in range(5):
        for dc in range(4):  # from row 64 on every x class meets every gradient scale
            assert ((cls[64:] == xc) & (dcls[64:] == dc)).sum() >= 1, (xc, dc)
    for args in C.CASES + C.H0_VARIANTS:
        c = C.case(*args)
        T1, B, n, K, m = c.shape
        assert c.x.shape == (B, T1, n, K) and c.dh_q.shape == (T1, c.R, H) and c.x.stride(-1) == 1
        assert c.x.is_contiguous() != c.time_major
        want = set(C.CLASSES) if c.regime != "outlier" else {a + p for a in C.CLASSES for p in ("/even", "/odd")}
        assert set(c.groups) == want
        for gi in range(len(c.groups)):
            assert (c.group == gi).any()
        xr = C.x_rows(c)
        for ci, mul in enumerate(C.MULT):  # a row keeps its class at every t
            rows = torch.as_tensor(cls == ci)
            top = xr[:, rows].abs().amax(-1)
            assert bool((top <= 6 * mul).all()) and (mul == 0 or bool((top > 0.5 * mul).all()))
        zero_d = torch.as_tensor(dcls == 3)
        assert not bool(c.dh_q[:, zero_d].any()) and bool((c.dh_q[:, ~zero_d].abs().amax(-1) > 0).all())
        if c.x_col is not None:
            assert not bool(xr[:, ::2, c.x_col].any()) and bool(xr[:, 1::2, c.x_col].any())
        if c.kind == "gru":
            assert not bool(c.dh_last[zero_d].any())
            if c.h0_mode == "dense":
                assert c.h0.shape == (c.R, H) and not bool(c.h0[:32].any()) and not bool(c.h0[::3].any())
            elif c.h0_mode == "broadcast":
                assert c.h0.shape == (1, H) and bool(c.h0.any())
            else:
                assert c.h0 is None
    sd, x_col, _ = C.make_ids_state(70, 55, 16, "outlier")
    sd0, _, _ = C.make_ids_state(70, 55, 16, "default")
    assert sd["fc1.weight"].shape == (64, 125) and x_col < 70  # the entry lies in the obs block
    assert int((sd["fc1.weight"] != sd0["fc1.weight"]).sum()) == 1
    tr, _, _ = C.make_ids_state(70, 55, 16, "trained")
    for layer, g in (("fc1", 8.0), ("fc2", 4.0), ("fc3", 16.0)):
        assert torch.equal(tr[layer + ".weight"], sd0[layer + ".weight"] * g)
        assert torch.equal(tr[layer + ".bias"], sd0[layer + ".bias"] * g)


def test_cases_hold_saturated_gates_and_an_identically_zero_backward_group():
    saturated = 0
    for args in [a for a in C.CASES if a[0] == "gru"]:
        p, _ = C.gru_chain(C.case(*args), torch.float32)
        saturated += int(((p["r"] == 0) | (p["r"] == 1) | (p["z"] == 0) | (p["z"] == 1)).sum())
    assert saturated > 0
    c = C.case("gru", C.SHAPES[1], "trained")
    p, h_prev = C.gru_chain(c, torch.float32)
    got = C.backward_reference(c, torch.float32, p, h_prev)
    rows, bad = C.backward_report(c, got, p, h_prev)
    zero = {(k, g) for k, g, _, _, tol in rows if tol == 0.0}
    # every group holds rows with D > 0 (test_case_layout_and_groups), so these are not D = 0 groups
    # (n = +-1 exactly on the x3e4 rows: dn_pre and with it dgh_n vanish; z is not saturated everywhere)
    assert ("dgh_n", "x3e4") in zero, zero
    assert not bad


@pytest.mark.parametrize("args", C.CASES, ids=str)
def test_small_rows_live_at_the_bias(args):
    """x1e-4 rows: |W1 x| < 1e-2 |b1| on average -- the regime the bias-order bug lives in."""
    c = C.case(*args)
    rows = torch.as_tensor(c.cls == C.CLASSES.index("x1e-4"))
    W1 = c.sd["fc1.weight"].double()[:, :c.K]
    wx = (C.x_rows(c)[:, rows].double() @ W1.t()).abs().mean().item()
    assert wx < 1e-2 * c.sd["fc1.bias"].double().abs().mean().item()


# ---- a float32 model of the kernels' accumulation -------------------------------------------------
def _mm(pairs, start=None):
    """sum over the (W [J, K], X [N, K]) pairs of X W^T as the kernels' MFMAs accumulate it: k-chunks
    of 16, in each chunk four steps e, a step adds the four exact products k = 16 kc + 4 q + e
    (q = 0..3) of each pair in turn and rounds once to float32."""
    N, J = pairs[0][1].shape[0], pairs[0][0].shape[0]
    K = pairs[0][0].shape[1]
    Kp = -(-K // 16) * 16
    pad = [(np.pad(W.astype(F64), ((0, 0), (0, Kp - K))), np.pad(X.astype(F64), ((0, 0), (0, Kp - K)))) for W, X in pairs]
    acc = np.zeros((N, J), F32) if start is None else np.broadcast_to(start.astype(F32), (N, J)).copy()
    for kc in range(Kp // 16):
        for e in range(4):
            ks = 16 * kc + 4 * np.arange(4) + e
            for W, X in pad:
                acc = (acc.astype(F64) + X[:, ks] @ W[:, ks].T).astype(F32)
    return acc


def _np(sd, kind):
    return [sd[k].numpy().astype(F32) for k in C.names(kind)]


def _sig(a):
    with np.errstate(over="ignore"):  # exp(-a) = inf for a saturated gate: 1 / inf = 0, as on the GPU
        return (F32(1) / (F32(1) + np.exp(-a, dtype=F32))).astype(F32)


def _model_gru(c):
    W1, Wih, Whh, W2, b1, bih, bhh, b2 = _np(c.sd, "gru")
    xr = C.x_rows(c).numpy()
    h = C.h0_rows(c).numpy().astype(F32)
    out = {k: [] for k in C.FWD_PLANES["gru"]}
    for t in range(c.T1):
        x1 = np.maximum(_mm([(W1, xr[t])]) + b1, F32(0))
        gr = _mm([(Wih[:H], x1), (Whh[:H], h)], bih[:H] + bhh[:H])
        gz = _mm([(Wih[H:2 * H], x1), (Whh[H:2 * H], h)], bih[H:2 * H] + bhh[H:2 * H])
        gni = _mm([(Wih[2 * H:], x1)], bih[2 * H:])
        gnh = _mm([(Whh[2 * H:], h)]) + bhh[2 * H:]
        r, z = _sig(gr), _sig(gz)
        n = np.tanh(gni + r * gnh, dtype=F32)
        h = n + z * (h - n)
        for k, v in (("x1", x1), ("r", r), ("z", z), ("n", n), ("gh_n", gnh), ("h", h), ("q", _mm([(W2, h)]) + b2)):
            assert v.dtype == F32
            out[k].append(v)
    return {k: torch.from_numpy(np.stack(v)) for k, v in out.items()}


def _model_gru_bwd(c, p, h_prev):
    Wih, Whh = c.sd["rnn.weight_ih"].numpy(), c.sd["rnn.weight_hh"].numpy()
    x1, r, z, n, gh = (p[k].numpy() for k in ("x1", "r", "z", "n", "gh_n"))
    hp, dhq = h_prev.numpy(), c.dh_q.numpy()
    dh = c.dh_last.numpy().copy()
    one = F32(1)
    out = {"dgi": [None] * c.T1, "dgh_n": [None] * c.T1, "dx1": [None] * c.T1}
    for t in range(c.T1 - 1, -1, -1):
        d = dh + dhq[t]
        dn, dz = d * (one - z[t]), d * (hp[t] - n[t])
        dnp = dn * (one - n[t] * n[t])
        drp = dnp * gh[t] * r[t] * (one - r[t])
        dzp = dz * z[t] * (one - z[t])
        dgn = dnp * r[t]
        ag = [_mm([(Wih[g * H:(g + 1) * H].T, v)]) for g, v in enumerate((drp, dzp, dnp))]
        out["dx1"][t] = np.where(x1[t] > 0, (ag[0] + ag[1]) + ag[2], F32(0))
        ah = [_mm([(Whh[g * H:(g + 1) * H].T, v)]) for g, v in enumerate((drp, dzp, dgn))]
        dh = d * z[t] + ((ah[0] + ah[1]) + ah[2])
        out["dgi"][t], out["dgh_n"][t] = np.concatenate([drp, dzp, dnp], axis=1), dgn
        assert dh.dtype == F32 and out["dx1"][t].dtype == F32
    got = {k: torch.from_numpy(np.stack(v)) for k, v in out.items()}
    got["dh0"] = torch.from_numpy(dh).unsqueeze(0)
    return got


def _model_mlp(c):
    W1, Wr, W2, b1, br, b2 = _np(c.sd, c.kind)
    x = C.x_rows(c).numpy().reshape(c.T1 * c.R, c.K)
    b = b1[None, :]
    if c.kind == "ids":  # products first, then W1[:, K + agent] + b1
        agent = np.tile(np.arange(c.R) % c.n, c.T1)
        b = W1[:, c.K + agent].T + b1[None, :]
        W1 = W1[:, :c.K]
    x1 = np.maximum(_mm([(W1, x)]) + b, F32(0))
    h = np.maximum(_mm([(Wr, x1)]) + br, F32(0))
    q = _mm([(W2, h)]) + b2
    return {k: torch.from_numpy(v.reshape(c.T1, c.R, -1)) for k, v in (("x1", x1), ("h", h), ("q", q))}


def _model_mlp_bwd(c, p):
    Wr = c.sd[C.names(c.kind)[1]].numpy()
    h, x1, dhq = (t.numpy().reshape(c.T1 * c.R, H) for t in (p["h"], p["x1"], c.dh_q))
    dh = np.where(h > 0, dhq, F32(0))
    dx1 = np.where(x1 > 0, _mm([(Wr.T, dh)]), F32(0))
    return {"dh": torch.from_numpy(dh).view(c.T1, c.R, H), "dx1": torch.from_numpy(dx1).view(c.T1, c.R, H)}


@pytest.mark.parametrize("args", [a for a in C.CASES if a[1] == C.SHAPES[0]], ids=str)
def test_a_correct_kernel_has_room(args):
    """Attainability: the model of the kernels' arithmetic, checked exactly as the GPU tests check
    the kernels (teacher-forced forward, pure-function backward), is within err / tol <= 0.6."""
    c = C.case(*args)
    if c.kind == "gru":
        got = _model_gru(c)
        h_prev = C.h_prev_of(c, got["h"])
        bwd = _model_gru_bwd(c, got, h_prev)
    else:
        got, h_prev = _model_mlp(c), None
        bwd = _model_mlp_bwd(c, got)
        assert torch.equal(bwd["dh"], torch.where(got["h"] > 0, c.dh_q, torch.zeros(())))
    rows, bad = C.forward_report(c, got, h_prev)
    rows_b, bad_b = C.backward_report(c, bwd, got, h_prev)
    worst = max(rows + rows_b, key=lambda r: r[2] / r[4] if r[4] > 0 else 0.0)
    print(f"model {args}: worst err / tol forward {C.worst_ratio(rows):.3f} backward {C.worst_ratio(rows_b):.3f} "
          f"at {worst[:2]}")
    assert not bad and not bad_b, (bad, bad_b)
    assert C.worst_ratio(rows) <= 0.6 and C.worst_ratio(rows_b) <= 0.6, worst
