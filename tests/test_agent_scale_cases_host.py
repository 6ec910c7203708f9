"""The preconditions of tests/test_gpu_agent_scales.py, on the CPU: the generated batches
(tests/agent_scale_cases.py) really hold what the GPU tests rely on, so those cannot pass by the
inputs having gone soft -- every row class present, the x 40 and x 3e4 rows past fc1's first
scale (max |x| >= 16: the tile re-runs fc1) and the x 1 rows below it, the kernels chosen by
shape, finite references, and room between the float64 top-2 Q values for the greedy-choice test."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import agent_scale_cases as C  # noqa: E402

ALL = [(s, rnn, reg) for s in C.SHAPES for rnn in (True, False) for reg in C.REGIMES]


def test_row_classes_layout():
    cls = C.row_classes()
    assert len(cls) == 165 and (cls[:32] == 0).all() and (cls[32:64] == 1).all()
    assert [int(c) for c in cls[64:74]] == [4, 0, 1, 2, 3, 4, 0, 1, 2, 3]
    # every class in every mixed 32-row tile and in the ragged 5-row tile
    for lo in (64, 96, 128, 160):
        assert set(cls[lo:lo + 32].tolist()) == {0, 1, 2, 3, 4}


def test_modes_by_shape():
    """asg_rnn_agent_mode: the split-f16 kernel up to n_out = 256, beyond it the f32-MFMA kernel
    with the three-way bf16 GRU."""
    from marl_sap_amd import _lib
    L = _lib.lib()
    for (_, K, m), rnn in [(s, r) for s in C.SHAPES for r in (1, 0)]:
        want = 4 if m <= 256 else L.asg_rnn_agent_mfma_mode()
        assert L.asg_rnn_agent_mode(K, 64, m, rnn) == want, (K, m, rnn)
    assert L.asg_rnn_agent_mfma_mode() != 4
    assert [C.blocked(K, m) for _, K, m in C.SHAPES] == [True, False, True, False]


@pytest.mark.parametrize("shape,use_rnn,regime", ALL)
def test_case_preconditions(shape, use_rnn, regime):
    c = C.case(shape, use_rnn, regime)
    R, K, m = shape
    assert c.x.shape == (R, K) and c.h.shape == (R, 64) and c.x.dtype == c.h.dtype == torch.float32
    for t in (c.q64, c.h64, c.q32, c.h32):
        assert bool(torch.isfinite(t).all())
    assert c.q64.dtype == torch.float64 and c.q32.dtype == torch.float32
    want = set(C.CLASSES) if regime != "outlier" else {n + p for n in C.CLASSES for p in ("/even", "/odd")}
    assert set(c.tol_h) == set(c.tol_q) == set(c.groups) == want
    for gi, name in enumerate(c.groups):  # a group lies inside one row class
        assert {C.CLASSES[i] for i in c.cls[c.group == gi]} == {name.split("/")[0]}
    rowmax = c.x.abs().max(1).values.numpy()
    body = c.x[:, m:] if C.blocked(K, m) else c.x
    assert (rowmax[c.cls == 0] < 16).all() and (rowmax[c.cls == 3] < 16).all()
    assert (rowmax[c.cls == 1] >= 16).all() and (rowmax[c.cls == 2] >= 16).all()
    assert rowmax[c.cls == 2].max() > 65504  # past f16's range unscaled
    assert (body[torch.as_tensor(c.cls == 4)] == 0).all() and (body.abs().max(1).values[c.cls != 4] > 0).all()
    if C.blocked(K, m):  # every prefix onehot or zero: the gather is taken in every tile
        pre = c.x[:, :m]
        assert bool(((pre == 0) | (pre == 1)).all()) and int(pre.sum(1).max()) == 1 and int(pre.sum(1).min()) == 0
    # hidden state: the zero tile, zero rows inside non-zero tiles, tiny rows
    hmax = c.h.abs().max(1).values
    assert (hmax[:32] == 0).all() and (hmax[torch.arange(R) % 3 == 0] == 0).all()
    tiny = (torch.arange(R) % 7 == 1) & (torch.arange(R) % 3 != 0) & (torch.arange(R) >= 32)
    assert bool(tiny.any()) and (hmax[tiny] < 1e-6).all() and (hmax[tiny] > 0).all()
    assert float(hmax.max()) <= float(np.float32(0.999))
    for lo in range(32, R, 32):
        assert bool((hmax[lo:lo + 32] > 0).any()) and bool((hmax[lo:lo + 32] == 0).any())
    # room for the greedy-choice test: at most 5 % of a class's rows undecided in float64
    for v in ([{}] + ([dict(hidden="init"), dict(prefix="nonhot")] if shape == C.SHAPES[0] else [])):
        for name, share in C.undecided_share(C.case(shape, use_rnn, regime, **v)).items():
            assert share <= 0.05, (v, name, share)
    # the floors: none for the Linear agent, the gate floor for the GRU
    sel = torch.as_tensor(c.group == 0)
    base = 4 * c.e32_h[c.groups[0]] + 1e-7 * c.h64[sel].abs().max().item()
    assert c.tol_h[c.groups[0]] == pytest.approx(base + (C.GATE_FLOOR if use_rnn else 0.0), rel=1e-12)
    if regime == "outlier":  # the split groups ask no less than their class would
        for name in C.CLASSES:
            s2 = torch.as_tensor(c.cls == C.CLASSES.index(name))
            whole = (4 * (c.h32.double() - c.h64)[s2].abs().max().item() + 1e-7 * c.h64[s2].abs().max().item()
                     + (C.GATE_FLOOR if use_rnn else 0.0))
            assert max(c.tol_h[name + "/even"], c.tol_h[name + "/odd"]) <= whole * (1 + 1e-12)


def test_regime_gains():
    sd0, _, _ = C.make_state(256, 64, True, "default")
    tr, _, _ = C.make_state(256, 64, True, "trained")
    sm, _, _ = C.make_state(256, 64, True, "small")
    ol, x_col, h_unit = C.make_state(256, 64, True, "outlier")
    want = {"fc1": 8.0, "rnn.weight_ih": 4.0, "rnn.bias_ih": 4.0, "rnn.weight_hh": 0.25, "rnn.bias_hh": 0.25,
            "fc2": 16.0}
    for k in sd0:
        g = next(v for p, v in want.items() if k.startswith(p))
        assert torch.equal(tr[k], sd0[k] * g), k
        assert torch.equal(sm[k], sd0[k] / 64.0), k
    for k, bound in (("fc1.weight", 1 / 16), ("rnn.weight_ih", 1 / 8), ("rnn.weight_hh", 1 / 8), ("fc2.weight", 1 / 8)):
        diff = ol[k] != sd0[k]
        assert int(diff.sum()) == 1 and float(ol[k].abs().max()) == 4096 * bound, k
        assert float(sd0[k].abs().max()) <= bound
    assert x_col >= 64 and int((ol["fc1.weight"][:, x_col].abs() == 256).sum()) == 1
    assert int((ol["rnn.weight_hh"][:, h_unit].abs() == 512).sum()) == 1
    c = C.case((165, 256, 64), True, "outlier")
    assert (c.x[::2, x_col] == 0).all() and (c.x[1::2, x_col] != 0).sum() > 60
    assert (c.h[::2, h_unit] == 0).all() and (c.h[1::2, h_unit] != 0).sum() > 30
    lin, _, _ = C.make_state(70, 16, False, "trained")
    lin0, _, _ = C.make_state(70, 16, False, "default")
    assert torch.equal(lin["rnn.weight"], lin0["rnn.weight"] * 4) and torch.equal(lin["rnn.bias"], lin0["rnn.bias"] * 4)


def test_variants():
    base = C.case((165, 256, 64), True, "default")
    init = C.case((165, 256, 64), True, "default", hidden="init")
    assert torch.equal(init.x, base.x) and not bool(init.h.any())
    bad = C.case((165, 256, 64), True, "default", prefix="nonhot")
    rows = (bad.x[:, :64] != base.x[:, :64]).any(1).nonzero().flatten().tolist()
    assert rows == [5, 40, 101, 163] and torch.equal(bad.x[:, 64:], base.x[:, 64:])
    assert C.case((165, 256, 64), True, "default") is base  # cached, shared
    with pytest.raises(ValueError):
        C.case((165, 70, 16), True, "default", prefix="nonhot")


def test_gate_floor_covers_the_float32_gate_formula():
    """The kernels' gate formula (sigmoid = 1 / (1 + 2^(-a log2 e)), tanh = 2 sigmoid - 1) in
    float32, on pre-activations that are float32 numbers (so the error is the formula's own, not
    the conditioning of i_n + r h_n, which PyTorch's fp32 shares), is within GATE_FLOOR of the
    float64 GRU update -- and not within the project's relative rule at small scales, which is why
    the floor exists."""
    g = torch.Generator().manual_seed(5)
    worst = 0.0
    for scale in (1.0, 1 / 64.0, 2.0, 1e-3):
        a_r, a_z, i_n, h_n = (scale * torch.randn(20000, generator=g).double() for _ in range(4))
        h = (0.5 * torch.randn(20000, generator=g, dtype=torch.float64)).clamp(-0.999, 0.999).float().double()
        r, z = torch.sigmoid(a_r), torch.sigmoid(a_z)
        n = torch.tanh(i_n + r * h_n)
        want = n + z * (h - n)
        f = lambda t: t.float()  # noqa: E731
        sig = lambda a: 1.0 / (1.0 + torch.exp2(a * np.float32(-1.4426950408889634)))  # noqa: E731
        r32, z32 = sig(f(a_r)), sig(f(a_z))
        n32 = 2.0 * sig(2.0 * (f(i_n) + r32 * f(h_n))) - 1.0
        got = n32 + z32 * (f(h) - n32)
        assert got.dtype == torch.float32
        worst = max(worst, (got.double() - want).abs().max().item())
    assert worst <= C.GATE_FLOOR, worst
    assert worst > 2e-8  # absolute, not relative, accuracy: above 1e-7 max|ref| at small scales
