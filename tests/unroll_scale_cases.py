"""Inputs, references and tolerances for the learner's unroll kernels outside default-init scales
(tests/test_gpu_unroll_scales.py; their preconditions and a CPU model of the kernels' accumulation:
tests/test_unroll_scale_cases_host.py).  Built on tests/agent_scale_cases.py: the same weight
regimes (make_state), the same five row classes mixed inside one wave tile (row_classes, MULT), the
same tolerance groups (the row classes, split even / odd in the outlier regime).  Everything here
runs on the CPU; a case is built once and cached, and nobody writes to its tensors.

A case is (kind, shape, regime): kind gru (asg_rnn_agent_unroll and its backward), mlp
(asg_mlp_agent_unroll and its backward) or ids (asg_mlp_agent_unroll_ids, the critic: an ACCritic
state with make_state's gains per layer, regimes default / trained / small, first shape only).
Shapes (T1, B, n, K, n_out), both with R = B n = 165 rows (two full 64-row workgroups, two full
16-row waves and a ragged 5-row wave; for mlp and ids N = 495 flattened rows, so tiles straddle time
boundaries):
  (3, 3, 55, 70, 16)    K % 4 != 0: scalar loads; nk = 5: the second fc1 register buffer with a
                        partial group; one fc2 tile; time-major storage seen as [B, T1, ..]
  (3, 5, 33, 132, 300)  K % 4 == 0: vector loads with a 4-wide last chunk; nk = 9: a second round of
                        the double buffer; 19 fc2 tiles with a scalar-store tail; batch-major
Row r = b n + agent has class row_classes(R)[r] at every t: x[b, t, agent] = randn * MULT[class].
h0 (gru) as agent_scale_cases.case: clamp(0.5 randn), rows r % 3 == 0 zero, r % 7 == 1 x 1e-6, rows
0..31 zero; h0 = "none" (NULL) and "broadcast" (one row, stride 0) are variants.  In the outlier
regime column x_col of x and unit h_unit of h0 are zero in every second row.

Loss gradients dh_q [T1, R, 64] (gru: and dh_last [R, 64]) are randn scaled per row by D[dclass],
D = (1, 1e3, 1e-6, 0), dclass = 0 for r < 64, else (r // 5) % 4: from row 64 on every x class meets
every gradient scale, whole rows of exact zeros included (masked steps).

References are plain torch restatements taking a dtype, evaluated in float64 (truth) and float32
(baseline): gru_step, mlp_rows, gru_bptt, mlp_bwd.  The forward check is teacher-forced -- the
reference of step t starts from the kernel's own h_all[t - 1] -- so every step is a single-step
comparison and no error accumulates over t.  The backward check is a pure-function check: kernel and
references get the same float32 planes (the forward kernel's own), so the ReLU masks are the same
bits on both sides.

Tolerances, with u = 2^-24, per group g (statistics: max over the group's rows, all units, all t):
    rule(plane, g) = 4 err32(g) + 1e-7 max|ref64|(g)
  x1, gh_n; the Linear agent's / critic's x1, h, q; every backward output:   rule
  the GRU's h':   rule + GATE_FLOOR
  the GRU's q:    rule + GATE_FLOOR max_j sum_k |W2[j, k]|
  the gates, through their Lipschitz constants from t_a = rule on the pre-activation planes (a
  max-norm rule on r fails for a correct kernel where a pre-activation is large in error but near
  zero in value, class x3e4):
    tol_r = t_ar / 4 + 4 u;  tol_z = t_az / 4 + 4 u
    tol_n = t_ani + max|gh_n|(g) tol_r + t_ghn + 8 u
Backward outputs are divided, in both references too, by the row's D where D > 0 before a group is
formed: the pass is linear in a row's gradient, so the groups stay the x classes and a x 1e3 row
cannot hide a x 1e-6 one.  Where a group's float64 reference is identically zero (rows with D = 0;
saturated gates) the kernel's output must be exactly zero; the Linear agent's dh must be
where(h > 0, dh_q, 0) bit for bit.

GATE_FLOOR = 18 u (agent_scale_cases) was derived for sigmoid = rcp(1 + exp2(-a log2 e)) on the
1-ulp hardware instructions and tanh = 2 sigmoid - 1.  The unroll kernel evaluates
sigmoid(a) = 1 / (1 + expf(-a)) with a true division and n = tanhf(.).  The same derivation for
that formula: expf is good to 1 ulp (its argument -a is exact), a relative 2 u that moves
s = 1 / (1 + e) by s (1 - s) <= 1/4 of it: u / 2; the rounding of 1 + e, relative u, moves s by at
most u; the division is correctly rounded, u / 2 at s < 1 (2.5 ulp, the loosest a HIP division is
allowed to be, would be 2.5 u): sigmoid is within 2 u (4 u), inside the 3.7 u (and the 4 u of tol_r,
tol_z) assumed.  tanhf is good to 2 ulp, 2 u at |n| < 1, and the two roundings of y = i_n + r h_n
move tanh by at most 2 u max y (1 - tanh^2 y) < u: n is within 3 u of the formula, inside the 8 u
assumed.  h' = n + z (h - n) with |h - n| < 2 then carries 3 + 2 * 2 (4) + the roundings of the
difference, the product and the sum (3 u at most): 10 u (14 u) <= 18 u.  The floor carries over as
it is, with room.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from tests import agent_scale_cases as A
from tests.agent_scale_cases import CLASSES, GATE_FLOOR, MULT, blocked, make_state, row_classes

U = 2.0 ** -24
HID = A.HID
R = A.R
SHAPES = ((3, 3, 55, 70, 16), (3, 5, 33, 132, 300))
REGIMES = A.REGIMES
IDS_REGIMES = ("default", "trained", "small")
D = (1.0, 1.0e3, 1.0e-6, 0.0)
GRU_NAMES = ("fc1.weight", "rnn.weight_ih", "rnn.weight_hh", "fc2.weight", "fc1.bias", "rnn.bias_ih",
             "rnn.bias_hh", "fc2.bias")  # the ABI's order
MLP_NAMES = ("fc1.weight", "rnn.weight", "fc2.weight", "fc1.bias", "rnn.bias", "fc2.bias")
IDS_NAMES = ("fc1.weight", "fc2.weight", "fc3.weight", "fc1.bias", "fc2.bias", "fc3.bias")
# (kind, shape, regime), and the GRU's h0 variants (kind, shape, regime, h0)
CASES = ([("gru", s, reg) for s in SHAPES for reg in REGIMES] + [("mlp", s, reg) for s in SHAPES for reg in REGIMES]
         + [("ids", SHAPES[0], reg) for reg in IDS_REGIMES])
H0_VARIANTS = [("gru", SHAPES[0], "trained", "none"), ("gru", SHAPES[0], "trained", "broadcast")]
FWD_PLANES = {"gru": ("x1", "r", "z", "n", "gh_n", "h", "q"), "mlp": ("x1", "h", "q"), "ids": ("x1", "h", "q")}
BWD_PLANES = {"gru": ("dgi", "dgh_n", "dx1", "dh0"), "mlp": ("dh", "dx1"), "ids": ("dh", "dx1")}

assert blocked(132, 300) is False and blocked(70, 16) is False  # no one-hot prefix in either shape


def names(kind):
    return {"gru": GRU_NAMES, "mlp": MLP_NAMES, "ids": IDS_NAMES}[kind]


def d_classes(rows=R):
    r = np.arange(rows)
    return np.where(r < 64, 0, (r // 5) % 4)


def make_ids_state(K, n, m, regime, seed=0):
    """An ACCritic state_dict (fc1 [64, K + n], fc2, fc3) with make_state's gains on fc1 / the
    middle layer / the last one; the outlier entry of fc1 lies in its obs block."""
    from tests.cont_ppo_ref import RefCritic
    torch.manual_seed(3000 + seed)
    sd = {k: v.clone() for k, v in RefCritic(obs=K, n=n, n_out=m).state_dict().items()}
    x_col = None
    if regime == "trained":
        for layer, g in (("fc1", 8.0), ("fc2", 4.0), ("fc3", 16.0)):
            sd[layer + ".weight"] *= g
            sd[layer + ".bias"] *= g
    elif regime == "small":
        for k in sd:
            sd[k] *= 1.0 / 64.0
    elif regime == "outlier":
        x_col = 5
        sd["fc1.weight"][17, x_col] = A.OUTLIER / (K + n) ** 0.5
        sd["fc2.weight"][23, 41] = -A.OUTLIER / HID ** 0.5
        j2 = int(sd["fc2.weight"][:, 17].abs().argmin())
        sd["fc3.weight"][min(7, m - 1), j2] = A.OUTLIER / HID ** 0.5
    elif regime != "default":
        raise ValueError(regime)
    return sd, x_col, None


# ---- the references: plain torch, any dtype ------------------------------------------------------
def gru_step(sd, x_t, h_prev, dtype):
    """One RNNAgent step with the gates written out: x_t [.., K], h_prev [.., 64] -> the planes
    x1, a_r, a_z, a_ni, gh_n (pre-activations), r, z, n, h (= h'), q."""
    w = {k: v.to(dtype) for k, v in sd.items()}
    x_t, h_prev = x_t.to(dtype), h_prev.to(dtype)
    x1 = F.relu(F.linear(x_t, w["fc1.weight"], w["fc1.bias"]))
    gi = F.linear(x1, w["rnn.weight_ih"], w["rnn.bias_ih"])
    gh = F.linear(h_prev, w["rnn.weight_hh"], w["rnn.bias_hh"])
    a_r = gi[..., :HID] + gh[..., :HID]
    a_z = gi[..., HID:2 * HID] + gh[..., HID:2 * HID]
    a_ni, gh_n = gi[..., 2 * HID:], gh[..., 2 * HID:]
    r, z = torch.sigmoid(a_r), torch.sigmoid(a_z)
    n = torch.tanh(a_ni + r * gh_n)
    h = n + z * (h_prev - n)
    q = F.linear(h, w["fc2.weight"], w["fc2.bias"])
    return dict(x1=x1, a_r=a_r, a_z=a_z, a_ni=a_ni, gh_n=gh_n, r=r, z=z, n=n, h=h, q=q)


def mlp_rows(sd, x, dtype):
    """The Linear agent (or, for an ACCritic state, the critic on [obs, eye(n)]) on x [B, T1, n, K]:
    x1, h [T1, R, 64] and q [T1, R, n_out] in the kernels' time-major row order."""
    ids = "fc3.weight" in sd
    W1, Wr, W2, b1, br, b2 = (sd[k].to(dtype) for k in (IDS_NAMES if ids else MLP_NAMES))
    B, T1, n, _ = x.shape
    inp = x.to(dtype)
    if ids:
        inp = torch.cat([inp, torch.eye(n, dtype=dtype).expand(B, T1, n, n)], dim=-1)
    inp = inp.permute(1, 0, 2, 3).reshape(T1, B * n, -1)
    x1 = F.relu(F.linear(inp, W1, b1))
    h = F.relu(F.linear(x1, Wr, br))
    return dict(x1=x1, h=h, q=F.linear(h, W2, b2))


def gru_bptt(planes, h_prev, dh_q, dh_last, W_ih, W_hh, dtype):
    """The recurrence documented above asg_rnn_agent_unroll_backward (include/asg.h): planes
    x1, r, z, n, gh_n and h_prev [T1, R, 64] (h_prev[t] = h_{t-1}), dh_q [T1, R, 64], dh_last [R, 64]
    or None -> dgi [T1, R, 192], dgh_n, dx1 [T1, R, 64], dh0 [R, 64]."""
    x1, r, z, n, gh_n = (planes[k].to(dtype) for k in ("x1", "r", "z", "n", "gh_n"))
    h_prev, dh_q, W_ih, W_hh = h_prev.to(dtype), dh_q.to(dtype), W_ih.to(dtype), W_hh.to(dtype)
    T1 = x1.shape[0]
    dh = torch.zeros_like(x1[0]) if dh_last is None else dh_last.to(dtype).clone()
    dgi, dghn, dx1 = [None] * T1, [None] * T1, [None] * T1
    for t in range(T1 - 1, -1, -1):
        dh = dh + dh_q[t]
        dn = dh * (1 - z[t])
        dz = dh * (h_prev[t] - n[t])
        dn_pre = dn * (1 - n[t] * n[t])
        dr_pre = dn_pre * gh_n[t] * r[t] * (1 - r[t])
        dz_pre = dz * z[t] * (1 - z[t])
        dgi[t] = torch.cat([dr_pre, dz_pre, dn_pre], dim=-1)
        dghn[t] = dn_pre * r[t]
        dx1[t] = (dgi[t] @ W_ih) * (x1[t] > 0)
        dh = dh * z[t] + torch.cat([dr_pre, dz_pre, dghn[t]], dim=-1) @ W_hh
    return dict(dgi=torch.stack(dgi), dgh_n=torch.stack(dghn), dx1=torch.stack(dx1), dh0=dh)


def mlp_bwd(dh_q, h, x1, W_r, dtype):
    """dh = dh_q (h > 0); dx1 = (dh @ W_r) (x1 > 0), rows [.., 64]."""
    dh_q, W_r = dh_q.to(dtype), W_r.to(dtype)
    dh = torch.where(h > 0, dh_q, torch.zeros_like(dh_q))
    return dict(dh=dh, dx1=(dh @ W_r) * (x1 > 0))


# ---- the cases -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(kind, shape, regime, h0="dense"):
    """Weights, x [B, T1, n, K] (a view of its storage order), h0, the loss gradients, row classes
    and tolerance groups.  Read-only: the cache hands the same tensors to every caller."""
    T1, B, n, K, m = shape
    rows = B * n
    assert rows == R
    if kind == "ids":
        sd, x_col, h_unit = make_ids_state(K, n, m, regime)
    else:
        sd, x_col, h_unit = make_state(K, m, kind == "gru", regime)
    g = torch.Generator().manual_seed(A.SEED + K + m + {"gru": 0, "mlp": 1, "ids": 2}[kind])
    cls = row_classes(rows)
    mult = torch.tensor([MULT[c] for c in cls], dtype=torch.float32).view(B, 1, n, 1)
    time_major = shape == SHAPES[0]
    if time_major:  # the runner's batch: [T1][B] storage seen as [B, T1, ..]
        x = torch.randn((T1, B, n, K), generator=g).transpose(0, 1)
    else:
        x = torch.randn((B, T1, n, K), generator=g)
    x.mul_(mult)
    even = (torch.arange(rows) % 2 == 0).view(B, 1, n)
    if x_col is not None:
        x[..., x_col].masked_fill_(even.expand(B, T1, n), 0.0)
    h = None
    if kind == "gru":
        h = (0.5 * torch.randn((rows, HID), generator=g)).clamp(-0.999, 0.999)
        ridx = torch.arange(rows)
        h[ridx % 7 == 1] *= 1.0e-6
        h[ridx % 3 == 0] = 0.0
        h[:32] = 0.0
        if h_unit is not None:
            h[::2, h_unit] = 0.0
        if h0 == "none":
            h = None
        elif h0 == "broadcast":
            h = (0.5 * torch.randn((1, HID), generator=g)).clamp(-0.999, 0.999)
        elif h0 != "dense":
            raise ValueError(h0)
    elif h0 != "dense":
        raise ValueError("h0 variants are the GRU's")
    dcls = d_classes(rows)
    dscale = torch.tensor([D[c] for c in dcls], dtype=torch.float32)
    dh_q = torch.randn((T1, rows, HID), generator=g) * dscale.view(1, rows, 1)
    dh_last = torch.randn((rows, HID), generator=g) * dscale.view(rows, 1) if kind == "gru" else None
    # the tolerance groups of agent_scale_cases (row classes; even / odd halves in the outlier regime)
    base = A.case((rows, K, m), kind == "gru", regime)
    assert (base.cls == cls).all()
    return SimpleNamespace(kind=kind, shape=shape, regime=regime, h0_mode=h0, T1=T1, B=B, n=n, K=K, m=m, R=rows,
                           sd=sd, x=x, h0=h, dh_q=dh_q, dh_last=dh_last, cls=cls, dcls=dcls, dscale=dscale,
                           group=base.group, groups=base.groups, x_col=x_col, h_unit=h_unit, time_major=time_major)


def x_rows(c):
    """x in the kernels' row order: [T1, R, K]"""
    return c.x.permute(1, 0, 2, 3).reshape(c.T1, c.R, c.K)


def h0_rows(c):
    """h0 as the [R, 64] rows the kernel starts from"""
    if c.h0 is None:
        return torch.zeros((c.R, HID))
    return c.h0.expand(c.R, HID)


def h_prev_of(c, h_all):
    """h_{t-1} for every t, [T1, R, 64]: h0 and the kernel's own float32 h_all"""
    return torch.cat([h0_rows(c).unsqueeze(0), h_all[:-1].cpu()], dim=0)


def forward_reference(c, dtype, h_prev=None):
    """Every plane of the case in dtype, [T1, R, ..]; gru: teacher-forced from h_prev [T1, R, 64]."""
    if c.kind == "gru":
        return gru_step(c.sd, x_rows(c), h_prev, dtype)
    return mlp_rows(c.sd, c.x, dtype)


def gru_chain(c, dtype):
    """The GRU reference chained over t from h0 (no teacher): planes [T1, R, ..] and h_prev."""
    h, steps, prev = h0_rows(c).to(dtype), [], []
    xr = x_rows(c)
    for t in range(c.T1):
        prev.append(h)
        steps.append(gru_step(c.sd, xr[t], h, dtype))
        h = steps[-1]["h"]
    return {k: torch.stack([s[k] for s in steps]) for k in steps[0]}, torch.stack(prev)


def backward_reference(c, dtype, planes, h_prev=None, dh_last="case"):
    """The backward outputs in dtype from float32 forward planes (gru: x1, r, z, n, gh_n and
    h_prev; mlp / ids: x1, h) and the case's loss gradients."""
    if c.kind == "gru":
        dl = c.dh_last if isinstance(dh_last, str) else dh_last
        out = gru_bptt(planes, h_prev, c.dh_q, dl, c.sd["rnn.weight_ih"], c.sd["rnn.weight_hh"], dtype)
        out["dh0"] = out["dh0"].unsqueeze(0)
        return out
    Wr = c.sd[names(c.kind)[1]]
    return mlp_bwd(c.dh_q, planes["h"], planes["x1"], Wr, dtype)


# ---- tolerances and reports ----------------------------------------------------------------------
def _gmax(t, sel):
    return t[:, sel].abs().max().item()


def _rule(p32, p64, sel):
    return 4.0 * _gmax(p32.double() - p64, sel) + 1e-7 * _gmax(p64, sel)


def forward_report(c, got, h_prev=None):
    """got: plane -> float32 [T1, R, ..] of FWD_PLANES[c.kind].  Returns (rows, bad): rows =
    (plane, group, err, err32, tol) for every plane and group, bad those with err > tol."""
    p64 = forward_reference(c, torch.float64, h_prev)
    p32 = forward_reference(c, torch.float32, h_prev)
    w2 = c.sd[names(c.kind)[3 if c.kind == "gru" else 2]].double().abs().sum(1).max().item()
    rows, bad = [], []
    for gi, g in enumerate(c.groups):
        sel = torch.as_tensor(c.group == gi)
        rule = {k: _rule(p32[k], p64[k], sel) for k in p64}
        tol = dict(rule)
        if c.kind == "gru":
            tol["h"] = rule["h"] + GATE_FLOOR
            tol["q"] = rule["q"] + GATE_FLOOR * w2
            tol["r"] = rule["a_r"] / 4 + 4 * U
            tol["z"] = rule["a_z"] / 4 + 4 * U
            tol["n"] = rule["a_ni"] + _gmax(p64["gh_n"], sel) * tol["r"] + rule["gh_n"] + 8 * U
        for k in FWD_PLANES[c.kind]:
            assert bool(torch.isfinite(got[k]).all()), k
            err = _gmax(got[k].double().cpu() - p64[k], sel)
            e32 = _gmax(p32[k].double() - p64[k], sel)
            rows.append((k, g, err, e32, tol[k]))
            if not err <= tol[k]:
                bad.append(rows[-1])
    return rows, bad


def backward_report(c, got, planes, h_prev=None, dh_last="case"):
    """got: plane -> float32 [T1, R, ..] (dh0: [1, R, 64]) of BWD_PLANES[c.kind] ("dh0" may be
    absent), computed from `planes`.  Every row is divided by its D where D > 0 first.  Returns
    (rows, bad) as forward_report; a group whose float64 reference is identically zero has
    tol = 0 (exactly zero asked), and so have the rows with D = 0."""
    p64 = backward_reference(c, torch.float64, planes, h_prev, dh_last)
    p32 = backward_reference(c, torch.float32, planes, h_prev, dh_last)
    inv = torch.where(c.dscale > 0, 1.0 / c.dscale.double(), torch.ones(c.R, dtype=torch.float64)).view(1, c.R, 1)
    dzero = c.dscale == 0
    rows, bad = [], []
    for k in BWD_PLANES[c.kind]:
        if k not in got:
            continue
        g32 = got[k].cpu()
        assert bool(torch.isfinite(g32).all()), k
        shape = (-1, c.R, g32.shape[-1])
        gk, r64, r32 = g32.double().view(shape) * inv, p64[k].view(shape) * inv, p32[k].double().view(shape) * inv
        if bool((g32.view(shape)[:, dzero] != 0).any()):
            bad.append((k, "D=0 rows", _gmax(g32.view(shape), dzero), 0.0, 0.0))
        for gi, g in enumerate(c.groups):
            sel = torch.as_tensor(c.group == gi)
            ref_zero = not bool((r64[:, sel] != 0).any())
            tol = 0.0 if ref_zero else 4.0 * _gmax(r32 - r64, sel) + 1e-7 * _gmax(r64, sel)
            err = _gmax(gk - r64, sel) if not ref_zero else _gmax(gk, sel)
            rows.append((k, g, err, _gmax(r32 - r64, sel), tol))
            if not err <= tol:
                bad.append(rows[-1])
    return rows, bad


def format_rows(tag, rows):
    return "\n".join(f"unroll scales {tag} {k} {g}: fused {e:.3e} torch32 {e32:.3e} tol {tol:.3e}"
                     for k, g, e, e32, tol in rows)


def worst_ratio(rows):
    """max err / tol over the rows with tol > 0"""
    return max((e / tol for _, _, e, _, tol in rows if tol > 0), default=0.0)
