"""Inputs and references for the agent kernels' scale paths (tests/test_gpu_agent_scales.py, and
their preconditions in tests/test_agent_scale_cases_host.py): weights that are not default-init,
observation rows of very different magnitudes inside one wave tile, and hidden states with zero
and tiny rows.  Everything here runs on the CPU; a case is built once and cached, and nobody
writes to its tensors.

Weight regimes (gains on a default-init state_dict, each weight with its bias):
  default   none
  trained   fc1 x 8, weight_ih (Linear agent: its middle layer) x 4, weight_hh x 1/4, fc2 x 16
  small     every matrix x 1/64
  outlier   default, plus one entry of each matrix set to 2^12 x that matrix's init bound
            (1 / sqrt(fan_in)); the input column the fc1 entry multiplies, and the hidden unit the
            weight_hh entry multiplies, are zero in every second row (the units the middle layer's
            and fc2's entries multiply are computed activations)

Row classes, mixed inside one batch of R = 165 rows (five 32-row wave tiles and a ragged 5-row
tile): rows 0..31 are all x 1 (that tile never re-runs fc1), rows 32..63 all x 40 (every row of
that tile re-runs it), and from row 64 on the class is r % 5: x 1, x 40, x 3e4 (past f16's range
unscaled), x 1e-4, all-zero.

Hidden state: clamp(0.5 randn, +-0.999); rows r % 3 == 0 zero; rows r % 7 == 1 scaled by 1e-6;
rows 0..31 zero (the wave-uniform zero-h branch).  hidden="init" is init_hidden() expanded.

Layout: where the kernel takes the input as blocks with a one-hot prefix (K a multiple >= 2 of
n_out >= 16, the mock env's obs), block 0 of every row is onehot(a) or zero and the classes scale
blocks 1..; prefix="nonhot" gives a few rows another prefix (a second 1, a 0.5, a 2).

The tolerance of a row class c, for h' and for Q (the project's rule, per class because one global
max |ref| would hide the small rows):
    tol(c) = 4 err_torch32(c) + 1e-7 max|ref|(c) + floor
with floor = 0 for the Linear agent and, for the GRU agent, GATE_FLOOR on h' and
GATE_FLOOR * max_j sum_k |W2[j, k]| on Q.  (In the outlier regime the classes are split further, see
case(): tighter, never looser.)

GATE_FLOOR = 18 * 2^-24 is derived from the kernels' gate formula, not measured.  They evaluate
sigmoid(a) = rcp(1 + exp2(-a log2 e)) with v_exp_f32 and v_rcp_f32, each good to 1 ulp: the
exponential's relative error (1 ulp, plus the rounding of its argument's product) moves
s = 1 / (1 + e) by at most s (1 - s) <= 1/4 of it, the rounding of 1 + e by as much, and the
reciprocal adds 1 ulp of s <= 1: together at most 3.7 * 2^-24 absolute -- accurate in absolute
terms, not relative to a small gate.  tanh(y) = 2 sigmoid(2 y) - 1 doubles that and rounds once
more: at most 8 * 2^-24.  h' = n + z (h - n) with |h - n| < 2 then carries 8 (from n) + 2 * 3.7
(from z) + the roundings of the product and the sum: at most 18 * 2^-24 = 1.07e-6.  (The same
formula evaluated in float32 on the CPU stays below 6.6e-7 in these regimes.)
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from marl_sap_amd.modules.agents import RNNAgent

R = 165
HID = 64
SHAPES = ((165, 256, 64), (165, 70, 16), (165, 1024, 256), (165, 132, 300))
REGIMES = ("default", "trained", "small", "outlier")
CLASSES = ("x1", "x40", "x3e4", "x1e-4", "zero")
MULT = (1.0, 40.0, 3.0e4, 1.0e-4, 0.0)
GATE_FLOOR = 18.0 * 2.0 ** -24
OUTLIER = 2.0 ** 12
# the generators' seed: one at which every case leaves the greedy-choice test its room (at most
# 5 % of a class's rows undecided in float64 -- a property of the inputs, asserted on the CPU by
# test_agent_scale_cases_host.py)
SEED = 104


def blocked(K, m):
    """the kernel's block geometry with a one-hot prefix (h2_geom): block 0 = the first m inputs"""
    return m >= 16 and K % m == 0 and K // m >= 2


def row_classes(rows=R):
    r = np.arange(rows)
    return np.where(r < 32, 0, np.where(r < 64, 1, r % 5))


def make_state(K, m, use_rnn, regime, seed=0):
    """(float32 state_dict, the x column and the h unit that are zero in every second row or None)"""
    torch.manual_seed(1000 + seed)
    sd = RNNAgent(K, SimpleNamespace(hidden_dim=HID, use_rnn=use_rnn, m=m)).state_dict()
    sd = {k: v.clone() for k, v in sd.items()}
    mid = ("rnn.weight_ih", "rnn.bias_ih") if use_rnn else ("rnn.weight", "rnn.bias")

    def gain(names, g):
        for k in names:
            sd[k] *= g

    x_col = h_unit = None
    if regime == "trained":
        gain(("fc1.weight", "fc1.bias"), 8.0)
        gain(mid, 4.0)
        if use_rnn:
            gain(("rnn.weight_hh", "rnn.bias_hh"), 0.25)
        gain(("fc2.weight", "fc2.bias"), 16.0)
    elif regime == "small":
        gain(tuple(sd.keys()), 1.0 / 64.0)
    elif regime == "outlier":
        x_col = (m + 5) if blocked(K, m) else 5
        h_unit = 9
        sd["fc1.weight"][17, x_col] = OUTLIER / K ** 0.5
        sd[mid[0]][23, 41] = -OUTLIER / HID ** 0.5
        if use_rnn:
            sd["rnn.weight_hh"][HID + 30, h_unit] = OUTLIER / HID ** 0.5
        # fc2's entry multiplies the hidden unit that fc1's amplified unit 17 feeds least, so the
        # two entries do not multiply each other into every Q of the amplified rows
        j2 = int(sd[mid[0]][:HID, 17].abs().argmin())
        sd["fc2.weight"][min(7, m - 1), j2] = OUTLIER / HID ** 0.5
    elif regime != "default":
        raise ValueError(regime)
    return sd, x_col, h_unit


def forward(sd, x, h, use_rnn, dtype):
    """The PyTorch RNNAgent with these weights on the CPU in `dtype`: (q, h')"""
    K, m = sd["fc1.weight"].shape[1], sd["fc2.weight"].shape[0]
    net = RNNAgent(K, SimpleNamespace(hidden_dim=HID, use_rnn=use_rnn, m=m)).to(dtype)
    net.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
    with torch.no_grad():
        q, h1 = net(x.to(dtype), h.to(dtype))
    return q, h1


@functools.lru_cache(maxsize=None)
def case(shape, use_rnn, regime, hidden="mixed", prefix="valid"):
    """One batch: weights, x [R, K], h [R, 64] (float32, CPU), its row classes and the float64 /
    float32 results.  Read-only: the cache hands the same tensors to every caller."""
    rows, K, m = shape
    sd, x_col, h_unit = make_state(K, m, use_rnn, regime)
    g = torch.Generator().manual_seed(SEED + K + m)
    cls = row_classes(rows)
    mult = torch.tensor([MULT[c] for c in cls], dtype=torch.float32)
    x = torch.randn((rows, K), generator=g) * mult[:, None]
    if blocked(K, m):
        a = torch.randint(0, m, (rows,), generator=g)
        x[:, :m] = torch.nn.functional.one_hot(a, m).float()
        x[torch.arange(rows) % 7 == 3, :m] = 0.0
        x[torch.as_tensor(cls == 4), :m] = 0.0
        if prefix == "nonhot":
            x[5, (a[5] + 1) % m] = 1.0       # a second 1 (rows of the no-retry tile)
            x[40, (a[40] + 2) % m] = 0.5     # the all-retry tile
            x[101, (a[101] + 3) % m] = 2.0   # a mixed tile
            x[163, :m] = 0.25                # the ragged tile
    elif prefix != "valid":
        raise ValueError("prefix variants need the blocked geometry")
    h = (0.5 * torch.randn((rows, HID), generator=g)).clamp(-0.999, 0.999)
    ridx = torch.arange(rows)
    h[ridx % 7 == 1] *= 1.0e-6
    h[ridx % 3 == 0] = 0.0
    h[:32] = 0.0
    if hidden == "init":
        h = torch.zeros((rows, HID))
    elif hidden != "mixed":
        raise ValueError(hidden)
    if x_col is not None:
        x[::2, x_col] = 0.0
        h[::2, h_unit] = 0.0
    q64, h64 = forward(sd, x, h, use_rnn, torch.float64)
    q32, h32 = forward(sd, x, h, use_rnn, torch.float32)
    w2_rowsum = sd["fc2.weight"].double().abs().sum(1).max().item()
    floor_h = GATE_FLOOR if use_rnn else 0.0
    floor_q = GATE_FLOOR * w2_rowsum if use_rnn else 0.0
    # tolerance groups: the row classes; in the outlier regime each class is split into the rows
    # the fc1 entry acts on (odd) and the rows whose column is zero (even) -- in the Linear agent
    # the first are some 100 x larger, and one tolerance for both would hide the second.  A group's
    # tolerance is never above its class's, so this asks more, not less.
    names, group = [], np.zeros(rows, dtype=np.int64)
    for ci, name in enumerate(CLASSES):
        for par in ((0, 1) if x_col is not None else (None,)):
            sel = (cls == ci) if par is None else ((cls == ci) & (np.arange(rows) % 2 == par))
            if sel.any():
                group[sel] = len(names)
                names.append(name if par is None else name + ("/even", "/odd")[par])
    tol_h, tol_q, e32_h, e32_q = {}, {}, {}, {}
    for gi, name in enumerate(names):
        sel = torch.as_tensor(group == gi)
        e32_h[name] = (h32.double() - h64)[sel].abs().max().item()
        e32_q[name] = (q32.double() - q64)[sel].abs().max().item()
        tol_h[name] = 4 * e32_h[name] + 1e-7 * h64[sel].abs().max().item() + floor_h
        tol_q[name] = 4 * e32_q[name] + 1e-7 * q64[sel].abs().max().item() + floor_q
    top2 = q64.topk(min(2, m), dim=1).values
    gap = (top2[:, 0] - top2[:, -1]) if m > 1 else torch.full((rows,), float("inf"), dtype=torch.float64)
    decided = torch.tensor([bool(gap[r] > 2 * tol_q[names[group[r]]]) for r in range(rows)])
    return SimpleNamespace(shape=shape, K=K, m=m, use_rnn=use_rnn, regime=regime, hidden=hidden, prefix=prefix,
                           sd=sd, x=x, h=h, cls=cls, group=group, groups=tuple(names), q64=q64, h64=h64, q32=q32,
                           h32=h32, tol_h=tol_h, tol_q=tol_q, e32_h=e32_h, e32_q=e32_q, decided=decided,
                           argmax64=q64.argmax(1))


def group_errors(c, got, want):
    """max |got - want| per tolerance group of case c"""
    d = (got.double().cpu() - want).abs()
    return {name: d[torch.as_tensor(c.group == gi)].max().item() for gi, name in enumerate(c.groups)}


def undecided_share(c):
    """per row class, the share of rows whose float64 top-2 Q gap is within twice their tolerance"""
    out = {}
    for i, name in enumerate(CLASSES):
        sel = torch.as_tensor(c.cls == i)
        out[name] = int((~c.decided[sel]).sum()) / int(sel.sum())
    return out
