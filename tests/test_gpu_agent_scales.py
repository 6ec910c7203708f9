"""The agent kernels' scale machinery, switched on: fc1's retry (rows with max |x| >= 16 inside a
tile of rows below it), per-row and per-matrix scales away from default init, zero and tiny hidden
rows, the n_out > 256 kernel's bf16 GRU -- against a float64 evaluation of the same module, on the
batches of tests/agent_scale_cases.py (their preconditions: tests/test_agent_scale_cases_host.py).

Accuracy is checked per row class (in the outlier regime per half class), not over the batch: a
global max |ref| would hide the small rows.  For h' and Q of RNNFusedAgent.forward
    err <= 4 err_torch32(class) + 1e-7 max|ref|(class) + floor
The Linear agent has floor = 0: every layer is a matmul and a ReLU, so the project's rule holds as
it stands, and this is the sharp test of the split, the retry and the scales.  The GRU agent has
floor = G on h' and G max_j sum_k |W2[j, k]| on Q with G = 18 * 2^-24, which is derived, not
measured: the kernels' sigmoid is rcp(1 + exp2(a)) on v_exp_f32 and v_rcp_f32 (1 ulp each), at
most 3.7 * 2^-24 off in ABSOLUTE terms; tanh = 2 sigmoid - 1 at most 8 * 2^-24; and
h' = n + z (h - n) with |h - n| < 2 at most 8 + 2 * 3.7 + roundings <= 18 * 2^-24.  Absolute, not
relative: with every matrix x 1/64 the formula alone is 5.9e-8 off on h' where the relative rule
would allow 2e-9 (the derivation in full: tests/agent_scale_cases.py).

Row independence is bit for bit: a row's h' and Q are the same whichever rows share its wave tile
(a no-retry row next to a retrying one, a zero-h row whether or not its wave skipped W_hh).  In the
blocked geometry the one-hot gather of block 0 is a per-tile decision, so the claim is made for
batches whose every prefix is one-hot or zero; a batch with other prefixes is held to the tolerance.

Found by these tests and fixed with them: the Linear agent's middle layer (and, in the n_out > 256
kernel, fc1 and fc2 too) started its accumulator from the bias, so every MFMA rounded at the
bias's magnitude; with every matrix x 1/64 (h' ~ b) that was 4.4e-10 .. 7.0e-10 on h' against
4.1e-10 .. 6.8e-10 allowed, PyTorch fp32 0.6e-10 .. 1.3e-10 -- far above the split's own bound for
the layer (2 * 2^-22 sum|w||x| ~ 3e-14), so the accumulation order, not the split.  The bias is now
added after the products.
"""
import functools
from types import SimpleNamespace

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from marl_sap_amd import _lib  # noqa: E402
from marl_sap_amd.modules.agents import RNNFusedAgent  # noqa: E402
from tests import agent_scale_cases as C  # noqa: E402

DEV = torch.device("cuda", 0)
ALL = [(s, rnn, reg) for s in C.SHAPES for rnn in (True, False) for reg in C.REGIMES]
# the (165, 256, 64) batch again: init_hidden() expanded (row stride 0), and a few prefixes that
# are not one-hot (those tiles run block 0 on the MFMAs)
VARIANTS = [(C.SHAPES[0], rnn, reg, v) for rnn in (True, False) for reg in ("default", "trained", "outlier")
            for v in (("init", "valid"), ("mixed", "nonhot"))]


def _module(c):
    agent = RNNFusedAgent(c.K, SimpleNamespace(hidden_dim=64, use_rnn=c.use_rnn, m=c.m)).to(DEV)
    agent.load_state_dict(c.sd)
    return agent


def _inputs(c, perm=None):
    idx = torch.arange(c.x.shape[0]) if perm is None else perm
    x = c.x[idx].to(DEV)
    if c.hidden == "init":
        h = torch.zeros((1, 64), device=DEV).unsqueeze(0).expand(1, x.shape[0], -1)
    else:
        h = c.h[idx].to(DEV)
    return x, h


def _forward(c, perm=None, agent=None):
    """(q, h') of the fused no-grad forward on the CPU, rows back in the case's order"""
    agent = _module(c) if agent is None else agent
    x, h = _inputs(c, perm)
    with torch.no_grad():
        q, h1 = agent(x, h)
    q, h1 = q.cpu(), h1.cpu()
    if perm is not None:
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(len(perm))
        q, h1 = q[inv], h1[inv]
    return q, h1


@functools.lru_cache(maxsize=None)
def _fused(shape, use_rnn, regime, hidden="mixed", prefix="valid"):
    return _forward(C.case(shape, use_rnn, regime, hidden, prefix))


def _check_accuracy(c, q, h1, tag):
    bad = []
    eh, eq = C.group_errors(c, h1, c.h64), C.group_errors(c, q, c.q64)
    for g in c.groups:
        print(f"scales {tag} {g}: h' fused {eh[g]:.3e} torch32 {c.e32_h[g]:.3e} tol {c.tol_h[g]:.3e} | "
              f"Q fused {eq[g]:.3e} torch32 {c.e32_q[g]:.3e} tol {c.tol_q[g]:.3e}")
        if not eh[g] <= c.tol_h[g]:
            bad.append((g, "h'", eh[g], c.tol_h[g]))
        if not eq[g] <= c.tol_q[g]:
            bad.append((g, "Q", eq[g], c.tol_q[g]))
    assert bool(torch.isfinite(q).all()) and bool(torch.isfinite(h1).all())
    assert not bad, (tag, bad)


def _tag(shape, use_rnn, regime, *v):
    return f"{shape[1]}x{shape[2]} {'gru' if use_rnn else 'lin'} {regime}" + "".join(" " + s for s in v)


def _mode(c):
    return _lib.lib().asg_rnn_agent_mode(c.K, 64, c.m, int(c.use_rnn))


@pytest.mark.parametrize("shape,use_rnn,regime", ALL)
def test_accuracy_against_float64_per_row_class(shape, use_rnn, regime):
    c = C.case(shape, use_rnn, regime)
    assert _mode(c) == (4 if c.m <= 256 else _lib.lib().asg_rnn_agent_mfma_mode())
    q, h1 = _fused(shape, use_rnn, regime)
    _check_accuracy(c, q, h1, _tag(shape, use_rnn, regime))


@pytest.mark.parametrize("shape,use_rnn,regime,variant", VARIANTS)
def test_accuracy_variants(shape, use_rnn, regime, variant):
    c = C.case(shape, use_rnn, regime, *variant)
    q, h1 = _fused(shape, use_rnn, regime, *variant)
    _check_accuracy(c, q, h1, _tag(shape, use_rnn, regime, *variant))


@pytest.mark.parametrize("shape,use_rnn,regime", ALL)
def test_greedy_choice_is_the_float64_one(shape, use_rnn, regime):
    """argmax Q == the float64 argmax on every row whose float64 top-2 gap exceeds twice its
    tolerance; at most 5 % of a class's rows are excused that way."""
    c = C.case(shape, use_rnn, regime)
    q, _ = _fused(shape, use_rnn, regime)
    for name, share in C.undecided_share(c).items():
        assert share <= 0.05, (name, share)
    got = q.argmax(1)
    wrong = ((got != c.argmax64) & c.decided).nonzero().flatten().tolist()
    assert not wrong, (wrong, [C.CLASSES[c.cls[r]] for r in wrong])


def _perms(R):
    g = torch.Generator().manual_seed(2024)
    return {"reversed": torch.arange(R - 1, -1, -1), "shuffled": torch.randperm(R, generator=g)}


@pytest.mark.parametrize("shape,use_rnn,regime,hidden", [a + ("mixed",) for a in ALL] + [
    (C.SHAPES[0], True, "trained", "init"), (C.SHAPES[2], True, "default", "init"),
    (C.SHAPES[3], True, "default", "init")])
def test_rows_are_independent_bit_for_bit(shape, use_rnn, regime, hidden):
    """The batch with its rows permuted gives, un-permuted, the same bits: a no-retry row keeps
    its value whether or not its tile retried (rows 0..31 sit in a tile that never does, after the
    permutation among rows that do), and so does a zero-h row whether or not its wave skipped
    W_hh.  Every prefix of the blocked shapes is one-hot or zero (see the module docstring)."""
    c = C.case(shape, use_rnn, regime, hidden)
    q, h1 = _fused(shape, use_rnn, regime, hidden)
    agent = _module(c)
    for name, perm in _perms(shape[0]).items():
        qp, hp = _forward(c, perm, agent)
        assert torch.equal(hp, h1), (name, (hp - h1).abs().max().item())
        assert torch.equal(qp, q), (name, (qp - q).abs().max().item())


@pytest.mark.parametrize("use_rnn,regime", [(True, "default"), (True, "trained"), (False, "trained")])
def test_permuted_rows_with_other_prefixes_stay_within_tolerance(use_rnn, regime):
    """A few prefixes that are not one-hot: their tiles run block 0 on the MFMAs instead of the
    gather, so a row's bits depend on its tile's company -- its accuracy must not."""
    c = C.case(C.SHAPES[0], use_rnn, regime, "mixed", "nonhot")
    agent = _module(c)
    for name, perm in _perms(C.SHAPES[0][0]).items():
        qp, hp = _forward(c, perm, agent)
        _check_accuracy(c, qp, hp, _tag(C.SHAPES[0], use_rnn, regime, "nonhot", name))


@pytest.mark.parametrize("eps", [0.0, 0.3])
@pytest.mark.parametrize("shape,use_rnn,regime", [(s, rnn, reg) for s in C.SHAPES for rnn in (True, False)
                                                  for reg in ("trained", "outlier")])
def test_forward_select_equals_forward_then_selector(shape, use_rnn, regime, eps):
    """asg_rnn_agent_select == asg_rnn_agent_forward + asg_epsilon_greedy on the mixed batches
    (165 rows = 15 envs x 11 agents, random availability): the same h' bits, the same actions."""
    from marl_sap_amd.action_selectors.classic_selectors import EpsilonGreedyActionSelector
    c = C.case(shape, use_rnn, regime)
    B, n, m = 15, 11, c.m
    args = SimpleNamespace(epsilon_start=eps, epsilon_finish=eps, epsilon_anneal_time=1, evaluation_epsilon=0.0,
                           seed=5)
    agent = _module(c)
    x, h = _inputs(c)
    g = torch.Generator().manual_seed(9)
    avail = (torch.rand((B, n, m), generator=g) > (0.2 if m <= 64 else 0.7)).to(DEV)
    avail[..., min(3, m - 1)] = True
    sel = EpsilonGreedyActionSelector(args)
    with torch.no_grad():
        q, h1 = agent(x, h)
        a1 = sel.select_action(q.view(B, n, m), avail, 0)
        sel2 = EpsilonGreedyActionSelector(args)
        e, seed, counter, status, base = sel2.fused_params(0, False, DEV)
        assert (seed, counter, base) == (sel.seed, sel.calls, 0)
        out = torch.full((B, n), -7, dtype=torch.int64, device=DEV)
        h2 = agent.forward_select(x, h, avail, n, e, seed, counter, out, status)
    q0, h0 = _fused(shape, use_rnn, regime)
    assert torch.equal(h1.cpu(), h0) and torch.equal(q.cpu(), q0)
    assert torch.equal(h2, h1)
    assert torch.equal(out, a1)
    assert int(status.item()) == 0
    assert bool(avail.view(B * n, m).gather(1, out.view(-1, 1)).all())


def _close(got, want):
    scale = want.abs().max().item()
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5 * scale)


@pytest.mark.parametrize("use_rnn", [True, False])
def test_repack_follows_weight_changes_on_a_live_module(use_rnn):
    """One live module on the GPU whose weights change under the packed copy: load_state_dict,
    an in-place no_grad update, an optimizer step.  After each the no-grad fused forward matches
    the module's own autograd-path forward and differs from the result before the change.  The
    documented exception: a write through `.data` does not bump the tensor's
    version, so the pack is stale until invalidate_pack()."""
    c = C.case(C.SHAPES[0], use_rnn, "default")
    agent = _module(c)
    # the rows below fc1's first scale: at 3e4 x the gates' pre-activations cancel at 1e4 and two
    # fp32 evaluations differ by more than 1e-5 (both are held to float64 above)
    keep = torch.as_tensor((c.cls == 0) | (c.cls == 3) | (c.cls == 4)).nonzero().flatten()
    x, h = _inputs(c, keep)

    def both():
        with torch.no_grad():
            qf, hf = agent(x, h)
        qa, ha = agent(x, h)  # autograd enabled: the PyTorch module itself
        assert qa.requires_grad and not qf.requires_grad
        return qf, hf, qa.detach(), ha.detach()

    def changed(prev):
        qf, hf, qa, ha = both()
        _close(qf, qa)
        _close(hf, ha)
        assert (qf - prev).abs().max().item() > 1e-3 * qa.abs().max().item()  # not the old weights' result
        return qf

    qf, hf, qa, ha = both()
    _close(qf, qa)
    _close(hf, ha)
    agent.load_state_dict(C.case(C.SHAPES[0], use_rnn, "trained").sd)
    qf = changed(qf)
    with torch.no_grad():
        for p in agent.parameters():
            p.mul_(0.5)
    qf = changed(qf)
    opt = torch.optim.Adam(agent.parameters(), lr=1e-2)
    q, h1 = agent(x, h)
    (q.square().mean() + h1.square().mean()).backward()
    opt.step()
    opt.zero_grad()
    qf = changed(qf)
    # the documented exception: `.data` writes are invisible to the version counters
    for w in (agent.fc1.weight, agent.fc2.weight):
        w.data.mul_(3.0)
    stale, _, qa, _ = both()
    assert (stale - qa).abs().max().item() > 1e-3 * qa.abs().max().item()
    assert torch.equal(stale, qf)  # biases untouched, weights still the packed ones
    agent.invalidate_pack()
    changed(qf)
