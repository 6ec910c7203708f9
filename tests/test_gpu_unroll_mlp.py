"""RNNFusedAgent.unroll for the Linear agent with fused_linear_unroll (asg_mlp_agent_unroll /
asg_mlp_agent_unroll_backward: the agent over all T1 * B * n rows of a batch in one launch each
way) against the PyTorch module looped over t in float64.  Tolerance: the rule of
tests/test_gpu_agent.py -- the kernels' max error against float64 may be at most 4 x the fp32
PyTorch autograd path's own error on the same inputs, plus 1e-7 max|reference|.  The rule needs
both precisions to take the same side of every ReLU, so the inputs are seeded (on the CPU, where
the seeds were chosen) such that no float64 pre-activation lies within 1e-5 of zero."""
from types import SimpleNamespace

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from marl_sap_amd.modules.agents import RNNAgent, RNNFusedAgent  # noqa: E402

DEV = torch.device("cuda", 0)
NAMES = ["fc1.weight", "fc1.bias", "rnn.weight", "rnn.bias", "fc2.weight", "fc2.bias"]
# (T1, B, n, K, n_out) -> seed: one partial tile; R = 15, so 16-row tiles straddle time
# boundaries; N ragged across waves and workgroups with K % 4 != 0; aligned, the workload's K
# and n_out; n_out > 256 with a partial last fc2 tile
SEEDS = {(1, 3, 5, 20, 7): 0, (4, 3, 5, 20, 7): 0, (5, 2, 37, 70, 20): 16, (3, 4, 16, 256, 64): 1,
         (2, 1, 20, 490, 450): 0}
SHAPES = list(SEEDS)
# the edges of fc1's two-buffer pipeline (2 chunks of 16 inputs per buffer): nk = ceil(K / 16) = 1 (the
# first buffer alone, partly filled), 3 (one chunk into the second buffer), 4 (both buffers full, one
# round), and 3 with K % 4 != 0 (scalar loads, a 1-wide last group); R = 17, N = 34 flattened rows:
# two full 16-row tiles, one across the time boundary, and a two-row tile; n_out = 5: one partial
# fc2 tile, scalar stores
PIPELINE_SEEDS = {(2, 1, 17, 3, 5): 0, (2, 1, 17, 48, 5): 0, (2, 1, 17, 64, 5): 0, (2, 1, 17, 37, 5): 0}
SEEDS.update(PIPELINE_SEEDS)
RELU_MARGIN = 1e-5


def _args(m, **kw):
    return SimpleNamespace(hidden_dim=64, use_rnn=False, m=m, **kw)


def _loop(agent, x, h0=None):
    """T1 successive RNNAgent.forward calls (the PyTorch module, any dtype)."""
    B, T1, n, K = x.shape
    h = torch.zeros((B * n, 64), dtype=x.dtype, device=x.device) if h0 is None else h0
    qs = []
    for t in range(T1):
        q, h = RNNAgent.forward(agent, x[:, t].reshape(B * n, K), h)
        qs.append(q.view(B, n, -1))
    return torch.stack(qs, 1), h


def _run(fn, agent, x, wq, wh):
    """(q, h_last, grads of the six parameter tensors) of loss = <q, wq> + <h_last, wh>."""
    agent.zero_grad()
    q, h_last = fn(agent, x)
    ((q * wq).sum() + (h_last * wh).sum()).backward()
    sd = dict(agent.named_parameters())
    return q.detach(), h_last.detach(), {k: sd[k].grad.clone() for k in NAMES}


def cpu_case(shape, seed):
    """The seeded inputs of a shape on the CPU, the float64 module's results on them, and the
    smallest |pre-activation| of the two ReLUs in float64."""
    T1, B, n, K, m = shape
    torch.manual_seed(seed)
    state = RNNAgent(K, _args(m)).state_dict()
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn((B, T1, n, K), generator=g)
    wq = torch.randn((B, T1, n, m), generator=g)  # the loss: random weights on q and h_last
    wh = torch.randn((B * n, 64), generator=g)
    ref64 = RNNAgent(K, _args(m)).double()
    ref64.load_state_dict({k: v.double() for k, v in state.items()})
    with torch.no_grad():
        pre1 = x.double().reshape(-1, K) @ ref64.fc1.weight.t() + ref64.fc1.bias
        pre2 = torch.relu(pre1) @ ref64.rnn.weight.t() + ref64.rnn.bias
        margin = min(pre1.abs().min().item(), pre2.abs().min().item())
    want = _run(_loop, ref64, x.double(), wq.double(), wh.double())
    return state, x, wq, wh, want, margin


_CASES = {}


def _case(shape):
    """cpu_case once per shape, shared (and left unchanged) by the tests that need it."""
    if shape not in _CASES:
        _CASES[shape] = cpu_case(shape, SEEDS[shape])
    return _CASES[shape]


def _agents(shape, state):
    K, m = shape[3], shape[4]
    ref = RNNAgent(K, _args(m)).to(DEV)
    fused = RNNFusedAgent(K, _args(m, fused_linear_unroll=True)).to(DEV)
    ref.load_state_dict(state)
    fused.load_state_dict(state)
    return ref, fused


def _layout(x, time_major):
    x = x.to(DEV)
    if time_major:  # the runner batch: [T1][B] storage seen as [B, T1, ...]
        x = x.transpose(0, 1).contiguous().transpose(0, 1)
    return x


@pytest.mark.parametrize("time_major", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_mlp_unroll_forward_and_gradients_match_float64(shape, time_major):
    _check_against_float64(shape, time_major)


@pytest.mark.parametrize("shape", list(PIPELINE_SEEDS))
def test_mlp_unroll_at_the_fc1_pipeline_edges(shape):
    _check_against_float64(shape, False)


def _check_against_float64(shape, time_major):
    T1, B, n, K, m = shape
    state, x, wq, wh, (q64, h64, g64), margin = _case(shape)
    # the condition on the inputs: no ReLU can flip between float64 and float32
    assert margin > RELU_MARGIN, margin
    ref, fused = _agents(shape, state)
    x, wq, wh = _layout(x, time_major), wq.to(DEV), wh.to(DEV)
    assert B == 1 or x.stride(0) == (n * K if time_major else T1 * n * K)
    q32, h32, g32 = _run(_loop, ref, x, wq, wh)
    unroll = lambda a, xx: a.unroll(xx, None)  # noqa: E731
    qf, hf, gf = _run(unroll, fused, x, wq, wh)
    assert qf.shape == (B, T1, n, m) and hf.shape == (B * n, 64) and set(gf) == set(NAMES)
    items = [("q", qf, q32, q64), ("h_last", hf, h32, h64)] + [(k, gf[k], g32[k], g64[k]) for k in NAMES]
    for name, got, base, want in items:
        assert got.shape == want.shape, name
        err_fused = (got.double().cpu() - want).abs().max().item()
        err_torch = (base.double().cpu() - want).abs().max().item()
        floor = 1e-7 * want.abs().max().item()
        print(f"{name}: max |err| vs float64: fused {err_fused:.3e}, torch fp32 {err_torch:.3e}, floor {floor:.1e}")
        assert err_fused <= 4 * err_torch + floor, (name, err_fused, err_torch, floor)
    # a second run on the same inputs: identical bits (no floating-point atomics)
    qf2, hf2, gf2 = _run(unroll, fused, x, wq, wh)
    assert torch.equal(qf2, qf) and torch.equal(hf2, hf)
    for k in gf:
        assert torch.equal(gf2[k], gf[k]), k


@pytest.mark.parametrize("shape", SHAPES)
def test_no_grad_mlp_unroll_matches_successive_forward_calls(shape):
    T1, B, n, K, m = shape
    state, x, _, _, _, _ = _case(shape)
    _, fused = _agents(shape, state)
    x = _layout(x, True)
    h0 = torch.randn((B * n, 64), device=DEV) * 0.5
    with torch.no_grad():
        for h_start in (None, h0):  # the Linear agent ignores its hidden state
            q, h_last = fused.unroll(x, h_start)
            h = fused.init_hidden().expand(B * n, 64) if h_start is None else h_start
            qs = []
            for t in range(T1):
                qt, h = fused(x[:, t].reshape(B * n, K), h)  # asg_rnn_agent_forward
                qs.append(qt.view(B, n, m))
            assert not q.requires_grad
            assert q.shape == (B, T1, n, m) and h_last.shape == (B * n, 64)
            torch.testing.assert_close(q, torch.stack(qs, 1), rtol=1e-5, atol=2e-5)
            torch.testing.assert_close(h_last, h, rtol=1e-5, atol=2e-5)


def test_mlp_unroll_with_only_h_last_used():
    """q receives no gradient: fc2's gradients are zero, the others those of the loop."""
    shape = (4, 3, 5, 20, 7)
    state, x, _, wh, _, _ = _case(shape)
    ref, fused = _agents(shape, state)
    x, wh = x.to(DEV), wh.to(DEV)
    h0 = torch.randn((15, 64), device=DEV).requires_grad_(True)
    ref.zero_grad()
    _, h_loop = _loop(ref, x)
    (h_loop * wh).sum().backward()
    _, h_last = fused.unroll(x, h0)
    (h_last * wh).sum().backward()
    assert h0.grad is None  # ignored, as RNNAgent.forward ignores it
    want = dict(ref.named_parameters())
    for k, v in fused.named_parameters():
        if k.startswith("fc2"):  # autograd leaves them None on the loop, the kernels' path zeros
            assert want[k].grad is None and torch.count_nonzero(v.grad) == 0, k
        else:
            torch.testing.assert_close(v.grad, want[k].grad, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(h_last.detach(), h_loop.detach(), rtol=1e-5, atol=2e-5)


@pytest.mark.parametrize("kw", [{}, {"fused_linear_unroll": False}, {"fused_linear_unroll": True, "unfused_unroll": True}])
def test_flag_off_returns_the_loop(kw):
    torch.manual_seed(2)
    B, T1, n, K, m = 2, 3, 5, 20, 7
    agent = RNNFusedAgent(K, _args(m, **kw)).to(DEV)
    x = torch.randn((B, T1, n, K), device=DEV)
    h0 = torch.randn((B * n, 64), device=DEV)
    q, h = agent.unroll(x, h0)
    q_loop, h_loop = _loop(agent, x, h0)
    assert torch.equal(q, q_loop) and torch.equal(h, h_loop) and q.requires_grad
