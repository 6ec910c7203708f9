"""The learner's sequence kernels under autograd: the GRU agent's unroll (asg_unroll.hip) and the
Linear agent's / ACCritic's (asg_unroll_mlp.hip).  Three layers: the launches (one ABI call each),
the parameter gradients as plain GEMMs over the flattened T1 * R rows (pure torch: any device,
any float dtype), and the autograd functions that join them.  The functions take their forward
launch as an argument, so a caller hands in its own module's attribute, looked up per call."""
import ctypes

import torch

from .. import _lib


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _outputs(x, H, n_out, planes):
    """q [T1, R, n_out], h_all [T1, R, H] and, if planes, the saved [planes.., T1, R, H]"""
    B, T1, n, _ = x.shape
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=x.device)  # noqa: E731
    return new(T1, B * n, n_out), new(T1, B * n, H), new(*planes, T1, B * n, H) if planes is not None else None


def h0_arg(h0, R, H):
    """h0 as the kernels take it: ([rows, H] tensor or None, row stride; 0 = one row broadcast)."""
    if h0 is None:
        return None, 0
    if h0.numel() == H:
        return h0.reshape(1, H).float().contiguous(), 0
    h = h0.reshape(R, H)
    if h.dtype != torch.float32 or h.stride(-1) != 1 or h.stride(0) % 4 != 0 or h.data_ptr() % 16 != 0:
        h = h.float().contiguous()
    return h, h.stride(0)


def gru_launch(x, h0, W1, b1, Wih, Whh, bih, bhh, W2, b2, save):
    """One asg_rnn_agent_unroll launch on x [B, T1, n, K] (any batch / time / agent strides):
    q [T1, R, n_out], h [T1, R, 64] and, with save, the planes x1, r, z, n, gh_n [5, T1, R, 64]."""
    B, T1, n, K = x.shape
    R, H, n_out = B * n, Wih.shape[1], W2.shape[0]
    q, h_all, sv = _outputs(x, H, n_out, (5,) if save else None)
    h0k, hs = h0_arg(h0, R, H)
    ws = [t.detach().contiguous() for t in (W1, Wih, Whh, W2, b1, bih, bhh, b2)]
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().asg_rnn_agent_unroll(
            ptr(x), _lib.i64arr([x.stride(1), x.stride(0), x.stride(2)]), T1, B, n, K, ptr(h0k), hs,
            *[ptr(w) for w in ws], H, n_out, 1, ptr(q), ptr(h_all), ptr(sv), _lib.stream_ptr(x.device)))
    return q, h_all, sv


def mlp_launch(x, W1, b1, Wr, br, W2, b2, save, ids=False):
    """One asg_mlp_agent_unroll launch (ids: asg_mlp_agent_unroll_ids, W1 [64, K + n] with the
    agent-id block) on x [B, T1, n, K] (any batch / time / agent strides): q [T1, R, n_out],
    h [T1, R, 64] and, with save, x1 [T1, R, 64]."""
    B, T1, n, K = x.shape
    q, h_all, x1 = _outputs(x, Wr.shape[1], W2.shape[0], () if save else None)
    ws = [t.detach().contiguous() for t in (W1, Wr, W2, b1, br, b2)]
    entry = _lib.lib().asg_mlp_agent_unroll_ids if ids else _lib.lib().asg_mlp_agent_unroll
    with torch.cuda.device(x.device):
        _lib.check(entry(ptr(x), _lib.i64arr([x.stride(1), x.stride(0), x.stride(2)]), T1, B, n, K,
                         *[ptr(w) for w in ws], Wr.shape[1], W2.shape[0], ptr(q), ptr(h_all), ptr(x1),
                         _lib.stream_ptr(x.device)))
    return q, h_all, x1


def _rows(x):
    """x [B, T1, n, K] as the kernels' [T1 * R, K] rows"""
    B, T1, n, K = x.shape
    return x.permute(1, 0, 2, 3).reshape(T1 * B * n, K)


def gru_param_grads(x, h_first, x1, h_all, dgi, dgh_n, dx1, dQ):
    """The GRU agent's parameter gradients, in the module's parameter order (fc1.weight, fc1.bias,
    rnn.weight_ih, rnn.weight_hh, rnn.bias_ih, rnn.bias_hh, fc2.weight, fc2.bias), from x
    [B, T1, n, K], the state before step 0 h_first [R, H], the planes x1 and h [T1, R, H] and the
    backward kernel's dgi [N, 3 H], dgh_n, dx1 [N, H]; dQ [N, n_out] is the loss gradient."""
    N, H = dx1.shape
    hf = h_all.reshape(N, H)
    h_prev = torch.cat([h_first, hf[:N - h_first.shape[0]]], dim=0)
    dgh = torch.cat([dgi[:, :2 * H], dgh_n], dim=1)
    return (dx1.t() @ _rows(x), dx1.sum(0), dgi.t() @ x1.reshape(N, H), dgh.t() @ h_prev, dgi.sum(0), dgh.sum(0),
            dQ.t() @ hf, dQ.sum(0))


def mlp_param_grads(x, x1, h_all, dh, dx1, dQ, ids):
    """The Linear agent's / critic's parameter gradients, in the module's parameter order (first
    layer, middle layer, last layer; weight, bias), from x [B, T1, n, K], the planes x1 and h
    [T1, R, H] and the backward kernel's dh, dx1 [N, H]; dQ [N, n_out] is the loss gradient.  ids:
    W1 has the agent-id block, whose gradient is the per-agent sums of dx1."""
    B, T1, n, _ = x.shape
    N, H = dx1.shape
    dW1 = dx1.t() @ _rows(x)
    if ids:
        dW1 = torch.cat([dW1, dx1.view(T1, B, n, H).sum((0, 1)).t()], dim=1)
    return dW1, dx1.sum(0), dh.t() @ x1.reshape(N, H), dh.sum(0), dQ.t() @ h_all.reshape(N, H), dQ.sum(0)


class _GRUUnroll(torch.autograd.Function):
    """asg_rnn_agent_unroll under autograd: the forward kernel saves x1, r, z, n and gh_n per
    step, asg_rnn_agent_unroll_backward walks the recurrence back, and the parameter
    gradients are GEMMs over the flattened T1 * R rows."""

    @staticmethod
    def forward(ctx, launch, x, h0, W1, b1, Wih, Whh, bih, bhh, W2, b2):
        q, h_all, save = launch(x, h0, W1, b1, Wih, Whh, bih, bhh, W2, b2, True)
        ctx.save_for_backward(x, h0, Wih, Whh, W2, h_all, save)
        B, T1, n, _ = x.shape
        return q.view(T1, B, n, -1).permute(1, 0, 2, 3), h_all[T1 - 1]

    @staticmethod
    def backward(ctx, dq, dh_last):
        x, h0, Wih, Whh, W2, h_all, save = ctx.saved_tensors
        B, T1, n, K = x.shape
        R, H, n_out = B * n, Wih.shape[1], W2.shape[0]
        N = T1 * R
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=x.device)  # noqa: E731
        dQ = dq.permute(1, 0, 2, 3).reshape(N, n_out).float().contiguous()
        dh_last = dh_last.reshape(R, H).float().contiguous()
        dh_q = dQ @ W2
        dgi, dgh_n, dx1 = new(N, 3 * H), new(N, H), new(N, H)
        dh0 = new(R, H) if ctx.needs_input_grad[2] else None
        h0k, hs = h0_arg(h0, R, H)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().asg_rnn_agent_unroll_backward(
                ptr(dh_q), ptr(dh_last), ptr(save), ptr(h_all), ptr(h0k), hs, ptr(Wih), ptr(Whh), T1, R, H, n_out, 1,
                ptr(dgi), ptr(dgh_n), ptr(dx1), ptr(dh0), _lib.stream_ptr(x.device)))
        h_first = torch.zeros_like(dx1[:R]) if h0k is None else h0k.expand(R, H)
        if dh0 is not None and h0 is not None:
            dh0 = dh0.sum(0, keepdim=True).view(h0.shape) if hs == 0 else dh0.view(h0.shape)
        return (None, None, dh0, *gru_param_grads(x, h_first, save[0], h_all, dgi, dgh_n, dx1, dQ))


class _MLPUnroll(torch.autograd.Function):
    """asg_mlp_agent_unroll (ids: asg_mlp_agent_unroll_ids, the critic) under autograd: the forward
    kernel saves x1 and h of every row, asg_mlp_agent_unroll_backward takes the gradient back
    through the two ReLUs and the middle layer, and the parameter gradients are GEMMs over the
    T1 * R rows.  Returns (q [B, T1, n, n_out], h_last [R, H]); ids: q [T1, R, n_out] alone."""

    @staticmethod
    def forward(ctx, launch, ids, x, W1, b1, Wr, br, W2, b2):
        q, h_all, x1 = launch(x, W1, b1, Wr, br, W2, b2, True)
        ctx.save_for_backward(x, Wr, W2, h_all, x1)
        ctx.ids = ids
        if ids:
            return q
        B, T1, n, _ = x.shape
        return q.view(T1, B, n, -1).permute(1, 0, 2, 3), h_all[T1 - 1]

    @staticmethod
    def backward(ctx, dq, dh_last=None):
        x, Wr, W2, h_all, x1 = ctx.saved_tensors
        B, T1, n, K = x.shape
        R, H, n_out = B * n, Wr.shape[1], W2.shape[0]
        N = T1 * R
        dQ = (dq if ctx.ids else dq.permute(1, 0, 2, 3)).reshape(N, n_out).float().contiguous()
        dh_q = dQ @ W2
        if dh_last is not None:
            dh_q[N - R:] += dh_last.reshape(R, H).float()
        dh, dx1 = torch.empty_like(dh_q), torch.empty_like(dh_q)
        Wrc = Wr.detach().contiguous()
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().asg_mlp_agent_unroll_backward(
                ptr(dh_q), ptr(h_all), ptr(x1), ptr(Wrc), N, H, ptr(dh), ptr(dx1), _lib.stream_ptr(x.device)))
        return (None, None, None, *mlp_param_grads(x, x1, h_all, dh, dx1, dQ, ctx.ids))
