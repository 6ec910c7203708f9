"""ACCritic (reference: modules/critics/ac.py:6-50): fc1 -> ReLU -> fc2 -> ReLU -> fc3 on
[obs, eye(n)], one value per agent -- or, with bids_as_actions, one per task -- for every row of
a batch; the critic of ippo_sap.yaml (critic_type: "ac_critic").

The network has the Linear agent's shape, and its agent-id inputs are a column gather of
fc1.weight: x1 = relu(W1[:, :K] obs + W1[:, K + agent] + b1).  On a GPU (hidden 64, 1 <= n_out
<= 512, args.fused_ppo not False) the forward over all rows is one launch of
asg_mlp_agent_unroll_ids and the sequential part of its backward pass one launch of
asg_mlp_agent_unroll_backward; the [obs, eye(n)] concatenation -- a copy of the whole observation
buffer -- is never built.  Elsewhere it is the plain PyTorch module."""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import _lib


class _MLPUnrollIds(torch.autograd.Function):
    """asg_mlp_agent_unroll_ids under autograd, _MLPUnroll with the agent-id block of W1: the
    forward kernel saves x1 and h of every row, asg_mlp_agent_unroll_backward takes the gradient
    back through the two ReLUs and the middle layer, and the parameter gradients are GEMMs over
    the T1 * R rows (the id block's: the per-agent sums of dx1).  Returns q [T1, R, n_out]."""

    @staticmethod
    def forward(ctx, x, W1, b1, Wr, br, W2, b2):
        q, h_all, x1 = _ids_launch(x, W1, b1, Wr, br, W2, b2, True)
        ctx.save_for_backward(x, Wr, W2, h_all, x1)
        return q

    @staticmethod
    def backward(ctx, dq):
        x, Wr, W2, h_all, x1 = ctx.saved_tensors
        B, T1, n, K = x.shape
        R, H, n_out = B * n, Wr.shape[1], W2.shape[0]
        N = T1 * R
        dev = x.device
        dQ = dq.reshape(N, n_out).float().contiguous()
        dh_q = dQ @ W2
        dh = torch.empty((N, H), dtype=torch.float32, device=dev)
        dx1 = torch.empty((N, H), dtype=torch.float32, device=dev)
        Wrc = Wr.detach().contiguous()
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().asg_mlp_agent_unroll_backward(
                p(dh_q), p(h_all), p(x1), p(Wrc), N, H, p(dh), p(dx1), _lib.stream_ptr(dev)))
        xf = x.permute(1, 0, 2, 3).reshape(N, K)
        dW1 = torch.cat([dx1.t() @ xf, dx1.view(T1, B, n, H).sum((0, 1)).t()], dim=1)
        return (None, dW1, dx1.sum(0), dh.t() @ x1.view(N, H), dh.sum(0), dQ.t() @ h_all.view(N, H), dQ.sum(0))


def _ids_launch(x, W1, b1, Wr, br, W2, b2, save):
    """One asg_mlp_agent_unroll_ids launch on x [B, T1, n, K] (any batch / time / agent strides):
    q [T1, R, n_out], h [T1, R, 64] and, with save, x1 [T1, R, 64]."""
    B, T1, n, K = x.shape
    R, H, n_out = B * n, Wr.shape[1], W2.shape[0]
    dev = x.device
    q = torch.empty((T1, R, n_out), dtype=torch.float32, device=dev)
    h_all = torch.empty((T1, R, H), dtype=torch.float32, device=dev)
    x1 = torch.empty((T1, R, H), dtype=torch.float32, device=dev) if save else None
    ws = [t.detach().contiguous() for t in (W1, Wr, W2, b1, br, b2)]
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().asg_mlp_agent_unroll_ids(
            p(x), _lib.i64arr([x.stride(1), x.stride(0), x.stride(2)]), T1, B, n, K, *[p(w) for w in ws], H, n_out,
            p(q), p(h_all), p(x1), _lib.stream_ptr(dev)))
    return q, h_all, x1


class ACCritic(nn.Module):
    def __init__(self, scheme, args):
        super().__init__()
        self.args = args
        self.m = args.m
        self.n = args.n
        input_shape = self._get_input_shape(scheme)
        self.output_type = "v"
        self.fc1 = nn.Linear(input_shape, args.hidden_dim)
        self.fc2 = nn.Linear(args.hidden_dim, args.hidden_dim)
        self.n_out = args.m if args.env_args.get("bids_as_actions", False) else 1
        self.fc3 = nn.Linear(args.hidden_dim, self.n_out)

    def forward(self, batch, t=None):
        """[B, T1, n, n_out] over every row of the batch, or [B, 1, n, n_out] at row t."""
        ts = slice(None) if t is None else slice(t, t + 1)
        obs = batch["obs"][:, ts]
        if self._fused(obs):
            B, T1 = obs.shape[0], obs.shape[1]
            return self._rows_fused(obs).view(T1, B, self.n, self.n_out).permute(1, 0, 2, 3)
        return self._module(obs)

    def rows(self, batch):
        """forward(batch) in the unroll kernels' flattened time-major order: [T1, B * n, n_out],
        the layout the loss-side kernels (asg_ppo.hip) work in."""
        obs = batch["obs"]
        if self._fused(obs):
            return self._rows_fused(obs)
        B, T1 = obs.shape[0], obs.shape[1]
        return self._module(obs).permute(1, 0, 2, 3).reshape(T1, B * self.n, self.n_out)

    def fused_ok(self):
        """The shapes asg_mlp_agent_unroll_ids takes, and the A/B switch."""
        return (self.args.hidden_dim == 64 and 1 <= self.n_out <= 512
                and getattr(self.args, "fused_ppo", True) is not False)

    def _fused(self, obs):
        return obs.is_cuda and self.fused_ok()

    def _module(self, obs):
        bs, max_t = obs.shape[0], obs.shape[1]
        eye = torch.eye(self.n, device=obs.device).unsqueeze(0).unsqueeze(0).expand(bs, max_t, -1, -1)
        inputs = torch.cat([obs.reshape(bs, max_t, self.n, -1).float(), eye], dim=-1)
        x = F.relu(self.fc1(inputs))
        x = F.relu(self.fc2(x))
        return self.fc3(x)

    def _rows_fused(self, obs):
        x = obs.reshape(obs.shape[0], obs.shape[1], self.n, -1)
        if x.dtype != torch.float32 or x.stride(-1) != 1:
            x = x.float().contiguous()
        x = x.detach()  # observations are data: no gradient flows into them
        ps = (self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias, self.fc3.weight, self.fc3.bias)
        if torch.is_grad_enabled() and any(w.requires_grad for w in ps):
            return _MLPUnrollIds.apply(x, *ps)
        return _ids_launch(x, *ps, False)[0]

    def _get_input_shape(self, scheme):
        return scheme["obs"]["vshape"] + self.n  # observations + the agent id
