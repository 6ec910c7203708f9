"""Shared-parameter agent network (reference: modules/agents/rnn_agent.py:7-31):
fc1 -> ReLU -> GRUCell (use_rnn) or Linear+ReLU -> fc2, fp32, run in PyTorch-ROCm."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import _lib
from .. import unroll as U

# the unroll kernels' forward launches (modules/unroll.py); unroll() looks them up here per call
_unroll_launch = U.gru_launch
_mlp_launch = U.mlp_launch


class RNNAgent(nn.Module):
    def __init__(self, input_shape, args, n_out=None):
        super().__init__()
        self.args = args
        self.n_out = args.m if n_out is None else int(n_out)
        self.fc1 = nn.Linear(input_shape, args.hidden_dim)
        if self.args.use_rnn:
            self.rnn = nn.GRUCell(args.hidden_dim, args.hidden_dim)
        else:
            self.rnn = nn.Linear(args.hidden_dim, args.hidden_dim)
        self.fc2 = nn.Linear(args.hidden_dim, self.n_out)

    def init_hidden(self):
        return self.fc1.weight.new(1, self.args.hidden_dim).zero_()

    def forward(self, inputs, hidden_state):
        x = F.relu(self.fc1(inputs))
        h_in = hidden_state.reshape(-1, self.args.hidden_dim)
        if self.args.use_rnn:
            h = self.rnn(x, h_in)
        else:
            h = F.relu(self.rnn(x))
        q = self.fc2(h)
        return q, h

    def unroll(self, x, h0=None):
        """The agent over a whole sequence: x [B, T1, n, K] -> (q [B, T1, n, n_out], h_last
        [B * n, hidden]), T1 successive forward calls starting from h0 (None: zeros), the
        loop the reference learner runs (learners/sap_q_learner.py:69-84)."""
        return self._unroll_loop(x, h0)

    def _unroll_loop(self, x, h0=None):
        B, T1, n, K = x.shape
        H = self.args.hidden_dim
        h = self.init_hidden().expand(B * n, H) if h0 is None else h0.reshape(-1, H)
        qs = []
        for t in range(T1):
            q, h = self.forward(x[:, t].reshape(B * n, K), h)
            qs.append(q.view(B, n, -1))
        return torch.stack(qs, dim=1), h


class RNNFusedAgent(RNNAgent):
    """RNNAgent with the same parameters / state_dict, whose inference forward (no autograd:
    the rollout's action selection) is one fused HIP kernel (asg_rnn_agent_forward: f32
    MFMA, fc1 + GRUCell + fc2 with every intermediate in registers; hidden 64, any input
    size, n_out = m up to 512 -- the real envs' m = 450 included).  With autograd enabled
    (learner training) it is the plain PyTorch module, so gradients are unchanged.  unroll()
    runs a whole sequence, and its backward pass, in one launch each (asg_unroll.hip; the
    Linear agent with args.fused_linear_unroll: asg_unroll_mlp.hip)."""

    def __init__(self, input_shape, args, n_out=None):
        super().__init__(input_shape, args, n_out)
        if not self.supports(input_shape, args, self.n_out):
            raise ValueError("rnn_fused needs hidden_dim == 64 and 1 <= n_out <= 512; use agent 'rnn_torch'")

    @staticmethod
    def supports(input_shape, args, n_out):
        """Shapes the fused inference kernels take (hidden 64, 1 <= n_out <= 512, any input)."""
        return args.hidden_dim == 64 and 1 <= int(n_out) <= 512 and int(input_shape) >= 1

    def _prep(self, inputs, hidden_state):
        x = inputs
        if x.dtype != torch.float32 or x.stride(-1) != 1 or x.stride(0) < x.shape[1]:
            x = x.float().contiguous()
        H = self.args.hidden_dim
        h = hidden_state
        if h.dim() == 3 and h.stride(0) == 0 and h.stride(1) == 0 and h.stride(2) == 1:
            hs = 0  # init_hidden's expanded zero row: one row broadcast to all agents
        else:
            h = h.reshape(-1, H)
            if h.stride(-1) != 1 or h.stride(0) % 4 != 0 or h.data_ptr() % 16 != 0:
                h = h.contiguous()
            hs = h.stride(0)
        return x, h, hs

    def _common(self, x, h, hs):
        R, K = x.shape
        rnn = bool(self.args.use_rnn)
        p = U.ptr
        h_out = torch.empty((R, self.args.hidden_dim), dtype=torch.float32, device=x.device)
        args = [p(x), x.stride(0), R, K, p(h), hs, p(self._packed(K, x.device)), p(self.fc1.bias),
                p(self.rnn.bias_ih if rnn else self.rnn.bias), p(self.rnn.bias_hh) if rnn else None,
                p(self.fc2.bias), self.args.hidden_dim, self.n_out, int(rnn), p(h_out)]
        return h_out, args, p

    def forward(self, inputs, hidden_state):
        if torch.is_grad_enabled() or not inputs.is_cuda:
            return super().forward(inputs, hidden_state)
        x, h, hs = self._prep(inputs, hidden_state)
        with torch.cuda.device(x.device):
            h_out, args, p = self._common(x, h, hs)
            q = torch.empty((x.shape[0], self.n_out), dtype=torch.float32, device=x.device)
            _lib.check(_lib.lib().asg_rnn_agent_forward(*args, p(q), _lib.stream_ptr(x.device)))
        return q, h_out

    def forward_select(self, inputs, hidden_state, avail, n, epsilon, seed, counter, out, status, q_out=None,
                       env_index_base=0):
        """forward + epsilon-greedy in one kernel (asg_rnn_agent_select): actions into `out`
        ([B, n] int64 view, e.g. the EpisodeBatch actions row); avail [B, n, m] bool;
        env_index_base: global index of env 0 (exploration draws are keyed by global row).
        Returns the new hidden state [B*n, hidden]."""
        x, h, hs = self._prep(inputs, hidden_state)
        if avail.dtype != torch.bool or avail.stride(-1) != 1:
            avail = (avail != 0).contiguous()
        with torch.cuda.device(x.device):
            h_out, args, p = self._common(x, h, hs)
            _lib.check(_lib.lib().asg_rnn_agent_select(
                *args, p(q_out), p(avail), _lib.i64arr(avail.stride()[:2]), n, float(epsilon),
                seed & 0xFFFFFFFFFFFFFFFF, counter, int(env_index_base), p(out), _lib.i64arr(out.stride()), p(status),
                _lib.stream_ptr(x.device)))
        return h_out

    def step_select_args(self, hidden_state, K, device, R):
        """The agent half of asg_rollout's arguments: packed weights, biases (GRU: b_ih, b_hh;
        Linear: its bias, NULL), K, hidden, use_rnn, h_in (+ row stride), and a fresh h_out
        tensor (last)."""
        H = self.args.hidden_dim
        h = hidden_state
        if h.dim() == 3 and h.stride(0) == 0 and h.stride(1) == 0 and h.stride(2) == 1:
            hs = 0  # init_hidden's expanded zero row
        else:
            h = h.reshape(-1, H)
            if h.stride(-1) != 1 or h.stride(0) % 4 != 0 or h.data_ptr() % 16 != 0:
                h = h.contiguous()
            hs = h.stride(0)
        if hs and h.shape[0] != R:
            raise ValueError(f"hidden state has {h.shape[0]} rows, the batch {R}")
        p = U.ptr
        self._h_keep = h  # alive until the kernel has read it (stream order)
        h_out = torch.empty((R, H), dtype=torch.float32, device=device)
        rnn = bool(self.args.use_rnn)
        return [p(self._packed(K, device)), p(self.fc1.bias), p(self.rnn.bias_ih if rnn else self.rnn.bias),
                p(self.rnn.bias_hh) if rnn else None, p(self.fc2.bias), int(K), int(H), int(rnn), p(h), int(hs),
                h_out]

    def unroll(self, x, h0=None):
        """x [B, T1, n, K] (any batch / time / agent strides, contiguous K) -> (q [B, T1, n,
        n_out], h_last [B * n, hidden]).  The GRU agent on the GPU runs the whole sequence
        in one launch (asg_rnn_agent_unroll; under autograd with its one-launch backward,
        asg_rnn_agent_unroll_backward, differentiable in the eight parameter tensors and h0).  The
        Linear agent on the GPU does the same with args.fused_linear_unroll = True
        (asg_mlp_agent_unroll / asg_mlp_agent_unroll_backward over the flattened T1 * B * n rows,
        differentiable in its six parameter tensors; it ignores h0, as forward does); without
        that flag it loops the module over t, as do CPU tensors and args.unfused_unroll = True
        (the A/B switch of tools/bench_learner.py)."""
        if not (x.is_cuda and x.dim() == 4) or getattr(self.args, "unfused_unroll", False):
            return self._unroll_loop(x, h0)
        if not self.args.use_rnn:
            if not getattr(self.args, "fused_linear_unroll", False):
                return self._unroll_loop(x, h0)
            return self._unroll_linear(x)
        if x.dtype != torch.float32 or x.stride(-1) != 1:
            x = x.float().contiguous()
        x = x.detach()  # observations are data: no gradient flows into them
        B, T1, n, _ = x.shape
        ps = (self.fc1.weight, self.fc1.bias, self.rnn.weight_ih, self.rnn.weight_hh, self.rnn.bias_ih,
              self.rnn.bias_hh, self.fc2.weight, self.fc2.bias)
        if torch.is_grad_enabled() and (any(w.requires_grad for w in ps) or (h0 is not None and h0.requires_grad)):
            return U._GRUUnroll.apply(_unroll_launch, x, h0, *ps)
        q, h_all, _ = _unroll_launch(x, h0, *ps, False)
        return q.view(T1, B, n, -1).permute(1, 0, 2, 3), h_all[T1 - 1]

    def _unroll_linear(self, x):
        if x.dtype != torch.float32 or x.stride(-1) != 1:
            x = x.float().contiguous()
        x = x.detach()  # observations are data: no gradient flows into them
        B, T1, n, _ = x.shape
        ps = (self.fc1.weight, self.fc1.bias, self.rnn.weight, self.rnn.bias, self.fc2.weight, self.fc2.bias)
        if torch.is_grad_enabled() and any(w.requires_grad for w in ps):
            return U._MLPUnroll.apply(_mlp_launch, False, x, *ps)
        q, h_all, _ = _mlp_launch(x, *ps, False)
        return q.view(T1, B, n, -1).permute(1, 0, 2, 3), h_all[T1 - 1]

    def _packed(self, K, device):
        """Weights in the kernel's fragment order, re-packed only when a weight changed
        (optimizer steps bump the tensors' version counters; load_state_dict and in-place
        no_grad updates too).  A write through `.data` bumps no counter: call
        invalidate_pack() after one."""
        rnn = self.args.use_rnn
        ws = [self.fc1.weight, self.rnn.weight_ih if rnn else self.rnn.weight,
              self.rnn.weight_hh if rnn else None, self.fc2.weight]
        key = (K, str(device), tuple((w.data_ptr(), w._version) for w in ws if w is not None))
        if getattr(self, "_pack_key", None) != key:
            L = _lib.lib()
            nbytes = L.asg_rnn_agent_packed_size(K, self.args.hidden_dim, self.n_out, int(bool(rnn)))
            _lib.check(int(nbytes) if nbytes < 0 else 0)
            buf = torch.empty(int(nbytes) // 4, dtype=torch.float32, device=device)
            p = U.ptr
            _lib.check(L.asg_rnn_agent_pack(p(ws[0]), p(ws[1]), p(ws[2]), p(ws[3]), K, self.args.hidden_dim,
                                            self.n_out, int(bool(rnn)), p(buf), _lib.stream_ptr(device)))
            self._pack_buf, self._pack_key = buf, key
        return self._pack_buf

    def invalidate_pack(self):
        """Forget the packed weights: the next inference call packs them again.  Needed only
        after a weight was written behind autograd's back (`w.data.mul_(..)`, a raw-pointer
        copy), which leaves (data_ptr, _version) as they were."""
        self._pack_key = None


class FlatConstAgent(RNNAgent):
    """FlatConstellationAgent (reference: modules/agents/flat_const_agent.py:9-34): the
    RNNAgent network with M + 1 outputs (one per top-M task and the baseline), the agent of
    the filtered real-env algorithms (filtered_reda.yaml, iql_sap.yaml)."""

    def __init__(self, input_shape, args):
        super().__init__(input_shape, args, n_out=int(args.env_args["M"]) + 1)


class FlatConstFusedAgent(RNNFusedAgent):
    """FlatConstAgent whose no-grad rollout forward is the fused HIP kernel."""

    def __init__(self, input_shape, args):
        super().__init__(input_shape, args, n_out=int(args.env_args["M"]) + 1)
