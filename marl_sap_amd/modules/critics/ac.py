"""ACCritic (reference: modules/critics/ac.py:6-50): fc1 -> ReLU -> fc2 -> ReLU -> fc3 on
[obs, eye(n)], one value per agent -- or, with bids_as_actions, one per task -- for every row of
a batch; the critic of ippo_sap.yaml (critic_type: "ac_critic").

The network has the Linear agent's shape, and its agent-id inputs are a column gather of
fc1.weight: x1 = relu(W1[:, :K] obs + W1[:, K + agent] + b1).  On a GPU (hidden 64, 1 <= n_out
<= 512, args.fused_ppo not False) the forward over all rows is one launch of
asg_mlp_agent_unroll_ids and the sequential part of its backward pass one launch of
asg_mlp_agent_unroll_backward; the [obs, eye(n)] concatenation -- a copy of the whole observation
buffer -- is never built.  Elsewhere it is the plain PyTorch module."""
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import unroll as U


# one asg_mlp_agent_unroll_ids launch (modules/unroll.py); _rows_fused looks it up here per call
_ids_launch = functools.partial(U.mlp_launch, ids=True)


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
            return U._MLPUnroll.apply(_ids_launch, True, x, *ps)
        return _ids_launch(x, *ps, False)[0]

    def _get_input_shape(self, scheme):
        return scheme["obs"]["vshape"] + self.n  # observations + the agent id
