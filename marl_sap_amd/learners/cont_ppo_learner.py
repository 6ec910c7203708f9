"""ContinuousPPOLearner: the training step of ippo_sap.yaml (reference: learners/
cont_ppo_learner.py:13-225) -- PPO on bids_as_actions episodes with a fixed-variance Gaussian
policy around the agent's outputs and an ACCritic -- with everything on the device.

train() follows the reference line by line: reward standardisation, the mask, the old policy's
log-probabilities, then per epoch the live policy on rows 0..T-1, one critic update
(train_critic_sequential: target values, n-step returns, the masked L2 loss, clipping, Adam)
whose masked TD error is the epoch's advantage, the clipped surrogate, clipping, Adam; then the
old-policy sync, the hard / soft target-critic update, the selector-agent sync and the stats.

On the GPU (args.fused_ppo, default True) the step runs in the unroll kernels' time-major row
order with these substitutions, which keep its results:

  * the 1 + epochs loops of mac.forward are agent.unroll (one launch for the fused agents; the
    raw logits are taken, the pi_logits softmax lives in the loss kernels);
  * the critic's forward and the sequential part of its backward are one launch each
    (asg_mlp_agent_unroll_ids, modules/critics/ac.py);
  * nstep_returns' T x (q_nstep + 1) small tensor ops are asg_nstep_returns;
  * the Gaussian log-probabilities, the ratio, the clipped surrogate and its gradient are
    asg_bids_log_prob (once, the old policy) and asg_ppo_bids_loss (once per epoch).

fused_ppo = False, or CPU tensors, runs the same step in plain PyTorch.  The agent unroll obeys
fused_linear_unroll / unfused_unroll as in the other learners.

The reference's old_mac is a deep copy taken at construction that never selects an action, so
its selector's `variance` stays what it was then while the live selector's follows its schedule:
old_variance is recorded here and used for the old log-probabilities.
"""
import copy

import torch
from torch.optim import Adam

from ..components.standarize_stream import RunningMeanStd
from ..modules.critics import REGISTRY as critic_REGISTRY
from . import ppo_kernels

CRITIC_STATS = ("critic_loss", "critic_grad_norm", "td_error_abs", "q_taken_mean", "target_mean")


class ContinuousPPOLearner:
    def __init__(self, mac, scheme, logger, args):
        self.args = args
        self.n = args.n
        self.m = args.m
        self.logger = logger
        if not getattr(args, "env_args", {}).get("bids_as_actions", False):
            raise ValueError("cont_ppo_learner needs a bids_as_actions env: its mask, rewards and critic values "
                             "are broadcast against the [B, T, n, m] bids")
        critic_type = getattr(args, "critic_type", None)
        if critic_type not in critic_REGISTRY:
            raise ValueError("Critic {} is not supported: the critics registry has {}"
                             .format(critic_type, sorted(critic_REGISTRY)))

        self.mac = mac
        # the old policy: a second controller over a copy of the agent (the reference deep-copies
        # the whole MAC; the selector and its env handles are not needed twice)
        self.old_mac = copy.copy(mac)
        self.old_mac.agent = copy.deepcopy(mac.agent)
        self.old_mac.selector_agent = self.old_mac.agent
        self.old_mac.hidden_states = None
        self.old_variance = mac.action_selector.variance
        self.agent_params = list(mac.parameters())
        self.agent_optimiser = Adam(params=self.agent_params, lr=args.lr)

        device = self.agent_params[0].device
        self.critic = critic_REGISTRY[critic_type](scheme, args).to(device)
        self.target_critic = copy.deepcopy(self.critic)
        self.critic_params = list(self.critic.parameters())
        self.critic_optimiser = Adam(params=self.critic_params, lr=args.lr)

        self.last_target_update_step = 0
        self.critic_training_steps = 0
        self.log_stats_t = -self.args.learner_log_interval - 1
        if getattr(self.args, "standardise_returns", False):
            self.ret_ms = RunningMeanStd(shape=(self.n,), device=device)
        if getattr(self.args, "standardise_rewards", False):
            self.rew_ms = RunningMeanStd(shape=(self.n,), device=device)

    def train(self, batch, t_env, episode_num):
        rewards = batch["rewards"][:, :-1].float()
        actions = batch["actions"][:, :-1]
        terminated = batch["terminated"][:, :-1].float()
        mask = batch["filled"][:, :-1].float()
        mask[:, 1:] = mask[:, 1:] * (1 - terminated[:, :-1])
        if getattr(self.args, "standardise_rewards", False):
            self.rew_ms.update(rewards)
            rewards = (rewards - self.rew_ms.mean) / torch.sqrt(self.rew_ms.var)
        log = t_env - self.log_stats_t >= self.args.learner_log_interval

        step = self._epochs_fused if self._fused(batch) else self._epochs_torch
        pg_loss, grad_norm, critic_stats, extra = step(batch, rewards, actions, mask, log)

        self.old_mac.load_state(self.mac)

        self.critic_training_steps += 1
        tau = self.args.target_update_interval_or_tau
        if tau > 1 and (self.critic_training_steps - self.last_target_update_step) / tau >= 1.0:
            self._update_targets_hard()
            self.last_target_update_step = self.critic_training_steps
        elif tau <= 1.0:
            self._update_targets_soft(tau)

        if not getattr(self.args, "use_mps_action_selection", False):
            self.mac.update_action_selector_agent()

        if log:
            ts_logged = len(critic_stats["critic_loss"])
            for key in CRITIC_STATS:
                self.logger.log_stat(key, sum(v.item() for v in critic_stats[key]) / ts_logged, t_env)
            self.logger.log_stat("advantage_mean", extra["advantage_mean"].item(), t_env)
            self.logger.log_stat("pg_loss", pg_loss.item(), t_env)
            self.logger.log_stat("agent_grad_norm", grad_norm.item(), t_env)
            self.logger.log_stat("max bid", extra["max_bid"].item(), t_env)
            self.log_stats_t = t_env
        self.critic_loss = critic_stats["critic_loss"][-1]
        return pg_loss.detach()

    def _fused(self, batch):
        return batch["obs"].is_cuda and getattr(self.args, "fused_ppo", True) is not False

    # ---- the reference's formulation in plain PyTorch ------------------------------------------
    def _epochs_torch(self, batch, rewards, actions, mask, log):
        T = batch.max_seq_length - 1
        # expand mask and rewards to match the bids
        mask = mask.unsqueeze(-1).repeat(1, 1, self.n, self.m)
        rewards = rewards.unsqueeze(-1).repeat(1, 1, 1, self.m)
        critic_mask = mask.clone()
        actions = actions.float()

        with torch.no_grad():
            old_pi = self.old_mac.forward_sequence(batch, rows=T).masked_fill(mask == 0, 1.0)
            # action_log_prob(pi, actions): the reference swaps the arguments, the density is symmetric
            old_log_pi_taken = torch.distributions.Normal(actions, self.old_variance).log_prob(old_pi)

        critic_stats = {k: [] for k in CRITIC_STATS}
        for _ in range(self.args.epochs):
            pi = self.mac.forward_sequence(batch, rows=T)
            advantages = self.train_critic_sequential(self.critic, self.target_critic, batch, rewards, critic_mask,
                                                      critic_stats).detach()
            pi = pi.masked_fill(mask == 0, 1.0)
            log_pi_taken = torch.distributions.Normal(actions, self.mac.action_selector.variance).log_prob(pi)

            ratios = torch.exp(log_pi_taken - old_log_pi_taken.detach())
            surr1 = ratios * advantages
            surr2 = torch.clamp(ratios, 1 - self.args.eps_clip, 1 + self.args.eps_clip) * advantages
            # no entropy term: the policy's variance is fixed and decays like epsilon
            pg_loss = -(torch.min(surr1, surr2) * mask).sum() / mask.sum()

            self.agent_optimiser.zero_grad()
            pg_loss.backward()
            grad_norm = self._clip_agent_grads()
            self.agent_optimiser.step()

        extra = {}
        if log:
            extra["advantage_mean"] = (advantages * mask).sum() / mask.sum()
            extra["max_bid"] = (pi.detach().max(dim=-1)[0] * mask[:, :, :, 0]).sum() / mask[:, :, :, 0].sum()
        return pg_loss, grad_norm, critic_stats, extra

    def train_critic_sequential(self, critic, target_critic, batch, rewards, mask, running_log):
        with torch.no_grad():
            target_vals = target_critic(batch)
            target_vals = target_vals.squeeze(3)
        if getattr(self.args, "standardise_returns", False):
            target_vals = target_vals * torch.sqrt(self.ret_ms.var) + self.ret_ms.mean

        target_returns = self.nstep_returns(rewards, mask, target_vals, self.args.q_nstep)
        if getattr(self.args, "standardise_returns", False):
            self.ret_ms.update(target_returns)
            target_returns = (target_returns - self.ret_ms.mean) / torch.sqrt(self.ret_ms.var)

        v = critic(batch)[:, :-1].squeeze(3)
        td_error = target_returns.detach() - v
        masked_td_error = td_error * mask
        mask_elems = mask.sum()
        loss = (masked_td_error ** 2).sum() / mask_elems
        self._critic_step(loss, running_log)
        with torch.no_grad():
            running_log["td_error_abs"].append(masked_td_error.abs().sum() / mask_elems)
            running_log["q_taken_mean"].append((v * mask).sum() / mask_elems)
            running_log["target_mean"].append((target_returns * mask).sum() / mask_elems)
        return masked_td_error

    def _critic_step(self, loss, running_log):
        self.critic_optimiser.zero_grad()
        loss.backward()
        grad_norm = self._clip_critic_grads()
        self.critic_optimiser.step()
        running_log["critic_loss"].append(loss.detach())
        running_log["critic_grad_norm"].append(grad_norm)

    def nstep_returns(self, rewards, mask, values, nsteps):
        nstep_values = torch.zeros_like(values[:, :-1])
        for t_start in range(rewards.size(1)):
            nstep_return_t = torch.zeros_like(values[:, 0])
            for step in range(nsteps + 1):
                t = t_start + step
                if t >= rewards.size(1):
                    break
                elif step == nsteps:
                    nstep_return_t += self.args.gamma ** (step) * values[:, t] * mask[:, t]
                elif t == rewards.size(1) - 1 and self.args.add_value_last_step:
                    nstep_return_t += self.args.gamma ** (step) * rewards[:, t] * mask[:, t]
                    nstep_return_t += self.args.gamma ** (step + 1) * values[:, t + 1]
                else:
                    nstep_return_t += self.args.gamma ** (step) * rewards[:, t] * mask[:, t]
            nstep_values[:, t_start, :] = nstep_return_t
        return nstep_values

    # ---- the same step on the kernels, in the time-major row order [T, B n, m] ------------------
    def _logits_rows(self, mac, x):
        """The agent's raw outputs on x [B, T, n, K] as [T, B n, m]: a view of what the unroll
        kernels wrote (no softmax: the loss kernels apply it)."""
        B, T = x.shape[0], x.shape[1]
        mac.init_hidden(B)
        q, mac.hidden_states = mac.agent.unroll(x, None)
        return q.permute(1, 0, 2, 3).reshape(T, B * self.n, -1)

    def _epochs_fused(self, batch, rewards, actions, mask, log):
        B, T, n, m = batch.batch_size, batch.max_seq_length - 1, self.n, self.m
        mask = mask.reshape(B, T)
        mask_rows = mask.t().reshape(T, B, 1, 1)
        count = mask.sum() * (n * m)  # mask.sum() over the expanded [B, T, n, m] mask
        inv_count = (1.0 / count).reshape(1)
        row_softmax = self.mac.agent_output_type == "pi_logits"
        x = self.mac._build_sequence_inputs(batch)[:, :T]

        with torch.no_grad():
            old_log_pi_taken = ppo_kernels.bids_log_prob(self._logits_rows(self.old_mac, x), actions, mask, n,
                                                         self.old_variance, row_softmax)

        critic_stats = {k: [] for k in CRITIC_STATS}
        for k in range(self.args.epochs):
            logits = self._logits_rows(self.mac, x)
            advantages = self._train_critic_rows(batch, rewards, mask, mask_rows, count, critic_stats)
            pg_loss, row_max = ppo_kernels.ppo_bids_loss(
                logits, actions, old_log_pi_taken, advantages, mask, inv_count, n, self.mac.action_selector.variance,
                self.args.eps_clip, row_softmax, want_max=log and k == self.args.epochs - 1)

            self.agent_optimiser.zero_grad()
            pg_loss.backward()
            grad_norm = self._clip_agent_grads()
            self.agent_optimiser.step()

        extra = {}
        if log:
            # advantages are the masked TD error: zero where the mask is
            extra["advantage_mean"] = advantages.sum() / count
            extra["max_bid"] = (row_max.view(T, B, n) * mask_rows[..., 0]).sum() / (mask.sum() * n)
        return pg_loss, grad_norm, critic_stats, extra

    def _train_critic_rows(self, batch, rewards, mask, mask_rows, count, running_log):
        """train_critic_sequential on [T, B n, m] rows: returns the masked TD error, detached."""
        B, T, n, m = batch.batch_size, batch.max_seq_length - 1, self.n, self.m
        with torch.no_grad():
            target_vals = self.target_critic.rows(batch)
        if getattr(self.args, "standardise_returns", False):
            target_vals = target_vals * torch.sqrt(self.ret_ms.var) + self.ret_ms.mean

        target_returns = ppo_kernels.nstep_returns(target_vals, rewards, mask, n, self.args.gamma, self.args.q_nstep,
                                                   self.args.add_value_last_step)
        if getattr(self.args, "standardise_returns", False):
            self.ret_ms.update(target_returns)
            target_returns = (target_returns - self.ret_ms.mean) / torch.sqrt(self.ret_ms.var)

        v = self.critic.rows(batch)[:T]
        td_error = target_returns.detach() - v
        masked_td_error = td_error.view(T, B, n, m) * mask_rows
        loss = (masked_td_error ** 2).sum() / count
        self._critic_step(loss, running_log)
        with torch.no_grad():
            running_log["td_error_abs"].append(masked_td_error.abs().sum() / count)
            running_log["q_taken_mean"].append((v.view(T, B, n, m) * mask_rows).sum() / count)
            running_log["target_mean"].append((target_returns.view(T, B, n, m) * mask_rows).sum() / count)
        return masked_td_error.detach().reshape(T, B * n, m)

    # ---- hooks, target updates, device, model files ---------------------------------------------
    def _clip_agent_grads(self):
        return torch.nn.utils.clip_grad_norm_(self.agent_params, self.args.grad_norm_clip)

    def _clip_critic_grads(self):
        return torch.nn.utils.clip_grad_norm_(self.critic_params, self.args.grad_norm_clip)

    def _update_targets_hard(self):
        self.target_critic.load_state_dict(self.critic.state_dict())

    def _update_targets_soft(self, tau):
        """target = target * (1 - tau) + param * tau (reference :200-202), written into the
        parameter tensors under no_grad, as SAPQLearner does, so their version counters move."""
        tps, ps = list(self.target_critic.parameters()), list(self.critic.parameters())
        with torch.no_grad():
            new = torch._foreach_mul(tps, 1.0 - tau)
            torch._foreach_add_(new, torch._foreach_mul(ps, tau))
            for tp, v in zip(tps, new):
                tp.copy_(v)

    def cuda(self):
        self.old_mac.cuda()
        self.mac.cuda()
        self.critic.cuda()
        self.target_critic.cuda()
        dev = next(iter(self.mac.parameters())).device
        for ms in (getattr(self, "ret_ms", None), getattr(self, "rew_ms", None)):
            if ms is not None:
                ms.mean, ms.var = ms.mean.to(dev), ms.var.to(dev)

    def save_models(self, path):
        self.mac.save_models(path)
        torch.save(self.critic.state_dict(), "{}/critic.th".format(path))
        torch.save(self.agent_optimiser.state_dict(), "{}/agent_opt.th".format(path))
        torch.save(self.critic_optimiser.state_dict(), "{}/critic_opt.th".format(path))

    def load_models(self, path):
        self.mac.load_models(path)
        load = lambda name: torch.load("{}/{}".format(path, name), map_location=lambda s, loc: s,  # noqa: E731
                                       weights_only=True)
        self.critic.load_state_dict(load("critic.th"))
        # not quite right, but the reference does not save target networks either
        self.target_critic.load_state_dict(self.critic.state_dict())
        self.agent_optimiser.load_state_dict(load("agent_opt.th"))
        self.critic_optimiser.load_state_dict(load("critic_opt.th"))
