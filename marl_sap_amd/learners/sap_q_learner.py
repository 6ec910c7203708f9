"""SAPQLearner: the training step of REDA (reference: learners/sap_q_learner.py:11-241,
mock_constellation_reda.yaml), with everything on the device.

train() follows the reference line by line -- reward standardisation, the live and target
unrolls, the -9999 mask, double-Q SAP targets, return standardisation, the 1-step target, the
masked L2 loss, gradient clipping, Adam, hard / soft target updates, the selector-agent sync
and the logged stats -- with three substitutions that keep its results:

  * the two loops of mac.forward over the T + 1 rows are BasicMAC.forward_sequence, one launch
    for the fused GRU agent and one more for its backward pass (asg_unroll.hip);
  * the scipy loop over (episode, t) is sap_target_max_qvals (one batched LSA launch);
  * calc_conflicting_actions / calc_raw_benefits are tensor expressions, where the reference
    runs triple Python loops with .item().

Only mixer = None (REDA's setting) is ported.
"""
import copy

import torch
from torch.optim import Adam

from ..components.standarize_stream import RunningMeanStd
from .sap_targets import sap_target_max_qvals


class SAPQLearner:
    def __init__(self, mac, scheme, logger, args):
        self.args = args
        self.mac = mac
        self.logger = logger
        if getattr(args, "mixer", None) is not None:
            raise ValueError("Mixer {} is not supported: {} is ported for mixer = None only"
                             .format(args.mixer, type(self).__name__))
        self.mixer = None
        self.params = list(mac.parameters())
        self.last_target_update_episode = 0
        self.optimiser = Adam(params=self.params, lr=args.lr)

        # the target network: a second controller over a copy of the agent (the reference
        # deep-copies the whole MAC; the selector and its env handles are not needed twice)
        self.target_mac = copy.copy(mac)
        self.target_mac.agent = copy.deepcopy(mac.agent)
        self.target_mac.selector_agent = self.target_mac.agent
        self.target_mac.hidden_states = None

        self.training_steps = 0
        self.last_target_update_step = 0
        self.log_stats_t = -self.args.learner_log_interval - 1
        self.n = args.n
        self.m = args.m
        device = self.params[0].device
        if getattr(self.args, "standardise_returns", False):
            self.ret_ms = RunningMeanStd(shape=(self.n,), device=device)
        if getattr(self.args, "standardise_rewards", False):
            self.rew_ms = RunningMeanStd(shape=(self.n,), device=device)

    def train(self, batch, t_env, episode_num):
        rewards = batch["rewards"][:, :-1].float()
        actions = batch["actions"][:, :-1].to(torch.int64)
        terminated = batch["terminated"][:, :-1].float()
        mask = batch["filled"][:, :-1].float()
        mask[:, 1:] = mask[:, 1:] * (1 - terminated[:, :-1])
        avail_actions = batch["avail_actions"]

        if getattr(self.args, "standardise_rewards", False):
            self.rew_ms.update(rewards)
            rewards = (rewards - self.rew_ms.mean) / torch.sqrt(self.rew_ms.var)

        # estimated Q-values of every row, and those of the actions taken
        mac_out = self.mac.forward_sequence(batch)
        chosen_action_qvals = torch.gather(mac_out[:, :-1], dim=3, index=actions).squeeze(3)

        # target-network Q-values (the first row is not needed for targets)
        with torch.no_grad():
            target_mac_out = self.target_mac.forward_sequence(batch)[:, 1:]
            target_max_qvals = self._target_max_qvals(target_mac_out, avail_actions, mac_out)

            if getattr(self.args, "standardise_returns", False):
                target_max_qvals = target_max_qvals * torch.sqrt(self.ret_ms.var) + self.ret_ms.mean

            # 1-step Q-learning targets
            targets = rewards + self.args.gamma * (1 - terminated) * target_max_qvals

            if getattr(self.args, "standardise_returns", False):
                self.ret_ms.update(targets)
                targets = (targets - self.ret_ms.mean) / torch.sqrt(self.ret_ms.var)

        td_error = chosen_action_qvals - targets
        mask = mask.expand_as(td_error)
        masked_td_error = td_error * mask  # 0-out the targets that came from padded data
        loss = (masked_td_error ** 2).sum() / mask.sum()

        self.optimiser.zero_grad()
        loss.backward()
        grad_norm = self._clip_grads()
        self.optimiser.step()

        self.training_steps += 1
        tau = self.args.target_update_interval_or_tau
        if tau > 1 and (self.training_steps - self.last_target_update_step) / tau >= 1.0:
            self._update_targets_hard()
            self.last_target_update_step = self.training_steps
        elif tau <= 1.0:
            self._update_targets_soft(tau)

        if not getattr(self.args, "use_mps_action_selection", False):
            self.mac.update_action_selector_agent()

        if t_env - self.log_stats_t >= self.args.learner_log_interval:
            self.logger.log_stat("loss", loss.item(), t_env)
            self.logger.log_stat("grad_norm", grad_norm.item(), t_env)
            mask_elems = mask.sum().item()
            self.logger.log_stat("td_error_abs", (masked_td_error.abs().sum().item() / mask_elems), t_env)
            self.logger.log_stat("q_taken_mean", (chosen_action_qvals * mask).sum().item() / (mask_elems * self.args.n),
                                 t_env)
            self.logger.log_stat("target_mean", (targets * mask).sum().item() / (mask_elems * self.args.n), t_env)
            self.log_stats_t = t_env
            self.logger.log_stat("avg_num_conflicts", self.calc_conflicting_actions(actions), t_env)
            self.logger.log_stat("avg_beta", self.calc_raw_benefits(batch["beta"], actions), t_env)
        return loss.detach()

    def _target_max_qvals(self, target_mac_out, avail_actions, mac_out):
        """The target network's value of the next row, [B, T, n], from target_mac_out [B, T, n, m]
        (rows 1..T), avail_actions and the live mac_out [B, T + 1, n, m]: unavailable actions at
        -9999, then the SAP maximum -- the assignment of the target Q (or, double_q, of the live
        Q) per (episode, t), and the target Q it picks."""
        return sap_target_max_qvals(target_mac_out, avail_actions, mac_out, double_q=bool(self.args.double_q),
                                    mask_value=-9999.0)

    def _clip_grads(self):
        return torch.nn.utils.clip_grad_norm_(self.params, self.args.grad_norm_clip)

    def calc_conflicting_actions(self, actions):
        """Agents beyond the first on a task, per (episode, step) on average (reference
        :167-181): one scatter-add of the task counts instead of the loops."""
        B, T = actions.shape[0], actions.shape[1]
        idx = actions[..., 0].to(torch.int64)
        counts = torch.zeros((B, T, self.m), dtype=torch.float64, device=actions.device)
        counts.scatter_add_(2, idx, torch.ones(idx.shape, dtype=torch.float64, device=actions.device))
        return torch.where(counts > 0, counts - 1, torch.zeros_like(counts)).sum().item() / B / T

    def calc_raw_benefits(self, beta, actions):
        """Mean benefit of the chosen (agent, task) pairs (reference :183-201): one gather."""
        if beta.dim() == 5:
            beta = beta[..., 0]
        elif beta.dim() != 4:
            raise ValueError("beta has unexpected shape.")
        B, T = actions.shape[0], actions.shape[1]
        picked = torch.gather(beta[:, :T], 3, actions.to(torch.int64))
        return picked.sum(dtype=torch.float64).item() / B / T / self.n

    def _update_targets_hard(self):
        self.target_mac.load_state(self.mac)  # load_state_dict: in-place copies, versions bump

    def _update_targets_soft(self, tau):
        """target = target * (1 - tau) + param * tau (reference :208-213), written into the
        parameter tensors themselves under no_grad, not through .data: the in-place copy bumps
        their version counters, which is what tells the fused agent to re-pack its weights."""
        tps, ps = list(self.target_mac.parameters()), list(self.mac.parameters())
        with torch.no_grad():
            new = torch._foreach_mul(tps, 1.0 - tau)
            torch._foreach_add_(new, torch._foreach_mul(ps, tau))
            for tp, v in zip(tps, new):
                tp.copy_(v)

    def cuda(self):
        self.mac.cuda()
        self.target_mac.cuda()
        dev = next(iter(self.mac.parameters())).device
        for ms in (getattr(self, "ret_ms", None), getattr(self, "rew_ms", None)):
            if ms is not None:
                ms.mean, ms.var = ms.mean.to(dev), ms.var.to(dev)

    def save_models(self, path):
        self.mac.save_models(path)
        torch.save(self.optimiser.state_dict(), "{}/opt.th".format(path))

    def load_models(self, path):
        self.mac.load_models(path)
        # not quite right, but the reference does not save target networks either
        self.target_mac.load_models(path)
        self.optimiser.load_state_dict(torch.load("{}/opt.th".format(path), map_location=lambda s, loc: s,
                                                  weights_only=True))
