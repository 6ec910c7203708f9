"""Shared by tests/test_ppo_host.py, tests/test_gpu_ppo_kernels.py and
tests/test_gpu_cont_ppo_learner.py: a restatement of the reference's learners/
cont_ppo_learner.py:48-192 and modules/critics/ac.py on the CPU in a given dtype -- the per-step
loop over the PyTorch agent, the materialised [obs, eye(n)] critic input, the Python n-step
loop, torch.distributions.Normal, th.min / th.clamp, RunningMeanStd, clipping, the two Adams,
the old-policy sync and the hard / soft target-critic update -- with a seeded synthetic bids
batch, and the loss-side expressions on their own for the kernel tests.  Tolerance: the project's
rule, tests/q_learner_ref.within (at most 4 x the float32 restatement's error against float64,
plus 1e-7 max|reference|)."""
import math
from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.nn.functional as F

from marl_sap_amd.components import EpisodeBatch
from marl_sap_amd.modules.agents import RNNAgent
from tests.q_learner_ref import _RMS, Logger, within  # noqa: F401

B, T, N, M, OBS = 4, 5, 4, 6, 10
# with this seed the float64 and the float32 restatement take the same clip branch at every
# element of every epoch of both steps, for every case: the tests assert it.  (Seeds 1 and 2 meet
# that too, but each leaves one comparison ill-conditioned on the CPU already, where only the
# RunningMeanStd update differs from the float32 restatement: seed 1 a weight entry with a gradient
# near zero, where Adam's normalised step turns a last-bit difference into 5e-7; seed 2 a policy
# loss that the float32 restatement happens to hit to a quarter ulp.)
SEED = 3
SIGMA_OLD, SIGMA_NEW = 0.3, 0.2
STATS = {"critic_loss", "critic_grad_norm", "td_error_abs", "q_taken_mean", "target_mean", "advantage_mean",
         "pg_loss", "agent_grad_norm", "max bid"}
# (target_update_interval_or_tau, q_nstep, use_rnn)
CASES = [(0.01, 5, False), (2, 5, False), (0.01, 1, False), (0.01, 5, True)]


def make_args(tau=0.01, q_nstep=5, use_rnn=False, **kw):
    a = SimpleNamespace(
        n=N, m=M, agent="rnn", hidden_dim=64, use_rnn=use_rnn, obs_last_action=False, obs_agent_id=False,
        agent_output_type="pi_logits", action_selector="continuous", softmax_agent_inputs=True,
        epsilon_start=SIGMA_OLD, epsilon_finish=0.05, epsilon_anneal_time=50000, evaluation_epsilon=0.0,
        env_args=dict(n=N, m=M, T=T, L=3, lambda_=0.5, bids_as_actions=True), critic_type="ac_critic", lr=1e-3,
        gamma=0.99, grad_norm_clip=10.0, eps_clip=0.2, epochs=4, q_nstep=q_nstep, add_value_last_step=True,
        target_update_interval_or_tau=tau, standardise_rewards=True, standardise_returns=False,
        learner_log_interval=0, use_mps_action_selection=False)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def make_scheme(n=N, m=M, obs=OBS):
    return {"obs": {"vshape": obs, "group": "agents"},
            "actions": {"vshape": (m,), "group": "agents", "dtype": torch.float32},
            "avail_actions": {"vshape": (m,), "group": "agents", "dtype": torch.int},
            "rewards": {"vshape": (n,)}, "terminated": {"vshape": (1,), "dtype": torch.uint8}}


def make_batch(seed, device):
    """A seeded synthetic bids batch: bids around a softmax, episode 1 terminated at t = 2 (its
    later rows are masked), the others at the last step."""
    g = torch.Generator().manual_seed(seed)
    batch = EpisodeBatch(make_scheme(), {"agents": N}, B, T + 1, device=device)
    term = torch.zeros((B, T, 1), dtype=torch.uint8)
    term[:, T - 1] = 1
    term[1, 2] = 1
    bids = torch.softmax(torch.randn((B, T, N, M), generator=g), -1) + 0.3 * torch.randn((B, T, N, M), generator=g)
    batch.update({"obs": torch.randn((B, T + 1, N, OBS), generator=g),
                  "avail_actions": torch.ones((B, T + 1, N, M), dtype=torch.int)})
    batch.update({"actions": bids, "rewards": torch.randn((B, T, N), generator=g) * 2 + 0.5, "terminated": term},
                 ts=slice(0, T))
    return batch


class RefCritic(nn.Module):
    """modules/critics/ac.py with bids_as_actions: fc3 has m outputs; the input is the
    materialised cat([obs, eye(n)])."""

    def __init__(self, obs=OBS, n=N, n_out=M, hidden=64):
        super().__init__()
        self.n = n
        self.fc1 = nn.Linear(obs + n, hidden)
        self.fc2 = nn.Linear(hidden, hidden)
        self.fc3 = nn.Linear(hidden, n_out)

    def forward(self, obs):
        bs, max_t = obs.shape[0], obs.shape[1]
        eye = torch.eye(self.n, dtype=obs.dtype, device=obs.device).unsqueeze(0).unsqueeze(0).expand(bs, max_t, -1, -1)
        x = F.relu(self.fc1(torch.cat([obs, eye], dim=-1)))
        x = F.relu(self.fc2(x))
        return self.fc3(x)


def init_states(seed, use_rnn=False):
    # the critic first: its training does not depend on the agent, so every case trains the same critic
    torch.manual_seed(seed)
    critic = RefCritic().state_dict()
    return RNNAgent(OBS, SimpleNamespace(hidden_dim=64, use_rnn=use_rnn, m=M)).state_dict(), critic


def log_prob(pi, bids, sigma):
    """action_log_prob(pi, actions) as the reference calls it (bet_selectors.py:23-24, arguments
    swapped): Normal(bids, sigma).log_prob(pi)."""
    return torch.distributions.Normal(bids, sigma).log_prob(pi)


def surrogate(pi, bids, old_logp, adv, mask, sigma, eps):
    """cont_ppo_learner.py:91-101 on pi (already 1 where the mask is 0): the loss and the clip
    branch of every element."""
    ratios = torch.exp(log_prob(pi, bids, sigma) - old_logp)
    surr1 = ratios * adv
    surr2 = torch.clamp(ratios, 1 - eps, 1 + eps) * adv
    loss = -(torch.min(surr1, surr2) * mask).sum() / mask.sum()
    branch = torch.stack([surr1 <= surr2, ratios < 1 - eps, ratios > 1 + eps]).detach()
    return loss, branch


def nstep_returns(rewards, mask, values, nsteps, gamma, add_value_last_step):
    """cont_ppo_learner.py:174-192: rewards, mask [B, T, n, m], values [B, T + 1, n, m]."""
    nstep_values = torch.zeros_like(values[:, :-1])
    for t_start in range(rewards.size(1)):
        nstep_return_t = torch.zeros_like(values[:, 0])
        for step in range(nsteps + 1):
            t = t_start + step
            if t >= rewards.size(1):
                break
            elif step == nsteps:
                nstep_return_t += gamma ** (step) * values[:, t] * mask[:, t]
            elif t == rewards.size(1) - 1 and add_value_last_step:
                nstep_return_t += gamma ** (step) * rewards[:, t] * mask[:, t]
                nstep_return_t += gamma ** (step + 1) * values[:, t + 1]
            else:
                nstep_return_t += gamma ** (step) * rewards[:, t] * mask[:, t]
        nstep_values[:, t_start, :] = nstep_return_t
    return nstep_values


class RefContPPO:
    """learners/cont_ppo_learner.py on the CPU in `dtype`.  branches: per epoch of every train()
    call, the clip branch of every element (surr1 <= surr2, ratio below, ratio above the range)."""

    def __init__(self, args, agent_state, critic_state, dtype):
        self.args, self.dtype = args, dtype
        mk = lambda: RNNAgent(OBS, SimpleNamespace(hidden_dim=64, use_rnn=args.use_rnn, m=M)).to(dtype)  # noqa: E731
        self.agent, self.old_agent = mk(), mk()
        self.critic, self.target_critic = RefCritic().to(dtype), RefCritic().to(dtype)
        for net, sd in ((self.agent, agent_state), (self.old_agent, agent_state), (self.critic, critic_state),
                        (self.target_critic, critic_state)):
            net.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
        self.agent_params, self.critic_params = list(self.agent.parameters()), list(self.critic.parameters())
        self.agent_opt = torch.optim.Adam(self.agent_params, lr=args.lr)
        self.critic_opt = torch.optim.Adam(self.critic_params, lr=args.lr)
        self.steps = self.last_hard = 0
        self.rew_ms = _RMS(N, dtype)
        self.branches = []

    def _policy(self, agent, obs):
        h = torch.zeros((B * N, 64), dtype=self.dtype)
        out = []
        for t in range(T):
            q, h = agent(obs[:, t].reshape(B * N, -1), h)
            out.append(torch.softmax(q, dim=-1).view(B, N, M))
        return torch.stack(out, 1)

    def train(self, batch):
        a, dt = self.args, self.dtype
        rewards = batch["rewards"][:, :-1].to(dt)
        actions = batch["actions"][:, :-1].to(dt)
        terminated = batch["terminated"][:, :-1].to(dt)
        mask = batch["filled"][:, :-1].to(dt)
        mask[:, 1:] = mask[:, 1:] * (1 - terminated[:, :-1])
        if a.standardise_rewards:
            self.rew_ms.update(rewards)
            rewards = (rewards - self.rew_ms.mean) / torch.sqrt(self.rew_ms.var)
        mask = mask.unsqueeze(-1).repeat(1, 1, N, M)
        rewards = rewards.unsqueeze(-1).repeat(1, 1, 1, M)
        obs = batch["obs"].to(dt)

        with torch.no_grad():
            old_pi = self._policy(self.old_agent, obs)
        old_pi[mask == 0] = 1.0
        old_logp = log_prob(old_pi, actions, SIGMA_OLD)

        for _ in range(a.epochs):
            pi = self._policy(self.agent, obs)
            # train_critic_sequential
            with torch.no_grad():
                target_vals = self.target_critic(obs)
            target_returns = nstep_returns(rewards, mask, target_vals, a.q_nstep, a.gamma, a.add_value_last_step)
            v = self.critic(obs)[:, :-1]
            masked_td_error = (target_returns.detach() - v) * mask
            critic_loss = (masked_td_error ** 2).sum() / mask.sum()
            self.critic_opt.zero_grad()
            critic_loss.backward()
            critic_grads = [p.grad.clone() for p in self.critic_params]
            torch.nn.utils.clip_grad_norm_(self.critic_params, a.grad_norm_clip)
            self.critic_opt.step()
            advantages = masked_td_error.detach()

            pi[mask == 0] = 1.0
            pg_loss, branch = surrogate(pi, actions, old_logp.detach(), advantages, mask, SIGMA_NEW, a.eps_clip)
            self.branches.append(branch)
            self.agent_opt.zero_grad()
            pg_loss.backward()
            agent_grads = [p.grad.clone() for p in self.agent_params]
            torch.nn.utils.clip_grad_norm_(self.agent_params, a.grad_norm_clip)
            self.agent_opt.step()

        self.old_agent.load_state_dict(self.agent.state_dict())
        self.steps += 1
        tau = a.target_update_interval_or_tau
        if tau > 1 and (self.steps - self.last_hard) / tau >= 1.0:
            self.target_critic.load_state_dict(self.critic.state_dict())
            self.last_hard = self.steps
        elif tau <= 1.0:
            for tp, p in zip(self.target_critic.parameters(), self.critic.parameters()):
                tp.data.copy_(tp.data * (1.0 - tau) + p.data * tau)
        return pg_loss.detach(), critic_loss.detach(), agent_grads, critic_grads


class RawGrads:
    """Mixin for ContinuousPPOLearner: keeps both gradient sets as they are before clipping."""

    def _clip_agent_grads(self):
        self.raw_agent_grads = [p.grad.clone() for p in self.agent_params]
        return super()._clip_agent_grads()

    def _clip_critic_grads(self):
        self.raw_critic_grads = [p.grad.clone() for p in self.critic_params]
        return super()._clip_critic_grads()


def nets(learner):
    return (("agent", learner.mac.agent), ("critic", learner.critic), ("old agent", learner.old_mac.agent),
            ("target critic", learner.target_critic))


def load_critic(learner, critic_state):
    learner.critic.load_state_dict(critic_state)
    learner.target_critic.load_state_dict(critic_state)


def check_two_steps(learner, args, agent_state, critic_state, device, after_step=None, base=None):
    """Two train() steps of `learner` (a RawGrads learner built with selector variance SIGMA_OLD)
    on `device`, trained at SIGMA_NEW, against the float64 restatement: both losses, the pre-clip
    gradients of agent and critic from the last epoch, the parameters of agent, critic, old
    agent and target critic, under the 4 x rule.  base: a second learner that stands in for the
    float32 restatement as the baseline (the PyTorch path on the same device)."""
    assert learner.old_variance == SIGMA_OLD
    cpu_batch = make_batch(SEED, "cpu")
    ref64 = RefContPPO(args, agent_state, critic_state, torch.float64)
    ref32 = RefContPPO(args, agent_state, critic_state, torch.float32)
    batch = make_batch(SEED, device)
    filled = batch["filled"].clone()
    for le in (learner, base):
        if le is not None:
            le.mac.action_selector.variance = SIGMA_NEW
    for step in range(2):
        pg64, cl64, ag64, cg64 = ref64.train(cpu_batch)
        pg32, cl32, ag32, cg32 = ref32.train(cpu_batch)
        # the condition on the inputs: both restatements take the same clip branch everywhere
        for b64, b32 in zip(ref64.branches[-args.epochs:], ref32.branches[-args.epochs:]):
            assert torch.equal(b64, b32)
        if base is not None:
            pg32 = base.train(batch, t_env=step, episode_num=step)
            cl32, ag32, cg32 = base.critic_loss, base.raw_agent_grads, base.raw_critic_grads
        pg = learner.train(batch, t_env=step, episode_num=step)
        within(f"step {step} pg_loss", pg, pg32, pg64)
        within(f"step {step} critic_loss", learner.critic_loss, cl32, cl64)
        for i, (k, _) in enumerate(ref64.agent.named_parameters()):
            within(f"step {step} agent grad {k}", learner.raw_agent_grads[i], ag32[i], ag64[i])
        for i, (k, _) in enumerate(ref64.critic.named_parameters()):
            within(f"step {step} critic grad {k}", learner.raw_critic_grads[i], cg32[i], cg64[i])
        r32 = dict(nets(base)) if base is not None else {
            "agent": ref32.agent, "critic": ref32.critic, "old agent": ref32.old_agent,
            "target critic": ref32.target_critic}
        r64 = {"agent": ref64.agent, "critic": ref64.critic, "old agent": ref64.old_agent,
               "target critic": ref64.target_critic}
        for tag, got in nets(learner):
            p32, p64 = dict(r32[tag].named_parameters()), dict(r64[tag].named_parameters())
            for k, v in got.named_parameters():
                within(f"step {step} {tag} {k}", v.detach(), p32[k].detach(), p64[k].detach())
        if after_step is not None:
            after_step(step, batch)
    if args.target_update_interval_or_tau == 2:  # the hard update ran on the second step
        for tp, p in zip(learner.target_critic.parameters(), learner.critic.parameters()):
            assert torch.equal(tp, p)
    for tp, p in zip(learner.old_mac.parameters(), learner.mac.parameters()):
        assert torch.equal(tp, p)
    assert torch.equal(batch["filled"], filled)
    assert STATS <= set(learner.logger.stats)
    assert all(math.isfinite(v) for v in learner.logger.stats.values())
