"""Shared by tests/test_unroll_mlp_host.py and tests/test_gpu_q_learner.py: a restatement of the
reference's learners/q_learner.py:54-140 (mixer: null) on the CPU in a given dtype -- the
per-step loop over the PyTorch module, the -9999999 mask, max / double-Q targets,
RunningMeanStd, the masked L2 loss, gradient clipping, Adam, hard / soft target updates --
with the synthetic batch of tests/test_gpu_sap_q_learner.py and the project's tolerance rule:
the error against float64 may be at most 4 x the error of the same restatement in float32, plus
1e-7 max|reference|."""
from types import SimpleNamespace

import torch

from marl_sap_amd.components import EpisodeBatch
from marl_sap_amd.components.transforms import OneHot
from marl_sap_amd.modules.agents import RNNAgent

B, T, N, M, OBS = 4, 5, 4, 6, 10
# (double_q, target_update_interval_or_tau, standardise_returns)
CASES = [(True, 0.01, False), (False, 0.01, False), (True, 2, False), (True, 0.01, True)]
# with this seed the float64 and the float32 restatement pick the same argmax at every
# (b, t, agent) of both steps, for every case and both agents: the tests assert it
SEED = 1
STATS = {"loss", "grad_norm", "td_error_abs", "q_taken_mean", "target_mean", "avg_num_conflicts", "avg_beta"}


class Logger:
    def __init__(self):
        self.stats = {}

    def log_stat(self, k, v, t):
        self.stats[k] = v


def make_args(double_q=True, tau=0.01, std_rewards=True, std_returns=False, use_rnn=False, **kw):
    a = SimpleNamespace(
        n=N, m=M, agent="rnn", hidden_dim=64, use_rnn=use_rnn, obs_last_action=False, obs_agent_id=False,
        agent_output_type="q", action_selector="epsilon_greedy", epsilon_start=0.0, epsilon_finish=0.0,
        epsilon_anneal_time=1, evaluation_epsilon=0.0, mixer=None, lr=1e-3, gamma=0.99, grad_norm_clip=10.0,
        double_q=double_q, target_update_interval_or_tau=tau, standardise_rewards=std_rewards,
        standardise_returns=std_returns, learner_log_interval=0, use_mps_action_selection=False)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def make_scheme(n=N, m=M, obs=OBS):
    return {"obs": {"vshape": obs, "group": "agents"},
            "actions": {"vshape": (1,), "group": "agents", "dtype": torch.long},
            "avail_actions": {"vshape": (m,), "group": "agents", "dtype": torch.int},
            "rewards": {"vshape": (n,)}, "terminated": {"vshape": (1,), "dtype": torch.uint8},
            "beta": {"vshape": (n, m)}}


def make_batch(seed, device):
    """A seeded synthetic batch: some unavailable actions with every row feasible, episode 1
    terminated early (its later rows are masked), the others at the last step."""
    g = torch.Generator().manual_seed(seed)
    pre = {"actions": ("actions_onehot", [OneHot(out_dim=M)])}
    batch = EpisodeBatch(make_scheme(), {"agents": N}, B, T + 1, preprocess=pre, device=device)
    avail = torch.rand((B, T + 1, N, M), generator=g) > 0.3
    avail |= torch.eye(N, M, dtype=torch.bool)
    actions = torch.multinomial(avail[:, :T].reshape(-1, M).float(), 1, generator=g).view(B, T, N, 1)
    term = torch.zeros((B, T, 1), dtype=torch.uint8)
    term[:, T - 1] = 1
    term[1, 2] = 1
    batch.update({"obs": torch.randn((B, T + 1, N, OBS), generator=g), "avail_actions": avail.int(),
                  "beta": torch.rand((B, T + 1, N, M), generator=g)})
    batch.update({"actions": actions, "rewards": torch.randn((B, T, N), generator=g) * 2 + 0.5, "terminated": term},
                 ts=slice(0, T))
    return batch


def init_state(seed, use_rnn=False):
    torch.manual_seed(seed)
    return RNNAgent(OBS, SimpleNamespace(hidden_dim=64, use_rnn=use_rnn, m=M)).state_dict()


class _RMS:
    """components/standarize_stream.py:9-46 in the given dtype."""

    def __init__(self, n, dtype):
        self.mean, self.var, self.count = torch.zeros(n, dtype=dtype), torch.ones(n, dtype=dtype), 1e-4

    def update(self, arr):
        arr = arr.reshape(-1, arr.size(-1))
        bm, bv, bc = arr.mean(0), arr.var(0), arr.shape[0]
        delta, tot = bm - self.mean, self.count + bc
        m2 = self.var * self.count + bv * bc + torch.square(delta) * self.count * bc / (self.count + bc)
        self.mean, self.var, self.count = self.mean + delta * bc / tot, m2 / (self.count + bc), bc + self.count


class RefQLearner:
    """learners/q_learner.py on the CPU in `dtype`.  argmaxes: per train() call, the action every
    (b, t, agent) takes its target at (double_q: of the masked live Q; else of the masked target Q)."""

    def __init__(self, args, state, dtype):
        self.args, self.dtype = args, dtype
        mk = lambda: RNNAgent(OBS, SimpleNamespace(hidden_dim=64, use_rnn=args.use_rnn, m=M)).to(dtype)  # noqa: E731
        self.agent, self.target = mk(), mk()
        sd = {k: v.to(dtype) for k, v in state.items()}
        self.agent.load_state_dict(sd)
        self.target.load_state_dict(sd)
        self.params = list(self.agent.parameters())
        self.opt = torch.optim.Adam(self.params, lr=args.lr)
        self.steps = self.last_hard = 0
        self.ret_ms, self.rew_ms = _RMS(N, dtype), _RMS(N, dtype)
        self.argmaxes = []

    def _unroll(self, agent, obs):
        h = torch.zeros((B * N, 64), dtype=self.dtype)
        out = []
        for t in range(obs.shape[1]):
            q, h = agent(obs[:, t].reshape(B * N, -1), h)
            out.append(q.view(B, N, M))
        return torch.stack(out, 1)

    def train(self, batch):
        a, dt = self.args, self.dtype
        rewards = batch["rewards"][:, :-1].to(dt)
        actions = batch["actions"][:, :-1]
        terminated = batch["terminated"][:, :-1].to(dt)
        mask = batch["filled"][:, :-1].to(dt)
        mask[:, 1:] = mask[:, 1:] * (1 - terminated[:, :-1])
        avail = batch["avail_actions"].to(torch.int64)
        if a.standardise_rewards:
            self.rew_ms.update(rewards)
            rewards = (rewards - self.rew_ms.mean) / torch.sqrt(self.rew_ms.var)
        obs = batch["obs"].to(dt)
        mac_out = self._unroll(self.agent, obs)
        chosen = torch.gather(mac_out[:, :-1], 3, actions).squeeze(3)
        with torch.no_grad():
            tq = self._unroll(self.target, obs)[:, 1:].clone()
        tq[avail[:, 1:] == 0] = -9999999
        if a.double_q:
            live = mac_out.clone().detach()
            live[avail == 0] = -9999999
            cur_max = live[:, 1:].max(dim=3, keepdim=True)[1]
            tmax = torch.gather(tq, 3, cur_max).squeeze(3)
            self.argmaxes.append(cur_max.squeeze(3).clone())
        else:
            tmax, idx = tq.max(dim=3)
            self.argmaxes.append(idx.clone())
        if a.standardise_returns:
            tmax = tmax * torch.sqrt(self.ret_ms.var) + self.ret_ms.mean
        targets = rewards + a.gamma * (1 - terminated) * tmax.detach()
        if a.standardise_returns:
            self.ret_ms.update(targets)
            targets = (targets - self.ret_ms.mean) / torch.sqrt(self.ret_ms.var)
        td = chosen - targets.detach()
        mask = mask.expand_as(td)
        loss = ((td * mask) ** 2).sum() / mask.sum()
        self.opt.zero_grad()
        loss.backward()
        grads = [p.grad.clone() for p in self.params]
        torch.nn.utils.clip_grad_norm_(self.params, a.grad_norm_clip)
        self.opt.step()
        self.steps += 1
        tau = a.target_update_interval_or_tau
        if tau > 1 and (self.steps - self.last_hard) / tau >= 1.0:
            self.target.load_state_dict(self.agent.state_dict())
            self.last_hard = self.steps
        elif tau <= 1.0:
            for tp, p in zip(self.target.parameters(), self.agent.parameters()):
                tp.data.copy_(tp.data * (1.0 - tau) + p.data * tau)
        return loss.detach(), grads


def within(name, got, base, want):
    err = (got.double().cpu() - want.double().cpu()).abs().max().item()
    err32 = (base.double().cpu() - want.double().cpu()).abs().max().item()
    floor = 1e-7 * want.abs().max().item()
    print(f"{name}: max |err| vs float64: got {err:.3e}, torch fp32 {err32:.3e}, floor {floor:.1e}")
    assert err <= 4 * err32 + floor, (name, err, err32, floor)


def check_two_steps(learner, args, state, device, after_step=None):
    """Two train() steps of `learner` (a recording learner: raw_grads holds the pre-clip gradients)
    on `device` against the float64 restatement: loss, pre-clip gradients, parameters and target
    parameters, under the 4 x rule.  after_step(step, batch): extra checks after each step."""
    cpu_batch = make_batch(SEED, "cpu")
    ref64, ref32 = RefQLearner(args, state, torch.float64), RefQLearner(args, state, torch.float32)
    batch = make_batch(SEED, device)
    filled = batch["filled"].clone()
    for step in range(2):
        loss64, g64 = ref64.train(cpu_batch)
        loss32, g32 = ref32.train(cpu_batch)
        # the condition on the inputs: no near-tie between the float64 and the float32 argmax
        assert torch.equal(ref64.argmaxes[-1], ref32.argmaxes[-1])
        loss = learner.train(batch, t_env=step, episode_num=step)
        within(f"step {step} loss", loss, loss32, loss64)
        for i, (k, _) in enumerate(ref64.agent.named_parameters()):
            within(f"step {step} grad {k}", learner.raw_grads[i], g32[i], g64[i])
        for tag, got, r32, r64 in (("param", learner.mac.agent, ref32.agent, ref64.agent),
                                   ("target", learner.target_mac.agent, ref32.target, ref64.target)):
            p32, p64 = dict(r32.named_parameters()), dict(r64.named_parameters())
            for k, v in got.named_parameters():
                within(f"step {step} {tag} {k}", v.detach(), p32[k].detach(), p64[k].detach())
        if after_step is not None:
            after_step(step, batch)
    if args.target_update_interval_or_tau == 2:  # the hard update ran on the second step
        for tp, p in zip(learner.target_mac.parameters(), learner.mac.parameters()):
            assert torch.equal(tp, p)
    assert torch.equal(batch["filled"], filled)
    assert STATS <= set(learner.logger.stats)
