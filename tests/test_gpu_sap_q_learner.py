"""SAPQLearner.train on the GPU (fused unrolls, batched LSA targets) against a float64 CPU
restatement of the reference learner (learners/sap_q_learner.py:56-165: per-step agent loop,
scipy LSA loop, RunningMeanStd, Adam, hard / soft target updates).  Tolerance: the rule of
tests/test_gpu_agent.py -- the GPU learner's max error against float64 may be at most 4 x the
error of the same restatement run in float32 PyTorch, plus 1e-7 max|reference|."""
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")
scipy_opt = pytest.importorskip("scipy.optimize")
pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from marl_sap_amd.components import EpisodeBatch, ReplayBuffer  # noqa: E402
from marl_sap_amd.components.transforms import OneHot  # noqa: E402
from marl_sap_amd.controllers import REGISTRY as mac_REGISTRY  # noqa: E402
from marl_sap_amd.learners import REGISTRY as le_REGISTRY, SAPQLearner  # noqa: E402
from marl_sap_amd.modules.agents import RNNAgent, RNNFusedAgent  # noqa: E402

DEV = torch.device("cuda", 0)
B, T, N, M, OBS = 4, 5, 4, 6, 10
SEED = 1  # scipy's assignments from the float64 and the float32 Q agree at every (b, t): asserted below


class _Logger:
    def __init__(self):
        self.stats = {}

    def log_stat(self, k, v, t):
        self.stats[k] = v


def _args(double_q=True, tau=0.01, std_rewards=True, std_returns=False, **kw):
    a = SimpleNamespace(
        n=N, m=M, agent="rnn", hidden_dim=64, use_rnn=True, obs_last_action=False, obs_agent_id=False,
        agent_output_type="q", action_selector="epsilon_greedy", epsilon_start=0.0, epsilon_finish=0.0,
        epsilon_anneal_time=1, evaluation_epsilon=0.0, mixer=None, lr=1e-3, gamma=0.99, grad_norm_clip=10.0,
        double_q=double_q, target_update_interval_or_tau=tau, standardise_rewards=std_rewards,
        standardise_returns=std_returns, learner_log_interval=0, use_mps_action_selection=False)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _scheme(n, m, obs):
    return {"obs": {"vshape": obs, "group": "agents"},
            "actions": {"vshape": (1,), "group": "agents", "dtype": torch.long},
            "avail_actions": {"vshape": (m,), "group": "agents", "dtype": torch.int},
            "rewards": {"vshape": (n,)}, "terminated": {"vshape": (1,), "dtype": torch.uint8},
            "beta": {"vshape": (n, m)}}


def _batch(seed, device):
    """A seeded synthetic batch: some unavailable actions with every row feasible, episode 1
    terminated early (its later rows are masked), the others at the last step."""
    g = torch.Generator().manual_seed(seed)
    pre = {"actions": ("actions_onehot", [OneHot(out_dim=M)])}
    batch = EpisodeBatch(_scheme(N, M, OBS), {"agents": N}, B, T + 1, preprocess=pre, device=device)
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


def _init_state(seed):
    torch.manual_seed(seed)
    return RNNAgent(OBS, SimpleNamespace(hidden_dim=64, use_rnn=True, m=M)).state_dict()


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


class _RefLearner:
    """learners/sap_q_learner.py on the CPU in `dtype`: the per-step loop over the PyTorch
    module, the scipy loop, and the reference's update arithmetic."""

    def __init__(self, args, state, dtype):
        self.args, self.dtype = args, dtype
        mk = lambda: RNNAgent(OBS, SimpleNamespace(hidden_dim=64, use_rnn=True, m=M)).to(dtype)  # noqa: E731
        self.agent, self.target = mk(), mk()
        sd = {k: v.to(dtype) for k, v in state.items()}
        self.agent.load_state_dict(sd)
        self.target.load_state_dict(sd)
        self.params = list(self.agent.parameters())
        self.opt = torch.optim.Adam(self.params, lr=args.lr)
        self.steps = self.last_hard = 0
        self.ret_ms, self.rew_ms = _RMS(N, dtype), _RMS(N, dtype)
        self.assignments = []

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
        avail = batch["avail_actions"]
        if a.standardise_rewards:
            self.rew_ms.update(rewards)
            rewards = (rewards - self.rew_ms.mean) / torch.sqrt(self.rew_ms.var)
        obs = batch["obs"].to(dt)
        mac_out = self._unroll(self.agent, obs)
        chosen = torch.gather(mac_out[:, :-1], 3, actions).squeeze(3)
        with torch.no_grad():
            tq = self._unroll(self.target, obs)[:, 1:].clone()
        tq[avail[:, 1:] == 0] = -9999
        cost = tq
        if a.double_q:
            cost = mac_out.detach().clone()
            cost[avail == 0] = -9999
            cost = cost[:, 1:]
        tmax = torch.zeros((B, T, N), dtype=dt)
        assign = np.zeros((B, T, N), dtype=np.int64)
        for b in range(B):
            for t in range(T):
                r, c = scipy_opt.linear_sum_assignment(cost[b, t].numpy(), maximize=True)
                tmax[b, t, :] = tq[b, t, r, c]
                assign[b, t] = c
        self.assignments.append(assign)
        if a.standardise_returns:
            tmax = tmax * torch.sqrt(self.ret_ms.var) + self.ret_ms.mean
        targets = rewards + a.gamma * (1 - terminated) * tmax
        if a.standardise_returns:
            self.ret_ms.update(targets)
            targets = (targets - self.ret_ms.mean) / torch.sqrt(self.ret_ms.var)
        td = chosen - targets
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


class _Recording(SAPQLearner):
    """SAPQLearner that keeps the gradients as they are before clipping."""

    def _clip_grads(self):
        self.raw_grads = [p.grad.clone() for p in self.params]
        return super()._clip_grads()


def _gpu_learner(args, state, cls=_Recording):
    mac = mac_REGISTRY["basic_mac"](_scheme(N, M, OBS), {"agents": N}, args)
    mac.agent.load_state_dict(state)
    mac.to(DEV)
    assert isinstance(mac.agent, RNNFusedAgent)
    return cls(mac, None, _Logger(), args)


def _module_q(agent, x, h):
    """The PyTorch module's forward on the agent's current weights."""
    with torch.no_grad():
        return RNNAgent.forward(agent, x, h)[0]


def _within(name, got, base, want):
    err = (got.double().cpu() - want).abs().max().item()
    err32 = (base.double() - want).abs().max().item()
    floor = 1e-7 * want.abs().max().item()
    print(f"{name}: max |err| vs float64: gpu {err:.3e}, torch fp32 {err32:.3e}, floor {floor:.1e}")
    assert err <= 4 * err32 + floor, (name, err, err32, floor)


@pytest.mark.parametrize("double_q,tau,std_returns", [(True, 0.01, False), (False, 0.01, False), (True, 2, False),
                                                      (True, 0.01, True)])
def test_two_train_steps_match_float64_reference(double_q, tau, std_returns):
    args = _args(double_q=double_q, tau=tau, std_returns=std_returns)
    state = _init_state(SEED)
    cpu_batch = _batch(SEED, "cpu")
    ref64, ref32 = _RefLearner(args, state, torch.float64), _RefLearner(args, state, torch.float32)
    learner = _gpu_learner(args, state)
    gpu_batch = _batch(SEED, DEV)
    filled = gpu_batch["filled"].clone()
    x0 = gpu_batch["obs"][:, 0].reshape(B * N, OBS)
    h0 = torch.zeros((B * N, 64), device=DEV)
    for step in range(2):
        # both fused inference paths have packed these weights before they change
        with torch.no_grad():
            learner.mac.selector_agent(x0, h0)
            learner.target_mac.agent(x0, h0)
        loss64, g64 = ref64.train(cpu_batch)
        loss32, g32 = ref32.train(cpu_batch)
        # the condition on the inputs: no near-tie between the float64 and float32 assignments
        assert np.array_equal(ref64.assignments[-1], ref32.assignments[-1])
        loss = learner.train(gpu_batch, t_env=step, episode_num=step)
        _within(f"step {step} loss", loss, loss32, loss64)
        for i, (k, _) in enumerate(ref64.agent.named_parameters()):
            _within(f"step {step} grad {k}", learner.raw_grads[i], g32[i], g64[i])
        for tag, got, r32, r64 in (("param", learner.mac.agent, ref32.agent, ref64.agent),
                                   ("target", learner.target_mac.agent, ref32.target, ref64.target)):
            p32, p64 = dict(r32.named_parameters()), dict(r64.named_parameters())
            for k, v in got.named_parameters():
                _within(f"step {step} {tag} {k}", v.detach(), p32[k].detach(), p64[k].detach())
        # the stale-cache trap: after the update the fused paths run the NEW weights -- the
        # target's unroll and single-step kernel, and the runner's selection forward
        tgt = learner.target_mac.agent
        with torch.no_grad():
            q_unroll, _ = tgt.unroll(gpu_batch["obs"])
            h, q_loop = h0, []
            for t in range(T + 1):
                q_t, h = RNNAgent.forward(tgt, gpu_batch["obs"][:, t].reshape(B * N, OBS), h)
                q_loop.append(q_t.view(B, N, M))
            torch.testing.assert_close(q_unroll, torch.stack(q_loop, 1), rtol=1e-5, atol=2e-5)
            for agent in (tgt, learner.mac.selector_agent):
                torch.testing.assert_close(agent(x0, h0)[0], _module_q(agent, x0, h0), rtol=1e-5, atol=2e-5)
    if tau == 2:  # the hard update ran on the second step
        for tp, p in zip(learner.target_mac.parameters(), learner.mac.parameters()):
            assert torch.equal(tp, p)
    assert torch.equal(gpu_batch["filled"], filled)
    assert {"loss", "grad_norm", "td_error_abs", "q_taken_mean", "target_mean", "avg_num_conflicts",
            "avg_beta"} <= set(learner.logger.stats)


def test_vectorised_stats_equal_the_reference_loops():
    learner = _gpu_learner(_args(), _init_state(SEED), SAPQLearner)
    batch = _batch(SEED, DEV)
    actions = batch["actions"][:, :-1]
    a, beta = actions.cpu(), batch["beta"].cpu()
    dup, total = 0.0, 0.0
    for b in range(B):  # learners/sap_q_learner.py:167-201
        for k in range(T):
            done = np.zeros(M)
            for i in range(N):
                done[a[b, k, i, 0].item()] += 1
                total += beta[b, k, i, a[b, k, i, 0].item()].item()
            dup += np.where(done > 0, done - 1, 0).sum()
    assert dup > 0
    assert learner.calc_conflicting_actions(actions) == dup / B / T
    assert abs(learner.calc_raw_benefits(batch["beta"], actions) - total / B / T / N) < 1e-6
    assert abs(learner.calc_raw_benefits(batch["beta"].unsqueeze(-1), actions) - total / B / T / N) < 1e-6


def test_save_load_round_trip_and_mixer_rejected(tmp_path):
    args = _args()
    learner = _gpu_learner(args, _init_state(SEED), SAPQLearner)
    batch = _batch(SEED, DEV)
    learner.train(batch, 0, 0)
    learner.save_models(str(tmp_path))
    other = _gpu_learner(args, _init_state(SEED + 1), SAPQLearner)
    other.load_models(str(tmp_path))
    for group in (other.mac, other.target_mac):
        for p, q in zip(group.parameters(), learner.mac.parameters()):
            assert torch.equal(p, q)
    s0, s1 = learner.optimiser.state_dict()["state"], other.optimiser.state_dict()["state"]
    assert s0.keys() == s1.keys() and len(s0) == 8
    for k in s0:
        assert torch.equal(s0[k]["exp_avg_sq"], s1[k]["exp_avg_sq"])
    assert torch.isfinite(other.train(batch, 1, 1))  # the loaded learner trains on
    with pytest.raises(ValueError, match="vdn"):
        _gpu_learner(_args(mixer="vdn"), _init_state(SEED), SAPQLearner)
    learner.cuda()
    assert le_REGISTRY["sap_q_learner"] is SAPQLearner


def test_rollout_to_train_end_to_end():
    """GpuVecRunner (8 envs, n = m = 16, T = 5) -> ReplayBuffer -> sample(4) -> train."""
    from marl_sap_amd.runners import REGISTRY as r_REGISTRY
    n = m = 16
    args = _args(
        n=n, m=m, T=5, batch_size_run=8, env="mock_constellation_env",
        env_args=dict(n=n, m=m, T=5, L=3, lambda_=0.5, bids_as_actions=False, seed=3), env_rng="philox",
        env_quirks=(), runner_protocol="episode", test_nepisode=1, runner_log_interval=10 ** 12,
        action_selector="sap", epsilon_start=0.1, epsilon_finish=0.1)
    runner = r_REGISTRY["gpu"](args, _Logger())
    env = runner.get_env()
    torch.manual_seed(4)
    mac = mac_REGISTRY["basic_mac"](env.scheme, {"agents": n}, args)
    mac.to(DEV)
    runner.setup(env.scheme, {"agents": n}, env.preprocess, mac)
    learner = le_REGISTRY["sap_q_learner"](mac, env.scheme, _Logger(), args)
    buf = ReplayBuffer(env.scheme, {"agents": n}, 8, 6, preprocess=env.preprocess, device=DEV)
    buf.insert_episode_batch(runner.run(test_mode=False))
    sample = buf.sample(4, rng=np.random.RandomState(0))
    filled = sample["filled"].clone()
    before = [p.detach().clone() for p in mac.parameters()]
    loss = learner.train(sample, runner.t_env, 8)
    assert torch.isfinite(loss)
    assert all(not torch.equal(p, q) for p, q in zip(mac.parameters(), before))
    assert torch.equal(sample["filled"], filled) and int(filled.sum()) == 4 * 6
    # the runner goes on with the updated agent
    assert runner.run(test_mode=False)["obs"].shape[0] == 8
