"""QLearner.train on the GPU (the Linear agent on asg_mlp_agent_unroll / its backward with
fused_linear_unroll, the GRU agent on asg_rnn_agent_unroll) against the float64 CPU restatement
of the reference's learners/q_learner.py in tests/q_learner_ref.py, and SAPQLearner with the
Linear agent on the new kernels against itself on the per-step loop.  Tolerance: the rule of
tests/test_gpu_agent.py -- the max error against float64 may be at most 4 x the error of the
same computation in float32 PyTorch, plus 1e-7 max|reference|."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from marl_sap_amd.action_selectors.lsa import linear_sum_assignment_batched  # noqa: E402
from marl_sap_amd.components import ReplayBuffer  # noqa: E402
from marl_sap_amd.controllers import REGISTRY as mac_REGISTRY  # noqa: E402
from marl_sap_amd.learners import REGISTRY as le_REGISTRY, QLearner, SAPQLearner  # noqa: E402
from marl_sap_amd.modules.agents import RNNAgent, RNNFusedAgent  # noqa: E402
from marl_sap_amd.modules.agents import rnn_agent  # noqa: E402
from tests import q_learner_ref as R  # noqa: E402

DEV = torch.device("cuda", 0)
B, T, N, M, OBS = R.B, R.T, R.N, R.M, R.OBS
JUMPSTART = dict(jumpstart_action_selector="haa_selector", jumpstart_epsilon_start=0.5, jumpstart_epsilon_finish=0.5,
                 jumpstart_epsilon_anneal_time=1, jumpstart_evaluation_epsilon=0.0,
                 env_args=dict(n=N, m=M, T=T, L=3, lambda_=0.5))


class _RawGrads:
    """Keeps the gradients as they are before clipping."""

    def _clip_grads(self):
        self.raw_grads = [p.grad.clone() for p in self.params]
        return super()._clip_grads()


class _Recording(_RawGrads, QLearner):
    pass


def _gpu_learner(args, state, cls, mac="basic_mac"):
    mac = mac_REGISTRY[mac](R.make_scheme(), {"agents": N}, args)
    mac.agent.load_state_dict(state)
    mac.to(DEV)
    assert isinstance(mac.agent, RNNFusedAgent)
    return cls(mac, None, R.Logger(), args)


def _count_launches(monkeypatch):
    """Counts the launches of the two unroll paths' forward kernels."""
    calls = {"mlp": 0, "gru": 0}
    mlp, gru = rnn_agent._mlp_launch, rnn_agent._unroll_launch

    def mlp_counted(*a):
        calls["mlp"] += 1
        return mlp(*a)

    def gru_counted(*a):
        calls["gru"] += 1
        return gru(*a)

    monkeypatch.setattr(rnn_agent, "_mlp_launch", mlp_counted)
    monkeypatch.setattr(rnn_agent, "_unroll_launch", gru_counted)
    return calls


@pytest.mark.parametrize("double_q,tau,std_returns,use_rnn,mac", [
    (*c, False, "basic_mac") for c in R.CASES] + [(True, 0.01, False, True, "basic_mac"),
                                                  (True, 0.01, False, False, "jumpstart_mac")])
def test_q_learner_two_train_steps_match_float64_reference(double_q, tau, std_returns, use_rnn, mac, monkeypatch):
    extra = JUMPSTART if mac == "jumpstart_mac" else {}
    args = R.make_args(double_q=double_q, tau=tau, std_returns=std_returns, use_rnn=use_rnn,
                       fused_linear_unroll=True, **extra)
    state = R.init_state(R.SEED, use_rnn)
    learner = _gpu_learner(args, state, _Recording, mac)
    calls = _count_launches(monkeypatch)
    x0 = R.make_batch(R.SEED, DEV)["obs"][:, 0].reshape(B * N, OBS)
    h0 = torch.zeros((B * N, 64), device=DEV)

    def prime():
        # both fused inference paths have packed these weights before they change
        with torch.no_grad():
            learner.mac.selector_agent(x0, h0)
            learner.target_mac.agent(x0, h0)

    def after_step(step, batch):
        # the stale-cache trap: after the update the fused paths run the NEW weights -- the
        # target's unroll and single-step kernel, and the runner's selection forward
        tgt = learner.target_mac.agent
        with torch.no_grad():
            q_unroll, _ = tgt.unroll(batch["obs"])
            h, q_loop = h0, []
            for t in range(T + 1):
                q_t, h = RNNAgent.forward(tgt, batch["obs"][:, t].reshape(B * N, OBS), h)
                q_loop.append(q_t.view(B, N, M))
            torch.testing.assert_close(q_unroll, torch.stack(q_loop, 1), rtol=1e-5, atol=2e-5)
            for agent in (tgt, learner.mac.selector_agent):
                want = RNNAgent.forward(agent, x0, h0)[0]
                torch.testing.assert_close(agent(x0, h0)[0], want, rtol=1e-5, atol=2e-5)
        prime()

    prime()
    R.check_two_steps(learner, args, state, DEV, after_step)
    # the train steps ran on the kernels: live + target unroll per step, and the check above
    kind, other = ("gru", "mlp") if use_rnn else ("mlp", "gru")
    assert calls[kind] == 6 and calls[other] == 0, calls


class _SAP64(_RawGrads, SAPQLearner):
    """SAPQLearner in float64: the module cast to double, the inputs widened, and the targets
    gathered in float64 (sap_target_max_qvals returns float32)."""

    def _target_max_qvals(self, target_mac_out, avail_actions, mac_out):
        Bn, T1, n, m = target_mac_out.shape
        unavailable = avail_actions[:, 1:] == 0
        tgt = target_mac_out.masked_fill(unavailable, -9999.0)
        cost = mac_out.detach()[:, 1:].masked_fill(unavailable, -9999.0) if self.args.double_q else tgt
        row, col = linear_sum_assignment_batched(cost.reshape(Bn * T1, n, m), maximize=True)
        self.assignment = col
        flat = tgt.reshape(Bn * T1, n, m)
        return flat[torch.arange(Bn * T1, device=flat.device).unsqueeze(1), row, col].view(Bn, T1, n)


class _SAPRecording(_RawGrads, SAPQLearner):
    def _target_max_qvals(self, target_mac_out, avail_actions, mac_out):
        unavailable = avail_actions[:, 1:] == 0
        cost = (mac_out.detach()[:, 1:] if self.args.double_q else target_mac_out).masked_fill(unavailable, -9999.0)
        _, self.assignment = linear_sum_assignment_batched(cost.reshape(-1, N, M), maximize=True)
        return super()._target_max_qvals(target_mac_out, avail_actions, mac_out)


def test_sap_q_learner_linear_agent_fused_against_the_loop(monkeypatch):
    """One SAPQLearner step with the Linear agent: fused_linear_unroll on, against the flag off
    (the float32 baseline) and the same learner in float64.  Rewards are not standardised here:
    RunningMeanStd keeps float32 statistics, which would put float32 rounding into the float64 run."""
    state = R.init_state(R.SEED)
    batch = R.make_batch(R.SEED, DEV)
    kw = dict(double_q=True, tau=0.01, std_rewards=False, use_rnn=False)
    on = _gpu_learner(R.make_args(fused_linear_unroll=True, **kw), state, _SAPRecording)
    off = _gpu_learner(R.make_args(fused_linear_unroll=False, **kw), state, _SAPRecording)
    args64 = R.make_args(agent="rnn_torch", **kw)
    mac64 = mac_REGISTRY["basic_mac"](R.make_scheme(), {"agents": N}, args64)
    mac64.agent.load_state_dict(state)
    mac64.to(DEV)
    mac64.agent.double()
    build = mac64._build_sequence_inputs
    mac64._build_sequence_inputs = lambda b: build(b).double()
    ref = _SAP64(mac64, None, R.Logger(), args64)
    assert next(ref.target_mac.parameters()).dtype == torch.float64
    calls = _count_launches(monkeypatch)
    loss_off = off.train(batch, 0, 0)
    assert calls["mlp"] == 0
    loss_on = on.train(batch, 0, 0)
    assert calls == {"mlp": 2, "gru": 0}
    loss64 = ref.train(batch, 0, 0)
    assert loss64.dtype == torch.float64
    # the condition on the inputs: the three runs solve to the same assignments
    assert torch.equal(on.assignment, ref.assignment) and torch.equal(off.assignment, ref.assignment)
    R.within("loss", loss_on, loss_off, loss64)
    for i, (k, _) in enumerate(ref.mac.agent.named_parameters()):
        R.within(f"grad {k}", on.raw_grads[i], off.raw_grads[i], ref.raw_grads[i])
    for tag, pick in (("param", lambda le: le.mac.agent), ("target", lambda le: le.target_mac.agent)):
        p_off, p64 = dict(pick(off).named_parameters()), dict(pick(ref).named_parameters())
        for k, v in pick(on).named_parameters():
            R.within(f"{tag} {k}", v.detach(), p_off[k].detach(), p64[k].detach())


def test_rollout_to_q_learner_train_end_to_end():
    """mock_constellation_iql.yaml's pieces: GpuVecRunner (8 envs, n = m = 16, T = 5, the Linear
    agent, jumpstart_mac + epsilon-greedy) -> ReplayBuffer -> sample(4) -> QLearner.train."""
    from marl_sap_amd.runners import REGISTRY as r_REGISTRY
    n = m = 16
    args = R.make_args(
        n=n, m=m, T=5, batch_size_run=8, env="mock_constellation_env", use_rnn=False, fused_linear_unroll=True,
        env_args=dict(n=n, m=m, T=5, L=3, lambda_=0.5, bids_as_actions=False, seed=3), env_rng="philox",
        env_quirks=(), runner_protocol="episode", test_nepisode=1, runner_log_interval=10 ** 12,
        action_selector="epsilon_greedy", epsilon_start=0.1, epsilon_finish=0.1, mac="jumpstart_mac",
        **{k: v for k, v in JUMPSTART.items() if k != "env_args"})
    np.random.seed(11)
    runner = r_REGISTRY["gpu"](args, R.Logger())
    env = runner.get_env()
    torch.manual_seed(4)
    mac = mac_REGISTRY["jumpstart_mac"](env.scheme, {"agents": n}, args)
    mac.to(DEV)
    runner.setup(env.scheme, {"agents": n}, env.preprocess, mac)
    learner = le_REGISTRY["q_learner"](mac, env.scheme, R.Logger(), args)
    assert type(learner) is QLearner
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
    env.close()
