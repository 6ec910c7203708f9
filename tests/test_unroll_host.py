"""Host-side pieces of the SAP Q-learner (no GPU): RunningMeanStd against a float64
restatement of the reference's arithmetic (components/standarize_stream.py:9-46), the agents'
unroll() and BasicMAC.forward_sequence on CPU tensors against the per-step loop they
replace (learners/sap_q_learner.py:69-84), the argument checks of the two unroll entries,
and the learner registry."""
import ctypes
from types import SimpleNamespace

import pytest

torch = pytest.importorskip("torch")

from marl_sap_amd.components import EpisodeBatch  # noqa: E402
from marl_sap_amd.components.standarize_stream import RunningMeanStd  # noqa: E402
from marl_sap_amd.components.transforms import OneHot  # noqa: E402
from marl_sap_amd.controllers.basic_controller import BasicMAC  # noqa: E402
from marl_sap_amd.modules.agents import RNNAgent, RNNFusedAgent  # noqa: E402


def test_running_mean_std_matches_float64():
    g = torch.Generator().manual_seed(3)
    rms = RunningMeanStd(shape=(5,))
    mean, var, count = torch.zeros(5, dtype=torch.float64), torch.ones(5, dtype=torch.float64), 1e-4
    for rows in (12, 7, 30):
        arr = torch.randn((2, rows, 5), generator=g) * 3 + 1
        rms.update(arr)
        a = arr.double().reshape(-1, 5)
        bm, bv, bc = a.mean(0), a.var(0), a.shape[0]
        delta, tot = bm - mean, count + bc
        m2 = var * count + bv * bc + delta ** 2 * count * bc / tot
        mean, var, count = mean + delta * bc / tot, m2 / tot, tot
        assert rms.mean.dtype == torch.float32 and rms.var.shape == (5,)
        torch.testing.assert_close(rms.mean.double(), mean, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(rms.var.double(), var, rtol=1e-5, atol=1e-6)
        assert abs(rms.count - count) < 1e-9


@pytest.mark.parametrize("cls", [RNNAgent, RNNFusedAgent])
@pytest.mark.parametrize("use_rnn", [True, False])
@pytest.mark.parametrize("with_h0", [False, True])
def test_unroll_on_cpu_is_the_module_loop(cls, use_rnn, with_h0):
    torch.manual_seed(5)
    B, T1, n, K, m = 3, 4, 5, 20, 7
    agent = cls(K, SimpleNamespace(hidden_dim=64, use_rnn=use_rnn, m=m))
    x = torch.randn((B, T1, n, K))
    h0 = torch.randn((B * n, 64)) * 0.5 if with_h0 else None
    q, h_last = agent.unroll(x, h0)
    h = torch.zeros((B * n, 64)) if h0 is None else h0
    qs = []
    for t in range(T1):
        qt, h = RNNAgent.forward(agent, x[:, t].reshape(B * n, K), h)
        qs.append(qt.view(B, n, m))
    assert q.shape == (B, T1, n, m) and h_last.shape == (B * n, 64)
    assert torch.equal(q, torch.stack(qs, 1)) and torch.equal(h_last, h)
    assert q.requires_grad  # the loop stays differentiable


@pytest.mark.parametrize("time_major", [False, True])
@pytest.mark.parametrize("last_action,agent_id,out_type", [
    (False, False, "q"), (True, False, "q"), (False, True, "q"), (True, True, "pi_logits")])
def test_forward_sequence_equals_stacked_forward(last_action, agent_id, out_type, time_major):
    torch.manual_seed(9)
    B, T, n, m, obs = 3, 4, 4, 6, 11
    scheme = {"obs": {"vshape": obs, "group": "agents"},
              "actions": {"vshape": (1,), "group": "agents", "dtype": torch.long}}
    pre = {"actions": ("actions_onehot", [OneHot(out_dim=m)])}
    batch = EpisodeBatch(scheme, {"agents": n}, B, T + 1, preprocess=pre, device="cpu", time_major=time_major)
    batch.update({"obs": torch.randn((B, T + 1, n, obs))})
    batch.update({"actions": torch.randint(0, m, (B, T, n, 1))}, ts=slice(0, T))
    args = SimpleNamespace(n=n, m=m, agent="rnn_fused", hidden_dim=64, use_rnn=True, obs_last_action=last_action,
                           obs_agent_id=agent_id, agent_output_type=out_type, action_selector="epsilon_greedy",
                           epsilon_start=0.0, epsilon_finish=0.0, epsilon_anneal_time=1, evaluation_epsilon=0.0)
    mac = BasicMAC(batch.scheme, {"agents": n}, args)
    with torch.no_grad():
        mac.init_hidden(B)
        want = torch.stack([mac.forward(batch, t) for t in range(T + 1)], dim=1)
        h_want = mac.hidden_states
        got = mac.forward_sequence(batch)
    assert got.shape == (B, T + 1, n, m)
    assert torch.equal(got, want) and torch.equal(mac.hidden_states, h_want)
    assert mac._build_sequence_inputs(batch).shape[-1] == obs + (m if last_action else 0) + (n if agent_id else 0)


def test_unroll_entries_validate_without_gpu():
    from marl_sap_amd import _lib, build
    build.build()
    L = _lib.lib()
    fake = ctypes.c_void_p(64)
    st = _lib.i64arr([80, 400, 16])

    def fwd(T1=4, B=2, n=5, K=16, hidden=64, n_out=7, use_rnn=1, h0=fake, hs=64):
        return L.asg_rnn_agent_unroll(fake, st, T1, B, n, K, h0, hs, *([fake] * 8), hidden, n_out, use_rnn, fake,
                                      fake, None, None)

    def bwd(T1=4, R=10, hidden=64, n_out=7, use_rnn=1, dgi=fake):
        return L.asg_rnn_agent_unroll_backward(fake, None, fake, fake, None, 0, fake, fake, T1, R, hidden, n_out,
                                               use_rnn, dgi, fake, fake, None, None)

    for f in (fwd, bwd):
        for kw, word in (({"hidden": 32}, "hidden"), ({"use_rnn": 0}, "use_rnn"), ({"n_out": 513}, "n_out"),
                         ({"n_out": 0}, "n_out"), ({"T1": 0}, "T1")):
            assert f(**kw) == _lib.ASG_E_INVALID_ARG, kw
            assert word in _lib.last_error(), (kw, _lib.last_error())
    assert fwd(B=0) == _lib.ASG_E_INVALID_ARG and bwd(R=0) == _lib.ASG_E_INVALID_ARG
    assert fwd(K=0) == _lib.ASG_E_INVALID_ARG
    assert fwd(h0=ctypes.c_void_p(68)) == _lib.ASG_E_INVALID_ARG and "misaligned" in _lib.last_error()
    assert fwd(hs=66) == _lib.ASG_E_INVALID_ARG
    assert bwd(dgi=ctypes.c_void_p(72)) == _lib.ASG_E_INVALID_ARG and "misaligned" in _lib.last_error()
    with pytest.raises(ValueError, match="hidden"):
        _lib.check(fwd(hidden=32))


def test_learner_registry():
    from marl_sap_amd import learners
    assert learners.REGISTRY["sap_q_learner"] is learners.SAPQLearner
    args = SimpleNamespace(mixer="vdn", lr=1e-3, n=2, m=3, learner_log_interval=1)
    mac = SimpleNamespace(parameters=lambda: [torch.nn.Parameter(torch.zeros(1))])
    with pytest.raises(ValueError, match="vdn"):
        learners.SAPQLearner(mac, {}, None, args)
