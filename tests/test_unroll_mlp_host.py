"""Host-side pieces of the Linear agent's sequence kernels and of QLearner (no GPU): the
argument checks of asg_mlp_agent_unroll / asg_mlp_agent_unroll_backward, the learner registry,
unroll() with fused_linear_unroll on CPU tensors (still the module loop), and QLearner.train on
the CPU -- it solves no assignment problem, so the whole step runs here -- against a float64
restatement of the reference's learners/q_learner.py (tests/q_learner_ref.py)."""
import ctypes
from types import SimpleNamespace

import pytest

torch = pytest.importorskip("torch")

from marl_sap_amd.controllers import REGISTRY as mac_REGISTRY  # noqa: E402
from marl_sap_amd.modules.agents import RNNAgent, RNNFusedAgent  # noqa: E402
from tests import q_learner_ref as R  # noqa: E402


def test_mlp_unroll_entries_validate_without_gpu():
    from marl_sap_amd import _lib, build
    build.build()
    L = _lib.lib()
    fake = ctypes.c_void_p(64)
    st = _lib.i64arr([80, 400, 16])

    def fwd(T1=4, B=2, n=5, K=16, hidden=64, n_out=7, x1=None, q=fake, W2=fake):
        return L.asg_mlp_agent_unroll(fake, st, T1, B, n, K, fake, fake, W2, fake, fake, fake, hidden, n_out, q,
                                      fake, x1, None)

    def bwd(N=40, hidden=64, dh=fake, dx1=fake):
        return L.asg_mlp_agent_unroll_backward(fake, fake, fake, fake, N, hidden, dh, dx1, None)

    for kw, word in (({"hidden": 32}, "hidden"), ({"n_out": 513}, "n_out"), ({"n_out": 0}, "n_out"),
                     ({"T1": 0}, "T1"), ({"B": 0}, "row"), ({"n": 0}, "row"), ({"K": 0}, "K")):
        assert fwd(**kw) == _lib.ASG_E_INVALID_ARG, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
    for kw, word in (({"hidden": 32}, "hidden"), ({"N": 0}, "row")):
        assert bwd(**kw) == _lib.ASG_E_INVALID_ARG, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
    assert fwd(q=None) == _lib.ASG_E_INVALID_ARG and "NULL" in _lib.last_error()
    assert bwd(dx1=None) == _lib.ASG_E_INVALID_ARG and "NULL" in _lib.last_error()
    assert fwd(x1=ctypes.c_void_p(68)) == _lib.ASG_E_INVALID_ARG and "misaligned" in _lib.last_error()
    assert fwd(W2=ctypes.c_void_p(72)) == _lib.ASG_E_INVALID_ARG and "misaligned" in _lib.last_error()
    assert bwd(dh=ctypes.c_void_p(72)) == _lib.ASG_E_INVALID_ARG and "misaligned" in _lib.last_error()
    with pytest.raises(ValueError, match="hidden"):
        _lib.check(bwd(hidden=32))


def test_q_learner_registry():
    from marl_sap_amd import learners
    assert learners.REGISTRY["q_learner"] is learners.QLearner
    assert learners.REGISTRY["sap_q_learner"] is learners.SAPQLearner
    assert issubclass(learners.QLearner, learners.SAPQLearner)
    args = SimpleNamespace(mixer="qmix", lr=1e-3, n=2, m=3, learner_log_interval=1)
    mac = SimpleNamespace(parameters=lambda: [torch.nn.Parameter(torch.zeros(1))])
    with pytest.raises(ValueError, match="qmix"):
        learners.QLearner(mac, {}, None, args)


@pytest.mark.parametrize("with_h0", [False, True])
def test_fused_linear_unroll_flag_on_cpu_is_the_module_loop(with_h0):
    torch.manual_seed(5)
    B, T1, n, K, m = 3, 4, 5, 20, 7
    agent = RNNFusedAgent(K, SimpleNamespace(hidden_dim=64, use_rnn=False, m=m, fused_linear_unroll=True))
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
    (q.sum() + h_last.sum()).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in agent.parameters())


@pytest.mark.parametrize("double_q,tau,std_returns", R.CASES)
def test_q_learner_two_train_steps_match_float64_reference_on_cpu(double_q, tau, std_returns):
    from marl_sap_amd.learners import QLearner

    class Recording(QLearner):
        def _clip_grads(self):
            self.raw_grads = [p.grad.clone() for p in self.params]
            return super()._clip_grads()

    args = R.make_args(double_q=double_q, tau=tau, std_returns=std_returns, use_rnn=False, fused_linear_unroll=True)
    state = R.init_state(R.SEED)
    mac = mac_REGISTRY["basic_mac"](R.make_scheme(), {"agents": R.N}, args)
    mac.agent.load_state_dict(state)
    R.check_two_steps(Recording(mac, None, R.Logger(), args), args, state, "cpu")
