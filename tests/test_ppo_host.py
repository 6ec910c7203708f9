"""Host-side pieces of ContinuousPPOLearner (no GPU): the argument checks of
asg_mlp_agent_unroll_ids, asg_bids_log_prob, asg_ppo_bids_loss and asg_nstep_returns, the
learner and critic registries, ACCritic's parameters against the reference's, and the learner's
PyTorch path on CPU tensors against the float64 restatement of the reference's learners/
cont_ppo_learner.py in tests/cont_ppo_ref.py."""
import ctypes

import pytest

torch = pytest.importorskip("torch")

from marl_sap_amd.controllers import REGISTRY as mac_REGISTRY  # noqa: E402
from tests import cont_ppo_ref as R  # noqa: E402


def test_ppo_entries_validate_without_gpu():
    from marl_sap_amd import _lib, build
    build.build()
    L = _lib.lib()
    fake, off4, off8 = ctypes.c_void_p(64), ctypes.c_void_p(68), ctypes.c_void_p(72)
    st = _lib.i64arr([80, 400, 16])
    bad = _lib.ASG_E_INVALID_ARG

    def ids(T1=4, B=2, n=5, K=16, hidden=64, n_out=7, x1=None, q=fake, W2=fake):
        return L.asg_mlp_agent_unroll_ids(fake, st, T1, B, n, K, fake, fake, W2, fake, fake, fake, hidden, n_out, q,
                                          fake, x1, None)

    def logp(T=4, B=2, n=5, m=8, sigma=0.3, logits=fake, bids=fake, out=fake, mask=fake):
        return L.asg_bids_log_prob(logits, bids, st, mask, st, T, B, n, m, sigma, 1, out, None)

    def loss(T=4, B=2, n=5, m=8, sigma=0.3, eps=0.2, logits=fake, adv=fake, inv=fake, dl=fake, rmax=None):
        return L.asg_ppo_bids_loss(logits, fake, st, fake, adv, fake, st, T, B, n, m, sigma, eps, inv, 1, fake, dl,
                                   rmax, None)

    def nstep(T=4, B=2, n=5, m=8, nsteps=5, values=fake, out=fake, rew=fake):
        return L.asg_nstep_returns(values, rew, st, fake, st, T, B, n, m, 0.99, nsteps, 1, out, None)

    for kw, word in (({"hidden": 32}, "hidden"), ({"n_out": 513}, "n_out"), ({"n_out": 0}, "n_out"),
                     ({"T1": 0}, "T1"), ({"B": 0}, "row"), ({"n": 0}, "row"), ({"K": 0}, "K")):
        assert ids(**kw) == bad, kw
        assert word in _lib.last_error() and "asg_mlp_agent_unroll_ids" in _lib.last_error(), (kw, _lib.last_error())
    assert ids(q=None) == bad and "NULL" in _lib.last_error()
    assert ids(x1=off4) == bad and "misaligned" in _lib.last_error()
    assert ids(W2=off8) == bad and "misaligned" in _lib.last_error()

    for fn, name in ((logp, "asg_bids_log_prob"), (loss, "asg_ppo_bids_loss"), (nstep, "asg_nstep_returns")):
        cases = [({"m": 0}, "m must"), ({"m": 513}, "m must"), ({"T": 0}, "T must"), ({"B": 0}, "row"),
                 ({"n": 0}, "row")]
        if fn is nstep:
            cases += [({"nsteps": 0}, "nsteps")]
        else:
            cases += [({"sigma": 0.0}, "sigma"), ({"sigma": -0.1}, "sigma")]
        for kw, word in cases:
            assert fn(**kw) == bad, (name, kw)
            assert word in _lib.last_error() and name in _lib.last_error(), (name, kw, _lib.last_error())
    assert loss(eps=-0.1) == bad and "eps_clip" in _lib.last_error()
    for call in (lambda: logp(logits=None), lambda: logp(out=None), lambda: loss(adv=None),
                 lambda: loss(inv=None), lambda: loss(dl=None), lambda: nstep(values=None), lambda: nstep(out=None)):
        assert call() == bad and "NULL" in _lib.last_error()
    for call in (lambda: logp(logits=off8), lambda: logp(out=off4), lambda: logp(bids=ctypes.c_void_p(66)),
                 lambda: loss(adv=off8), lambda: loss(dl=off4), lambda: loss(rmax=ctypes.c_void_p(66)),
                 lambda: nstep(values=off8), lambda: nstep(out=off4), lambda: nstep(rew=ctypes.c_void_p(66))):
        assert call() == bad and "misaligned" in _lib.last_error()
    with pytest.raises(ValueError, match="sigma"):
        _lib.check(logp(sigma=0.0))


def test_registries_resolve():
    from marl_sap_amd import learners
    from marl_sap_amd.modules import critics
    assert learners.REGISTRY["cont_ppo_learner"] is learners.ContinuousPPOLearner
    assert critics.REGISTRY["ac_critic"] is critics.ACCritic


@pytest.mark.parametrize("bids,n_out", [(True, R.M), (False, 1)])
def test_ac_critic_parameters_match_the_reference(bids, n_out):
    """modules/critics/ac.py:18-23: fc1 Linear(obs + n, hidden), fc2 Linear(hidden, hidden), fc3
    Linear(hidden, m) with bids_as_actions, else Linear(hidden, 1)."""
    from marl_sap_amd.modules.critics import ACCritic
    args = R.make_args()
    args.env_args["bids_as_actions"] = bids
    critic = ACCritic(R.make_scheme(), args)
    shapes = {k: tuple(v.shape) for k, v in critic.state_dict().items()}
    assert shapes == {"fc1.weight": (64, R.OBS + R.N), "fc1.bias": (64,), "fc2.weight": (64, 64), "fc2.bias": (64,),
                      "fc3.weight": (n_out, 64), "fc3.bias": (n_out,)}
    assert list(critic.state_dict()) == list(R.RefCritic().state_dict())
    # on CPU tensors it is the reference's module on the concatenated input
    batch = R.make_batch(R.SEED, "cpu")
    want = R.RefCritic(n_out=n_out)
    want.load_state_dict(critic.state_dict())
    assert torch.equal(critic(batch), want(batch["obs"]))
    assert torch.equal(critic(batch, t=2), want(batch["obs"][:, 2:3]))
    assert torch.equal(critic.rows(batch), want(batch["obs"]).permute(1, 0, 2, 3).reshape(R.T + 1, R.B * R.N, n_out))


def _cpu_learner(args, agent_state, critic_state):
    from marl_sap_amd.learners import ContinuousPPOLearner

    class Recording(R.RawGrads, ContinuousPPOLearner):
        pass

    mac = mac_REGISTRY["basic_mac"](R.make_scheme(), {"agents": R.N}, args)
    mac.agent.load_state_dict(agent_state)
    learner = Recording(mac, R.make_scheme(), R.Logger(), args)
    R.load_critic(learner, critic_state)
    return learner


def test_learner_refuses_what_the_reference_cannot_run():
    from marl_sap_amd.learners import ContinuousPPOLearner
    args = R.make_args()
    args.env_args["bids_as_actions"] = False
    mac = mac_REGISTRY["basic_mac"](R.make_scheme(), {"agents": R.N}, args)
    with pytest.raises(ValueError, match="bids_as_actions"):
        ContinuousPPOLearner(mac, R.make_scheme(), R.Logger(), args)
    args = R.make_args(critic_type="coma_critic")
    mac = mac_REGISTRY["basic_mac"](R.make_scheme(), {"agents": R.N}, args)
    with pytest.raises(ValueError, match="coma_critic"):
        ContinuousPPOLearner(mac, R.make_scheme(), R.Logger(), args)


def test_forward_sequence_rows_is_the_first_rows():
    args = R.make_args()
    mac = mac_REGISTRY["basic_mac"](R.make_scheme(), {"agents": R.N}, args)
    batch = R.make_batch(R.SEED, "cpu")
    with torch.no_grad():
        full, part = mac.forward_sequence(batch), mac.forward_sequence(batch, rows=R.T)
    assert part.shape == (R.B, R.T, R.N, R.M) and torch.equal(part, full[:, :R.T])


@pytest.mark.parametrize("tau,q_nstep,use_rnn", R.CASES)
def test_cont_ppo_two_train_steps_match_float64_reference_on_cpu(tau, q_nstep, use_rnn):
    """The learner is built with selector variance 0.3 and trained with it at 0.2: the old
    policy's log-probabilities keep 0.3."""
    args = R.make_args(tau=tau, q_nstep=q_nstep, use_rnn=use_rnn, fused_linear_unroll=True)
    agent_state, critic_state = R.init_states(R.SEED, use_rnn)
    learner = _cpu_learner(args, agent_state, critic_state)
    R.check_two_steps(learner, args, agent_state, critic_state, "cpu")
    assert learner.critic_training_steps == 2


def test_save_and_load_models_use_the_reference_file_names(tmp_path):
    args = R.make_args()
    agent_state, critic_state = R.init_states(R.SEED)
    learner = _cpu_learner(args, agent_state, critic_state)
    learner.mac.action_selector.variance = R.SIGMA_NEW
    learner.train(R.make_batch(R.SEED, "cpu"), 0, 0)
    learner.save_models(str(tmp_path))
    assert {p.name for p in tmp_path.iterdir()} == {"agent.th", "critic.th", "agent_opt.th", "critic_opt.th"}
    other = _cpu_learner(args, agent_state, critic_state)
    other.load_models(str(tmp_path))
    for (_, a), (_, b) in zip(R.nets(learner), R.nets(other)):
        if a is learner.old_mac.agent or a is learner.target_critic:
            continue
        for p, q in zip(a.parameters(), b.parameters()):
            assert torch.equal(p, q)
    for tp, p in zip(other.target_critic.parameters(), other.critic.parameters()):
        assert torch.equal(tp, p)
