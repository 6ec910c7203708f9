"""The kernels under ContinuousPPOLearner on the GPU, each against the reference's expressions in
float64 (tests/cont_ppo_ref.py): ACCritic on asg_mlp_agent_unroll_ids (values and all six
parameter gradients, against the module on the materialised [obs, eye(n)] input),
asg_nstep_returns against the reference's loop, asg_bids_log_prob and asg_ppo_bids_loss against
autograd through torch.distributions.Normal, th.min and th.clamp.  Tolerance: the project's rule
(at most 4 x the float32 PyTorch error against float64, plus 1e-7 max|reference|).  The rule needs
both precisions on the same side of every ReLU and of every clip decision: the inputs are seeded
(on the CPU, where the seeds were chosen) so that they are, and the tests assert it."""
from types import SimpleNamespace

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from marl_sap_amd.learners import ppo_kernels as K  # noqa: E402
from marl_sap_amd.modules.agents import RNNAgent, RNNFusedAgent  # noqa: E402
from marl_sap_amd.modules.critics import ACCritic, ac  # noqa: E402
from tests import cont_ppo_ref as R  # noqa: E402

DEV = torch.device("cuda", 0)
NAMES = ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias"]
# (B, T1, n, K, n_out) -> seed: 60 rows with a ragged last tile, K and K + n no multiples of 4;
# two workgroups, K + n and K multiples of 4; the workload's n, K and m; one value per agent
CRITIC_SEEDS = {(3, 4, 5, 10, 6): 0, (2, 3, 20, 100, 25): 0, (1, 2, 64, 256, 64): 1, (2, 3, 5, 12, 1): 0}
RELU_MARGIN = 1e-5
_CACHE = {}


def _cached(key, make):
    """CPU references: computed once, shared by the tests that need them and left unchanged."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def rows(x):
    """[B, T, n, m] -> the kernels' [T, B n, m]."""
    B, T, n, m = x.shape
    return x.permute(1, 0, 2, 3).reshape(T, B * n, m).contiguous()


def _layout(x, time_major):
    x = x.to(DEV)
    if time_major:  # the runner batch: [T1][B] storage seen as [B, T1, ...]
        x = x.transpose(0, 1).contiguous().transpose(0, 1)
    return x


# ---- the critic -------------------------------------------------------------------------------
def _critic_run(net, x, wq, call=None):
    """(values, grads of the six parameter tensors) of loss = <values, wq>."""
    net.zero_grad()
    q = net(x) if call is None else call(x)
    (q * wq).sum().backward()
    sd = dict(net.named_parameters())
    return q.detach(), {k: sd[k].grad.clone() for k in NAMES}


def critic_case(shape, seed):
    B, T1, n, Kobs, n_out = shape
    torch.manual_seed(seed)
    state = R.RefCritic(obs=Kobs, n=n, n_out=n_out).state_dict()
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn((B, T1, n, Kobs), generator=g)
    wq = torch.randn((B, T1, n, n_out), generator=g)
    ref64 = R.RefCritic(obs=Kobs, n=n, n_out=n_out).double()
    ref64.load_state_dict({k: v.double() for k, v in state.items()})
    with torch.no_grad():
        eye = torch.eye(n, dtype=torch.float64).expand(B, T1, n, n)
        pre1 = torch.cat([x.double(), eye], -1) @ ref64.fc1.weight.t() + ref64.fc1.bias
        pre2 = torch.relu(pre1) @ ref64.fc2.weight.t() + ref64.fc2.bias
        margin = min(pre1.abs().min().item(), pre2.abs().min().item())
    return state, x, wq, _critic_run(ref64, x.double(), wq.double()), margin


def _critics(shape, state):
    B, T1, n, Kobs, n_out = shape
    args = SimpleNamespace(n=n, m=n_out, hidden_dim=64, env_args={"bids_as_actions": n_out != 1})
    fused = ACCritic({"obs": {"vshape": Kobs}}, args).to(DEV)
    fused.load_state_dict(state)
    ref = R.RefCritic(obs=Kobs, n=n, n_out=n_out).to(DEV)
    ref.load_state_dict(state)
    return ref, fused


@pytest.mark.parametrize("time_major", [False, True])
@pytest.mark.parametrize("shape", list(CRITIC_SEEDS))
def test_critic_values_and_gradients_match_float64(shape, time_major, monkeypatch):
    B, T1, n, Kobs, n_out = shape
    state, x, wq, (q64, g64), margin = _cached(("critic", shape), lambda: critic_case(shape, CRITIC_SEEDS[shape]))
    # the condition on the inputs: no ReLU can flip between float64 and float32
    assert margin > RELU_MARGIN, margin
    ref, fused = _critics(shape, state)
    x, wq = _layout(x, time_major), wq.to(DEV)
    assert B == 1 or x.stride(0) == (n * Kobs if time_major else T1 * n * Kobs)
    q32, g32 = _critic_run(ref, x, wq)
    launches = []
    inner = ac._ids_launch
    monkeypatch.setattr(ac, "_ids_launch", lambda *a: launches.append(1) or inner(*a))
    on_batch = lambda xx: fused({"obs": xx})  # noqa: E731
    qf, gf = _critic_run(fused, x, wq, on_batch)
    assert len(launches) == 1 and qf.shape == (B, T1, n, n_out)
    for name, got, base, want in [("v", qf, q32, q64)] + [(k, gf[k], g32[k], g64[k]) for k in NAMES]:
        assert got.shape == want.shape, name
        R.within(name, got, base, want)
    # a second run on the same inputs: identical bits
    qf2, gf2 = _critic_run(fused, x, wq, on_batch)
    assert torch.equal(qf2, qf) and all(torch.equal(gf2[k], gf[k]) for k in NAMES)
    with torch.no_grad():
        # the single row at t, the time-major rows, and the PyTorch module behind fused_ppo = False
        assert torch.equal(fused({"obs": x}, t=1), qf[:, 1:2])
        assert torch.equal(fused.rows({"obs": x}), rows(qf))
        assert len(launches) == 4
        fused.args.fused_ppo = False
        assert torch.equal(fused({"obs": x}), ref(x))
    assert len(launches) == 4


def test_existing_mlp_unroll_instance_is_unchanged():
    """The Linear agent's asg_mlp_agent_unroll is built from the same kernel source as the critic's
    instance: on the critic test's data it still gives the module's values at the existing tests'
    tolerance (tests/test_gpu_unroll_mlp.py) and the same bits twice."""
    B, T1, n, Kobs, m = 3, 4, 5, 10, 6
    torch.manual_seed(0)
    args = SimpleNamespace(hidden_dim=64, use_rnn=False, m=m, fused_linear_unroll=True)
    agent = RNNFusedAgent(Kobs, args).to(DEV)
    x = torch.randn((B, T1, n, Kobs), generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        q1, h1 = agent.unroll(x)
        q2, h2 = agent.unroll(x)
        h, qs = torch.zeros((B * n, 64), device=DEV), []
        for t in range(T1):
            q_t, h = RNNAgent.forward(agent, x[:, t].reshape(B * n, Kobs), h)
            qs.append(q_t.view(B, n, m))
    assert torch.equal(q1, q2) and torch.equal(h1, h2)
    torch.testing.assert_close(q1, torch.stack(qs, 1), rtol=1e-5, atol=2e-5)
    torch.testing.assert_close(h1, h, rtol=1e-5, atol=2e-5)


# ---- n-step returns ---------------------------------------------------------------------------
def nstep_case(m):
    B, T, n = R.B, R.T, R.N
    g = torch.Generator().manual_seed(7 + m)
    values = torch.randn((B, T + 1, n, m), generator=g)
    rewards = torch.randn((B, T + 1, n), generator=g) * 2 + 0.5  # the batch's rows: T of T + 1 are used
    mask = torch.ones((B, T))
    mask[1, 3:] = 0  # episode 1 terminated at t = 2
    return values, rewards, mask


@pytest.mark.parametrize("add_last", [True, False])
@pytest.mark.parametrize("nsteps", [1, 5, 7])
@pytest.mark.parametrize("m", [6, 25])
def test_nstep_returns_match_the_reference_loop(m, nsteps, add_last):
    B, T, n = R.B, R.T, R.N
    values, rewards, mask = _cached(("nstep", m), lambda: nstep_case(m))
    gamma = 0.99

    def ref(dt):
        mask4 = mask.to(dt).view(B, T, 1, 1).repeat(1, 1, n, m)
        rew4 = rewards[:, :T].to(dt).unsqueeze(-1).repeat(1, 1, 1, m)
        return rows(R.nstep_returns(rew4, mask4, values.to(dt), nsteps, gamma, add_last))

    want, base = _cached(("nstep ref", m, nsteps, add_last), lambda: (ref(torch.float64), ref(torch.float32)))
    rew_dev = rewards.to(DEV)[:, :T]  # strided: a slice of the T + 1 rows
    assert not rew_dev.is_contiguous()
    got = K.nstep_returns(rows(values).to(DEV), rew_dev, mask.to(DEV), n, gamma, nsteps, add_last)
    assert got.shape == (T, B * n, m)
    R.within("nstep returns", got, base, want)
    assert torch.equal(got, K.nstep_returns(rows(values).to(DEV), rew_dev, mask.to(DEV), n, gamma, nsteps, add_last))
    # time-major rewards and mask (the runner batch's layout) give the same bits
    rew_tm = rewards.to(DEV).transpose(0, 1).contiguous().transpose(0, 1)[:, :T]
    mask_tm = mask.to(DEV).t().contiguous().t()
    assert torch.equal(got, K.nstep_returns(rows(values).to(DEV), rew_tm, mask_tm, n, gamma, nsteps, add_last))


# ---- log-probability and the clipped surrogate --------------------------------------------------
LOSS_SEED = 1
EPS = 0.2


def loss_case(shape, m, row_softmax):
    """Standard-normal logits and advantages, the old logits perturbed by 0.3 N(0, 1), bids = the
    old policy's output + 0.3 N(0, 1); the float64 and float32 results of the reference's
    expressions (autograd for the gradient), and each one's clip branches."""
    B, T, n = shape
    g = torch.Generator().manual_seed(LOSS_SEED)
    logits = torch.randn((B, T, n, m), generator=g)
    adv = torch.randn((B, T, n, m), generator=g)
    old = logits + 0.3 * torch.randn((B, T, n, m), generator=g)
    policy = (lambda z: torch.softmax(z, -1)) if row_softmax else (lambda z: z)
    bids = torch.zeros((B, T + 1, n, m))
    bids[:, :T] = policy(old) + 0.3 * torch.randn((B, T, n, m), generator=g)
    mask = torch.ones((B, T))
    if B > 1:
        mask[1, 1:] = 0

    def ref(dt):
        z = logits.to(dt).clone().requires_grad_(True)
        mask4 = mask.to(dt).view(B, T, 1, 1).repeat(1, 1, n, m)
        a = bids[:, :T].to(dt)
        old_pi = policy(old.to(dt)).masked_fill(mask4 == 0, 1.0)
        old_logp = R.log_prob(old_pi, a, R.SIGMA_OLD)
        pi = policy(z).masked_fill(mask4 == 0, 1.0)
        loss, branch = R.surrogate(pi, a, old_logp, adv.to(dt), mask4, R.SIGMA_NEW, EPS)
        dz, = torch.autograd.grad(loss, z)
        return dict(old_logp=rows(old_logp), loss=loss.detach(), dlogits=rows(dz),
                    row_max=pi.detach().max(-1)[0].permute(1, 0, 2).reshape(T, B * n), branch=branch)

    return logits, adv, old, bids, mask, ref(torch.float64), ref(torch.float32)


@pytest.mark.parametrize("row_softmax", [True, False])
@pytest.mark.parametrize("shape", [(4, 3, 5), (1, 1, 1)])  # 60 rows, 1 row
@pytest.mark.parametrize("m", [6, 25, 64, 130])  # sub-vector, ragged, one full 16-lane row, several tiles
def test_log_prob_and_ppo_loss_match_float64_autograd(m, shape, row_softmax):
    B, T, n = shape
    logits, adv, old, bids, mask, r64, r32 = _cached(("loss", shape, m, row_softmax),
                                                     lambda: loss_case(shape, m, row_softmax))
    # the condition on the inputs: both precisions take the same branch at every element
    assert torch.equal(r64["branch"], r32["branch"])
    if B > 1:  # both clip sides are hit
        assert r64["branch"][1].any() and r64["branch"][2].any()
    bids_dev = bids.to(DEV)[:, :T]  # strided, as batch["actions"][:, :-1] is
    mask_dev = mask.to(DEV)
    inv_count = (1.0 / (mask_dev.sum() * (n * m))).reshape(1)  # a device scalar
    old_logp = K.bids_log_prob(rows(old).to(DEV), bids_dev, mask_dev, n, R.SIGMA_OLD, row_softmax)
    R.within("old_logp", old_logp, r32["old_logp"], r64["old_logp"])

    def run():
        z = rows(logits).to(DEV).requires_grad_(True)
        loss, row_max = K.ppo_bids_loss(z, bids_dev, old_logp, rows(adv).to(DEV), mask_dev, inv_count, n,
                                        R.SIGMA_NEW, EPS, row_softmax, want_max=True)
        (3.0 * loss).backward()
        return loss.detach(), z.grad / 3.0, row_max

    loss, dlogits, row_max = run()
    R.within("loss", loss, r32["loss"], r64["loss"])
    R.within("dlogits", dlogits, r32["dlogits"], r64["dlogits"])
    R.within("row_max", row_max, r32["row_max"], r64["row_max"])
    masked = rows(mask.view(B, T, 1, 1).expand(B, T, n, m)) == 0
    if masked.any():
        # masked rows: exactly zero gradient, pi = 1 in the log-probability and the maxima
        assert torch.count_nonzero(dlogits[masked.to(DEV)]) == 0
        want = R.log_prob(torch.ones((), dtype=torch.float64), rows(bids[:, :T]).double()[masked], R.SIGMA_OLD)
        base = R.log_prob(torch.ones(()), rows(bids[:, :T])[masked], R.SIGMA_OLD)
        R.within("masked logp", old_logp[masked.to(DEV)], base, want)
        assert (row_max[masked[..., 0].to(DEV)] == 1.0).all()
    loss2, dlogits2, row_max2 = run()
    assert torch.equal(loss2, loss) and torch.equal(dlogits2, dlogits) and torch.equal(row_max2, row_max)
    assert K.ppo_bids_loss(rows(logits).to(DEV), bids_dev, old_logp, rows(adv).to(DEV), mask_dev, inv_count, n,
                           R.SIGMA_NEW, EPS, row_softmax)[1] is None
