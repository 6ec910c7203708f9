"""The wave-pair mapping of the 64 x 64 rollout instances (rollout_envs_pair): two waves share
an env, each keeps its 32 agents' hidden state in registers between a launch's passes, and the
selected tasks pass between them through an LDS double buffer behind one workgroup barrier per
step.  What can go wrong there and nowhere else: workgroups whose pairs are partly idle, a pair's
scratch and registers reused from env to env, the hidden state at launch seams (read by a
launch's first pass, written only by its last), and the hand-off itself.  Everything is byte
equality against the split launches (or the one-launch episode) on a batch poisoned with 0xA5,
with the helpers of test_gpu_rollout_rows.py; n = m = 64 throughout, the only shape that reaches
this code."""
from types import SimpleNamespace

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from test_gpu_rollout_rows import DEV, _episodes, _poison, _raw, _same  # noqa: E402

N = M = 64


@pytest.mark.parametrize("use_rnn", [True, False])
@pytest.mark.parametrize("E", [1, 3, 4, 5])
def test_partly_filled_workgroups(E, use_rnn):
    """4 envs per workgroup: idle pairs (1, 3), one full workgroup (4), one full plus one nearly
    empty (5).  An idle pair skips the work and still takes every barrier."""
    kw = dict(n=N, m=M, T=4, L=3, E=E, use_rnn=use_rnn)
    split = _episodes(fused=False, **kw)
    assert all(ep[3] for ep in split)
    for mode in ("always", "step"):
        fused = _episodes(fused=mode, **kw)
        _same(fused, split)
        assert all(ep[3] for ep in fused), mode


def test_smallest_launch():
    """E = 1, T = 2: one active pair beside three idle ones, two passes."""
    kw = dict(n=N, m=M, T=2, L=1, E=1, episodes=1)
    _same(_episodes(fused="always", **kw), _episodes(fused=False, **kw))


def test_pair_takes_several_envs():
    """More envs than 4 per CU: every pair runs a second env after its first (scratch, parity
    buffers and the h registers reused), and the last round is partly filled."""
    E = 4 * torch.cuda.get_device_properties(DEV).multi_processor_count + 5
    kw = dict(n=N, m=M, T=2, L=1, E=E)
    split = _episodes(fused=False, **kw)
    for mode in ("always", "step"):
        _same(_episodes(fused=mode, **kw), split)


@pytest.mark.parametrize("benefits,rng,selector", [
    ("injected", "philox", "epsilon_greedy"),
    ("bump", "mt19937", "epsilon_greedy"),
    ("bump", "philox", "sap"),
])
def test_other_64x64_instances_three_envs(benefits, rng, selector):
    """The table modes and the Q-output schedule with an idle pair (E = 3; E = 5 is
    test_gpu_rollout_rows.py's point)."""
    kw = dict(n=N, m=M, T=4, L=3, E=3, benefits=benefits, rng=rng, selector=selector)
    split = _episodes(fused=False, **kw)
    assert all(ep[3] for ep in split)
    for mode in ((True,) if selector == "sap" else ("always", "step")):
        fused = _episodes(fused=mode, **kw)
        _same(fused, split)
        assert all(ep[3] for ep in fused), mode


def test_hand_off_is_deterministic():
    """The same fused episodes three times from the same seeds: a race in the LDS hand-off
    would show as a run-to-run difference."""
    kw = dict(n=N, m=M, T=4, L=3, E=5, eps=0.2, fused="always")
    first = _episodes(**kw)
    for _ in range(2):
        _same(_episodes(**kw), first)


@pytest.mark.parametrize("contiguous_hin", [False, True])
def test_hidden_state_across_launch_seams(contiguous_hin):
    """One episode of T = 4 as launches [0, 1), [1, 3), [3, 4), each into an h_out buffer filled
    with NaN: only a launch's last agent pass writes it, and it must write every row.  Rows,
    returns and the final hidden state equal the one-launch episode's.  The first launch reads
    either init_hidden's expanded zero row (stride 0) or a contiguous h_in."""
    from marl_sap_amd.envs import AssignEnvBatch
    from marl_sap_amd.components import EpisodeBatch
    from marl_sap_amd.modules.agents import RNNFusedAgent
    from marl_sap_amd.action_selectors.classic_selectors import EpsilonGreedyActionSelector
    T, L, E = 4, 3, 5

    def run(chunks):
        env = AssignEnvBatch(N, M, T, L, 0.5, seed=3, num_envs=E, device=DEV)
        b = EpisodeBatch(env.scheme, {"agents": N}, E, T + 1, preprocess=env.preprocess, device=DEV, time_major=True)
        torch.manual_seed(9)
        agent = RNNFusedAgent(M * (L + 1), SimpleNamespace(hidden_dim=64, use_rnn=True, m=M)).to(DEV)
        sel = EpsilonGreedyActionSelector(SimpleNamespace(epsilon_start=0.2, epsilon_finish=0.2,
                                                          epsilon_anneal_time=1, evaluation_epsilon=0.0, seed=4))
        inner = agent.step_select_args

        def nan_h_out(*a, **k):
            args = inner(*a, **k)
            args[-1].fill_(float("nan"))
            return args

        agent.step_select_args = nan_h_out
        _poison(b)
        env.reset(b, 0)
        h = agent.init_hidden().unsqueeze(0).expand(E, N, -1)
        if contiguous_hin:
            h = h.contiguous()
        with torch.no_grad():
            for i, (t0, t1) in enumerate(chunks):
                last = t1 == T
                # selections of the launch: the reset row's (first launch) and one per
                # transition, but none after the episode's last
                calls = (t1 - t0) + (1 if i == 0 else 0) - (1 if last else 0)
                eps, seed, c, st, _ = sel.fused_params(0, False, DEV, calls=calls)
                hn = env.rollout(b, t0, t1 - t0, agent, h, eps, seed, c, st, select_first=i == 0,
                                 select_last=not last)
                env.sync()
                if calls:  # a launch without a selection leaves its h_out alone
                    assert not torch.isnan(hn).any(), (t0, t1)
                    h = hn
        out = {k: _raw(v) for k, v in b.data.transition_data.items()}
        ret = _raw(env.get_returns())
        env.close()
        return out, ret, _raw(h)

    one = run([(0, T)])
    seams = run([(0, 1), (1, 3), (3, 4)])
    assert one[0].keys() == seams[0].keys()
    for k in one[0]:
        assert torch.equal(one[0][k], seams[0][k]), k
    assert torch.equal(one[1], seams[1])
    assert torch.equal(one[2], seams[2])
