"""The deferred transitions of the wave-pair rollout instances (rollout_envs_pair): the steps of a
launch run in groups of G = asg_rollout_defer_steps(64, 64, L, use_rnn); within a group a wave
runs its tiles back to back, the selected tasks going into G + 1 rows of LDS history, and the
group's transitions run afterwards, shared between the pair's two waves, their float64 reward
sums folded into the return in step order.  What can go wrong there and nowhere else: the rows
carried from one group to the next (and the previous tasks with them), launches whose length is
not a multiple of G, launch seams inside a group, a wave with no transition to run, the history
and counts reused from env to env, and the fold's order of additions.  Everything is byte equality
(batch fields, the returns' float64 bits, the final hidden state) against the split launches, or
the one-launch episode, on a batch poisoned with 0xA5; n = m = 64 throughout, the only shape
that reaches this code, and L = 1 wherever L is not the point."""
from types import SimpleNamespace

import numpy as np
import pytest

N = M = 64


@pytest.fixture(scope="module")
def L_():
    from marl_sap_amd import build, _lib
    build.build()
    return _lib.lib()


def test_defer_steps_without_gpu(L_):
    """The group size is a property of the LDS plan: at least one step wherever the pair mapping
    runs, 0 elsewhere, and never at the price of a resident fc1 slice."""
    for L in (1, 3):
        for use_rnn in (0, 1):
            assert L_.asg_rollout_defer_steps(64, 64, L, use_rnn) >= 1
    assert L_.asg_rollout_defer_steps(20, 25, 3, 1) == 0
    assert L_.asg_rollout_defer_steps(256, 256, 3, 1) == 0
    assert L_.asg_rollout_defer_steps(64, 64, 0, 1) == 0
    assert L_.asg_rollout_l2_slices(64, 64, 3, 1) == 1


def _G(L=1, use_rnn=True):
    from marl_sap_amd import _lib
    G = _lib.lib().asg_rollout_defer_steps(N, M, L, int(use_rnn))
    assert G >= 1
    return G


@pytest.fixture(scope="module")
def rows():
    """test_gpu_rollout_rows.py's helpers (_episodes, _same, _poison, _raw): imported here, not at
    module level, because that module skips itself without a GPU"""
    import test_gpu_rollout_rows
    return test_gpu_rollout_rows


def _direct(rows, T, L, E, chunks, nan_h=False, **env_kw):
    """One episode on a poisoned batch through the env's own calls: `chunks` = the (t0, t1) of the
    fused launches, or None = the split launches (reset, then agent-select and step in turn).
    nan_h: every launch's h_out starts as NaN.  Returns the fields' bytes, the returns' and the
    final hidden state's."""
    import torch
    from marl_sap_amd.envs import AssignEnvBatch
    from marl_sap_amd.components import EpisodeBatch
    from marl_sap_amd.modules.agents import RNNFusedAgent
    from marl_sap_amd.action_selectors.classic_selectors import EpsilonGreedyActionSelector
    DEV = rows.DEV
    env = AssignEnvBatch(N, M, T, L, 0.5, seed=3, num_envs=E, device=DEV, **env_kw)
    b = EpisodeBatch(env.scheme, {"agents": N}, E, T + 1, preprocess=env.preprocess, device=DEV, time_major=True)
    torch.manual_seed(9)
    agent = RNNFusedAgent(M * (L + 1), SimpleNamespace(hidden_dim=64, use_rnn=True, m=M)).to(DEV)
    sel = EpsilonGreedyActionSelector(SimpleNamespace(epsilon_start=0.2, epsilon_finish=0.2, epsilon_anneal_time=1,
                                                      evaluation_epsilon=0.0, seed=4))
    if nan_h:
        inner = agent.step_select_args

        def nan_h_out(*a, **k):
            args = inner(*a, **k)
            args[-1].fill_(float("nan"))
            return args

        agent.step_select_args = nan_h_out
    rows._poison(b)
    env.reset(b, 0)
    with torch.no_grad():
        if chunks is None:
            h = torch.zeros((E * N, 64), device=DEV)

            def select(t, h):
                eps, seed, c, st, base = sel.fused_params(0, False, DEV)
                return agent.forward_select(b["obs"][:, t].reshape(E * N, -1), h, b["avail_actions"][:, t], N, eps, seed,
                                            c, b["actions"][:, t, :, 0], st, env_index_base=base)

            h = select(0, h)
            for t in range(T):
                env.step(b, t)
                if t + 1 < T:
                    h = select(t + 1, h)
        else:
            h = agent.init_hidden().unsqueeze(0).expand(E, N, -1)
            for i, (t0, t1) in enumerate(chunks):
                last = t1 == T
                calls = (t1 - t0) + (1 if i == 0 else 0) - (1 if last else 0)
                eps, seed, c, st, _ = sel.fused_params(0, False, DEV, calls=calls)
                hn = env.rollout(b, t0, t1 - t0, agent, h, eps, seed, c, st, select_first=i == 0, select_last=not last)
                env.sync()
                if calls:  # a launch without a selection leaves its h_out alone
                    assert not torch.isnan(hn).any(), (t0, t1)
                    h = hn
    env.sync()
    out = {k: rows._raw(v) for k, v in b.data.transition_data.items()}
    ret = rows._raw(env.get_returns())
    env.close()
    return out, ret, rows._raw(h.reshape(E * N, -1))


def _same_direct(a, b):
    import torch
    assert a[0].keys() == b[0].keys()
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), k
    assert torch.equal(a[1], b[1])
    assert torch.equal(a[2], b[2])


@pytest.mark.gpu
@pytest.mark.parametrize("use_rnn", [True, False])
@pytest.mark.parametrize("dT", ["G-1", "G", "G+1", "2G+1"])
def test_group_boundaries(rows, dT, use_rnn):
    """Episodes that end one step before, at and one step after a group boundary, and in a third
    group; E = 5: one full workgroup plus a nearly empty one.  The whole-episode launch runs
    T + 1 steps of the kernel's loop (the reset row's selection first): exactly one group at
    T = G - 1, a second group of one step at T = G and of two at T = G + 1, two full groups and
    a third of two steps at T = 2 G + 1."""
    G = _G(1, use_rnn)
    T = {"G-1": G - 1, "G": G, "G+1": G + 1, "2G+1": 2 * G + 1}[dT]
    kw = dict(n=N, m=M, T=max(T, 2), L=1, E=5, use_rnn=use_rnn)
    split = rows._episodes(fused=False, **kw)
    fused = rows._episodes(fused="always", **kw)
    rows._same(fused, split)
    assert all(ep[3] for ep in fused)


@pytest.mark.gpu
def test_group_boundaries_headline_plan(rows):
    """The GRU plan at L = 3 (the headline's: the smallest G, one fc1 slice through L2)."""
    G = _G(3, True)
    kw = dict(n=N, m=M, T=2 * G + 1, L=3, E=5, episodes=1)
    rows._same(rows._episodes(fused="always", **kw), rows._episodes(fused=False, **kw))


@pytest.mark.gpu
def test_one_wave_without_a_transition(rows):
    """E = 1, T = 2 launched whole: three passes, two transitions, one pair beside three idle ones."""
    kw = dict(n=N, m=M, T=2, L=1, E=1, episodes=1)
    rows._same(rows._episodes(fused="always", **kw), rows._episodes(fused=False, **kw))


@pytest.mark.gpu
def test_one_transition_in_a_two_pass_launch(rows):
    """A chunk of one step with select_first and select_last inside a longer episode: two agent
    passes, so the pair mapping, and a single transition, so one wave of the pair has none."""
    T = 4
    split = _direct(rows, T, 1, 3, None)
    _same_direct(_direct(rows, T, 1, 3, [(0, 1), (1, T)]), split)
    _same_direct(_direct(rows, T, 1, 3, [(0, T)]), split)


@pytest.mark.gpu
def test_launch_seams_inside_groups(rows):
    """T = G + 3 as launches [0, 1), [1, G + 2), [G + 2, G + 3): the later ones start without a
    selection, their first transition takes its tasks from the batch row, and the second runs
    G + 1 steps -- a full group and one more.  h_out is NaN before every launch."""
    G = _G()
    T = G + 3
    one = _direct(rows, T, 1, 5, [(0, T)])
    seams = _direct(rows, T, 1, 5, [(0, 1), (1, G + 2), (G + 2, T)], nan_h=True)
    _same_direct(seams, one)


@pytest.mark.gpu
def test_pair_takes_several_envs(rows):
    """More envs than 4 per CU: the history, the counts and the sums are reused from env to env,
    and the last round is partly filled."""
    import torch
    G = _G()
    E = 4 * torch.cuda.get_device_properties(rows.DEV).multi_processor_count + 5
    kw = dict(n=N, m=M, T=G + 1, L=1, E=E, episodes=1)
    rows._same(rows._episodes(fused="always", **kw), rows._episodes(fused=False, **kw))


@pytest.mark.gpu
@pytest.mark.parametrize("benefits,rng", [("injected", "philox"), ("bump", "mt19937")])
def test_table_instances_three_envs(rows, benefits, rng):
    """The table modes' pair instances (TAB = 1, 2) with an idle pair, two groups."""
    kw = dict(n=N, m=M, T=_G() + 1, L=1, E=3, benefits=benefits, rng=rng, episodes=1)
    split = rows._episodes(fused=False, **kw)
    fused = rows._episodes(fused="always", **kw)
    rows._same(fused, split)
    assert all(ep[3] for ep in fused)


@pytest.mark.gpu
def test_injected_T_trans_three_envs(rows):
    """An injected transition-cost matrix: the deferred transition reads T_trans[prev][task] with
    prev = the history row before the step's."""
    T = _G() + 1
    tt = np.random.RandomState(11).rand(M, M) * 2.0
    _same_direct(_direct(rows, T, 1, 3, [(0, T)], T_trans=tt), _direct(rows, T, 1, 3, None, T_trans=tt))


@pytest.mark.gpu
def test_quirks_three_envs(rows):
    """prev_assigns rows of zeros and the parallel runner's terminated flags."""
    T = _G() + 1
    kw = dict(quirks=("prev_assigns_zero", "parallel_terminated"))
    _same_direct(_direct(rows, T, 1, 3, [(0, T)], **kw), _direct(rows, T, 1, 3, None, **kw))


@pytest.mark.gpu
def test_history_is_deterministic(rows):
    """The same fused episodes three times from the same seeds: a race on the task history would
    show as a run-to-run difference."""
    kw = dict(n=N, m=M, T=_G() + 1, L=1, E=5, eps=0.2, fused="always")
    first = rows._episodes(**kw)
    for _ in range(2):
        rows._same(rows._episodes(**kw), first)
