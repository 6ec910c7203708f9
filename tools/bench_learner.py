"""A learner's train() on a REDA-shaped problem (n = m = 64, L = 3, T = 20, 32 episodes sampled
from a runner-filled ReplayBuffer, double_q), timed two ways in the same process, alternating:

  fused    the agent's unroll() is asg_rnn_agent_unroll / asg_rnn_agent_unroll_backward
           (--use-rnn 0, the Linear agent: asg_mlp_agent_unroll / asg_mlp_agent_unroll_backward,
           args.fused_linear_unroll)
  unfused  unroll() is forced to the per-step loop (args.unfused_unroll): the live network the
           PyTorch module under autograd, the target network one asg_rnn_agent_forward per
           step -- what a learner had before the unroll kernels

--learner picks SAPQLearner (the default, with the SAP selector filling the buffer) or QLearner
(epsilon-greedy).  With --use-rnn 0 a third timing, flat_torch_ms, is the PyTorch module applied
once to x.reshape(N, K) and its backward pass: the agent forward + backward alone, the honest
PyTorch baseline for a feed-forward net (the per-step loop is only what the code does without the
flag); fused_agent_ms is the same pass through unroll() (the two kernels and the parameter-gradient
GEMMs), and fwd_kernel_ms / bwd_kernel_ms the kernels alone.

Device events around each train() call after warm-up; one JSON line: median ms per train
step of both paths, their spread (max - min over the repeats), the ratio, and the forward /
backward kernel times alone.  `faster` is true when the fused median beats the unfused one
by more than the unfused path's own spread.

--learner cont_ppo_learner times ContinuousPPOLearner.train (ippo_sap.yaml: the Linear agent on
pi_logits, the continuous selector on the bids schedule filling the buffer, ACCritic, 4 epochs,
q_nstep 5; --episodes defaults to the config's batch_size, 10) three ways, alternating:

  fused      everything on the kernels: the agent and critic unrolls, asg_nstep_returns,
             asg_bids_log_prob, asg_ppo_bids_loss
  torch_loss fused_ppo = False with fused_linear_unroll: the agent unroll on its kernels, the
             critic, the n-step loop and the loss in PyTorch
  reference  fused_ppo = False and the per-step agent loop (unfused_unroll): the reference's
             formulation, the baseline

and reports the device activities (kernel launches and copies, from torch.profiler) of one
train() of each.

    python tools/bench_learner.py [--repeats 10] [--warmup 3] [--episodes 32]
                                  [--learner sap_q_learner|q_learner|cont_ppo_learner] [--use-rnn 1|0]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402


def timed(fn, repeats):
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


kInner = 20  # launches per sample of the Linear agent's kernels timed alone


def device_activities(fn):
    """Kernel launches and copies on the device during fn(), from torch.profiler; None where
    the profiler is not available."""
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(e.count for e in prof.key_averages() if e.device_type == DeviceType.CUDA) or None
    except Exception as e:  # noqa: BLE001
        print(f"launch count unavailable: {e!r}", file=sys.stderr)
        return None


def main_ppo(o):
    from marl_sap_amd.components import ReplayBuffer
    from marl_sap_amd.controllers import REGISTRY as mac_REGISTRY
    from marl_sap_amd.learners import REGISTRY as le_REGISTRY
    from marl_sap_amd.runners import REGISTRY as r_REGISTRY

    dev = torch.device("cuda", 0)
    E, n, T = o.episodes, o.n, o.T
    a = bench.parse(["--n", str(n), "--m", str(n), "--T", str(T), "--cpu-baseline", "0", "--secondary", "0"])
    args = bench.make_args(
        a, E, selector="bids", agent="rnn", fused_linear_unroll=True, reuse_batch=False, lr=3e-4, gamma=0.99,
        grad_norm_clip=10.0, critic_type="ac_critic", epochs=4, eps_clip=0.2, q_nstep=5, add_value_last_step=True,
        target_update_interval_or_tau=0.01, standardise_rewards=True, standardise_returns=False,
        learner_log_interval=10 ** 12, use_mps_action_selection=False, unfused_unroll=False, fused_ppo=True)
    runner = r_REGISTRY["gpu"](args, bench.NullLogger())
    env = runner.get_env()
    torch.manual_seed(a.seed)
    mac = mac_REGISTRY["basic_mac"](env.scheme, {"agents": n}, args)
    mac.to(dev)
    runner.setup(env.scheme, {"agents": n}, env.preprocess, mac)
    learner = le_REGISTRY[o.learner](mac, env.scheme, bench.NullLogger(), args)
    learner.log_stats_t = 0  # no logging branch (its .item() calls) in the timed steps
    buf = ReplayBuffer(env.scheme, {"agents": n}, E, T + 1, preprocess=env.preprocess, device=dev)
    buf.insert_episode_batch(runner.run(test_mode=False))
    batch = buf.sample(E, rng=np.random.RandomState(a.seed))
    legs = {"fused": (True, False), "torch_loss": (False, False), "reference": (False, True)}
    step = [0]

    def train(leg):
        args.fused_ppo, args.unfused_unroll = legs[leg]
        learner.train(batch, step[0], step[0])
        step[0] += 1

    for _ in range(o.warmup):
        for leg in legs:
            train(leg)
    times = {leg: [] for leg in legs}
    for _ in range(o.repeats):  # alternating, so drift hits all alike
        for leg in legs:
            times[leg] += timed(lambda: train(leg), 1)
    launches = {leg: device_activities(lambda: train(leg)) for leg in legs}
    med = {leg: statistics.median(v) for leg, v in times.items()}
    spread = {leg: max(v) - min(v) for leg, v in times.items()}
    K = mac._build_sequence_inputs(batch).shape[-1]
    out = {"metric": o.learner + "_train_ms", "shape": {"episodes": E, "n": n, "m": n, "L": a.L, "T": T, "K": K,
                                                        "epochs": args.epochs, "q_nstep": args.q_nstep},
           "repeats": o.repeats}
    for leg in legs:
        out[leg + "_ms"] = round(med[leg], 4)
        out[leg + "_spread_ms"] = round(spread[leg], 4)
        out[leg + "_device_activities"] = launches[leg]
    out["ratio_reference_over_fused"] = round(med["reference"] / med["fused"], 3)
    out["ratio_torch_loss_over_fused"] = round(med["torch_loss"] / med["fused"], 3)
    out["faster"] = bool(med["reference"] - med["fused"] > spread["reference"])
    print(json.dumps(out))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--episodes", type=int, default=None)
    p.add_argument("--n", type=int, default=64)
    p.add_argument("--T", type=int, default=20)
    p.add_argument("--learner", default="sap_q_learner", choices=["sap_q_learner", "q_learner", "cont_ppo_learner"])
    p.add_argument("--use-rnn", type=int, default=1, choices=[1, 0])
    o = p.parse_args()
    if o.repeats < 5:
        p.error("--repeats must be at least 5")
    if o.episodes is None:
        o.episodes = 10 if o.learner == "cont_ppo_learner" else 32
    if o.learner == "cont_ppo_learner":
        return main_ppo(o)
    from marl_sap_amd import _lib
    from marl_sap_amd.components import ReplayBuffer
    from marl_sap_amd.controllers import REGISTRY as mac_REGISTRY
    from marl_sap_amd.learners import REGISTRY as le_REGISTRY
    from marl_sap_amd.modules.agents import rnn_agent
    from marl_sap_amd.runners import REGISTRY as r_REGISTRY

    dev = torch.device("cuda", 0)
    E, n, T = o.episodes, o.n, o.T
    a = bench.parse(["--n", str(n), "--m", str(n), "--T", str(T), "--cpu-baseline", "0", "--secondary", "0"])
    use_rnn = bool(o.use_rnn)
    args = bench.make_args(
        a, E, selector="sap" if o.learner == "sap_q_learner" else "eps", agent="rnn", use_rnn=use_rnn,
        fused_linear_unroll=not use_rnn, reuse_batch=False, epsilon_start=0.1, epsilon_finish=0.1,
        mixer=None, lr=5e-4, gamma=0.99, grad_norm_clip=10.0, double_q=True, target_update_interval_or_tau=0.01,
        standardise_rewards=True, standardise_returns=False, learner_log_interval=10 ** 12,
        use_mps_action_selection=False, unfused_unroll=False)
    runner = r_REGISTRY["gpu"](args, bench.NullLogger())
    env = runner.get_env()
    torch.manual_seed(a.seed)
    mac = mac_REGISTRY["basic_mac"](env.scheme, {"agents": n}, args)
    mac.to(dev)
    runner.setup(env.scheme, {"agents": n}, env.preprocess, mac)
    learner = le_REGISTRY[o.learner](mac, env.scheme, bench.NullLogger(), args)
    buf = ReplayBuffer(env.scheme, {"agents": n}, E, T + 1, preprocess=env.preprocess, device=dev)
    buf.insert_episode_batch(runner.run(test_mode=False))
    batch = buf.sample(E, rng=np.random.RandomState(a.seed))
    agents = (mac.agent, learner.target_mac.agent)

    step = [0]

    def train(unfused):
        for ag in agents:
            ag.args.unfused_unroll = unfused
        learner.train(batch, step[0], step[0])
        step[0] += 1

    for _ in range(o.warmup):
        train(False)
        train(True)
    fused, unfused = [], []
    for _ in range(o.repeats):  # alternating, so drift hits both alike
        fused += timed(lambda: train(False), 1)
        unfused += timed(lambda: train(True), 1)
    for ag in agents:
        ag.args.unfused_unroll = False

    # the two kernels alone, on the batch's inputs
    x = mac._build_sequence_inputs(batch).detach()
    ag = mac.agent
    B, T1, _, K = x.shape
    R = B * n
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    dh_q = torch.randn((T1 * R, 64), device=dev)
    dx1 = torch.empty((T1 * R, 64), device=dev)
    extra, per_sample = {}, 1
    if use_rnn:
        ps = [t.detach() for t in (ag.fc1.weight, ag.fc1.bias, ag.rnn.weight_ih, ag.rnn.weight_hh, ag.rnn.bias_ih,
                                   ag.rnn.bias_hh, ag.fc2.weight, ag.fc2.bias)]
        q, h_all, save = rnn_agent._unroll_launch(x, None, *ps, True)
        fwd = timed(lambda: rnn_agent._unroll_launch(x, None, *ps, True), o.repeats)
        dgi = torch.empty((T1 * R, 192), device=dev)
        dghn = torch.empty((T1 * R, 64), device=dev)

        def bwd_kernel():
            _lib.check(_lib.lib().asg_rnn_agent_unroll_backward(
                vp(dh_q), None, vp(save), vp(h_all), None, 0, vp(ps[2]), vp(ps[3]), T1, R, 64, ag.n_out, 1, vp(dgi),
                vp(dghn), vp(dx1), None, _lib.stream_ptr(dev)))
    else:
        ps = [t.detach() for t in (ag.fc1.weight, ag.fc1.bias, ag.rnn.weight, ag.rnn.bias, ag.fc2.weight,
                                   ag.fc2.bias)]
        q, h_all, x1 = rnn_agent._mlp_launch(x, *ps, True)
        dh = torch.empty((T1 * R, 64), device=dev)
        xs = _lib.i64arr([x.stride(1), x.stride(0), x.stride(2)])

        # these kernels run for tens of microseconds, about what a launch through Python costs:
        # each sample is kInner back-to-back launches into preallocated outputs, divided by kInner
        def fwd_kernel():
            _lib.check(_lib.lib().asg_mlp_agent_unroll(
                vp(x), xs, T1, B, n, K, vp(ps[0]), vp(ps[2]), vp(ps[4]), vp(ps[1]), vp(ps[3]), vp(ps[5]), 64,
                ag.n_out, vp(q), vp(h_all), vp(x1), _lib.stream_ptr(dev)))

        def bwd_one():
            _lib.check(_lib.lib().asg_mlp_agent_unroll_backward(
                vp(dh_q), vp(h_all), vp(x1), vp(ps[2]), T1 * R, 64, vp(dh), vp(dx1), _lib.stream_ptr(dev)))

        def bwd_kernel():
            for _ in range(kInner):
                bwd_one()

        for _ in range(o.warmup):
            fwd_kernel()
        fwd = [t / kInner for t in timed(lambda: [fwd_kernel() for _ in range(kInner)], o.repeats)]
        per_sample = kInner

        # the PyTorch module once over the flattened rows, forward and backward
        xf = x.reshape(T1 * R, K)
        h_any = torch.zeros((1, 64), device=dev)
        dq = torch.randn((T1 * R, ag.n_out), device=dev)

        def flat_torch():
            ag.zero_grad(set_to_none=True)
            rnn_agent.RNNAgent.forward(ag, xf, h_any)[0].backward(dq)

        for _ in range(o.warmup):
            flat_torch()
        # and the same pass through unroll(): the two kernels and the parameter-gradient GEMMs
        dq4 = dq.view(T1, B, n, ag.n_out).permute(1, 0, 2, 3)

        def fused_agent():
            ag.zero_grad(set_to_none=True)
            ag.unroll(x)[0].backward(dq4)

        for _ in range(o.warmup):
            fused_agent()
        flat, fa = [], []
        for _ in range(o.repeats):
            flat += timed(flat_torch, 1)
            fa += timed(fused_agent, 1)
        ag.zero_grad(set_to_none=True)
        extra = {"flat_torch_ms": round(statistics.median(flat), 4),
                 "flat_torch_spread_ms": round(max(flat) - min(flat), 4),
                 "fused_agent_ms": round(statistics.median(fa), 4),
                 "fused_agent_spread_ms": round(max(fa) - min(fa), 4)}

    bwd_kernel()
    bwd = [t / per_sample for t in timed(bwd_kernel, o.repeats)]

    med = statistics.median
    f, u = med(fused), med(unfused)
    f_spread, u_spread = max(fused) - min(fused), max(unfused) - min(unfused)
    print(json.dumps({
        "metric": o.learner + "_train_ms", "shape": {"episodes": E, "n": n, "m": n, "L": a.L, "T": T, "K": K},
        "repeats": o.repeats, "fused_ms": round(f, 4), "unfused_ms": round(u, 4),
        "fused_spread_ms": round(f_spread, 4), "unfused_spread_ms": round(u_spread, 4),
        "ratio_unfused_over_fused": round(u / f, 3), "faster": bool(u - f > u_spread),
        "fwd_kernel_ms": round(med(fwd), 4), "bwd_kernel_ms": round(med(bwd), 4), **extra}))


if __name__ == "__main__":
    main()
