// rollout_env.h -- the env side of the fused rollout kernel: what a wave does for its env before
// the steps (the prologue) and one transition.  Lane = agent; the env's state sits in the LDS
// scratch of rollout_args.h.
#pragma once
#include "rollout_args.h"

#pragma clang fp contract(fast)

namespace asg {

__device__ __forceinline__ float task_scale(const uint64_t *s_scl, int j) {
    return ((s_scl[j >> 6] >> (j & 63)) & 1ull) ? 10.0f : 1.0f;
}

// the launch's first transition without a selection before it: its tasks come from the
// batch's actions row (read in the env prologue, so the transitions themselves issue no
// global load -- a wait for one would drain the previous tile's stores every step)
template <class RA>
__device__ __forceinline__ void rollout_actions_from_batch(RA &ra, int64_t e, int ts, uint16_t *s_act) {
    const int lane = threadIdx.x & 63;
    const int n = ra.n, m = ra.m;
    int err = 0;
    for (int i = lane; i < n; i += 64) {
        const int64_t a64 = ra.assign ? (int64_t)ra.assign[e * n + i] : ra.act[((int64_t)ts * ra.E + e) * n + i];
        int a = (a64 >= 0 && a64 < m) ? (int)a64 : -1;
        if (a < 0) err = ASG_E_ACTION_RANGE;
        s_act[i] = (uint16_t)(a < 0 ? 0 : a);
    }
    err = wave_or_i32(err);
    if (lane == 0 && err) atomicCAS(ra.env_err, 0, err);
}

// The env prologue, one wave's lanes over the env's agents: the previous tasks into s_prev (the
// env's state, or with ra.reset the reset's permutation), the reset row's prev_assigns / filled,
// s_act zeroed (the reset row's tasks) or, without a selection first, read from the batch, and
// the return into *s_ret.  n, m: the env's shape (constants in the SQ64 callers, so the loops
// fold); s_cnt: scratch of the permutation.  The caller fences.
template <int TAB, class RA>
__device__ __forceinline__ void rollout_env_prologue(RA &ra, int64_t e, const EnvKey &key, int n, int m, int lane,
                                                     int *s_cnt, uint16_t *s_act, uint16_t *s_prev, double *s_ret) {
    const int mp = rollout_mp(m), np = rollout_np(n);
    if (!TAB && ra.reset) {
        // asg_reset (reset_kernel): prev_assigns = the first n of a Philox Fisher-Yates
        // permutation of the m tasks (choice(m, n, replace=False), mock :99-105), drawn
        // from the top; the draws are independent of the permutation, so the lanes make
        // them in parallel and one lane applies the swaps (u16 halves of s_cnt: perm, draw)
        uint16_t *s_perm = reinterpret_cast<uint16_t *>(s_cnt), *s_jj = s_perm + mp;
        for (int j = lane; j < m; j += 64) {
            s_perm[j] = (uint16_t)j;
            const u32x4 rr = philox4x32_10(u32x4{(uint32_t)j, 0u, kCtrPerm, ra.episode}, key.k0, key.k1);
            s_jj[j] = (uint16_t)(((uint64_t)rr.x * (uint64_t)(j + 1)) >> 32);
        }
        wave_lds_fence();
        if (lane == 0)
            for (int i = m - 1; i >= 1; --i) {
                const int jj = s_jj[i];
                const uint16_t t = s_perm[i];
                s_perm[i] = s_perm[jj];
                s_perm[jj] = t;
            }
        wave_lds_fence();
        for (int i = lane; i < np; i += 64) {
            const int p = i < n ? (int)s_perm[i] : 0;
            s_prev[i] = (uint16_t)p;
            s_act[i] = 0;
            if (i < n && ra.prevb)
                ra.prevb[((int64_t)ra.ts0 * ra.E + e) * n + i] = (ra.quirks & ASG_QUIRK_PREV_ASSIGNS_ZERO) ? 0 : p;
        }
        if (lane == 0 && ra.filled) ra.filled[(int64_t)ra.ts0 * ra.E + e] = 1;
    } else {
        for (int i = lane; i < np; i += 64) {
            const int p = i < n ? ra.prev[e * n + i] : 0;
            s_prev[i] = (uint16_t)p;
            s_act[i] = 0;
            // table modes' reset in this launch: the permutation the reset's draw kernel
            // left in prev; the reset row's prev_assigns / filled here, its obs by the tiles
            if (TAB && ra.reset && i < n && ra.prevb)
                ra.prevb[((int64_t)ra.ts0 * ra.E + e) * n + i] = (ra.quirks & ASG_QUIRK_PREV_ASSIGNS_ZERO) ? 0 : p;
        }
        if (TAB && ra.reset && lane == 0 && ra.filled) ra.filled[(int64_t)ra.ts0 * ra.E + e] = 1;
    }
    if (lane == 0) *s_ret = ra.reset ? 0.0 : ra.returns[e];
    if (!ra.select_first) rollout_actions_from_batch(ra, e, ra.ts0, s_act);
}

// one transition (mock_constellation_env.py:116-162 + the runner's rows): rewards, returns,
// terminated / filled / prev_assigns rows; the tasks come from the LDS (selected in this
// launch, or read from the batch by the env prologue).  DEFER (the wave-pair mapping, which runs
// a group's transitions after its tiles): the previous tasks are only read (the row of the task
// history before the step's) and the step's reward sum goes to *s_ret as it is; the caller
// folds the sums into the return in step order
template <int TAB, int SQ, bool DEFER = false, class RA>
__device__ __forceinline__ void rollout_transition(RA &ra, int64_t e, int k, int ts, const EnvKey &key,
                                                   const uint64_t *s_scl, int *s_cnt, uint16_t *s_act,
                                                   uint16_t *s_prev, double *s_ret) {
    asm volatile("" : "+s"(e), "+s"(ts));
    // the lane index is recomputed here, not kept across the step loop (spilled, its reload
    // waited behind the previous tile's stores every step)
    int lane_ = threadIdx.x & 63;
    asm volatile("" : "+v"(lane_));
    const int lane = lane_;
    const int n = rs_n<SQ>(ra), m = rs_m<SQ>(ra), mp = rollout_mp(m);
    for (int j = lane; j < mp; j += 64) s_cnt[j] = 0;
    wave_lds_fence();
    for (int i = lane; i < n; i += 64) atomicAdd(&s_cnt[s_act[i]], 1);
    wave_lds_fence();
    const BumpShape bsh = bump_shape(ra.T, ra.wmin, ra.wmax);
    (void)bsh;
    double sum = 0.0;  // Python's sum(rewards), left to right: lane order within each 64-agent chunk
    // two copies of the loop, with and without an injected T_trans: merged, the join after
    // the table load made every transition wait for the previous tile's stores (vmcnt)
    auto rewards = [&](auto with_table) {
        constexpr bool TT = decltype(with_table)::value;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            double rr = 0.0;
            if (i < n) {
                const int j = s_act[i], p = s_prev[i];
                double beta;
                if constexpr (TAB) {
                    beta = ra.par ? mt_par_value(ra.par[(e * m + j) * n + i], k)
                                  : ra.table[(((int64_t)e * ra.T + k) * n + i) * m + j];
                } else if (ASG_ROLLOUT_XSKIP & 1024) {
                    beta = (double)(j & 3) * 0.25;
                } else {
                    const Bump32 b =
                        philox_bump32(key, ra.episode, i * m + j, task_scale(s_scl, j), bsh, ra.dense != 0);
                    beta = bump64_at(b, k);
                }
                const double tt = TT ? ra.T_trans[(int64_t)p * m + j] : (j == p ? 0.0 : 1.0);
                const double pen = tt * (beta > 1e-12 ? 1.0 : 0.0);
                const double bh = beta - ra.lambda_ * pen;
                rr = bh > 0.0 ? bh / (double)s_cnt[j] : bh;
                if (ra.rew) ra.rew[((int64_t)ts * ra.E + e) * n + i] = (float)rr;
                if (!DEFER) s_prev[i] = (uint16_t)j;
                if (ra.prevb)
                    ra.prevb[((int64_t)(ts + 1) * ra.E + e) * n + i] =
                        (ra.quirks & ASG_QUIRK_PREV_ASSIGNS_ZERO) ? 0 : j;
            }
            const int lo = __double2loint(rr), hi = __double2hiint(rr);
            const int cnt = n - i0 < 64 ? n - i0 : 64;
            for (int l2 = 0; l2 < ((ASG_ROLLOUT_XSKIP & 512) ? 1 : cnt); ++l2)
                sum += __hiloint2double(__builtin_amdgcn_readlane(hi, l2), __builtin_amdgcn_readlane(lo, l2));
        }
    };
    if (ra.T_trans) rewards(std::true_type{});
    else rewards(std::false_type{});
    if (lane == 0) {
        // the return lives in LDS: a register copy spilled, its reload drained the stores
        if (DEFER) *s_ret = sum;
        else *s_ret += sum;
        bool term = k + 1 >= ra.T;  // terminated = done != info.get("T", False)
        if (ra.quirks & ASG_QUIRK_PARALLEL_TERMINATED) term = (e != 0);
        if (ra.term) ra.term[(int64_t)ts * ra.E + e] = term;
        if (ra.filled) ra.filled[(int64_t)(ts + 1) * ra.E + e] = 1;
    }
    wave_lds_fence();
}

}  // namespace asg
