// rollout_kernel.h -- the fused rollout kernel: the two env loops over the tiles of
// rollout_tile.h (a wave per env, or a wave pair), the kernel and its instance launcher.
// Included by the three translation units that hold the instances: asg_h2.hip (Philox bumps,
// epsilon-greedy; also the host side, launch_rollout), asg_rollout_tab.hip (table modes) and
// asg_rollout_q.hip (Q output).
#pragma once
#include "rollout_tile.h"

#pragma clang fp contract(fast)

namespace asg {

// One wave per env, its tiles in turn: the run-time-shape instances, and the SQ64 launches with
// a single agent pass (one launch per step, the Q-output schedule), where there is no hidden
// state to keep between passes and the pair mapping's idle wave during the prologue and the
// transition costs 2.8 % (profiles/ab_pairs_headline.txt).
template <bool RNN, bool W2L, bool GEN, int TAB, bool QOUT, int SQ>
__device__ __forceinline__ void rollout_envs_wave(const RolloutArgs &ra, u32x4v *s_h2, const int (&sw)[4]) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = rs_n<SQ>(ra), m = rs_m<SQ>(ra), mp = rollout_mp(m), np = rollout_np(n);
    char *scr = reinterpret_cast<char *>(s_h2 + ra.scratch_off) + wv * rollout_scratch_bytes(n, m);
    uint64_t *s_scl = reinterpret_cast<uint64_t *>(scr + kWaveSclOff);
    double *s_ret = reinterpret_cast<double *>(scr + kWaveRetOff);
    int *s_cnt = reinterpret_cast<int *>(scr + kWaveCntOff);
    uint16_t *s_act = reinterpret_cast<uint16_t *>(s_cnt + mp);
    uint16_t *s_prev = s_act + np;
    const int ntile = np / (16 * kH2NT);
    const int64_t GW = (int64_t)gridDim.x * kH2Waves;
    for (int64_t e0 = (int64_t)blockIdx.x * kH2Waves + wv; e0 < ra.E; e0 += GW) {
        // addresses are recomputed from e each env: strength-reduced per-lane pointers carried
        // across the env loop were spilled around the tile loop, and their reloads waited for
        // every store of the env
        int64_t e = e0;
        asm volatile("" : "+s"(e));
        const EnvKey key = env_key(ra.seed, ra.env_base + e);
        // task scales (choice([1, 1, 1, 10]) per task) as bits (Philox mode), the env's
        // previous tasks
        for (int c = 0; c < (TAB ? 0 : (mp + 63) / 64); ++c) {
            const int j = 64 * c + lane;
            const bool ten = j < m && philox_task_scale(key, ra.episode, j) == 10.0f;
            const uint64_t bits = __ballot(ten);
            if (lane == 0) s_scl[c] = bits;
        }
        rollout_env_prologue<TAB>(ra, e, key, n, m, lane, s_cnt, s_act, s_prev, s_ret);
        wave_lds_fence();
        // iteration 0 with select_first: the selection on the reset row (no transition);
        // every other iteration: transition k, then the agent tiles of row k + 1 (or, past the
        // launch's last selection, the row alone) -- one call site per tile kind
        KRolloutArgs *const kra = (KRolloutArgs *)__builtin_amdgcn_kernarg_segment_ptr();
        const int sf = ra.select_first ? 1 : 0;
        const int nit = ra.k1 - ra.k0 + sf;
        int pass = 0;
        f32x4 hN[4][kH2NT];  // the next agent tile's h_t rows (prefetched by the tile before it)
        bool hpf = false;
        auto has_agent = [&](auto &rr, int it) {
            return rollout_has_agent(it, nit, sf, rr.k0, rr.k1, rr.T, rr.select_last);
        };
        for (int it = 0; it < nit; ++it) {
            auto &ri = rollout_args(kra);  // this iteration's reads of the launch arguments
            const int k = ri.k0 + it - sf;  // k0 - 1 on the select_first iteration
            const int ts = ri.ts0 + (k - ri.k0);
            const bool first_sel = it < sf;
            if (!first_sel && !(ASG_ROLLOUT_XSKIP & 256))
                rollout_transition<TAB, SQ>(rollout_args(kra), e, k, ts, key, s_scl, s_cnt, s_act, s_prev, s_ret);
            const int kk = k + 1;
            if (has_agent(ri, it)) {
                const bool next_agent = has_agent(ri, it + 1);
                for (int sub = 0; sub < ntile; ++sub) {
                    // the next agent tile: this pass's next tile (same h_t source), else tile 0
                    // of the next pass (h_t = the h' this pass writes)
                    HNext nx{nullptr, kHid, 0, 0};
                    if (sub + 1 < ntile) nx = HNext{pass == 0 ? ri.Hin : ri.Hout, pass == 0 ? ri.hs : kHid,
                                                    (int64_t)(16 * kH2NT) * (sub + 1), 1};
                    else if (next_agent) nx = HNext{ri.Hout, kHid, 0, 1};
                    // the reset row (select_first) is stored here when the reset runs in this launch
                    rollout_tile<RNN, W2L, GEN, TAB, QOUT, true, SQ>(rollout_args(kra), e, sub, kk, ts + 1,
                                                                     !first_sel || ri.reset, !first_sel, pass, key, s_scl,
                                                                     s_act, s_act, s_h2, sw, hN, hpf, nx);
                    hpf = nx.mode != 0;
                }
                ++pass;
            } else {
                for (int sub = 0; sub < ntile; ++sub)
                    rollout_tile<RNN, W2L, GEN, TAB, QOUT, false, SQ>(rollout_args(kra), e, sub, kk, ts + 1, true, true, 0,
                                                                      key, s_scl, s_act, s_act, s_h2, sw, hN, false,
                                                                      HNext{nullptr, kHid, 0, 0});
            }
            wave_lds_fence();
        }
        for (int i = lane; i < n; i += 64) ra.prev[e * n + i] = s_prev[i];
        if (lane == 0) ra.returns[e] = *s_ret;
        wave_lds_fence();  // the next env reuses the scratch
    }
}

// A wave pair per env, n = m = 64 (the SQ64 instances): waves 2 p and 2 p + 1 of the workgroup
// are pair p, which takes envs 4 b + p, + 4 gridDim.x, ...; wave `sub` of the pair runs tile
// `sub` of its env in every pass, so its next agent tile is the same 32 agents one step later
// and the hidden state stays in its registers between passes (hN <- h' after the recurrent
// layer): Hin is read by the launch's first agent pass, Hout written by its last.
// Nothing in a step's tiles reads what the step's transition produces, and a tile reads only
// its own 32 of the selected tasks, which its wave wrote: so the steps run in groups of G.
// Within a group a wave runs its tiles back to back with no barrier; the selection of the
// group's j-th step writes row j + 1 of the pair's task history (each wave its own 32 entries)
// and the wave's next tile reads its own 32 of that row.  At the group's end, behind one
// barrier, the two waves share out the group's transitions (the steps of each wave's parity,
// lane = agent, each wave its own counts): step j's tasks are row j, its previous tasks row
// j - 1 (s_prev for the group's first), its float64 reward sum goes to row j's tail.  Behind a
// second barrier one lane folds the sums into the env's return in step order -- the additions
// of the per-step code -- and each wave carries its 32 entries of the group's last rows over
// (row G -> row 0, the last step's tasks -> s_prev, or the env's state after the last group).
// Two barriers per group and one per env for the prologue; every wave of the workgroup executes
// the same number of them (see pair_barrier).
template <bool RNN, bool W2L, int TAB, bool QOUT>
__device__ __forceinline__ void rollout_envs_pair(const RolloutArgs &ra, u32x4v *s_h2, const int (&sw)[4]) {
    constexpr int SQ = 64, n = 64, m = 64;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pr = wv >> 1, sub = wv & 1;
    const bool trw = sub == (pr >> 1);  // the prologue's and the return's wave (on another SIMD from pair to pair)
    char *scr = reinterpret_cast<char *>(s_h2 + ra.scratch_off) + pr * pair_scratch_bytes(ra.defer);
    uint64_t *s_scl = reinterpret_cast<uint64_t *>(scr + kPairSclOff + kPairSclStride * sub);
    double *s_ret = reinterpret_cast<double *>(scr + kPairRetOff);
    int *s_cnt = reinterpret_cast<int *>(scr + kPairCntOff + kPairCntStride * sub);
    uint16_t *s_prev = reinterpret_cast<uint16_t *>(scr + kPairPrevOff);
    uint16_t *s_hist = reinterpret_cast<uint16_t *>(scr + kPairHistOff);
    auto s_sum = [&](int j) { return reinterpret_cast<double *>(s_hist + kPairRow * j + kPairSumOff); };
    constexpr int kPairs = kH2Waves / 2;
    const int64_t GP = (int64_t)gridDim.x * kPairs;
    // the loop bound is the workgroup's: a pair past E skips the work and takes the barriers
    for (int64_t eb = (int64_t)blockIdx.x * kPairs; eb < ra.E; eb += GP) {
        int64_t e = eb + pr;
        asm volatile("" : "+s"(e));
        const bool active = e < ra.E;
        const EnvKey key = env_key(ra.seed, ra.env_base + e);
        // the lane index anew for the prologue (and below for the group's end): per-lane addresses
        // formed from a kernel-wide one were hoisted out of the env loop and spilled
        int lane = threadIdx.x & 63;
        asm volatile("" : "+v"(lane));
        if (active) {
            // task scales as bits (Philox mode): each wave its own copy
            if (!TAB) {
                const bool ten = philox_task_scale(key, ra.episode, lane) == 10.0f;
                const uint64_t bits = __ballot(ten);
                if (lane == 0) s_scl[0] = bits;
            }
            // the step's tasks: row 0 of the history
            if (trw) rollout_env_prologue<TAB>(ra, e, key, n, m, lane, s_cnt, s_hist, s_prev, s_ret);
        }
        wave_lds_fence();
        pair_barrier();  // the batch's tasks (row 0) and the previous tasks reach the other wave
        KRolloutArgs *const kra = (KRolloutArgs *)__builtin_amdgcn_kernarg_segment_ptr();
        const int sf = ra.select_first ? 1 : 0;
        const int nit = ra.k1 - ra.k0 + sf;
        f32x4 hN[4][kH2NT];  // the wave's h_t rows: loaded by pass 0, h' of the pass before after it
        auto has_agent = [&](auto &rr, int it) {
            return rollout_has_agent(it, nit, sf, rr.k0, rr.k1, rr.T, rr.select_last);
        };
        // groups of G steps: the tiles of each step, then the group's transitions.  Every trip
        // count below is launch-uniform (nit, G), so each wave of the workgroup meets the same
        // barriers
        for (int g0 = 0; g0 < nit; g0 += rollout_args(kra).defer) {
            const int gn = min(rollout_args(kra).defer, nit - g0);
            // a pass's index is its step's: only the launch's last step can lack an agent pass
            for (int j = 0; j < gn; ++j) {
                const int it = g0 + j, pass = it;
                auto &ri = rollout_args(kra);
                const int k = ri.k0 + it - sf;
                const int ts = ri.ts0 + (k - ri.k0);
                const bool first_sel = it < sf;
                const bool agent = has_agent(ri, it);
                // the step's tasks: row j of the history; its selection writes row j + 1
                uint16_t *const sa = s_hist + kPairRow * j, *const saw = sa + kPairRow;
                if (active) {
                    const int kk = k + 1;
                    if (agent) {
                        // the launch's last agent pass stores h' (a scalar: as a bool it went through
                        // a byte of scratch, reloaded behind the tile's stores)
                        const int last = __builtin_amdgcn_readfirstlane(has_agent(ri, it + 1) ? 0 : 1);
                        rollout_tile<RNN, W2L, false, TAB, QOUT, true, SQ>(rollout_args(kra), e, sub, kk, ts + 1,
                                                                           !first_sel || ri.reset, !first_sel, pass, key,
                                                                           s_scl, sa, saw, s_h2, sw, hN, pass > 0,
                                                                           HKeep{last});
                    } else {
                        rollout_tile<RNN, W2L, false, TAB, QOUT, false, SQ>(rollout_args(kra), e, sub, kk, ts + 1, true, true,
                                                                            0, key, s_scl, sa, saw, s_h2, sw, hN, false,
                                                                            HKeep{0});
                    }
                }
                wave_lds_fence();
            }
            pair_barrier();  // the group's tasks (rows 0 .. gn) reach both waves' transitions
            // the wave's 32 entries of what the next group (or the env's state) takes over: the
            // previous tasks after the group's last step, and the tasks its last selection chose.
            // Read before the second barrier, written after it: between the two barriers the
            // rows and s_prev are read-only
            int lane = threadIdx.x & 63;
            asm volatile("" : "+v"(lane));
            const int own = 32 * sub + (lane & 31);
            const bool moved = g0 + gn > sf;  // the group's last step has a transition
            uint16_t t_last = 0, t_next = 0;
            if (active) {
                // steps of the wave's parity (of the launch's step index: an odd G alternates)
                for (int j = (sub + g0) & 1; j < gn; j += 2) {
                    const int it = g0 + j;
                    if (it < sf || (ASG_ROLLOUT_XSKIP & 256)) continue;  // the reset row's selection: no transition
                    auto &ri = rollout_args(kra);
                    const int k = ri.k0 + it - sf;
                    const int ts = ri.ts0 + (k - ri.k0);
                    // the tasks before step j's: the step before it in this group, else s_prev
                    uint16_t *const pv = (j == 0 || it - 1 < sf) ? s_prev : s_hist + kPairRow * (j - 1);
                    rollout_transition<TAB, SQ, true>(rollout_args(kra), e, k, ts, key, s_scl, s_cnt, s_hist + kPairRow * j,
                                                      pv, s_sum(j));
                }
                t_last = moved ? s_hist[kPairRow * (gn - 1) + own] : s_prev[own];
                t_next = s_hist[kPairRow * gn + own];
            }
            pair_barrier();  // the sums reach the fold; the history is free for the next group
            if (active) {
                const bool more = g0 + gn < nit;
                if (lane < 32) {
                    if (more) {
                        s_prev[own] = t_last;
                        s_hist[own] = t_next;
                    } else {
                        ra.prev[e * n + own] = t_last;
                    }
                }
                if (trw && lane == 0) {
                    // ret = (ret + S_j) + S_j+1 ...: the per-step code's additions, in its order
                    double ret = *s_ret;
                    for (int j = 0; j < gn; ++j)
                        if (g0 + j >= sf && !(ASG_ROLLOUT_XSKIP & 256)) ret += *s_sum(j);
                    *s_ret = ret;
                    if (!more) ra.returns[e] = ret;
                }
            }
            wave_lds_fence();
        }
    }
}

template <bool RNN, bool W2L, bool GEN, int TAB, bool QOUT, int SQ, bool PAIR = false>
__global__ void __launch_bounds__(64 * kH2Waves) __attribute__((amdgpu_waves_per_eu(kH2WavesPerSimd)))
rollout_kernel(RolloutArgs ra) {
    static_assert(!PAIR || (SQ == 64 && !GEN && !QOUT), "the wave-pair mapping: n = m = 64, selecting instances");
    extern __shared__ u32x4v s_h2[];
    int sw[4];
    h2_stage<RNN, W2L>(rollout_h2args(ra), s_h2, sw);
    __syncthreads();
    if constexpr (PAIR) rollout_envs_pair<RNN, W2L, TAB, QOUT>(ra, s_h2, sw);
    else rollout_envs_wave<RNN, W2L, GEN, TAB, QOUT, SQ>(ra, s_h2, sw);
}

// TAB: 0 = Philox bumps, 1 = the dense float32 table (injected sat_prox_mat), 2 = the compact
// one (MT19937 draws: RolloutArgs::tmask)
template <int TAB, bool QOUT>
static hipError_t launch_rollout_inst(const RolloutArgs &ra, const RolloutLaunch &lc, hipStream_t s) {
#define LR_(RNN, W2L, GEN, SQ, PAIR)                                                                            \
    hipLaunchKernelGGL((rollout_kernel<RNN, W2L, GEN, TAB, QOUT, SQ, PAIR>), dim3(lc.grid), dim3(64 * kH2Waves), lc.lds, \
                       s, ra)
#define LR2_(RNN)                                                                              \
    do {                                                                                       \
        if (lc.sq64 && lc.pair) {                                                              \
            if constexpr (QOUT) return hipErrorInvalidValue; /* single-pass launches only */   \
            else LR_(RNN, true, false, 64, true);                                              \
        } else if (lc.sq64) {                                                                  \
            LR_(RNN, true, false, 64, false);                                                  \
        } else if (lc.w2l) {                                                                   \
            if (lc.gen) LR_(RNN, true, true, 0, false); else LR_(RNN, true, false, 0, false);   \
        } else {                                                                               \
            if (lc.gen) LR_(RNN, false, true, 0, false); else LR_(RNN, false, false, 0, false); \
        }                                                                                      \
    } while (0)
    if (lc.rnn) LR2_(true); else LR2_(false);
#undef LR2_
#undef LR_
    return hipGetLastError();
}
hipError_t launch_rollout_tab(const RolloutArgs &ra, const RolloutLaunch &lc, hipStream_t s);
hipError_t launch_rollout_q(const RolloutArgs &ra, const RolloutLaunch &lc, hipStream_t s);

}  // namespace asg
