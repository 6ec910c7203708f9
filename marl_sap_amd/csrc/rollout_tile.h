// rollout_tile.h -- the fused rollout kernel (device side) and its instance launcher, shared
// by the three translation units that hold its instances: asg_h2.hip (Philox bumps,
// epsilon-greedy; also the host side, launch_rollout), asg_rollout_tab.hip (table modes) and
// asg_rollout_q.hip (Q output).
//
// Reference: envs/mock_constellation_env.py:94-175 (reset, step, pre-transition data),
// runners/episode_runner.py:60-127 (the loop the kernel fuses: select(0); for t: step(t),
// select(t + 1)); the agent and the selection as in h2_tile.h.
#pragma once
#include "h2_tile.h"

#pragma clang fp contract(fast)

namespace asg {

// =====================================================================================
// Fused rollout (mock env, Philox bumps): for every env, transitions k0 .. k1 - 1 and the
// agent forward + epsilon-greedy selection of the rows in between, in one launch.  One wave
// per env (persistent over envs): the transition runs with lane = agent (collision counts,
// float64 rewards summed in agent order, the env's previous / selected tasks and task scales
// in the wave's LDS scratch -- never re-read from HBM); the env's 32-agent tiles then
// generate the next observation row in the split-f16 MFMA operand layout (lane (r, q)
// evaluates the Philox bumps of tasks 32 u + 16 c + 4 q + v), write it to the batch and feed
// fc1 from registers: the agent never reads an observation back.  Selected tasks go to the
// batch's actions row and to the LDS, where the next transition reads them.  The hidden
// state lives in Hout between passes (Hin for the first) -- except in the n = m = 64 launches
// with two or more agent passes, where a wave PAIR shares the env, each wave runs the same
// 32-agent tile in every pass and keeps its h in registers (rollout_envs_pair: Hin read by the
// first pass, Hout written by the last).  Results are those of the separate
// launches: asg_reset / asg_step rows, and the agent kernel's actions and hidden state
// (per-row scales make a row's result independent of its tile's other rows).
// =====================================================================================
struct RolloutArgs {
    // time-major batch: row 0 of each field ([T+1][E][..] storage: row t at base + t * E * ..,
    // the row strides derived from E, n, m, K); NULL = absent
    float *obs, *beta, *rew;
    uint8_t *avail, *term;
    int64_t *onehot, *act, *prevb, *filled;
    int ts0;  // batch row of transition k0
    // env state
    int *prev;
    double *returns;
    const double *T_trans;
    int *env_err;
    double lambda_;
    uint64_t seed;
    int64_t env_base, E;
    uint32_t episode, quirks;
    int n, m, T, L, dense;
    float wmin, wmax;
    int k0, k1, select_first, select_last;
    int reset;  // the envs' reset (asg_reset) runs first, in this launch
    // benefits: NULL = Philox bumps regenerated in registers; else the handle's float64 table
    // [E][T][n][m] (MT19937 compat / injected sat_prox_mat), read for the L lookahead rows
    const double *table;   // injected float64 benefits (rewards), or
    const double2 *par;    // the MT19937 reset's draws: rewards evaluated from them (mt_par_value)
    const float *table32;  // the benefits rounded to float32: the lookahead rows' reads
    // MT19937 draws: table32 is COMPACT (per (env, t) slice the bump pairs only, (agent, task)
    // order; asg_env_mt.hip:mt_table_kernel): their masks [E][n][W] and each word's first index
    const uint64_t *tmask;
    const int *toff;
    // QOUT instances: the agent's Q rows [E n][m] f32 (the forward of asg_rnn_agent_forward)
    // instead of the epsilon-greedy selection -- a selector outside the kernel (SAP) acts on them
    float *Q;
    // agent
    const u32x4v *pk;
    const float *W1T, *Hin;
    int64_t hs;
    float *Hout;
    const float *b1, *bi, *bh, *b2;
    int w1_lds, w1_off;  // LDS-resident W1 slices: [s0 + w1_off, s0 + w1_off + w1_lds)
    float epsilon;
    uint32_t sk0, sk1, counter;
    int *sel_err;
    int64_t scratch_off;  // LDS scratch (u32x4v units): a slot per wave, or pair_scratch_bytes(defer) per wave pair
    int defer;            // the pair mapping: steps per group of deferred transitions (G >= 1)
    // bids_as_actions (asg_step_forward): the tasks of transition k0 are the handle's LSA
    // assignments of the bids row [E][n] instead of the batch's actions row
    const int *assign;
};

// The launch arguments as the tiles and transitions read them: a kernarg-segment pointer made
// opaque per call, so each call re-reads what it uses with scalar loads instead of the kernel
// keeping ~40 uniform values live from its entry (they overflowed the SGPR file and were spilled
// to VGPR lanes, ~500 v_readlane reloads in the tile body).
typedef __attribute__((address_space(4))) const RolloutArgs KRolloutArgs;
__device__ __forceinline__ KRolloutArgs &rollout_args(KRolloutArgs *p) {
    asm volatile("" : "+s"(p));
    return *p;
}

__host__ __device__ constexpr int rollout_mp(int m) { return (m + 31) / 32 * 32; }
__host__ __device__ constexpr int rollout_np(int n) { return (n + 31) / 32 * 32; }
// per wave: task-scale bits [4] u64 | the env's return f64 | collision counts [mp] int |
// selected / previous tasks [np] u16 each
__host__ __device__ constexpr int rollout_scratch_bytes(int n, int m) {
    return (40 + 4 * rollout_mp(m) + 4 * rollout_np(n) + 15) / 16 * 16;
}

// Orders one wave's LDS scratch accesses across its lanes (the collision counts, the actions /
// previous tasks, the env's return).  A wave's LDS instructions complete in issue order, so a
// wavefront-scope fence (compiler ordering, no wait) is enough (a workgroup-scope fence's
// release also waits for every outstanding global store, s_waitcnt vmcnt(0): three drains of
// the previous tile's row stores per transition).
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The env shape as the rollout code reads it: SQ = 0 takes n, m from the launch arguments; the
// SQ = 64 instances (n = m = 64, configs[2]'s shape; Philox and table modes alike) see them as
// compile-time constants, so the tile's loops unroll and its row / task offsets fold into
// immediates.  (L stays a runtime value: with L = 3 fixed too the unrolled lookahead loop
// spilled 28 VGPRs instead of 14 and ran 0.71 vs 0.57 ms/step.)
template <int SQ, class RA>
__device__ __forceinline__ int rs_n(RA &ra) { return SQ ? SQ : ra.n; }
template <int SQ, class RA>
__device__ __forceinline__ int rs_m(RA &ra) { return SQ ? SQ : ra.m; }

template <int SQ = 0, class RA>
__device__ __forceinline__ H2Args rollout_h2args(RA &ra) {
    H2Args a{};
    const int n = rs_n<SQ>(ra), m = rs_m<SQ>(ra), L = ra.L;
    a.R = ra.E * n;
    a.g.K = m * (L + 1);
    a.g.P = m;
    a.g.NB = L + 1;
    a.g.Pp = rollout_mp(m);
    a.g.Kp = a.g.Pp * (L + 1);
    a.g.prefix = 1;
    a.g.nout = m;
    a.g.nct = (m + 15) / 16;
    a.pre = 1;
    a.pk = ra.pk;
    a.W1T = ra.W1T;
    a.b1 = ra.b1;
    a.bi = ra.bi;
    a.bh = ra.bh;
    a.b2 = ra.b2;
    a.Hout = ra.Hout;
    a.w1_lds = ra.w1_lds;
    a.w1_off = ra.w1_off;
    a.sel = SelectArgs{nullptr, 0, 0, n, ra.epsilon, ra.sk0, ra.sk1, ra.counter, ra.env_base * n, nullptr,
                       (int64_t)n, 1, ra.sel_err};
    return a;
}

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

__device__ __forceinline__ void st_f4(float *p, float a, float b, float c, float d) {
    *reinterpret_cast<f32x4 *>(p) = f32x4{a, b, c, d};
}
__device__ __forceinline__ void st_i64x2(int64_t *p, long long a, long long b) {
    *reinterpret_cast<i64x2v *>(p) = i64x2v{a, b};
}

// The rows of a 32-agent tile that depend on nothing but the tile's actions, n = m = 64 (the
// SQ64 instances): obs block 0 = onehot(a), actions_onehot (oh, NULL = none) and avail = 1 (av,
// NULL = none), every store instruction 1 KiB of whole lines instead of the MFMA operand layout
// of the generated blocks (16 rows x 64 B per instruction for block 0, 16-B pieces at a 32-B
// stride for the int64 one-hot).  Any lane can read any row's action from the wave's LDS:
//   actions_onehot: the tile's 32 rows x 512 B are one 16 KiB span; instruction i writes rows
//     2 i and 2 i + 1 whole: lane l takes row 2 i + (l >> 5), columns 2 (l & 31) and the next
//   obs block 0: instruction i writes rows 4 i .. 4 i + 3, 256 B each: lane l takes row
//     4 i + (l >> 4), columns 4 (l & 15) .. + 3
//   avail: the tile's 2 KiB, two instructions
// ob / oh / av: the tile's first row (wave-uniform), K the obs row length; sa: the tile's
// actions; have_act false (the reset row): block 0 is zeros.  The lane index is laundered
// here and every address is a uniform base plus a 32-bit lane offset: no per-lane 64-bit
// pointer to keep across tiles.
__device__ __forceinline__ void tile_action_rows64(float *ob, int64_t *oh, uint8_t *av, int K, const uint16_t *sa,
                                                   bool have_act) {
    constexpr int RT = 16 * kH2NT, M = 64;
    int lane = threadIdx.x & 63;
    asm volatile("" : "+v"(lane));
    {
        const int rl = lane >> 4, c0 = 4 * (lane & 15);
        const uint32_t lo = (uint32_t)(rl * K + c0);
        // no action: a column no action reaches (one select per tile; the LDS reads stay
        // unconditional, a branch per instruction would wait for each read on its own)
        const int cc = have_act ? c0 : 0x10000;
#pragma unroll
        for (int i = 0; i < RT / 4; ++i) {
            const int d = (int)sa[4 * i + rl] - cc;
            st_f4(ob + (uint32_t)(4 * i * K) + lo, d == 0, d == 1, d == 2, d == 3);
        }
    }
    if (oh) {
        const int rl = lane >> 5, c0 = 2 * (lane & 31);
        const uint32_t lo = (uint32_t)(2 * lane);
#pragma unroll
        for (int i = 0; i < RT / 2; ++i) {
            const int d = (int)sa[2 * i + rl] - c0;
            st_i64x2(oh + 2 * M * i + lo, d == 0, d == 1);
        }
    }
    if (av) {
        const uint32_t lo = (uint32_t)(16 * lane);
#pragma unroll
        for (int i = 0; i < RT * M / 1024; ++i)
            *reinterpret_cast<u32x4v *>(av + 1024 * i + lo) = u32x4v{0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u};
    }
}

// One 32-agent tile of env e for observation row kk (batch row tsr): write the row (STORES:
// one-hot block and actions_onehot of the transition before it, avail, lookahead blocks,
// beta) and, AGENT, run fc1 on the generated blocks plus the recurrent layer, fc2 and the
// selection of row kk.  have_act: block 0 is onehot(s_act) (else zeros: the reset row).
// The agent tile's h_t rows (RNN): hN holds them on entry when the previous agent tile
// prefetched them (hpf), else they are loaded at the tile start; either way they are waited
// for with the one-hot gather, before the tile's stores (a wait after fc1 would drain every
// store of the tile: gfx9's vmcnt retires memory operations in order).  After the recurrent
// layer the tile issues the NEXT agent tile's h_t loads into hN (nsrc: its source rows, row
// nrow0 on, stride nhs; NULL source = zeros; nmode 0 = no next agent tile in this env).
// With a wave pair per env (HKeep) hN instead takes this tile's h' in registers: hpf is true
// from the launch's second pass on and nothing is loaded.
// The compact same-seed table (RolloutArgs::tmask): the 4 tasks j0 .. j0 + 3 of a row (j0 % 4 == 0,
// one mask word) are the set bits `nib` of the row's mask word at sh = j0 % 64, and their values
// sit at consecutive compact indices from pos = the word's first index + the bumps below sh.  One
// 16-byte load at pos (4-byte aligned; nib == 0: no load) then the expansion below
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ f32x4 compact_quad_load(const float *slice, uint64_t mw, int off, int sh, bool okrow,
                                                   uint32_t *nib_out) {
    const uint32_t nib = okrow ? (uint32_t)(mw >> sh) & 15u : 0u;
    *nib_out = nib;
    if (nib == 0u) return f32x4{0.f, 0.f, 0.f, 0.f};
    const int pos = off + (int)__popcll(mw & ((1ull << sh) - 1ull));
    if (ASG_ROLLOUT_XSKIP & 2048) return f32x4{0.5f, 0.25f, 0.125f, (float)pos};
    const f32x4u x = *reinterpret_cast<const f32x4u *>(slice + pos);
    return f32x4{x.x, x.y, x.z, x.w};
}
__device__ __forceinline__ uint32_t compact_nib(uint64_t mw, int sh, bool okrow) {
    return okrow ? (uint32_t)(mw >> sh) & 15u : 0u;
}
// the quad's 4 values from its packed bumps x (value v = the (rank of v)-th packed one, 0 off the mask)
__device__ __forceinline__ float4 compact_expand(f32x4 x, uint32_t nib) {
    if (ASG_ROLLOUT_XSKIP & 4096) return make_float4(x.x, x.y, x.z, x.w + (float)nib);
    const bool b0 = nib & 1u, b1 = nib & 2u, b2 = nib & 4u, b3 = nib & 8u;
    const float a01 = b0 ? x.y : x.x, a12 = b0 ? x.z : x.y, a23 = b0 ? x.w : x.z;  // rank shifted by b0
    const float r2 = b1 ? a12 : a01;                                               // rank b0 + b1
    const float r3 = b2 ? (b1 ? a23 : a12) : (b1 ? a12 : a01);                     // rank b0 + b1 + b2
    return make_float4(b0 ? x.x : 0.f, b1 ? a01 : 0.f, b2 ? r2 : 0.f, b3 ? r3 : 0.f);
}

struct HNext {
    const float *src;
    int64_t stride, row0;
    int mode;
};
// The SQ64 instances (wave pair per env, below) have no next-tile loads: a wave's next agent
// tile is the same 32 agents one step later, so hN takes h' in registers after the recurrent
// layer, and h' goes to Hout only when `store` says so (the launch's last agent pass).
struct HKeep {
    int store;
};

// With W2 in LDS and an fc1 slice in L2 (64 x 64: 1 of 6; the SQ64 instances), that slice is
// the tile's first (w1_off = 1; as the last one its weights were read behind nearly all the
// tile's stores: 0.556-0.559 vs 0.575 ms/step; its rows stored after its MFMAs as well spilled
// 43 VGPRs and ran 0.65 ms).
// The table modes load each chunk's first lookahead blocks at the chunk start: kTabPre blocks
// of the dense table, kTabPreCmp of the compact one (MT19937 draws; SQ64 GRU instance: 0 VGPRs
// spilled with 1 block, 51 with 2, 84 with 3; the dense instance: 36 / 19 / 36)
constexpr int kTabPre = 2;
constexpr int kTabPreCmp = 1;
// s_act: the env's tasks the row is built from; s_actw: where the selection puts the row's own
// (the same array with one wave per env; the other parity buffer with a wave pair per env).
// nx: HNext (run-time shapes), HKeep (SQ64).
template <bool RNN, bool W2L, bool GEN, int TAB, bool QOUT, bool AGENT, int SQ, class HX, class RA>
__device__ __forceinline__ void rollout_tile(RA &ra, int64_t e, int sub, int kk, int tsr, bool stores,
                                             bool have_act, int pass, const EnvKey &key, const uint64_t *s_scl,
                                             const uint16_t *s_act, uint16_t *s_actw, const u32x4v *Wl,
                                             const int (&sw)[4], f32x4 (&hN)[4][kH2NT], bool hpf, HX nx) {
    constexpr int NT = kH2NT;
    constexpr int RT = 16 * NT;  // rows per tile
    // opaque env / row indices and lane: addresses are formed here from them, not hoisted out
    // of the step and env loops (live across every tile they spill)
    asm volatile("" : "+s"(e), "+s"(tsr), "+s"(kk));
    int lane_ = threadIdx.x & 63;
    asm volatile("" : "+v"(lane_));
    const int lane = lane_, r = lane & 15, q = lane >> 4;
    const int n = rs_n<SQ>(ra), m = rs_m<SQ>(ra), T = ra.T, L = ra.L;
    const int K = m * (L + 1);
    const int Ub = rollout_mp(m) >> 5;
    const int64_t row0 = e * n + RT * sub;
    int64_t rows[NT];
    bool ok[NT];
    int ia[NT], act[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        ia[nt] = RT * sub + 16 * nt + r;
        ok[nt] = !GEN || ia[nt] < n;
        rows[nt] = e * n + ia[nt];
        act[nt] = (have_act && ok[nt]) ? (int)s_act[ia[nt]] : -1;
    }
    // the compact same-seed table's mask words / offsets of the lane's rows (chunk u's word is
    // u / 2): loaded here, with the gather, before the tile's stores -- once per tile when the
    // shape is compile-time 64 tasks (one word), per chunk otherwise
    constexpr bool cmp = TAB == 2;  // the compact same-seed table (MT19937 draws)
    uint64_t cmw[NT];
    int cof[NT];
    auto load_cm = [&](int w) {
        const int W = (m + 63) >> 6;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int64_t r = (e * n + (ok[nt] ? ia[nt] : 0)) * W + w;
            cmw[nt] = cmp ? ra.tmask[r] : 0ull;
            cof[nt] = cmp ? ra.toff[r] : 0;
        }
    };
    if (cmp && SQ == 64) load_cm(0);
    // row stores: batch row tsr (timing variant 32: row 1, env e & 7)
    const int tss = (ASG_ROLLOUT_XSKIP & 32) ? 1 : tsr;
    const int64_t sro = (ASG_ROLLOUT_XSKIP & 32) ? ((e & 7) - e) * n : 0;
    float *obs_r = ra.obs + ((int64_t)tss * ra.E * n + sro) * K;
    // fc1 accumulators start from the one-hot block's W1 columns, gathered (and consumed)
    // before the tile's stores (a load behind them would wait for their acknowledgements:
    // gfx9's vmcnt retires memory operations in order); a rescaled retry gathers again
    f32x4 acc[4][NT];
    int sx[NT];
    if (AGENT) {
        const float scS = pow2f(sw[0] + kH2SxInit);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            sx[nt] = kH2SxInit;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const float4 g = (act[nt] >= 0 && !(ASG_ROLLOUT_XSKIP & 2))
                                     ? *reinterpret_cast<const float4 *>(ra.W1T + act[nt] * kHid + 16 * mt + 4 * q)
                                     : make_float4(0.f, 0.f, 0.f, 0.f);
                acc[mt][nt] = f32x4{g.x, g.y, g.z, g.w} * scS;
            }
        }
    }
    if (AGENT && RNN) {
        if (!hpf) {
            const float *hin = pass == 0 ? ra.Hin : ra.Hout;
            const int64_t hs = pass == 0 ? ra.hs : kHid;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    hN[t][nt] = hin ? *reinterpret_cast<const f32x4 *>(hin + (ok[nt] ? rows[nt] : 0) * hs + 16 * t + 4 * q)
                                    : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        // waited for here, with the gather
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) asm volatile("" : "+v"(hN[t][nt]));
    }
    // w1_off (the SQ64 instances): the L2-resident fc1 slice is the tile's FIRST main slice, so
    // the wait for its weights covers only the prefix rows and the first block's rows of the
    // tile -- as the last slice (round 4) it waited for nearly all of the tile's stores
    if (stores && !(ASG_ROLLOUT_XSKIP & 1)) {
        // obs block 0 = onehot(a) (row kk), actions_onehot (row kk - 1), avail = 1 (row kk)
        // actions_onehot of the transition before the row (none before the reset row)
        int64_t *oh_r = (ra.onehot && have_act) ? ra.onehot + ((int64_t)(tss - 1) * ra.E * n + sro) * m : nullptr;
        uint8_t *ab = ra.avail ? ra.avail + ((int64_t)tss * ra.E * n + sro + row0) * m : nullptr;
        // n = m = 64: the three as whole-line instructions; else in the generated blocks' layout
        if constexpr (SQ == 64)
            tile_action_rows64(obs_r + row0 * K, oh_r ? oh_r + row0 * m : nullptr, ab, K, s_act + RT * sub, have_act);
        for (int u = 0; u < (SQ == 64 ? 0 : Ub); ++u)
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int j0 = 32 * u + 16 * c + 4 * q;
                    const int aa = act[nt];
                    if (!GEN) {
                        st_f4(obs_r + rows[nt] * K + j0, aa == j0, aa == j0 + 1, aa == j0 + 2, aa == j0 + 3);
                        if (oh_r) {
                            st_i64x2(oh_r + rows[nt] * m + j0, aa == j0, aa == j0 + 1);
                            st_i64x2(oh_r + rows[nt] * m + j0 + 2, aa == j0 + 2, aa == j0 + 3);
                        }
                    } else if (ok[nt]) {
#pragma unroll
                        for (int v = 0; v < 4; ++v)
                            if (j0 + v < m) {
                                obs_r[rows[nt] * K + j0 + v] = aa == j0 + v ? 1.0f : 0.0f;
                                if (oh_r) oh_r[rows[nt] * m + j0 + v] = aa == j0 + v;
                            }
                    }
                }
        if (SQ != 64 && ab) {
            const int nrow = GEN ? min(RT, n - RT * sub) : RT;
            int off0 = (GEN ? 1 : 16) * lane;
            asm volatile("" : "+v"(off0));  // not hoisted: a per-lane 64-bit address kept across loops spilled
            if (!GEN) {
                // RT m = 1 KiB x Ub: a uniform trip count, 16 B per lane and whole lines per instruction
                for (int i = 0; i < Ub; ++i)
                    *reinterpret_cast<u32x4v *>(ab + 1024 * i + (uint32_t)off0) =
                        u32x4v{0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u};
            } else {
                for (int off = off0; off < nrow * m; off += 64) ab[off] = 1;
            }
        }
    }
    // ---- the lookahead blocks 1..L (times kk .. kk + L - 1), fc1 on them -------------------
    BumpShape bsh = bump_shape(T, ra.wmin, ra.wmax);
    bsh.q = __builtin_amdgcn_readfirstlane(bsh.q);  // uniform: keep the grid exponent scalar
    const lds_f4v Bs = (lds_f4v)(Wl + rec_f4(RNN));
    const u32x4v *W1g = ra.pk + 1;
    const int s0 = Ub, s_l2 = s0 + ra.w1_off + ra.w1_lds;
    float *beta_r = ra.beta ? ra.beta + ((int64_t)tss * ra.E * n + sro) * m : nullptr;
    const bool live = kk < T;  // rows past T are zeros: no bump parameters needed
    for (int attempt = 0;; ++attempt) {
        float scx[NT], rmax[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            scx[nt] = pow2f(AGENT ? sx[nt] : 0);
            rmax[nt] = 0.f;
        }
        if (AGENT && attempt > 0) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const float scS = pow2f(sw[0] + sx[nt]);
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    const float4 g = act[nt] >= 0
                                         ? *reinterpret_cast<const float4 *>(ra.W1T + act[nt] * kHid + 16 * mt + 4 * q)
                                         : make_float4(0.f, 0.f, 0.f, 0.f);
                    acc[mt][nt] = f32x4{g.x, g.y, g.z, g.w} * scS;
                }
            }
        }
        const bool st_now = stores && attempt == 0 && !(ASG_ROLLOUT_XSKIP & 1);
        for (int u = 0; u < Ub; ++u) {
            // bump parameters of the lane's 16 (row, task) pairs of this chunk (Philox mode)
            Bump32 bp[2][4][NT];
            // table modes: the chunk's lookahead values of the first kTabPre blocks, loaded at
            // once at the chunk start (in place of the Philox parameters): one wait behind the
            // tile's stores per chunk instead of one per block (gfx9's in-order vmcnt)
            constexpr int kPre = TAB == 2 ? kTabPreCmp : kTabPre;
            float4 tv[kPre][2][NT];
            if (cmp && SQ != 64) load_cm(u >> 1);
            if constexpr (TAB != 0) {
#pragma unroll
                for (int l = 1; l <= kPre; ++l) {
                    const int t = kk + l - 1;
                    if (l > L || t >= T) continue;
                    const float *trow = ra.table32 + ((int64_t)e * T + t) * n * m;
#pragma unroll
                    for (int c = 0; c < 2; ++c)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) {
                            const int j0 = 32 * u + 16 * c + 4 * q;
                            const float *tp = trow + (int64_t)ia[nt] * m + j0;
                            if constexpr (cmp) {  // the packed bumps: expanded at their use
                                uint32_t nb;
                                const f32x4 x = compact_quad_load(trow, cmw[nt], cof[nt], j0 & 63, ok[nt] && j0 < m, &nb);
                                tv[l - 1][c][nt] = make_float4(x.x, x.y, x.z, x.w);
                            } else if (!GEN) {
                                tv[l - 1][c][nt] = *reinterpret_cast<const float4 *>(tp);
                            } else {
                                float v4[4];
#pragma unroll
                                for (int v = 0; v < 4; ++v) v4[v] = (ok[nt] && j0 + v < m) ? tp[v] : 0.f;
                                tv[l - 1][c][nt] = make_float4(v4[0], v4[1], v4[2], v4[3]);
                            }
                        }
                }
            }
            if constexpr (!TAB) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int jw = 32 * u + 16 * c + 4 * q;
                const uint64_t sbits = s_scl[jw >> 6];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    if (!live) {
#pragma unroll
                        for (int v = 0; v < 4; ++v) bp[c][v][nt] = Bump32{0.f, 0.f, 0.f};
                    } else if (ASG_ROLLOUT_XSKIP & 64) {
#pragma unroll
                        for (int v = 0; v < 4; ++v)
                            bp[c][v][nt] = Bump32{1.0f, (float)((jw + v + ia[nt]) & 15), 0.25f};
                    } else if (!GEN) {
                        // the lane's 4 pairs (j .. j + 3) are one Philox call (m % 4 == 0); their task
                        // scales from one 4-bit field of the scale bits (jw % 4 == 0: no wrap), each
                        // 1.0f or 10.0f as bits (0x3f800000 + b 0x01a00000)
                        float sv[4];
                        const uint32_t nib = (uint32_t)(sbits >> (jw & 63)) & 15u;
#pragma unroll
                        for (int v = 0; v < 4; ++v) sv[v] = __builtin_bit_cast(float, 0x3f800000u + ((nib >> v) & 1u) * 0x01a00000u);
                        Bump32 b4[4];
                        philox_bump32x4(key, ra.episode, ia[nt] * m + jw, sv, bsh, ra.dense != 0, b4);
#pragma unroll
                        for (int v = 0; v < 4; ++v) bp[c][v][nt] = b4[v];
                    } else {
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const int j = jw + v;
                            const bool in = j < m;
                            const float sv = ((sbits >> (j & 63)) & 1ull) ? 10.0f : 1.0f;
                            bp[c][v][nt] = philox_bump32(key, ra.episode, ia[nt] * m + (in ? j : 0), sv, bsh,
                                                         ra.dense != 0);
                            if (!in) bp[c][v][nt].scale = 0.f;
                        }
                    }
                }
            }
            }
            for (int l = 1; l <= L; ++l) {
                const int t = kk + l - 1;

                // the 2 x NT x 4 bump values, straight-line (one uniform branch per block: rows
                // past T are zeros)
                float4 xv[2][NT];
                if (TAB && t < T && l <= kPre) {
#pragma unroll
                    for (int c = 0; c < 2; ++c)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) {
                            // l is a loop variable: the preloaded block by a uniform select
                            float4 x = tv[0][c][nt];
#pragma unroll
                            for (int ll = 2; ll <= kPre; ++ll) x = l == ll ? tv[ll - 1][c][nt] : x;
                            if constexpr (cmp) {
                                const int j0 = 32 * u + 16 * c + 4 * q;
                                x = compact_expand(f32x4{x.x, x.y, x.z, x.w},
                                                   compact_nib(cmw[nt], j0 & 63, ok[nt] && j0 < m));
                            }
                            xv[c][nt] = x;
                        }
                } else if (TAB && t < T) {
                    // the table's benefits rounded to float32 (the batch's dtype, as the separate
                    // step's rows), from its float32 copy: B[e][t][row][j0 .. j0 + 3], one 16-byte
                    // load (the float64 table would take two behind the tile's stores)
                    const float *trow = ra.table32 + ((int64_t)e * T + t) * n * m;
#pragma unroll
                    for (int c = 0; c < 2; ++c)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) {
                            const int j0 = 32 * u + 16 * c + 4 * q;
                            const float *tp = trow + (int64_t)ia[nt] * m + j0;
                            if constexpr (cmp) {
                                uint32_t nb;
                                const f32x4 x = compact_quad_load(trow, cmw[nt], cof[nt], j0 & 63, ok[nt] && j0 < m, &nb);
                                xv[c][nt] = compact_expand(x, nb);
                            } else if (!GEN) {
                                xv[c][nt] = *reinterpret_cast<const float4 *>(tp);
                            } else {
                                float v4[4];
#pragma unroll
                                for (int v = 0; v < 4; ++v) v4[v] = (ok[nt] && j0 + v < m) ? tp[v] : 0.f;
                                xv[c][nt] = make_float4(v4[0], v4[1], v4[2], v4[3]);
                            }
                        }
                } else if (!TAB && t < T) {
#pragma unroll
                    for (int c = 0; c < 2; ++c)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt)
                            xv[c][nt] = make_float4(bump32_at(bp[c][0][nt], t), bump32_at(bp[c][1][nt], t),
                                                    bump32_at(bp[c][2][nt], t), bump32_at(bp[c][3][nt], t));
                } else {
#pragma unroll
                    for (int c = 0; c < 2; ++c)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) xv[c][nt] = make_float4(0.f, 0.f, 0.f, 0.f);
                }
                auto store_rows = [&]() {
#pragma unroll
                    for (int c = 0; c < 2; ++c)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) {
                            const float vv[4] = {xv[c][nt].x, xv[c][nt].y, xv[c][nt].z, xv[c][nt].w};
                            const int j0 = 32 * u + 16 * c + 4 * q;
                            if (!GEN) {
                                st_f4(obs_r + rows[nt] * K + m * l + j0, vv[0], vv[1], vv[2], vv[3]);
                                if (l == 1 && beta_r) st_f4(beta_r + rows[nt] * m + j0, vv[0], vv[1], vv[2], vv[3]);
                            } else if (ok[nt]) {
#pragma unroll
                                for (int v = 0; v < 4; ++v)
                                    if (j0 + v < m) {
                                        obs_r[rows[nt] * K + m * l + j0 + v] = vv[v];
                                        if (l == 1 && beta_r) beta_r[rows[nt] * m + j0 + v] = vv[v];
                                    }
                            }
                        }
                };
                // an L2 weight slice (no W2 in LDS: the large shapes, 19 of 24 slices at 256 x 256):
                // its weights are loaded before this block's row stores and the stores follow the
                // MFMAs, so the loads wait for the previous block's stores only
                const bool late = !W2L && AGENT && l * Ub + u >= s_l2;
                if (st_now && !late) store_rows();
                if (AGENT) {
                    // the agent kernel's slice: abs-max, split, 4 output tiles x NT rows of MFMAs
                    const int sl = l * Ub + u;
                    u32x4v xp[NT][2];
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        rmax[nt] = absmax4(absmax4(rmax[nt], xv[0][nt]), xv[1][nt]);
                        const float x8[8] = {xv[0][nt].x, xv[0][nt].y, xv[0][nt].z, xv[0][nt].w,
                                             xv[1][nt].x, xv[1][nt].y, xv[1][nt].z, xv[1][nt].w};
                        split2s(x8, scx[nt], xp[nt][0], xp[nt][1]);
                    }
                    // two copies of the MFMA block: merged after an LDS-or-global select, the
                    // MFMAs would wait for vmcnt(0) -- every store of the tile -- each slice
                    auto mma = [&](bool lds) {
#pragma unroll
                        for (int mt = 0; mt < 4; ++mt) {
                            u32x4v w[2];
                            if (lds) {
                                const lds_u4p W1s = (lds_u4p)(Wl + lds_w1_off(RNN, (m + 15) / 16, W2L));
#pragma unroll
                                for (int pl = 0; pl < 2; ++pl)
                                    w[pl] = W1s[w1_idx((ASG_ROLLOUT_XSKIP & 4) && sl >= s_l2 ? 0 : sl - s0 - ra.w1_off, mt,
                                                       pl, lane)];
                            } else {
#pragma unroll
                                for (int pl = 0; pl < 2; ++pl) w[pl] = W1g[w1_idx(sl, mt, pl, lane)];
                            }
#pragma unroll
                            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = mfma_h2(w, xp[nt], acc[mt][nt]);
                        }
                    };
                    if ((sl >= s0 + ra.w1_off && sl < s_l2) || (ASG_ROLLOUT_XSKIP & 4))
                        mma(true);
                    else
                        mma(false);
                }
                if (st_now && late) store_rows();
            }
        }
        if (!AGENT) return;
        bool over[NT], any = false;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const float rm = row_max4(rmax[nt]);
            over[nt] = rm * scx[nt] >= 32768.f;
            any = any || over[nt];
            if (over[nt]) sx[nt] = h2_scale(rm, -90, 90 - sw[0]);
        }
        if (attempt > 0 || __ballot(any) == 0) break;
    }
    if constexpr (AGENT) {
        H2Args a = rollout_h2args<SQ>(ra);
        a.sel.counter = ra.counter + (uint32_t)pass;
        a.sel.out = ra.act + (int64_t)tsr * ra.E * n;
        if constexpr (QOUT) a.Q = ra.Q;
        float4 hB[4][NT];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                hB[t][nt] = (ASG_ROLLOUT_XSKIP & 8) ? make_float4(0.5f, 0.25f, -0.5f, 0.125f)
                            : RNN ? make_float4(hN[t][nt][0], hN[t][nt][1], hN[t][nt][2], hN[t][nt][3])
                                  : make_float4(0.f, 0.f, 0.f, 0.f);
        f32x4 xB[4][NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const float un = pow2f(-(sw[0] + sx[nt]));
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const f32x4 bb = Bs[4 * mt + q];
#pragma unroll
                for (int v = 0; v < 4; ++v) xB[mt][nt][v] = fmaxf(acc[mt][nt][v] * un + bb[v], 0.f);
            }
        }
        if constexpr (std::is_same<HX, HKeep>::value) {
            // the wave's next agent tile is this one a step later: its h_t is this h'
            auto keep = [&](const f32x4(&hp)[4][NT]) {
                if (!RNN) return;
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) hN[t][nt] = hp[t][nt];
            };
            h2_tail<NT, RNN, !QOUT, W2L, true, GEN, true>(a, Wl, sw, row0, rows, ok, hB, xB, s_actw, RT * sub, keep,
                                                          nx.store != 0);
        } else {
        // the next agent tile's h_t, issued once this tile's recurrent layer is done
        auto prefetch = [&](const auto &) {
            if (!RNN || nx.mode == 0) return;
            const int64_t nb = e * n + nx.row0;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int ni = (int)nx.row0 + 16 * nt + r;
                    const bool nok = !GEN || ni < n;
                    hN[t][nt] = nx.src ? *reinterpret_cast<const f32x4 *>(nx.src + (nok ? nb + 16 * nt + r : 0) * nx.stride +
                                                                        16 * t + 4 * q)
                                       : f32x4{0.f, 0.f, 0.f, 0.f};
                }
        };
        h2_tail<NT, RNN, !QOUT, W2L, true, GEN>(a, Wl, sw, row0, rows, ok, hB, xB, s_actw, RT * sub, prefetch);
        }
    }
}

// One wave per env, its tiles in turn: the run-time-shape instances, and the SQ64 launches with
// a single agent pass (one launch per step, the Q-output schedule), where there is no hidden
// state to keep between passes and the pair mapping's idle wave during the prologue and the
// transition costs 2.8 % (profiles/ab_pairs_headline.txt).
template <bool RNN, bool W2L, bool GEN, int TAB, bool QOUT, int SQ>
__device__ __forceinline__ void rollout_envs_wave(const RolloutArgs &ra, u32x4v *s_h2, const int (&sw)[4]) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = rs_n<SQ>(ra), m = rs_m<SQ>(ra), mp = rollout_mp(m), np = rollout_np(n);
    char *scr = reinterpret_cast<char *>(s_h2 + ra.scratch_off) + wv * rollout_scratch_bytes(n, m);
    uint64_t *s_scl = reinterpret_cast<uint64_t *>(scr);
    double *s_ret = reinterpret_cast<double *>(scr + 32);
    int *s_cnt = reinterpret_cast<int *>(scr + 40);
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
            const int kk = rr.k0 + it - sf + 1;
            return it < nit && kk < rr.T && (kk < rr.k1 || rr.select_last);
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

// The pair hand-off: every LDS write of the wave has landed (lgkmcnt), then the workgroup's
// barrier.  No fence of workgroup scope: its release would also wait for every outstanding
// global store (vmcnt(0): the tile's row stores; see wave_lds_fence).  Every wave of the
// workgroup executes the same number of these (trip counts from launch-uniform values only).
__device__ __forceinline__ void pair_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// pair scratch (bytes), G = steps per group of deferred transitions: task-scale bits, one u64
// per wave at 8 sub | the env's return f64 at 16 | collision counts [64] int per wave at
// 32 + 256 sub | previous tasks [64] u16 at 544 | from 672 the task history, G + 1 rows of
// 136 bytes: the step's tasks [64] u16, then its reward sum f64 (none in the last row).  Every
// offset is a constant: nothing but the pair's base depends on G.  The launch sizes G to the LDS
// the fc1 slices leave (rollout_defer_steps).
constexpr int kPairHistOff = 672;
constexpr int kPairRow = 68;        // history row stride (u16 units)
constexpr int kMaxDeferSteps = 16;  // with room to spare (Linear agent, L = 1): a T = 20 episode in two groups
__host__ __device__ constexpr int pair_scratch_bytes(int G) {
    return (kPairHistOff + 2 * kPairRow * G + 128 + 15) / 16 * 16;
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
    uint64_t *s_scl = reinterpret_cast<uint64_t *>(scr + 8 * sub);
    double *s_ret = reinterpret_cast<double *>(scr + 16);
    int *s_cnt = reinterpret_cast<int *>(scr + 32 + 256 * sub);
    uint16_t *s_prev = reinterpret_cast<uint16_t *>(scr + 544);
    uint16_t *s_hist = reinterpret_cast<uint16_t *>(scr + kPairHistOff);
    auto s_sum = [&](int j) { return reinterpret_cast<double *>(s_hist + kPairRow * j + 64); };
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
            if (trw) {
                if (!TAB && ra.reset) {
                    // asg_reset: see rollout_envs_wave
                    uint16_t *s_perm = reinterpret_cast<uint16_t *>(s_cnt), *s_jj = s_perm + m;
                    s_perm[lane] = (uint16_t)lane;
                    const u32x4 rr = philox4x32_10(u32x4{(uint32_t)lane, 0u, kCtrPerm, ra.episode}, key.k0, key.k1);
                    s_jj[lane] = (uint16_t)(((uint64_t)rr.x * (uint64_t)(lane + 1)) >> 32);
                    wave_lds_fence();
                    if (lane == 0)
                        for (int i = m - 1; i >= 1; --i) {
                            const int jj = s_jj[i];
                            const uint16_t t = s_perm[i];
                            s_perm[i] = s_perm[jj];
                            s_perm[jj] = t;
                        }
                    wave_lds_fence();
                    const int p = (int)s_perm[lane];
                    s_prev[lane] = (uint16_t)p;
                    if (ra.prevb)
                        ra.prevb[((int64_t)ra.ts0 * ra.E + e) * n + lane] = (ra.quirks & ASG_QUIRK_PREV_ASSIGNS_ZERO) ? 0 : p;
                    if (lane == 0 && ra.filled) ra.filled[(int64_t)ra.ts0 * ra.E + e] = 1;
                } else {
                    const int p = ra.prev[e * n + lane];
                    s_prev[lane] = (uint16_t)p;
                    if (TAB && ra.reset && ra.prevb)
                        ra.prevb[((int64_t)ra.ts0 * ra.E + e) * n + lane] = (ra.quirks & ASG_QUIRK_PREV_ASSIGNS_ZERO) ? 0 : p;
                    if (TAB && ra.reset && lane == 0 && ra.filled) ra.filled[(int64_t)ra.ts0 * ra.E + e] = 1;
                }
                s_hist[lane] = 0;
                if (lane == 0) *s_ret = ra.reset ? 0.0 : ra.returns[e];
                if (!ra.select_first) rollout_actions_from_batch(ra, e, ra.ts0, s_hist);
            }
        }
        wave_lds_fence();
        pair_barrier();  // the batch's tasks (row 0) and the previous tasks reach the other wave
        KRolloutArgs *const kra = (KRolloutArgs *)__builtin_amdgcn_kernarg_segment_ptr();
        const int sf = ra.select_first ? 1 : 0;
        const int nit = ra.k1 - ra.k0 + sf;
        f32x4 hN[4][kH2NT];  // the wave's h_t rows: loaded by pass 0, h' of the pass before after it
        auto has_agent = [&](auto &rr, int it) {
            const int kk = rr.k0 + it - sf + 1;
            return it < nit && kk < rr.T && (kk < rr.k1 || rr.select_last);
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

// The rollout kernel's instances, one launcher per translation unit (the instances dominate
// the build: asg_h2.hip holds the Philox epsilon-greedy ones, asg_rollout_tab.hip the table
// modes', asg_rollout_q.hip the Q-output ones of both benefit sources).
struct RolloutLaunch {
    unsigned grid;
    size_t lds;
    bool rnn, w2l, gen;
    bool sq64;  // n = m = 64 (W2 in LDS, no ragged tiles): the compile-time-shape instances
    bool pair;  // sq64 launches with two or more agent passes: a wave pair per env (rollout_envs_pair)
};
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
