// rollout_args.h -- what the fused rollout kernel's stages share: the launch arguments and how
// the device code reads them, the env shape, the two LDS scratch layouts, the LDS fences and
// the launch description.  The stages: rollout_env.h (prologue, transition), rollout_rows.h (row
// stores, compact table), rollout_tile.h (a 32-agent tile), rollout_kernel.h (env loops, kernel).
//
// Reference: envs/mock_constellation_env.py:94-175 (reset, step, pre-transition data),
// runners/episode_runner.py:60-127 (the loop the kernel fuses: select(0); for t: step(t),
// select(t + 1)); the agent and the selection as in h2_tile.h.
#pragma once
#include "h2_tile.h"

#pragma clang fp contract(fast)

namespace asg {

// Fused rollout (mock env, Philox bumps): for every env, transitions k0 .. k1 - 1 and the
// agent forward + epsilon-greedy selection of the rows in between, in one launch.  One wave
// per env (persistent over envs): the transition runs with lane = agent (collision counts,
// float64 rewards summed in agent order, the env's previous / selected tasks and task scales
// in the wave's LDS scratch -- never re-read from HBM); the env's 32-agent tiles then
// generate the next observation row in the split-f16 MFMA operand layout (lane (r, q)
// evaluates the Philox bumps of tasks 32 u + 16 c + 4 q + v), write it to the batch and feed
// fc1 from registers: the agent never reads an observation back.  Selected tasks go to the
// batch's actions row and to the LDS, where the next transition reads them.  The hidden
// state lives in Hout between passes (Hin for the first), or in the registers of a wave pair
// (rollout_envs_pair).  Results are those of the separate launches: asg_reset / asg_step rows,
// and the agent kernel's actions and hidden state (per-row scales make a row's result
// independent of its tile's other rows).
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
// The wave slot (one wave per env), byte offsets: task-scale bits [4] u64 (a bit per task,
// m <= 256) | the env's return f64 | collision counts [mp] int, behind them the selected and
// the previous tasks, [np] u16 each
constexpr int kWaveSclOff = 0;
constexpr int kWaveRetOff = 32;
constexpr int kWaveCntOff = 40;
__host__ __device__ constexpr int rollout_scratch_bytes(int n, int m) {
    return (kWaveCntOff + 4 * rollout_mp(m) + 2 * 2 * rollout_np(n) + 15) / 16 * 16;
}
static_assert(kWaveSclOff + 8 * (256 / 64) <= kWaveRetOff && kWaveRetOff % 8 == 0 && kWaveRetOff + 8 <= kWaveCntOff &&
                  kWaveCntOff % 4 == 0 && rollout_scratch_bytes(256, 256) >= kWaveCntOff + 4 * 256 + 2 * 2 * 256 &&
                  rollout_scratch_bytes(1, 16) >= kWaveCntOff + 4 * 32 + 2 * 2 * 32,
              "wave slot: regions overlap, a float64 is misaligned, or the size does not cover them");

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

// The pair slot (a wave pair per env, n = m = 64), byte offsets, G = steps per group of deferred
// transitions: task-scale bits, one u64 per wave | the env's return f64 | collision counts [64]
// int per wave | previous tasks [64] u16 | the task history, G + 1 rows of kPairRow u16: the
// step's tasks [64] u16, then its reward sum f64 (none in the last row).  Every offset is a
// constant: nothing but the pair's base depends on G.  The launch sizes G to the LDS the fc1
// slices leave (rollout_defer_steps).
constexpr int kPairSclOff = 0, kPairSclStride = 8;     // + kPairSclStride * sub
constexpr int kPairRetOff = 16;
constexpr int kPairCntOff = 32, kPairCntStride = 256;  // + kPairCntStride * sub
constexpr int kPairPrevOff = 544;
constexpr int kPairHistOff = 672;
constexpr int kPairRow = 68;        // history row stride (u16 units)
constexpr int kPairSumOff = 64;     // the reward sum within a row (u16 units)
constexpr int kMaxDeferSteps = 16;  // with room to spare (Linear agent, L = 1): a T = 20 episode in two groups
__host__ __device__ constexpr int pair_scratch_bytes(int G) {
    return (kPairHistOff + 2 * kPairRow * G + 2 * 64 + 15) / 16 * 16;
}
static_assert(kPairSclOff + 2 * kPairSclStride <= kPairRetOff && kPairRetOff + 8 <= kPairCntOff &&
                  kPairCntStride >= 4 * 64 && kPairCntOff + 2 * kPairCntStride <= kPairPrevOff &&
                  kPairPrevOff + 2 * 64 <= kPairHistOff && kPairSumOff >= 64 && 2 * kPairSumOff + 8 <= 2 * kPairRow,
              "pair slot: regions overlap");
static_assert(kPairRetOff % 8 == 0 && kPairHistOff % 8 == 0 && (2 * kPairRow) % 8 == 0 && (2 * kPairSumOff) % 8 == 0 &&
                  pair_scratch_bytes(1) >= kPairHistOff + 2 * kPairRow + 2 * 64 &&
                  pair_scratch_bytes(kMaxDeferSteps) >= kPairHistOff + 2 * kPairRow * kMaxDeferSteps + 2 * 64,
              "pair slot: a float64 is misaligned, or the size does not cover the history's G + 1 rows");

// Whether iteration `it` of a launch's nit = k1 - k0 + sf iterations (sf: a selection on the
// first row comes first) has an agent pass: its row kk lies within the episode and is either
// followed by a transition of this launch or selected on at its end.  The env loops and the
// launch's choice of the pair mapping (launch_rollout's pass count) both ask this function.
__host__ __device__ constexpr bool rollout_has_agent(int it, int nit, int sf, int k0, int k1, int T, int select_last) {
    const int kk = k0 + it - sf + 1;
    return it < nit && kk < T && (kk < k1 || select_last);
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

}  // namespace asg
