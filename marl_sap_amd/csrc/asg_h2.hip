// asg_h2.hip -- the RNNAgent forward on two-way-split f16 MFMAs (gfx950), and the fused
// rollout kernel that runs the mock env's transitions, the agent and the epsilon-greedy
// selection for a range of steps of every env -- a whole episode in one launch.
//
// This file holds the host side of both (input geometry, weight packing, LDS plan, launch)
// and the kernels instantiated here: the agent kernel, the pack kernels and the rollout
// kernel's Philox epsilon-greedy instances.  The device code lives in headers: h2_tile.h (the
// split-f16 arithmetic and one wave tile of the agent) and, for the rollout kernel, one per
// stage: rollout_args.h (arguments, LDS scratch layouts), rollout_env.h (env prologue,
// transition), rollout_rows.h (whole-line row stores, compact table), rollout_tile.h (the
// 32-agent tile) and rollout_kernel.h (env loops, kernel, instance launcher; shared with
// asg_rollout_tab.hip and asg_rollout_q.hip, which hold the other instances).
#include "rollout_kernel.h"

#pragma clang fp contract(fast)

namespace asg {

// ---- geometry and packed layout -----------------------------------------------------------
H2Geom h2_geom(int K, int nout) {
    H2Geom g;
    g.K = K;
    g.nout = nout;
    g.nct = (nout + 15) / 16;
    const bool blocked = nout >= 16 && K % nout == 0 && K / nout >= 2;
    g.P = blocked ? nout : K;
    g.NB = blocked ? K / nout : 1;
    g.prefix = blocked ? 1 : 0;
    g.Pp = (g.P + 31) / 32 * 32;
    g.Kp = g.Pp * g.NB;
    return g;
}
bool h2_ok(int K, int nout) { return K >= 1 && nout >= 1 && nout <= 256; }
int64_t h2_packed_f4(int K, int nout, int use_rnn) {
    const H2Geom g = h2_geom(K, nout);
    return w1t_f4(g) + 1 + w1s_f4(g.Kp) + rec_f4(use_rnn != 0) + w2s_f4(g.nct);
}

typedef __attribute__((address_space(4))) const H2Args KH2Args;
// Persistent: one 512-thread workgroup per CU stages the LDS image, then its 8 waves walk
// 256-row tiles.
template <bool RNN, bool SEL, bool W2L, bool GEN>
__global__ void __launch_bounds__(64 * kH2Waves) __attribute__((amdgpu_waves_per_eu(kH2WavesPerSimd)))
rnn_agent_h2_kernel(H2Args a) {
    extern __shared__ u32x4v s_h2[];
    int sw[4];
    h2_stage<RNN, W2L>(a, s_h2, sw);
    __syncthreads();
    constexpr int NT = kH2NT;
    const int64_t ntiles = (a.R + kH2Waves * (16 * NT) - 1) / (kH2Waves * (16 * NT));
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = (tile * kH2Waves + (threadIdx.x >> 6)) * (16 * NT);
        // each tile re-reads the launch arguments (scalar loads): kept live from the kernel
        // entry they overflow the SGPR file (see rollout_args)
        KH2Args *p = (KH2Args *)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(p));
        agent_rows_h2<NT, RNN, SEL, W2L, GEN>(row0, *p, s_h2, sw);
    }
}

// ---- packing: max|W| -> scale exponent, then the scaled f16 planes ------------------------
__global__ void h2_exp_kernel(const float *W, int64_t n, int *out) {
    __shared__ float s_m[16];
    float m = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) m = fmaxf(m, __builtin_fabsf(W[i]));
    m = wave_allreduce(m, [](float a, float b) { return fmaxf(a, b); });
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = fmaxf(m, s_m[w]);
        *out = h2_scale(m, -60, 60);
    }
}
// W [C][Kin] row-major -> planes of tiles (ct, sl): lane l = (r, q) holds the 8 values of
// padded inputs 32 sl + slice_k(q, j) of row 16 ct + r, scaled by 2^s and split into (h, l).
// Padded input kp is block kp / Pp, element kp % Pp of it (zero past P); order slice-major
// (W1: [sl][ct]) or unit-major (recurrent [ct = 4 g + hb][sl], W2 [c][sl]).
__global__ void h2_pack_kernel(const float *W, int C, int Kin, int P, int Pp, int nct, int nsl, int slice_major,
                               const int *sexp, u32x4v *out) {
    const int64_t total = (int64_t)nct * nsl * 64;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int lane = (int)(i & 63);
    const int64_t tix = i >> 6;
    const int ct = slice_major ? (int)(tix % nct) : (int)(tix / nsl);
    const int sl = slice_major ? (int)(tix / nct) : (int)(tix % nsl);
    const int row = 16 * ct + (lane & 15), q = lane >> 4;
    const float sc = pow2f(*sexp);
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int kp = 32 * sl + slice_k(q, j);
        const int blk = kp / Pp, jj = kp - blk * Pp;
        const int k = blk * P + jj;
        x[j] = (row < C && jj < P && k < Kin) ? W[(int64_t)row * Kin + k] * sc : 0.f;
    }
    u32x4v h, l;
    split2(x, h, l);
    const int64_t o = (slice_major ? ((int64_t)sl * nct + ct) : ((int64_t)ct * nsl + sl)) * 2 * 64 + lane;
    out[o] = h;
    out[o + 64] = l;
}

hipError_t launch_h2_pack(const float *W1, const float *Wih, const float *Whh, const float *W2, int K, int nout,
                          int use_rnn, float4 *packed, hipStream_t s) {
    const H2Geom g = h2_geom(K, nout);
    const bool rnn = use_rnn != 0;
    if (g.prefix) (void)launch_w1t_pack(W1, K, g.P, reinterpret_cast<float *>(packed), s);
    u32x4v *sec = reinterpret_cast<u32x4v *>(packed + w1t_f4(g));
    int *hdr = reinterpret_cast<int *>(sec);
    const float *mats[4] = {W1, Wih, rnn ? Whh : Wih, W2};
    const int64_t sizes[4] = {(int64_t)kHid * K, (rnn ? 3 : 1) * kHid * kHid, (rnn ? 3 : 1) * kHid * kHid,
                              (int64_t)nout * kHid};
    for (int i = 0; i < 4; ++i)
        hipLaunchKernelGGL(h2_exp_kernel, dim3(1), dim3(1024), 0, s, mats[i], sizes[i], hdr + i);
    auto pack = [&](const float *W, int C, int Kin, int P, int Pp, int nct, int nsl, int smaj, int e, u32x4v *out) {
        const int64_t n = (int64_t)nct * nsl * 64;
        hipLaunchKernelGGL(h2_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, W, C, Kin, P, Pp, nct,
                           nsl, smaj, hdr + e, out);
    };
    u32x4v *o = sec + 1;
    pack(W1, kHid, K, g.P, g.Pp, 4, g.Kp / 32, 1, 0, o);
    o += w1s_f4(g.Kp);
    if (rnn) {
        pack(Wih, 3 * kHid, kHid, kHid, kHid, 12, 2, 0, 1, o);
        o += 3 * kGateF4;
        pack(Whh, 3 * kHid, kHid, kHid, kHid, 12, 2, 0, 2, o);
        o += 3 * kGateF4;
    } else {
        pack(Wih, kHid, kHid, kHid, kHid, 4, 2, 0, 1, o);
        o += kGateF4;
    }
    pack(W2, nout, kHid, kHid, kHid, g.nct, 2, 0, 3, o);
    return hipGetLastError();
}

hipError_t launch_h2_agent(const float *X, int64_t xs, int64_t R, int K, const float *Hin, int64_t hs,
                           const float4 *packed, const float *b1, const float *bih, const float *bhh, const float *b2,
                           int nout, int use_rnn, float *Hout, float *Q, const SelectArgs *sel, hipStream_t s) {
    const H2Geom g = h2_geom(K, nout);
    const bool rnn = use_rnn != 0;
    H2Args ha{};
    ha.X = X;
    ha.xs = xs;
    ha.R = R;
    ha.g = g;
    ha.pre = g.prefix && onehot_prefix_enabled();
    ha.Hin = Hin;
    ha.hs = hs;
    ha.W1T = reinterpret_cast<const float *>(packed);
    ha.pk = reinterpret_cast<const u32x4v *>(packed + w1t_f4(g));
    ha.b1 = b1;
    ha.bi = bih;
    ha.bh = bhh;
    ha.b2 = b2;
    ha.Hout = Hout;
    ha.Q = Q;
    ha.sel = sel ? *sel : SelectArgs{};
    const H2Lds plan = h2_lds_plan(g, rnn, ha.pre ? g.Pp / 32 : 0, 0);
    ha.w1_lds = plan.w1_lds;
    const bool gen = g.P % 32 != 0 || (xs & 3) != 0 || (reinterpret_cast<uintptr_t>(X) & 15) != 0 || nout % 16 != 0;
    const int ncu = stream_cus(s);
    const int64_t ntiles = (R + kH2Waves * 16 * kH2NT - 1) / (kH2Waves * 16 * kH2NT);
    const unsigned grid = (unsigned)(ntiles < ncu ? ntiles : ncu);
    if (grid == 0) return hipSuccess;
#define LH_(RNN, SEL, W2L, GEN) \
    hipLaunchKernelGGL((rnn_agent_h2_kernel<RNN, SEL, W2L, GEN>), dim3(grid), dim3(64 * kH2Waves), plan.bytes, s, ha)
#define LH2_(RNN, SEL)                                                      \
    do {                                                                    \
        if (plan.w2l) {                                                     \
            if (gen) LH_(RNN, SEL, true, true); else LH_(RNN, SEL, true, false);   \
        } else {                                                            \
            if (gen) LH_(RNN, SEL, false, true); else LH_(RNN, SEL, false, false); \
        }                                                                   \
    } while (0)
    if (rnn) {
        if (sel) LH2_(true, true); else LH2_(true, false);
    } else {
        if (sel) LH2_(false, true); else LH2_(false, false);
    }
#undef LH2_
#undef LH_
    return hipGetLastError();
}

// shapes the rollout kernel takes: the split-f16 agent with the mock env's obs layout
// (K = m (L + 1), one-hot prefix geometry), n, m <= 256
bool rollout_shape_ok(int n, int m, int L, int K) {
    if (n < 1 || m < 16 || m > 256 || n > 256 || L < 1 || K != m * (L + 1) || !h2_ok(K, m)) return false;
    return onehot_prefix_enabled() && h2_geom(K, m).prefix;
}

// the rollout kernel's LDS plan: the agent's image, then a scratch slot per wave (u32x4v units)
static int64_t rollout_scratch_f4(int n, int m) {
    return ((int64_t)rollout_scratch_bytes(n, m) * kH2Waves + 15) / 16;
}
static H2Lds rollout_lds_plan(const H2Geom &g, int n, int m, bool rnn) {
    return h2_lds_plan(g, rnn, g.Pp / 32, rollout_scratch_f4(n, m));
}

int rollout_l2_slices(int n, int m, int L, int use_rnn) {
    if (!rollout_shape_ok(n, m, L, m * (L + 1))) return -1;
    return rollout_lds_plan(h2_geom(m * (L + 1), m), n, m, use_rnn != 0).l2_slices;
}

// The pair mapping's group size G (steps whose transitions are deferred together): what the
// LDS behind the plan's fc1 slices holds per wave pair (pair_scratch_bytes), the plan itself
// left as it is -- a resident fc1 slice is worth more than a longer group.  0: not a shape of
// the pair mapping.
int rollout_defer_steps(int n, int m, int L, int use_rnn) {
    if (n != 64 || m != 64 || !rollout_shape_ok(n, m, L, m * (L + 1))) return 0;
    const H2Lds plan = rollout_lds_plan(h2_geom(m * (L + 1), m), n, m, use_rnn != 0);
    if (!plan.w2l) return 0;
    const int64_t room = (kH2LdsBytes - plan.scratch_off * 16) / (kH2Waves / 2);  // bytes per pair
    int G = kMaxDeferSteps;
    while (G > 0 && pair_scratch_bytes(G) > room) --G;
    return G;
}

hipError_t launch_rollout(const RolloutSlabs &sl, const EnvState &st, int ts, int k0, int steps, int select_first,
                          int select_last, int reset, const float4 *packed, const float *b1, const float *bi, const float *bh,
                          const float *b2, int use_rnn, const float *Hin, int64_t hs, float *Hout, float *Q, float epsilon,
                          uint64_t seed, uint32_t counter, int64_t row_base, int *err, hipStream_t s) {
    const int K = st.m * (st.L + 1), nout = st.m;
    const H2Geom g = h2_geom(K, nout);
    const bool rnn = use_rnn != 0;
    RolloutArgs ra{};
    ra.obs = sl.obs;
    ra.beta = sl.beta;
    ra.avail = sl.avail;
    ra.onehot = sl.onehot;
    ra.act = sl.act;
    ra.rew = sl.rew;
    ra.prevb = sl.prevb;
    ra.term = sl.term;
    ra.filled = sl.filled;
    ra.ts0 = ts;
    ra.prev = st.prev;
    ra.returns = st.returns;
    ra.T_trans = st.T_trans;
    ra.env_err = st.err;
    ra.lambda_ = st.lambda_;
    ra.seed = st.seed;
    ra.env_base = st.env_base;
    ra.E = st.E;
    ra.episode = st.episode;
    ra.quirks = st.quirks;
    ra.n = st.n;
    ra.m = st.m;
    ra.T = st.T;
    ra.L = st.L;
    ra.dense = st.benefit_mode == ASG_BENEFIT_DENSE;
    ra.wmin = (float)st.wmin;
    ra.wmax = (float)st.wmax;
    ra.k0 = k0;
    ra.k1 = k0 + steps;
    ra.select_first = select_first;
    ra.select_last = select_last;
    ra.reset = reset;
    const bool tab = st.rng_mode == ASG_RNG_MT19937 || st.benefit_mode == ASG_BENEFIT_INJECTED;
    ra.table = tab ? st.table : nullptr;
    ra.par = tab ? st.mtpar : nullptr;
    ra.table32 = tab ? st.table32 : nullptr;
    ra.tmask = tab ? st.tmask : nullptr;  // set only in the MT19937 draws mode (compact table)
    ra.toff = tab ? st.toff : nullptr;
    // the table modes' reset in this launch: the MT19937 draws ran before it (asg_reset_rollout)
    // Q output: one transition and the forward of the row after it (asg_step_forward)
    // or (asg_reset_forward) the envs' reset and the forward on the reset row, no transition
    const bool q_step = steps == 1 && !select_first && select_last && !reset;
    const bool q_reset = steps == 0 && select_first && select_last && reset;
    if (Q && !q_step && !q_reset) return hipErrorInvalidValue;
    if (!Q && steps < 1) return hipErrorInvalidValue;
    ra.Q = Q;
    ra.assign = st.bids ? st.assign : nullptr;
    if (st.bids && !Q) return hipErrorInvalidValue;  // bids: asg_step_forward only
    ra.W1T = reinterpret_cast<const float *>(packed);
    ra.pk = reinterpret_cast<const u32x4v *>(packed + w1t_f4(g));
    ra.Hin = Hin;
    ra.hs = hs;
    ra.Hout = Hout;
    ra.b1 = b1;
    ra.bi = bi;
    ra.bh = bh;
    ra.b2 = b2;
    ra.epsilon = epsilon;
    ra.sk0 = (uint32_t)seed;
    ra.sk1 = (uint32_t)(seed >> 32) ^ 0x5bd1e995u;
    ra.counter = counter;
    (void)row_base;  // = env_base * n (the selection keys by global row)
    ra.sel_err = err;
    const H2Lds plan = rollout_lds_plan(g, st.n, st.m, rnn);
    ra.w1_lds = plan.w1_lds;
    ra.w1_off = 0;  // 1 with the SQ64 instances (below)
    ra.scratch_off = plan.scratch_off;
    const int ncu = stream_cus(s);
    RolloutLaunch lc;
    lc.lds = plan.bytes;
    lc.rnn = rnn;
    lc.w2l = plan.w2l;
    lc.gen = st.m % 32 != 0 || st.n % 32 != 0;
    lc.sq64 = st.n == 64 && st.m == 64 && plan.w2l;
    // agent passes of the launch, as the kernel counts them: with two or more, the SQ64 selecting
    // instances keep the hidden state in registers between them (rollout_envs_pair); a single
    // pass has nothing to keep and runs one wave per env
    int passes = 0;
    const int sf = select_first ? 1 : 0, nit = steps + sf;
    for (int it = 0; it < nit; ++it) passes += rollout_has_agent(it, nit, sf, ra.k0, ra.k1, ra.T, ra.select_last);
    lc.pair = lc.sq64 && !Q && passes >= 2;
    if (lc.pair) {
        // the pairs' scratch takes the wave slots' place, and the room behind them for the task history
        ra.defer = rollout_defer_steps(st.n, st.m, st.L, use_rnn);
        if (ra.defer < 1) return hipErrorInvalidValue;
        const int64_t pair_f4 = (int64_t)pair_scratch_bytes(ra.defer) * (kH2Waves / 2) / 16;
        if (pair_f4 > rollout_scratch_f4(st.n, st.m)) lc.lds = (size_t)(plan.scratch_off + pair_f4) * 16;
    }
    // envs in flight per workgroup: one per wave, or one per wave pair, whose scratch is the
    // pair's two wave slots of the plan above
    const int per_wg = lc.pair ? kH2Waves / 2 : kH2Waves;
    const int64_t wgs = (st.E + per_wg - 1) / per_wg;
    lc.grid = (unsigned)(wgs < ncu ? wgs : ncu);
    // the L2 fc1 slice read first, before the tile's stores (rollout_tile's w1_off)
    if (lc.sq64 && plan.l2_slices >= 1) ra.w1_off = 1;
    if (Q) return launch_rollout_q(ra, lc, s);
    if (tab) return launch_rollout_tab(ra, lc, s);
    return launch_rollout_inst<0, false>(ra, lc, s);
}

}  // namespace asg
