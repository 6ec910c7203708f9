// h2_tile.h -- the RNNAgent forward on two-way-split f16 MFMAs (gfx950), device side: the
// split primitives, the packed weight layout and LDS image, and one 32-row wave tile of the
// agent (agent_rows_h2; its recurrent layer + fc2 + selection, h2_tail, is shared with the
// rollout tile of rollout_tile.h).  The kernels that run it are in asg_h2.hip; the rollout
// kernel around its tile is in rollout_kernel.h (with rollout_args.h, rollout_env.h and
// rollout_rows.h).
//
// Reference: modules/agents/rnn_agent.py:23-31 (fc1 -> ReLU -> GRUCell | Linear + ReLU ->
// fc2), controllers/basic_controller.py:19-48 (select_actions), action_selectors/
// classic_selectors.py:28-54 (epsilon-greedy).
//
// Split-f16 products.  Every f32 operand x (pre-scaled by a power of two so |x| < 2^15) is
// split x ~ h + l with h = RNE_f16(x), l = RNE_f16(x - h) (x - h is exact in f32):
// |x - h - l| <= 2^-22 |x|, and a product is summed as wh.xh + wh.xl + wl.xh on
// v_mfma_f32_16x16x32_f16 (the dropped wl.xl is below 2^-22 relative): 3 MFMAs per 32-deep
// slice, products exact in the f32 accumulator, summation in f32 -- fp32-level accuracy
// (tests/test_gpu_agent.py measures it against float64).
//
// Transposed layers: out^T = W . act^T.  The MFMA A operand is a packed weight fragment (1 KiB
// per wave, contiguous), the B operand an activation fragment; with the 16x16 layouts the
// accumulator of output tile mt IS the B operand of the next layer's k-chunk, so fc1 ->
// recurrent layer -> fc2 hand activations over in registers.  One wave owns 32 agent rows
// (two 16-row tiles nt); lane (r, q) = (l & 15, l >> 4) holds rows r and 16 + r.
//
// Scales are per ROW (each lane's accumulator column is one row): weights by 2^sw per
// matrix (pack time), a row's activations by 2^s from the row's own max |x| (a reduction
// over its 4 lanes).  So every row's result is a function of that row's inputs alone -- the
// same whichever rows share its wave tile (envs of 20 agents in 32-row tiles, sharded runs,
// the fused rollout's one-env tiles vs the agent kernel's flat tiles: bit-identical).  fc1's
// input scale is chosen before the values are seen (2^11: |x| < 16 needs no retry) and a
// tile re-runs fc1 when some row would exceed 2^15 (that row at its own smaller scale).
//
// Geometry.  The input row is NB blocks of P values; each block is zero-padded to
// Pp = roundup(P, 32) so a 32-deep slice never straddles two blocks.  For the mock env's
// obs ([onehot(previous task) | B(k) .. B(k + L - 1)], P = m, NB = L + 1) block 0 is the
// one-hot prefix: a tile whose block 0 is verified one-hot (or zero) adds W1[:, a] (one
// gathered column per row) instead of running those slices' MFMAs.  Any other input is one
// block (P = K).
#pragma once
#include <type_traits>

#include "asg_agent_common.h"

// The library builds with -ffp-contract=off (the env's float64 arithmetic); the agent's f32
// math may fuse.  A file-scope pragma: it holds for the rest of the including translation
// unit, which restates it after its includes.
#pragma clang fp contract(fast)

namespace asg {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2v __attribute__((ext_vector_type(2)));
typedef long long i64x2v __attribute__((ext_vector_type(2)));
typedef const u32x4v __attribute__((address_space(3))) * lds_u4p;
typedef const f32x4 __attribute__((address_space(3))) * lds_f4v;

__device__ __forceinline__ f32x4 mfma_h(const u32x4v &a, const u32x4v &b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0,
                                                  0);
}
// (wh, wl) . (xh, xl) = wh.xh + wh.xl + wl.xh; the correction terms first
__device__ __forceinline__ f32x4 mfma_h2(const u32x4v (&w)[2], const u32x4v (&x)[2], f32x4 c) {
    c = mfma_h(w[1], x[0], c);
    c = mfma_h(w[0], x[1], c);
    c = mfma_h(w[0], x[0], c);
    return c;
}
// 8 (scaled) f32 -> f16 planes h, l (element j in half j & 1 of dword j >> 1)
__device__ __forceinline__ void split2(const float (&x)[8], u32x4v &h, u32x4v &l) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const f16x2v hh = {(_Float16)x[2 * p], (_Float16)x[2 * p + 1]};
        const float ra = x[2 * p] - (float)hh[0], rb = x[2 * p + 1] - (float)hh[1];
        const f16x2v ll = {(_Float16)ra, (_Float16)rb};
        h[p] = __builtin_bit_cast(uint32_t, hh);
        l[p] = __builtin_bit_cast(uint32_t, ll);
    }
}
// The split of 8 UNSCALED values at scale sc (a power of two): h = RNE_f16(x * sc) and the
// residual fma(x, sc, -h) (exact in f32) rounded once to f16 by v_fma_mix{lo,hi}_f16.
__device__ __forceinline__ void split2s(const float (&x)[8], float sc, u32x4v &h, u32x4v &l) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const f16x2v hh = {(_Float16)(x[2 * p] * sc), (_Float16)(x[2 * p + 1] * sc)};
        const uint32_t hv = __builtin_bit_cast(uint32_t, hh);
        uint32_t lv = 0;
        asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "+v"(lv) : "v"(x[2 * p]), "v"(sc), "v"(hv));
        asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
            : "+v"(lv)
            : "v"(x[2 * p + 1]), "v"(sc), "v"(hv));
        h[p] = hv;
        l[p] = lv;
    }
}
// max(m, |a|, |b|) in one v_max3_f32
__device__ __forceinline__ float max3_abs(float m, float a, float b) {
    float r;
    asm("v_max3_f32 %0, %1, |%2|, |%3|" : "=v"(r) : "v"(m), "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float absmax4(float m, const float4 &v) { return max3_abs(max3_abs(m, v.x, v.y), v.z, v.w); }
__device__ __forceinline__ float absmax4(float m, const f32x4 &v) {
    return max3_abs(max3_abs(m, v[0], v[1]), v[2], v[3]);
}
// 2^s as a float (s clamped to the normal range [-126, 127])
__device__ __forceinline__ float pow2f(int s) {
    s = s < -126 ? -126 : (s > 127 ? 127 : s);
    return __builtin_bit_cast(float, (uint32_t)(s + 127) << 23);
}
// the scale exponent s with m * 2^s < 2^15 (m = max |x| >= 0), clamped to [lo, hi]
__device__ __forceinline__ int h2_scale(float m, int lo, int hi) {
    const int e = m > 0.f ? (int)((__builtin_bit_cast(uint32_t, m) >> 23) & 0xff) - 126 : -200;  // m < 2^e
    const int s = 15 - e;
    return s < lo ? lo : (s > hi ? hi : s);
}
// maximum over the 4 lanes of a row (q = 0..3: lanes l, l ^ 16, l ^ 32, l ^ 48); v >= 0
__device__ __forceinline__ float row_max4(float v) {
    const SwapPair a = swap16(__builtin_bit_cast(uint32_t, v));
    const float x = fmaxf(__builtin_bit_cast(float, a.a), __builtin_bit_cast(float, a.b));
    const SwapPair b = swap32(__builtin_bit_cast(uint32_t, x));
    return fmaxf(__builtin_bit_cast(float, b.a), __builtin_bit_cast(float, b.b));
}
// element j of lane quad q of a 32-deep slice: units 4q + v of its two 16-tiles (the
// accumulator layout of the layer before, so activations feed the MFMA in place)
__host__ __device__ inline int slice_k(int q, int j) { return j < 4 ? 4 * q + j : 16 + 4 * q + j - 4; }

// packed h2 section (u32x4v units): [header: int sw1, sw_r1, sw_r2, sw2]
//   [W1 planes: slice Kp / 32][mt 4][plane 2][lane 64]
//   [recurrent planes: GRU W_ih (gate 3)(hb 4)(slice 2)(plane 2)(lane 64), then W_hh; or the
//    Linear W_rnn as one gate]
//   [W2 planes: tile nct][slice 2][plane 2][lane 64]
// preceded (one-hot prefix geometry) by W1^T of block 0: [P][64] f32
constexpr int kGateF4 = 4 * 2 * 2 * 64;
__host__ __device__ inline int64_t rec_f4(bool rnn) { return rnn ? 6 * kGateF4 : kGateF4; }
__host__ __device__ inline int64_t w1s_f4(int Kp) { return (int64_t)(Kp / 32) * 4 * 2 * 64; }
__host__ __device__ inline int64_t w2s_f4(int nct) { return (int64_t)nct * 2 * 2 * 64; }
__device__ __forceinline__ int gate_idx(int g, int hb, int sl, int pl, int lane) {
    return (((g * 4 + hb) * 2 + sl) * 2 + pl) * 64 + lane;
}
__device__ __forceinline__ int64_t w1_idx(int sl, int mt, int pl, int lane) {
    return (((int64_t)sl * 4 + mt) * 2 + pl) * 64 + lane;
}
__device__ __forceinline__ int w2_idx(int c, int sl, int pl, int lane) { return ((c * 2 + sl) * 2 + pl) * 64 + lane; }
static inline int64_t w1t_f4(const H2Geom &g) { return g.prefix ? (int64_t)g.P * 16 : 0; }

// LDS image (u32x4v units): [recurrent planes][biases][W2 planes (W2L)][W1 slices][scratch]
// biases (floats): b1 [64] | GRU: b_ir + b_hr, b_iz + b_hz, b_in, b_hn [4 x 64]; Linear: b_rnn,
// 0, 0, 0 | b2 [16 nct] (zero past n_out)
__host__ __device__ inline int64_t bias_f4(int nct) { return 80 + 4 * (int64_t)nct; }
__host__ __device__ inline int64_t lds_w2_off(bool rnn, int nct) { return rec_f4(rnn) + bias_f4(nct); }
__host__ __device__ inline int64_t lds_w1_off(bool rnn, int nct, bool w2l) {
    return lds_w2_off(rnn, nct) + (w2l ? w2s_f4(nct) : 0);
}

struct H2Args {
    const float *X;
    int64_t xs, R;
    H2Geom g;
    int pre;           // one-hot gather shortcut on block 0 (prefix geometry, ASG_AGENT_ONEHOT)
    const float *Hin;
    int64_t hs;
    const u32x4v *pk;  // h2 section
    const float *W1T;  // [P][64] f32: W1 columns of block 0
    const float *b1, *bi, *bh, *b2;  // GRU: b_ih, b_hh; Linear: b_rnn, unused
    float *Hout, *Q;
    SelectArgs sel;
    int w1_lds;        // W1 slices [s0 + w1_off, s0 + w1_off + w1_lds) staged in LDS (s0 = pre ? Pp / 32 : 0)
    int w1_off;        // 1: the first main slice (s0) stays in L2 (the rollout reads it before its stores)
};

constexpr int kH2NT = 2;                        // 16-row tiles per wave: 32 rows
constexpr int kH2WavesPerSimd = 2;              // register budget 256 VGPRs
constexpr int kH2Waves = 4 * kH2WavesPerSimd;   // waves per workgroup (one workgroup per CU)
constexpr int kH2XBuf = 2;                      // observation slices in flight per wave in fc1
constexpr int kH2SxInit = 11;                   // fc1 input scale of the first attempt
// Timing-only switches (WRONG results; refused without -DASG_TIMING_EXPERIMENTS):
// ASG_ROLLOUT_XSKIP bit 1: no batch row stores in the rollout tiles; bit 2: no one-hot W1
// column gather (zeros); bit 4: fc1 slices that live in L2 read LDS slot 0 instead; bit 8:
// h_t not loaded (constants); bit 16: h' not stored (the SQ64 wave-pair rollout instances keep h
// in registers between a launch's passes: there bit 8 still replaces h_t by the constants in
// every pass -- the carried h' is ignored -- but the load it no longer waits for happens once
// per launch, and bit 16 drops the launch's one h' store); bit 32: the tile's row stores go to a
// small region that stays in L2 (env e & 7, batch row 1): same instructions, no HBM writes;
// bit 64: the tiles' bump parameters from a cheap hash instead of Philox (VALU); bit 256: no env
// transition between the steps (rewards, returns, the transition's rows); bit 512: the return
// not summed in agent order (one readlane); bit 1024: the transition's rewards without the bump
// (Philox + float64 exp: beta = 0); bit 2048: the compact table's quads not loaded (a constant,
// the mask / expansion kept); bit 4096: the compact quads loaded but not expanded
#if defined(ASG_ROLLOUT_XSKIP) && !defined(ASG_TIMING_EXPERIMENTS)
#error "ASG_ROLLOUT_XSKIP gives wrong results: timing experiments only (-DASG_TIMING_EXPERIMENTS)"
#endif
#ifndef ASG_ROLLOUT_XSKIP
#define ASG_ROLLOUT_XSKIP 0
#endif

template <class A>
__device__ __forceinline__ int h2_s0(A &a) { return a.pre ? (a.g.Pp >> 5) : 0; }

template <bool RNN, bool W2L>
__device__ __forceinline__ void h2_stage(const H2Args &a, u32x4v *s, int (&sw)[4]) {
    const H2Geom &g = a.g;
    const u32x4v *rec = a.pk + 1 + w1s_f4(g.Kp);  // recurrent planes, then W2
    const int64_t nrec = rec_f4(RNN);
    for (int64_t i = threadIdx.x; i < nrec; i += blockDim.x) s[i] = rec[i];
    float *bs = reinterpret_cast<float *>(s + nrec);
    for (int i = threadIdx.x; i < 5 * kHid + 16 * g.nct; i += blockDim.x) {
        const int blk = i >> 6, u = i & 63;
        float v;
        if (blk == 0) v = a.b1[u];
        else if (blk < 5) {
            if (RNN) v = blk == 1 ? a.bi[u] + a.bh[u]
                       : blk == 2 ? a.bi[kHid + u] + a.bh[kHid + u]
                       : blk == 3 ? a.bi[2 * kHid + u] : a.bh[2 * kHid + u];
            else v = blk == 1 ? a.bi[u] : 0.f;
        } else {
            const int j = i - 5 * kHid;
            v = j < g.nout ? a.b2[j] : 0.f;
        }
        bs[i] = v;
    }
    if (W2L) {
        const int64_t n2 = w2s_f4(g.nct), off = lds_w2_off(RNN, g.nct);
        for (int64_t i = threadIdx.x; i < n2; i += blockDim.x) s[off + i] = rec[nrec + i];
    }
    {
        const u32x4v *w1 = a.pk + 1 + w1_idx(h2_s0(a) + a.w1_off, 0, 0, 0);
        const int64_t n1 = (int64_t)a.w1_lds * 4 * 2 * 64, off = lds_w1_off(RNN, g.nct, W2L);
        for (int64_t i = threadIdx.x; i < n1; i += blockDim.x) s[off + i] = w1[i];
    }
    const int4 hdr = *reinterpret_cast<const int4 *>(a.pk);
    sw[0] = hdr.x;
    sw[1] = hdr.y;
    sw[2] = hdr.z;
    sw[3] = hdr.w;
}

// The recurrent layer, fc2 and selection of one 32-row wave tile (shared by the agent kernel
// and the rollout kernel): xB = relu(fc1) fragments, hB = h_in rows (GRU).
// ALLAV: every task is available (the rollout wrote avail = 1 itself).  act_lds (rollout):
// also receives each row's selected task (index lrow0 + row within the tile).
struct NoTailHook {
    template <class H>
    __device__ void operator()(const H &) const {}
};

// after_rec(hp): called once the recurrent layer has consumed hB and stored h', with the h'
// fragments (the layout hB came in; the rollout issues the next agent tile's h_t loads there,
// or -- the SQ64 instances -- keeps hp as that tile's h_t).  HCOND: h' goes to Hout only when
// store_h says so (the wave-pair rollout: the launch's last agent pass); false = always.
template <int NT, bool RNN, bool SEL, bool W2L, bool ALLAV, bool GEN, bool HCOND = false, class Hook = NoTailHook,
          class A>
__device__ __forceinline__ void h2_tail(A &a, const u32x4v *Wl, const int (&sw)[4], int64_t row0,
                                        const int64_t (&rows)[NT], const bool (&ok)[NT], const float4 (&hB)[4][NT],
                                        const f32x4 (&xB)[4][NT], uint16_t *act_lds = nullptr, int lrow0 = 0,
                                        const Hook &after_rec = Hook{}, bool store_h = true) {
    // lane-derived addresses are recomputed here, not hoisted out of the callers' step / env
    // loops (there they would be live across every tile and spill; their reloads would wait
    // behind the tile stores in the in-order vmcnt queue)
    int lane_ = threadIdx.x & 63;
    asm volatile("" : "+v"(lane_));
    const int lane = lane_, r = lane & 15, q = lane >> 4;
    const int nout = a.g.nout, nct = a.g.nct;
    const lds_u4p Wr = (lds_u4p)Wl;
    const lds_f4v Bs = (lds_f4v)(Wl + rec_f4(RNN));  // biases
    // availability words of fc2's first four output tiles: issued now, used after the
    // recurrent layer
    auto &sel = a.sel;
    const uint8_t *arow[NT];
    int64_t oidx[NT];
    bool av4 = false;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        arow[nt] = nullptr;
        oidx[nt] = 0;
    }
    if (SEL) {
        const int64_t b0 = row0 / sel.n;
        const int i0 = (int)(row0 - b0 * sel.n);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            int64_t b = b0;
            int i = i0 + 16 * nt + r;
            while (i >= sel.n) {
                i -= sel.n;
                ++b;
            }
            arow[nt] = ALLAV ? nullptr : sel.avail + (ok[nt] ? b * sel.a0 + (int64_t)i * sel.a1 : 0);
            oidx[nt] = b * sel.o0 + (int64_t)i * sel.o1;
        }
        av4 = !ALLAV && !GEN && ((reinterpret_cast<uintptr_t>(sel.avail) | (uintptr_t)sel.a0 | (uintptr_t)sel.a1) & 3u) == 0;
    }
    // 4 availability bytes of tasks 16 c + 4 q .. + 3 (0 past n_out)
    auto load_av = [&](int c, int nt) -> uint32_t {
        const int j0 = 16 * c + 4 * q;
        if (!SEL || !ok[nt]) return 0u;
        if (ALLAV) {
            if (!GEN) return 0x01010101u;
            const int nv = nout - j0;
            return nv >= 4 ? 0x01010101u : (nv <= 0 ? 0u : (0x01010101u & ((1u << (8 * nv)) - 1u)));
        }
        const uint8_t *ap = arow[nt] + j0;
        if (av4) return *reinterpret_cast<const uint32_t *>(ap);
        uint32_t w = 0;
#pragma unroll
        for (int v = 0; v < 4; ++v)
            if (!GEN || j0 + v < nout) w |= (uint32_t)ap[v] << (8 * v);
        return w;
    };
    uint32_t avw[4][NT];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) avw[c][nt] = c < nct ? load_av(c, nt) : 0u;

    // ---- recurrent layer: per-row scales, operand planes ---------------------------------
    float mx[NT], mh[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        mx[nt] = 0.f;
        mh[nt] = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            mx[nt] = absmax4(mx[nt], xB[t][nt]);
            if (RNN) mh[nt] = absmax4(mh[nt], hB[t][nt]);
        }
        mx[nt] = row_max4(mx[nt]);
        if (RNN) mh[nt] = row_max4(mh[nt]);
    }
    int Sg[NT];
    bool hz_all = true;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const bool hz = !RNN || !(mh[nt] > 0.f);  // zero h rows (init_hidden): no W_hh products
        hz_all = hz_all && hz;
        int s = min(sw[1] + h2_scale(mx[nt], -90, 90), hz ? 1000 : sw[2] + h2_scale(mh[nt], -90, 90));
        Sg[nt] = s > 100 ? 100 : (s < -100 ? -100 : s);
    }
    const bool h_zero = !RNN || __ballot(!hz_all) == 0;  // wave-uniform: skip the W_hh MFMAs
    u32x4v xP[2][NT][2], hP[2][NT][2];
#pragma unroll
    for (int sl = 0; sl < 2; ++sl)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            float v8[8], h8[8];
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    v8[4 * c + v] = xB[2 * sl + c][nt][v];
                    h8[4 * c + v] = RNN ? comp(hB[2 * sl + c][nt], v) : 0.f;
                }
            split2s(v8, pow2f(Sg[nt] - sw[1]), xP[sl][nt][0], xP[sl][nt][1]);
            if (RNN) split2s(h8, pow2f(Sg[nt] - sw[2]), hP[sl][nt][0], hP[sl][nt][1]);
        }
    f32x4 hp[4][NT];
    if (RNN) {
        // sigmoid(g 2^-S) = 1 / (1 + 2^(g c1)), tanh(y 2^-S) = 2 / (1 + 2^(y c2)) - 1
        float c1[NT], c2[NT], scS[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            c1[nt] = -1.4426950408889634f * pow2f(-Sg[nt]);
            c2[nt] = 2.0f * c1[nt];
            scS[nt] = pow2f(Sg[nt]);
        }
        const lds_u4p Wih = Wr, Whh = (lds_u4p)(Wl + 3 * kGateF4);
        // the whole recurrent layer per h_zero case: no branch between the four hidden blocks,
        // so the scheduler can overlap one block's gate math with the next block's MFMAs
        auto gru = [&](auto hz_tag) {
        constexpr bool HZ = decltype(hz_tag)::value;
#pragma unroll
        for (int hb = 0; hb < 4; ++hb) {
            // r and z sum the input and hidden products in one accumulator, from b_i + b_h;
            // n keeps them apart (n = tanh(i_n + r * h_n))
            const f32x4 br = Bs[16 + 4 * hb + q], bz = Bs[32 + 4 * hb + q], bn = Bs[48 + 4 * hb + q],
                        bhn = Bs[64 + 4 * hb + q];
            f32x4 gr[NT], gz[NT], gni[NT], gnh[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                gr[nt] = br * scS[nt];
                gz[nt] = bz * scS[nt];
                gni[nt] = bn * scS[nt];
                gnh[nt] = bhn * scS[nt];
            }
#pragma unroll
            for (int sl = 0; sl < 2; ++sl)
#pragma unroll
                for (int g = 0; g < 3; ++g) {
                    const u32x4v w[2] = {Wih[gate_idx(g, hb, sl, 0, lane)], Wih[gate_idx(g, hb, sl, 1, lane)]};
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        f32x4 &acc_ = g == 0 ? gr[nt] : (g == 1 ? gz[nt] : gni[nt]);
                        acc_ = mfma_h2(w, xP[sl][nt], acc_);
                    }
                }
            if (!HZ && !h_zero) {
#pragma unroll
                for (int sl = 0; sl < 2; ++sl)
#pragma unroll
                    for (int g = 0; g < 3; ++g) {
                        const u32x4v w[2] = {Whh[gate_idx(g, hb, sl, 0, lane)], Whh[gate_idx(g, hb, sl, 1, lane)]};
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) {
                            f32x4 &acc_ = g == 0 ? gr[nt] : (g == 1 ? gz[nt] : gnh[nt]);
                            acc_ = mfma_h2(w, hP[sl][nt], acc_);
                        }
                    }
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const float rg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(gr[nt][v] * c1[nt]));
                    const float zg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(gz[nt][v] * c1[nt]));
                    const float ng =
                        2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f((gni[nt][v] + rg * gnh[nt][v]) * c2[nt])) -
                        1.0f;
                    const float hv = comp(hB[hb][nt], v);  // the exact h (the planes carry it to 2^-22)
                    hp[hb][nt][v] = ng + zg * (hv - ng);
                }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                if (ok[nt] && !(ALLAV && (ASG_ROLLOUT_XSKIP & 16)) && (!HCOND || store_h))
                    *reinterpret_cast<float4 *>(a.Hout + rows[nt] * kHid + 16 * hb + 4 * q) =
                        make_float4(hp[hb][nt][0], hp[hb][nt][1], hp[hb][nt][2], hp[hb][nt][3]);
        }
        };
        if (h_zero) gru(std::true_type{});
        else gru(std::false_type{});
    } else {
        // Linear + ReLU (use_rnn = False): h' = relu(W_rnn x + b_rnn), one gate of planes.  The
        // bias is added once, after the products (as fc1 and fc2 do): an accumulator that starts
        // from b 2^S rounds at the bias's magnitude with each of the six MFMAs, which with small
        // weights is ~4 ulp of h' where PyTorch's fp32 has half of one.  The accumulators start
        // from b * 0 with the zero in a register the compiler cannot see through: started from
        // literal zeros, the GEN select and rollout instantiations came out 6e-5 off on rows
        // 16..31, units 0..15 of every tile (hipcc of ROCm 7, gfx950; cause not found), and the
        // bit-identity tests caught it.  Same instruction count as before.
        float scS[NT], un[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            un[nt] = pow2f(-Sg[nt]);
            scS[nt] = 0.f;
            asm volatile("" : "+v"(scS[nt]));
        }
#pragma unroll
        for (int hb = 0; hb < 4; ++hb) {
            const f32x4 bb = Bs[16 + 4 * hb + q];
            f32x4 acc[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = bb * scS[nt];
#pragma unroll
            for (int sl = 0; sl < 2; ++sl) {
                const u32x4v w[2] = {Wr[gate_idx(0, hb, sl, 0, lane)], Wr[gate_idx(0, hb, sl, 1, lane)]};
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[nt] = mfma_h2(w, xP[sl][nt], acc[nt]);
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
                for (int v = 0; v < 4; ++v) hp[hb][nt][v] = fmaxf(__builtin_fmaf(acc[nt][v], un[nt], bb[v]), 0.f);
                if (ok[nt] && (!HCOND || store_h))
                    *reinterpret_cast<float4 *>(a.Hout + rows[nt] * kHid + 16 * hb + 4 * q) =
                        make_float4(hp[hb][nt][0], hp[hb][nt][1], hp[hb][nt][2], hp[hb][nt][3]);
            }
        }
    }

    after_rec(hp);
    // ---- fc2 (+ selection state), per-row scale --------------------------------------------
    int S3[NT];
    u32x4v hq[2][NT][2];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        float m3 = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) m3 = absmax4(m3, hp[t][nt]);
        m3 = row_max4(m3);
        const int s3 = h2_scale(m3, -90, 90 - sw[3]);
        S3[nt] = sw[3] + s3;
        const float c3 = pow2f(s3);
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
            float v8[8];
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int v = 0; v < 4; ++v) v8[4 * c + v] = hp[2 * sl + c][nt][v];
            split2s(v8, c3, hq[sl][nt][0], hq[sl][nt][1]);
        }
    }
    float best[NT], un3[NT];
    int bj[NT];
    uint64_t amask[NT][2];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        best[nt] = -__builtin_inff();
        bj[nt] = 0x7fffffff;
        amask[nt][0] = amask[nt][1] = 0;
        un3[nt] = pow2f(-S3[nt]);
    }
    int lane2 = lane;
    // the rollout recomputes the lane's W2 address here each tile (hoisted, it was spilled and
    // its reload waited for every store of the tile)
    if (ALLAV) asm volatile("" : "+v"(lane2));
    const lds_u4p W2s = (lds_u4p)(Wl + lds_w2_off(RNN, nct));
    const u32x4v *W2g = a.pk + 1 + w1s_f4(a.g.Kp) + rec_f4(RNN);
    for (int c0 = 0; c0 < nct; c0 += 4) {
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            const int c = c0 + cc;
            if (c >= nct) break;
            const int j0 = 16 * c + 4 * q;
            uint32_t av[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const uint32_t w = avw[cc][nt];
                av[nt] = ((w & 0xffu) != 0) | (((w >> 8) & 0xffu) != 0) << 1 | (((w >> 16) & 0xffu) != 0) << 2 |
                         ((w >> 24) != 0) << 3;
                if (c + 4 < nct) avw[cc][nt] = load_av(c + 4, nt);  // the ring: 4 tiles ahead
            }
            f32x4 a2[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) a2[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int sl = 0; sl < 2; ++sl) {
                u32x4v w[2];
#pragma unroll
                for (int pl = 0; pl < 2; ++pl)
                    w[pl] = W2L ? W2s[w2_idx(c, sl, pl, lane2)] : W2g[w2_idx(c, sl, pl, lane2)];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) a2[nt] = mfma_h2(w, hq[sl][nt], a2[nt]);
            }
            const f32x4 bq = Bs[80 + 4 * c + q];  // b2[16 c + 4 q ..] (zero past n_out)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const f32x4 qv = a2[nt] * un3[nt] + bq;
                if (a.Q && ok[nt]) {
                    float *qp = a.Q + rows[nt] * nout + j0;
                    if (!GEN) {
                        *reinterpret_cast<float4 *>(qp) = make_float4(qv[0], qv[1], qv[2], qv[3]);
                    } else {
#pragma unroll
                        for (int v = 0; v < 4; ++v)
                            if (j0 + v < nout) qp[v] = qv[v];
                    }
                }
                if (SEL && ALLAV && !GEN) {
                    // every task available and inside the row (the rollout at m % 32 == 0): the
                    // lane's first task (c = 0, v = 0) is its first candidate, then strictly
                    // greater or the first NaN -- the torch.max order below without the
                    // availability / range terms
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int j = j0 + v;
                        const float x = qv[v];
                        const bool b = (c == 0 && v == 0) | ((best[nt] == best[nt]) & !(x <= best[nt]));
                        best[nt] = b ? x : best[nt];
                        bj[nt] = b ? j : bj[nt];
                    }
                } else if (SEL) {
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        // a lane meets its tasks in increasing j, so torch.max order reduces
                        // to: the first candidate, then strictly greater, or the first NaN
                        const int j = j0 + v;
                        const float x = ((av[nt] >> v) & 1u) ? qv[v] : -__builtin_inff();
                        const bool b = ((bj[nt] == 0x7fffffff) & (j < nout)) |
                                       ((best[nt] == best[nt]) & !(x <= best[nt]) & (j < nout));
                        best[nt] = b ? x : best[nt];
                        bj[nt] = b ? j : bj[nt];
                    }
                    amask[nt][0] |= (uint64_t)av[nt] << (4 * (c & 15));
                }
            }
        }
    }
    if (SEL && ALLAV && !GEN) {
        // the availability masks the exploration draw reads: every task of the lane's tiles
        const uint64_t all = nct >= 16 ? ~0ull : ((1ull << (4 * nct)) - 1ull);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) amask[nt][0] = all;
    }
    if (SEL) {
        const int act = select_finish<false, NT>(best, bj, amask, rows, ok, oidx, nct, sel, q);
        const int nt = NT == 1 ? 0 : (q & 1);
        if (act_lds && q < NT && ok[nt]) act_lds[lrow0 + 16 * nt + r] = (uint16_t)act;
    }
}

// One wave, 32 agent rows of a flat [R][K] input: fc1 -> recurrent layer -> fc2 (+ selection).
template <int NT, bool RNN, bool SEL, bool W2L, bool GEN, class A>
__device__ __forceinline__ void agent_rows_h2(int64_t row0, A &a, const u32x4v *Wl, const int (&sw)[4]) {
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    if (row0 >= a.R) return;
    auto &g = a.g;
    int64_t rows[NT];
    bool ok[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        rows[nt] = row0 + 16 * nt + r;
        ok[nt] = rows[nt] < a.R;
    }
    const lds_f4v Bs = (lds_f4v)(Wl + rec_f4(RNN));
    const u32x4v *W1g = a.pk + 1;
    const float *xr[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) xr[nt] = a.X + (ok[nt] ? rows[nt] : 0) * a.xs;
    const int Ub = g.Pp >> 5, nsl = g.Kp >> 5;
    const int s0 = h2_s0(a);

    // padded slice sl of every row: block sl / Ub, inputs 32 (sl % Ub) + 16 c + 4 q + e of it
    auto load_x = [&](int sl, float4 (&xv)[2][NT]) {
        if (!GEN) {
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    xv[c][nt] = *reinterpret_cast<const float4 *>(xr[nt] + 32 * sl + 16 * c + 4 * q);
        } else {
            const int blk = sl / Ub, jj0 = 32 * (sl - blk * Ub);
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int jj = jj0 + 16 * c + 4 * q;
                    const float *p = xr[nt] + (int64_t)blk * g.P + jj;
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (ok[nt] && jj + e < g.P) ? p[e] : 0.f;
                    xv[c][nt] = make_float4(v[0], v[1], v[2], v[3]);
                }
        }
    };
    // block 0 chunks t4 .. t4 + 3 (16 inputs each)
    auto load_pa = [&](int t4, float4 (&pa)[4][NT]) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int jj = 16 * (t4 + c) + 4 * q;
                if (t4 + c >= (g.Pp >> 4)) {
                    pa[c][nt] = make_float4(0.f, 0.f, 0.f, 0.f);
                } else if (!GEN) {
                    pa[c][nt] = *reinterpret_cast<const float4 *>(xr[nt] + jj);
                } else {
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (ok[nt] && jj + e < g.P) ? xr[nt][jj + e] : 0.f;
                    pa[c][nt] = make_float4(v[0], v[1], v[2], v[3]);
                }
            }
    };
    float4 pa[4][NT];
    if (a.pre) load_pa(0, pa);
    // main-loop slice order: with the prefix geometry (blocks 1 .. NB - 1 of Ub chunks), chunk
    // u outer and block inner -- the order in which the rollout kernel generates them
    const int nmain = nsl - s0;
    const int nblk = g.NB - 1;
    auto sl_of = [&](int idx) { return a.pre ? (idx % nblk + 1) * Ub + idx / nblk : idx; };
    float4 xbuf[kH2XBuf][2][NT];
#pragma unroll
    for (int b = 0; b < kH2XBuf; ++b)
        if (b < nmain) load_x(sl_of(b), xbuf[b]);

    // ---- one-hot prefix: rows whose block 0 is onehot(a) or zero add W1[:, a] (W1T, f32)
    // instead of running those slices' MFMAs
    int pos[NT];
    bool onehot = false;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) pos[nt] = -1;
    if (a.pre) {
        bool bad = false;
        for (int t4 = 0; t4 < (g.Pp >> 4); t4 += 4) {
            if (t4 > 0) load_pa(t4, pa);
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float v = comp(pa[c][nt], e);
                        const bool one = v == 1.0f;
                        bad |= (one && pos[nt] >= 0) || (!one && v != 0.0f);
                        pos[nt] = one ? 16 * (t4 + c) + 4 * q + e : pos[nt];
                    }
        }
        bool rows_ok = true;  // a row's 1 may sit in only one of its 4 lanes
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const uint64_t mk = __ballot(pos[nt] >= 0);
            const uint64_t g0 = mk & 0xffffull, g1 = (mk >> 16) & 0xffffull, g2 = (mk >> 32) & 0xffffull, g3 = mk >> 48;
            rows_ok = rows_ok && ((g0 & g1) | (g0 & g2) | (g0 & g3) | (g1 & g2) | (g1 & g3) | (g2 & g3)) == 0;
            int p = pos[nt];
            p = max(p, __shfl_xor(p, 16));
            p = max(p, __shfl_xor(p, 32));
            pos[nt] = p;
        }
        onehot = rows_ok && __ballot(bad) == 0;
    }
    // ---- fc1 on split f16 MFMAs, per-row input scale ----------------------------------------
    f32x4 acc[4][NT];
    int sx[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) sx[nt] = kH2SxInit;
    float4 hB[4][NT];
    auto load_h = [&]() {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                hB[t][nt] = (RNN && a.Hin) ? *reinterpret_cast<const float4 *>(a.Hin + (ok[nt] ? rows[nt] : 0) * a.hs +
                                                                              16 * t + 4 * q)
                                           : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    for (int attempt = 0;; ++attempt) {
        if (attempt > 0) {
#pragma unroll
            for (int b = 0; b < kH2XBuf; ++b)
                if (b < nmain) load_x(sl_of(b), xbuf[b]);
        }
        float scx[NT], rmax[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            scx[nt] = pow2f(sx[nt]);
            rmax[nt] = 0.f;
            const float scS = pow2f(sw[0] + sx[nt]);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const float4 gv = (onehot && pos[nt] >= 0)
                                      ? *reinterpret_cast<const float4 *>(a.W1T + pos[nt] * kHid + 16 * mt + 4 * q)
                                      : make_float4(0.f, 0.f, 0.f, 0.f);
                acc[mt][nt] = f32x4{gv.x, gv.y, gv.z, gv.w} * scS;
            }
        }
        auto slice = [&](int sl, const float4 (&xv)[2][NT], bool lds) {
            u32x4v xp[NT][2];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                rmax[nt] = absmax4(absmax4(rmax[nt], xv[0][nt]), xv[1][nt]);
                const float x8[8] = {xv[0][nt].x, xv[0][nt].y, xv[0][nt].z, xv[0][nt].w,
                                     xv[1][nt].x, xv[1][nt].y, xv[1][nt].z, xv[1][nt].w};
                split2s(x8, scx[nt], xp[nt][0], xp[nt][1]);
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                u32x4v w[2];
                if (lds) {
                    const lds_u4p W1s = (lds_u4p)(Wl + lds_w1_off(RNN, g.nct, W2L));
#pragma unroll
                    for (int pl = 0; pl < 2; ++pl) w[pl] = W1s[w1_idx(sl - s0, mt, pl, lane)];
                } else {
#pragma unroll
                    for (int pl = 0; pl < 2; ++pl) w[pl] = W1g[w1_idx(sl, mt, pl, lane)];
                }
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = mfma_h2(w, xp[nt], acc[mt][nt]);
            }
        };
        // block 0 of a tile that is not one-hot: its slices through L2
        for (int sl = 0; sl < ((a.pre && !onehot) ? s0 : 0); ++sl) {
            float4 xv[2][NT];
            load_x(sl, xv);
            slice(sl, xv, false);
        }
        const int s_l2 = s0 + a.w1_lds;  // first slice read through L2
        for (int i0 = 0; i0 < nmain; i0 += kH2XBuf) {
#pragma unroll
            for (int b = 0; b < kH2XBuf; ++b) {
                if (i0 + b < nmain) {
                    const int sl = sl_of(i0 + b);
                    if (sl < s_l2) slice(sl, xbuf[b], true);
                    else slice(sl, xbuf[b], false);
                    if (i0 + b + kH2XBuf < nmain) load_x(sl_of(i0 + b + kH2XBuf), xbuf[b]);
                }
            }
        }
        if (attempt == 0 && RNN) load_h();  // after fc1: 32 fewer VGPRs live through it
        // the split needs |x| 2^sx < 2^15 (|h| <= 65504): rows that overflow redo at their own
        // smaller scale (the others keep theirs, so their values are unchanged)
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
    f32x4 xB[4][NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const float un = pow2f(-(sw[0] + sx[nt]));
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const f32x4 bb = Bs[4 * mt + q];  // b1[16 mt + 4 q ..]
#pragma unroll
            for (int v = 0; v < 4; ++v) xB[mt][nt][v] = fmaxf(acc[mt][nt][v] * un + bb[v], 0.f);
        }
    }
    h2_tail<NT, RNN, SEL, W2L, false, GEN>(a, Wl, sw, row0, rows, ok, hB, xB);
}

// LDS plan: recurrent planes, biases, W2 planes when they fit, then as many W1 slices (from
// s0) as fit; `reserve` bytes per workgroup kept for a per-wave scratch
struct H2Lds {
    bool w2l;
    int w1_lds, l2_slices;
    int64_t scratch_off;  // u32x4v units
    size_t bytes;
};
constexpr int64_t kH2LdsBytes = 160 * 1024;
static inline H2Lds h2_lds_plan(const H2Geom &g, bool rnn, int s0, int64_t reserve_f4) {
    constexpr int64_t kCap = kH2LdsBytes / 16;
    H2Lds p{};
    p.w2l = lds_w2_off(rnn, g.nct) + w2s_f4(g.nct) + reserve_f4 <= kCap;
    const int64_t w1off = lds_w1_off(rnn, g.nct, p.w2l);
    const int64_t slices = g.Kp / 32 - s0, fit = (kCap - reserve_f4 - w1off) / (4 * 2 * 64);
    p.w1_lds = (int)(fit < slices ? (fit > 0 ? fit : 0) : slices);
    p.l2_slices = (int)(slices - p.w1_lds);
    p.scratch_off = w1off + (int64_t)p.w1_lds * 4 * 2 * 64;
    p.bytes = (size_t)(p.scratch_off + reserve_f4) * 16;
    return p;
}

}  // namespace asg
