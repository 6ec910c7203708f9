// asg_agent.hip -- the RNNAgent forward for 256 < n_out <= 512: f32 fc1 / fc2, split-bf16 GRU
// (gfx950).  Every shape with n_out <= 256 runs the split-f16 path (asg_h2.hip); the entry
// points here (pack, forward, forward + selection) hand those over and keep the rest.
//
// RNNAgent.forward (modules/agents/rnn_agent.py:23-31) over all B*n agent rows of one
// env step, in ONE pass over the observation slab:
//     x  = relu(obs @ W1^T + b1)
//     gi = x @ W_ih^T + b_ih ; gh = h @ W_hh^T + b_hh            (use_rnn: GRUCell)
//     r = sigmoid(gi_r + gh_r); z = sigmoid(gi_z + gh_z); n = tanh(gi_n + r * gh_n)
//     h' = n + z * (h - n)
//   or h' = relu(x @ W_rnn^T + b_rnn)                             (use_rnn = False)
//     q  = h' @ W2^T + b2
// Every intermediate stays in registers / LDS: HBM sees the observation rows once, h in, h'
// and q out.
//
// Arithmetic: fc1, the Linear layer and fc2 on v_mfma_f32_16x16x4_f32 -- exact fp32 products,
// fp32 accumulation (a k-ordered fmaf chain); only the summation order differs from
// hipBLASLt's.  The GRU's products on bf16 MFMAs with a three-way operand split (below).
// One wave owns 32 agent rows; all activations stay in registers (see the transposed
// formulation below), W1 comes from L1/L2 in a pre-packed fragment order, the recurrent
// weights (and W2 when it fits beside them) from LDS.
//
// Also here, for every agent path: stream_cus, onehot_prefix_enabled and the W1^T pack of
// the one-hot prefix (launch_w1t_pack, used by the split-f16 pack).
#include <type_traits>

#include "asg_agent_common.h"

// The library builds with -ffp-contract=off so the env and LSA kernels round every float64
// add/mul as numpy does.  The agent's results are fp32-accurate, not bit-matched to a
// reference order, so its elementwise math (bias epilogues, GRU gates, Q unscaling) may
// fuse into FMAs: fewer VALU instructions, one rounding instead of two.
#pragma clang fp contract(fast)

namespace asg {

constexpr int kNT = 2;  // 16-row tiles per wave: 32 rows per wave at 2 waves per SIMD
constexpr int kRowsPerWave = 16 * kNT;
constexpr int kLdsWavesPerSimd = 2;  // waves per SIMD the register budget is fitted to
constexpr int kLdsWaves = 4 * kLdsWavesPerSimd;

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// GRU products on bf16 MFMAs with a three-way operand split: an f32 x is truncated into
// hi + mid + lo bf16 parts with x == hi + mid + lo exactly (each residual is exact and fits 8
// significant bits), and x . w is summed from the six cross products down to 2^-16 relative
// (hi.hi, hi.mid, mid.hi, hi.lo, lo.hi, mid.mid): the dropped terms are below 2^-22 relative,
// so the gates match the fp32 module to ~1e-7.  Each bf16 MFMA covers 32 k at 16 cycles, the
// f32 MFMA 4 k at 32 cycles: 6 bf16 vs 8 f32 MFMAs per 32-deep k-slice = 2.7x less
// matrix-pipe time.  Non-finite inputs come out NaN.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
// packed W_ih / W_hh: [gate 3][slab hb 4][k-slice 2][plane 3][lane 64] x 8 bf16
constexpr int kGruX3F4 = 3 * 4 * 2 * 3 * 64;
__device__ __forceinline__ int gru_x3_idx(int g, int hb, int s, int plane, int lane) {
    return (((g * 4 + hb) * 2 + s) * 3 + plane) * 64 + lane;
}
// the k of element j in lane quad q of k-slice s: the f32 accumulator layout of the layer
// before (units 4q + v of tiles 2s and 2s + 1), so activations feed the MFMA in place
__device__ __forceinline__ int gru_x3_k(int s, int q, int j) { return 32 * s + (j < 4 ? 4 * q + j : 16 + 4 * q + j - 4); }

__device__ __forceinline__ f32x4 mfma_bf16(const u32x4v &a, const u32x4v &b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c,
                                                   0, 0, 0);
}
// 8 f32 -> three bf16x8 planes (element j in half j & 1 of dword j >> 1)
__device__ __forceinline__ void split3(const float (&x)[8], u32x4v &h, u32x4v &m, u32x4v &l) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const uint32_t xa = __builtin_bit_cast(uint32_t, x[2 * p]), xb = __builtin_bit_cast(uint32_t, x[2 * p + 1]);
        const float ra = x[2 * p] - __builtin_bit_cast(float, xa & 0xffff0000u);
        const float rb = x[2 * p + 1] - __builtin_bit_cast(float, xb & 0xffff0000u);
        const uint32_t ua = __builtin_bit_cast(uint32_t, ra), ub = __builtin_bit_cast(uint32_t, rb);
        const float sa = ra - __builtin_bit_cast(float, ua & 0xffff0000u);
        const float sb = rb - __builtin_bit_cast(float, ub & 0xffff0000u);
        // upper halves of (a, b) -> one dword (v_perm_b32: bytes 2, 3 of a, then of b)
        h[p] = __builtin_amdgcn_perm(xb, xa, 0x07060302u);
        m[p] = __builtin_amdgcn_perm(ub, ua, 0x07060302u);
        l[p] = __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, sb), __builtin_bit_cast(uint32_t, sa), 0x07060302u);
    }
}
// sum of the six significant cross products of (wh, wm, wl) . (xh, xm, xl)
__device__ __forceinline__ f32x4 mfma_x3(const u32x4v (&w)[3], const u32x4v (&x)[3], f32x4 c) {
    c = mfma_bf16(w[0], x[0], c);
    c = mfma_bf16(w[0], x[1], c);
    c = mfma_bf16(w[1], x[0], c);
    c = mfma_bf16(w[0], x[2], c);
    c = mfma_bf16(w[2], x[0], c);
    c = mfma_bf16(w[1], x[1], c);
    return c;
}

__device__ __forceinline__ float4 ldg4(const float *p, bool ok) {
    return ok ? *reinterpret_cast<const float4 *>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// GRU nonlinearities on the hardware transcendental units (v_exp_f32, v_rcp_f32): a few
// ulp from the correctly rounded libm forms, far inside the 1e-5 parity tolerance.
__device__ __forceinline__ float sigmoidf_(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float tanhf_(float x) { return 2.0f * sigmoidf_(2.0f * x) - 1.0f; }

// Packed weight layout ("fragment order"): for W [C][K] row-major (torch nn.Linear), block
// (t, ct) holds, for lane l, W[16 ct + (l & 15)][16 t + 4 (l >> 4) .. + 3] as one float4,
// so one wave loads a whole MFMA B-operand chunk as 1 KiB of contiguous memory.  K is
// zero-padded to a multiple of 16.  The packed buffer, in float4:
//   W1: [K16/16][4][64]; GRU: W_ih, W_hh as bf16 planes (kGruX3F4 each), Linear: W_rnn
//   [4][4][64]; W2: [4][nq][64], nq = ceil(n_out / 16) (zero rows pad the last output tile)
__device__ __forceinline__ int64_t pk(int t, int ct, int nct, int lane) { return ((int64_t)t * nct + ct) * 64 + lane; }

__global__ void pack_weights_kernel(const float *W, int C, int K, float4 *out) {
    const int nct = (C + 15) / 16, nt = (K + 15) / 16;  // rows >= C (the n_out tail) are zero
    const int64_t total = (int64_t)nt * nct * 64;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int lane = (int)(i & 63);
        const int ct = (int)((i >> 6) % nct);
        const int t = (int)((i >> 6) / nct);
        const int row = 16 * ct + (lane & 15), k = 16 * t + 4 * (lane >> 4);
        const bool okr = row < C;
        float4 v;
        v.x = okr && k + 0 < K ? W[(int64_t)row * K + k + 0] : 0.f;
        v.y = okr && k + 1 < K ? W[(int64_t)row * K + k + 1] : 0.f;
        v.z = okr && k + 2 < K ? W[(int64_t)row * K + k + 2] : 0.f;
        v.w = okr && k + 3 < K ? W[(int64_t)row * K + k + 3] : 0.f;
        out[i] = v;
    }
}

// ---------------------------------------------------------------------------------
// Transposed formulation: every layer computes out^T = W . act^T, i.e. the MFMA A operand
// is a packed weight fragment and the B operand an activation fragment.  With the
// 16x16x4 f32 MFMA layouts
//     A: lane l gives W[16 mt + (l & 15)][k = 16 t + 4 (l >> 4) + e]        (packed float4)
//     B: lane l gives act[row 16 nt + (l & 15)][k = 16 t + 4 (l >> 4) + e]  (float4 of a row)
//     C: lane l holds out[row 16 nt + (l & 15)][unit 16 mt + 4 (l >> 4) + v], v = 0..3
// the accumulator of output tile mt IS the B-operand float4 of the next layer's k-chunk
// t = mt, so activations go from layer to layer in registers: no LDS, no transposes, no
// barriers.  One wave owns 32 rows (nt = 0, 1); lane (r, q) = (l & 15, l >> 4).
// ---------------------------------------------------------------------------------
// Any K, any n_out <= 512 (checked by the ABI): guarded row loads, and the last output tile
// partial when n_out % 16 != 0 (zero weight rows, masked bias / Q / availability).  A lane
// keeps 4 availability bits per output tile in two u64 (tiles 0-15, 16-31).

// (the fused epsilon-greedy epilogue, select_finish, is in asg_agent_common.h)

// W2l: W2 staged in LDS (w2l_on), else W2p is read through L2
template <bool RNN, bool SEL>
__device__ __forceinline__ void agent_rows(
    int64_t row0, const float *__restrict__ X, int64_t xs, int64_t R, int K, const float *__restrict__ Hin, int64_t hs,
    const float4 *__restrict__ W1p, const float *__restrict__ b1, const float4 *__restrict__ Wihp,
    const float *__restrict__ bih, const float4 *__restrict__ Whhp, const float *__restrict__ bhh,
    const float4 *__restrict__ W2p, const float *__restrict__ b2, int nout, float *__restrict__ Hout,
    float *__restrict__ Q, const SelectArgs &sel, const float4 *W2l, bool w2l_on) {
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    if (row0 >= R) return;  // whole wave idle
    int64_t rows[kNT];
    bool ok[kNT];
#pragma unroll
    for (int nt = 0; nt < kNT; ++nt) {
        rows[nt] = row0 + 16 * nt + r;
        ok[nt] = rows[nt] < R;
    }

    // ---- h_in fragments (B operand of W_hh, and h of the GRU update): issued before fc1 so
    // they arrive under its MFMAs (issued after it, every tile's GRU waited on them) -------
    float4 hB[4][kNT];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int nt = 0; nt < kNT; ++nt)
            hB[t][nt] = ldg4(Hin + (ok[nt] ? rows[nt] : 0) * hs + 16 * t + 4 * q, RNN && Hin && ok[nt]);

    // ---- fc1: x^T = relu(W1 X^T + b1), X rows streamed from HBM, 2 chunks in flight ----
    f32x4 xB[4][kNT];
    {
        // the bias is added once, after the products (C layout: unit 16 mt + 4 q + v): an
        // accumulator that starts from it rounds at the bias's magnitude with every MFMA --
        // with small weights or inputs several ulps of the result, where PyTorch has half of one
        f32x4 acc[4][kNT];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < kNT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float *xr[kNT];
#pragma unroll
        for (int nt = 0; nt < kNT; ++nt) xr[nt] = X + (ok[nt] ? rows[nt] : 0) * xs;
        const int nk = (K + 15) / 16;
        // float4 row loads when K, the row stride and X are 16-B aligned; else guarded scalars
        const bool xvec = ((K | xs) & 3) == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
        float4 aA[kNT], wA[4], aB[kNT], wB[4];
        auto load = [&](int t, float4 (&a4)[kNT], float4 (&w4)[4]) {
            const int k = 16 * t + 4 * q;
            if (xvec) {
#pragma unroll
                for (int nt = 0; nt < kNT; ++nt) a4[nt] = ldg4(xr[nt] + k, ok[nt] && k < K);
            } else {
#pragma unroll
                for (int nt = 0; nt < kNT; ++nt) {
                    const float *p = xr[nt] + k;
                    a4[nt].x = ok[nt] && k + 0 < K ? p[0] : 0.f;
                    a4[nt].y = ok[nt] && k + 1 < K ? p[1] : 0.f;
                    a4[nt].z = ok[nt] && k + 2 < K ? p[2] : 0.f;
                    a4[nt].w = ok[nt] && k + 3 < K ? p[3] : 0.f;
                }
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) w4[mt] = W1p[pk(t, mt, 4, lane)];
        };
        auto chunk = [&](const float4 (&a4)[kNT], const float4 (&w4)[4]) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int nt = 0; nt < kNT; ++nt)
                        acc[mt][nt] = mfma4(comp(w4[mt], e), comp(a4[nt], e), acc[mt][nt]);
        };
        // two register buffers: a buffer is refilled right after its chunk's MFMAs are issued,
        // so two chunks stay in flight
        load(0, aA, wA);
        if (nk > 1) load(1, aB, wB);
        for (int t = 0; t < nk; ++t) {
            float4 a4[kNT];
#pragma unroll
            for (int i = 0; i < kNT; ++i) a4[i] = aA[i];
            float4 w4[4] = {wA[0], wA[1], wA[2], wA[3]};
#pragma unroll
            for (int i = 0; i < kNT; ++i) aA[i] = aB[i];
#pragma unroll
            for (int i = 0; i < 4; ++i) wA[i] = wB[i];
            if (t + 2 < nk) load(t + 2, aB, wB);
            chunk(a4, w4);
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const float4 bb = *reinterpret_cast<const float4 *>(b1 + 16 * mt + 4 * q);
#pragma unroll
            for (int nt = 0; nt < kNT; ++nt)
#pragma unroll
                for (int v = 0; v < 4; ++v) xB[mt][nt][v] = fmaxf(acc[mt][nt][v] + comp(bb, v), 0.f);
        }
    }

    // ---- recurrent layer -> h'^T in registers (hp[hb] = B operand of fc2's chunk hb) ----
    bool h_zero = false;
    if (RNN) {
        bool nz = false;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int nt = 0; nt < kNT; ++nt)
                nz |= (hB[t][nt].x != 0.f) | (hB[t][nt].y != 0.f) | (hB[t][nt].z != 0.f) | (hB[t][nt].w != 0.f);
        h_zero = __ballot(nz) == 0;
    }
    f32x4 hp[4][kNT];
#pragma unroll
    for (int hb = 0; hb < 4; ++hb) {
        if (RNN) {
            // gate pre-activations: r and z sum the input and hidden products in one
            // accumulator; n keeps them apart (n = tanh(i_n + r * h_n))
            // accumulators start from the biases: r, z from b_i + b_h; n's halves apart
            const int u = 16 * hb + 4 * q;
            const float4 bir = *reinterpret_cast<const float4 *>(bih + u);
            const float4 biz = *reinterpret_cast<const float4 *>(bih + kHid + u);
            const float4 bin = *reinterpret_cast<const float4 *>(bih + 2 * kHid + u);
            const float4 bhr = *reinterpret_cast<const float4 *>(bhh + u);
            const float4 bhz = *reinterpret_cast<const float4 *>(bhh + kHid + u);
            const float4 bhn = *reinterpret_cast<const float4 *>(bhh + 2 * kHid + u);
            const f32x4 r0 = {bir.x + bhr.x, bir.y + bhr.y, bir.z + bhr.z, bir.w + bhr.w};
            const f32x4 z0 = {biz.x + bhz.x, biz.y + bhz.y, biz.z + bhz.z, biz.w + bhz.w};
            f32x4 gr[kNT], gz[kNT], gni[kNT], gnh[kNT];
#pragma unroll
            for (int nt = 0; nt < kNT; ++nt) {
                gr[nt] = r0;
                gz[nt] = z0;
                gni[nt] = f32x4{bin.x, bin.y, bin.z, bin.w};
                gnh[nt] = f32x4{bhn.x, bhn.y, bhn.z, bhn.w};
            }
            // a tile whose h is all zero (BasicMAC.init_hidden at t = 0) skips the W_hh
            // products (exact zeros): a third of the GRU's MFMAs on those steps
            const u32x4v *Wih3 = reinterpret_cast<const u32x4v *>(Wihp);
            const u32x4v *Whh3 = reinterpret_cast<const u32x4v *>(Whhp);
            auto gates = [&](auto with_h) {
#pragma unroll
                for (int sl = 0; sl < 2; ++sl) {
                    // k-slice sl = f32 chunks 2 sl and 2 sl + 1 of x (then h), split per use
                    // and the input and hidden products one after the other: registers, not
                    // VALU, are the scarce resource at two waves per SIMD
#pragma unroll
                    for (int src = 0; src < (with_h ? 2 : 1); ++src) {
                        u32x4v a3[kNT][3];
#pragma unroll
                        for (int nt = 0; nt < kNT; ++nt) {
                            float v8[8];
#pragma unroll
                            for (int c = 0; c < 2; ++c)
#pragma unroll
                                for (int v = 0; v < 4; ++v)
                                    v8[4 * c + v] = src == 0 ? xB[2 * sl + c][nt][v] : comp(hB[2 * sl + c][nt], v);
                            split3(v8, a3[nt][0], a3[nt][1], a3[nt][2]);
                        }
                        __builtin_amdgcn_sched_barrier(0);  // keep the weight reads of
                        // later slices from being hoisted here (register pressure)
                        const u32x4v *W3 = src == 0 ? Wih3 : Whh3;
#pragma unroll
                        for (int g = 0; g < 3; ++g) {
                            u32x4v w3[3];
#pragma unroll
                            for (int pl = 0; pl < 3; ++pl) w3[pl] = W3[gru_x3_idx(g, hb, sl, pl, lane)];
#pragma unroll
                            for (int nt = 0; nt < kNT; ++nt) {
                                f32x4 &acc = g == 0 ? gr[nt] : (g == 1 ? gz[nt] : (src == 0 ? gni[nt] : gnh[nt]));
                                acc = mfma_x3(w3, a3[nt], acc);
                            }
                        }
                    }
                }
            };
            if (h_zero)
                gates(std::false_type{});
            else
                gates(std::true_type{});
#pragma unroll
            for (int nt = 0; nt < kNT; ++nt)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const float rg = sigmoidf_(gr[nt][v]);
                    const float zg = sigmoidf_(gz[nt][v]);
                    const float ng = tanhf_(gni[nt][v] + rg * gnh[nt][v]);
                    const float hv = comp(hB[hb][nt], v);
                    hp[hb][nt][v] = ng + zg * (hv - ng);
                }
        } else {
            const float4 bb = *reinterpret_cast<const float4 *>(bih + 16 * hb + 4 * q);
            f32x4 a2[kNT];
#pragma unroll
            for (int nt = 0; nt < kNT; ++nt) a2[nt] = f32x4{0.f, 0.f, 0.f, 0.f};  // bias last, as fc1
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float4 w = Wihp[pk(t, hb, 4, lane)];
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int nt = 0; nt < kNT; ++nt) a2[nt] = mfma4(comp(w, e), xB[t][nt][e], a2[nt]);
            }
#pragma unroll
            for (int nt = 0; nt < kNT; ++nt)
#pragma unroll
                for (int v = 0; v < 4; ++v) hp[hb][nt][v] = fmaxf(a2[nt][v] + comp(bb, v), 0.f);
        }
        // h' block -> HBM (the new hidden state), one float4 per lane and row
#pragma unroll
        for (int nt = 0; nt < kNT; ++nt)
            if (ok[nt])
                *reinterpret_cast<float4 *>(Hout + rows[nt] * kHid + 16 * hb + 4 * q) =
                    make_float4(hp[hb][nt][0], hp[hb][nt][1], hp[hb][nt][2], hp[hb][nt][3]);
    }

    // ---- selection state: (env, agent) of each row, running argmax, availability bits ----
    const uint8_t *arow[kNT];
    bool av4 = false;
    float best[kNT];
    int bj[kNT];
    uint64_t amask[kNT][2];  // [row][c >> 4] bit 4 (c & 15) + v <-> task 16 c + 4 q + v
    int64_t oidx[kNT];
#pragma unroll
    for (int nt = 0; nt < kNT; ++nt) {
        arow[nt] = nullptr;
        best[nt] = -__builtin_inff();
        bj[nt] = 0x7fffffff;
        amask[nt][0] = amask[nt][1] = 0;
        oidx[nt] = 0;
    }
    if (SEL) {
        const int64_t b0 = row0 / sel.n;
        const int i0 = (int)(row0 - b0 * sel.n);
#pragma unroll
        for (int nt = 0; nt < kNT; ++nt) {
            int64_t b = b0;
            int i = i0 + 16 * nt + r;
            while (i >= sel.n) {
                i -= sel.n;
                ++b;
            }
            arow[nt] = sel.avail + (ok[nt] ? b * sel.a0 + (int64_t)i * sel.a1 : 0);
            oidx[nt] = b * sel.o0 + (int64_t)i * sel.o1;
        }
        av4 = ((reinterpret_cast<uintptr_t>(sel.avail) | (uintptr_t)sel.a0 | (uintptr_t)sel.a1) & 3u) == 0;
    }

    // ---- fc2 one 16-output tile at a time: q^T = W2 h'^T + b2; Q store and/or argmax ----
    const int nct = (nout + 15) / 16;
    const bool qvec = (nout & 3) == 0;
    for (int c = 0; c < nct; ++c) {
        const bool full = 16 * c + 16 <= nout;  // wave-uniform: only the last tile can be partial
        const int j0 = 16 * c + 4 * q;          // this lane's first task of the tile
        uint32_t av[kNT];  // 4 availability bits of this lane's tasks, per row
#pragma unroll
        for (int nt = 0; nt < kNT; ++nt) av[nt] = 0u;
        if (SEL) {
#pragma unroll
            for (int nt = 0; nt < kNT; ++nt) {
                const uint8_t *ap = arow[nt] + j0;
                uint32_t w = 0;
                if (ok[nt]) {
                    if (!full) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) w |= j0 + e < nout ? (uint32_t)ap[e] << (8 * e) : 0u;
                    } else if (av4) {
                        w = *reinterpret_cast<const uint32_t *>(ap);
                    } else {
                        w = (uint32_t)ap[0] | ((uint32_t)ap[1] << 8) | ((uint32_t)ap[2] << 16) | ((uint32_t)ap[3] << 24);
                    }
                }
                av[nt] = ((w & 0xffu) != 0) | (((w >> 8) & 0xffu) != 0) << 1 | (((w >> 16) & 0xffu) != 0) << 2 |
                         ((w >> 24) != 0) << 3;
            }
        }
        float4 bq;
        if (full) {
            bq = *reinterpret_cast<const float4 *>(b2 + j0);
        } else {
            bq.x = j0 + 0 < nout ? b2[j0 + 0] : 0.f;
            bq.y = j0 + 1 < nout ? b2[j0 + 1] : 0.f;
            bq.z = j0 + 2 < nout ? b2[j0 + 2] : 0.f;
            bq.w = j0 + 3 < nout ? b2[j0 + 3] : 0.f;
        }
        f32x4 a2[kNT];
#pragma unroll
        for (int nt = 0; nt < kNT; ++nt) a2[nt] = f32x4{0.f, 0.f, 0.f, 0.f};  // bias last, as fc1
        float4 w2[4];
        if (w2l_on) {  // staged in LDS: ds_read, not a flat load through a merged pointer
            typedef const f32x4 __attribute__((address_space(3))) * lds_f4p;
            const lds_f4p W2s = (lds_f4p)W2l;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const f32x4 v = W2s[pk(t, c, nct, lane)];
                w2[t] = make_float4(v[0], v[1], v[2], v[3]);
            }
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) w2[t] = W2p[pk(t, c, nct, lane)];
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int nt = 0; nt < kNT; ++nt) a2[nt] = mfma4(comp(w2[t], e), hp[t][nt][e], a2[nt]);
#pragma unroll
        for (int nt = 0; nt < kNT; ++nt) {
            a2[nt] += f32x4{bq.x, bq.y, bq.z, bq.w};
            if (Q && ok[nt]) {
                float *qp = Q + rows[nt] * nout + j0;
                if (full && qvec) {
                    *reinterpret_cast<float4 *>(qp) = make_float4(a2[nt][0], a2[nt][1], a2[nt][2], a2[nt][3]);
                } else {
#pragma unroll
                    for (int v = 0; v < 4; ++v)
                        if (j0 + v < nout) qp[v] = a2[nt][v];
                }
            }
            if (SEL) {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int j = j0 + v;
                    const float x = ((av[nt] >> v) & 1u) ? a2[nt][v] : -__builtin_inff();
                    const bool b = better(x, j, best[nt], bj[nt]);
                    best[nt] = b ? x : best[nt];
                    bj[nt] = b ? j : bj[nt];
                }
                const uint64_t bits = (uint64_t)av[nt] << (4 * (c & 15));
                if (c < 16) amask[nt][0] |= bits;
                else amask[nt][1] |= bits;
            }
        }
    }
    if (!SEL) return;
    select_finish<true>(best, bj, amask, rows, ok, oidx, nct, sel, q);
}

// Persistent: one 512-thread workgroup per CU copies the recurrent weights (and the output
// weights when they fit: nrf4 float4 of packed fragments from Wrp) into LDS once, then its 8
// waves walk 256-row tiles; the gate and fc2 A operands become conflict-free ds_read_b128
// instead of L2 round trips.
template <bool RNN, bool SEL>
__global__ void __launch_bounds__(64 * kLdsWaves) __attribute__((amdgpu_waves_per_eu(kLdsWavesPerSimd)))
rnn_agent_lds_kernel(
    const float *__restrict__ X, int64_t xs, int64_t R, int K, const float *__restrict__ Hin, int64_t hs,
    const float4 *__restrict__ W1p, const float *__restrict__ b1, const float4 *__restrict__ Wrp, int64_t nrf4,
    const float *__restrict__ bih, const float *__restrict__ bhh, const float *__restrict__ b2, int nout,
    float *__restrict__ Hout, float *__restrict__ Q, int64_t wr_f4, int64_t w2_lds, SelectArgs sel) {
    extern __shared__ float4 s_w[];
    for (int64_t i = threadIdx.x; i < nrf4; i += blockDim.x) s_w[i] = Wrp[i];
    __syncthreads();
    const float4 *Wih = s_w;
    const float4 *Whh = s_w + (RNN ? kGruX3F4 : 0);
    // W2 staged after the recurrent weights when it fit (w2_lds >= 0), else read through L2
    const float4 *W2 = Wrp + wr_f4;
    const float4 *W2l = s_w + (w2_lds >= 0 ? w2_lds : 0);
    const int64_t ntiles = (R + kLdsWaves * kRowsPerWave - 1) / (kLdsWaves * kRowsPerWave);
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = (tile * kLdsWaves + (threadIdx.x >> 6)) * kRowsPerWave;
        agent_rows<RNN, SEL>(row0, X, xs, R, K, Hin, hs, W1p, b1, Wih, bih, Whh, bhh, W2, b2, nout, Hout, Q, sel, W2l,
                             w2_lds >= 0);
    }
}

// float4 counts of the packed sections: W1, the recurrent layer, W2
static int64_t w1_f4(int K) { return (int64_t)((K + 15) / 16) * 4 * 64; }
static int64_t wr_f4(int use_rnn) { return use_rnn ? 2 * kGruX3F4 : 4 * 4 * 64; }
static int64_t w2_f4(int nout) { return 4 * (int64_t)((nout + 15) / 16) * 64; }

// float4 count of the packed weight buffer: the split-f16 layout (asg_h2.hip) for every shape
// it takes, else the f32 / split-bf16 layout above
int64_t rnn_agent_packed_f4(int K, int nout, int use_rnn) {
    if (h2_ok(K, nout)) return h2_packed_f4(K, nout, use_rnn);
    return w1_f4(K) + wr_f4(use_rnn) + w2_f4(nout);
}

// W_ih / W_hh [3 * 64][64] -> kGruX3F4 x 8 bf16 (gru_x3_idx order, k order gru_x3_k)
__global__ void pack_gru_x3_kernel(const float *W, u32x4v *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= kGruX3F4) return;
    const int lane = i & 63, pl = (i >> 6) % 3, sl = (i / (64 * 3)) & 1, hb = (i / (64 * 3 * 2)) & 3,
              g = i / (64 * 3 * 2 * 4);
    const int row = g * kHid + 16 * hb + (lane & 15), q = lane >> 4;
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = W[(int64_t)row * kHid + gru_x3_k(sl, q, j)];
    u32x4v h, m, l;
    split3(x, h, m, l);
    out[i] = pl == 0 ? h : (pl == 1 ? m : l);
}

// W1^T of the first P columns ([P][64] f32): the one-hot prefix section of the split-f16 pack
__global__ void pack_w1t_kernel(const float *W1, int K, int P, float *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;  // out[a][u] = W1[u][a]
    if (i < P * kHid) out[i] = W1[(int64_t)(i % kHid) * K + i / kHid];
}

hipError_t launch_w1t_pack(const float *W1, int K, int P, float *out, hipStream_t s) {
    if (P > 0) hipLaunchKernelGGL(pack_w1t_kernel, dim3((P * kHid + 255) / 256), dim3(256), 0, s, W1, K, P, out);
    return hipGetLastError();
}

hipError_t launch_rnn_agent_pack(const float *W1, const float *Wih, const float *Whh, const float *W2, int K, int nout,
                                 int use_rnn, float4 *packed, hipStream_t s) {
    if (h2_ok(K, nout)) return launch_h2_pack(W1, Wih, Whh, W2, K, nout, use_rnn, packed, s);
    float4 *p = packed;
    auto one = [&](const float *W, int C, int KK) {
        const int64_t n = (int64_t)((KK + 15) / 16) * ((C + 15) / 16) * 64;
        hipLaunchKernelGGL(pack_weights_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, W, C, KK, p);
        p += n;
    };
    one(W1, kHid, K);
    if (use_rnn) {
        for (const float *W : {Wih, Whh}) {
            hipLaunchKernelGGL(pack_gru_x3_kernel, dim3((kGruX3F4 + 255) / 256), dim3(256), 0, s, W,
                               reinterpret_cast<u32x4v *>(p));
            p += kGruX3F4;
        }
    } else {
        one(Wih, kHid, kHid);
    }
    one(W2, nout, kHid);
    return hipGetLastError();
}

// CUs a stream may run on (hipExtStreamCreateWithCUMask): the persistent grids are sized to
// them, so a CU-masked agent stream leaves the other CUs to a concurrent env-step stream.
int stream_cus(hipStream_t s) {
    int dev = 0, ncu = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    static thread_local hipStream_t last = nullptr;
    static thread_local int last_n = 0;
    if (!s) return ncu;
    if (s == last && last_n > 0) return last_n < ncu ? last_n : ncu;
    uint32_t mask[32] = {0};
    int n = 0;
    if (hipExtStreamGetCUMask(s, 32, mask) == hipSuccess)
        for (int i = 0; i < 32; ++i) n += __builtin_popcount(mask[i]);
    else
        (void)hipGetLastError();
    last = s;
    last_n = n > 0 ? n : ncu;
    return last_n < ncu ? last_n : ncu;
}

// Build-time A/B switch (no runtime environment knobs in the shipped library):
// -DASG_AGENT_ONEHOT=0 disables the split-f16 path's one-hot prefix shortcut (and with it the
// rollout kernel, whose tiles rely on it).
#ifndef ASG_AGENT_ONEHOT
#define ASG_AGENT_ONEHOT 1
#endif
bool onehot_prefix_enabled() { return ASG_AGENT_ONEHOT != 0; }

hipError_t launch_rnn_agent_fwd(const float *X, int64_t xs, int64_t R, int K, const float *Hin, int64_t hs,
                                const float4 *packed, const float *b1, const float *bih, const float *bhh,
                                const float *b2, int nout, int use_rnn, float *Hout, float *Q, const SelectArgs *sel,
                                hipStream_t s) {
    if (h2_ok(K, nout)) return launch_h2_agent(X, xs, R, K, Hin, hs, packed, b1, bih, bhh, b2, nout, use_rnn, Hout, Q,
                                               sel, s);
    const float4 *W1p = packed;
    const float4 *Wrp = W1p + w1_f4(K);
    const SelectArgs sa = sel ? *sel : SelectArgs{};
    // LDS image: the recurrent weights (GRU: 144 KiB, Linear: 16 KiB), then the output weights
    // when they fit beside them (else read through L2)
    constexpr size_t kLdsMax = 160 * 1024;
    const int64_t wr = wr_f4(use_rnn);
    int64_t nrf4 = wr, w2_lds = -1;
    if ((size_t)(nrf4 + w2_f4(nout)) * sizeof(float4) <= kLdsMax) {
        w2_lds = nrf4;
        nrf4 += w2_f4(nout);
    }
    const size_t lds = (size_t)nrf4 * sizeof(float4);
    const int ncu = stream_cus(s);
    const int64_t ntiles = (R + kLdsWaves * kRowsPerWave - 1) / (kLdsWaves * kRowsPerWave);
    const unsigned grid = (unsigned)(ntiles < ncu ? ntiles : ncu);
#define LL_(RNN, SEL)                                                                                              \
    hipLaunchKernelGGL((rnn_agent_lds_kernel<RNN, SEL>), dim3(grid), dim3(64 * kLdsWaves), lds, s, X, xs, R, K, Hin, hs, \
                       W1p, b1, Wrp, nrf4, bih, bhh, b2, nout, Hout, Q, wr, w2_lds, sa)
    if (use_rnn) {
        if (sel) LL_(true, true); else LL_(true, false);
    } else {
        if (sel) LL_(false, true); else LL_(false, false);
    }
#undef LL_
    return hipGetLastError();
}

hipError_t launch_rnn_agent_select(const float *X, int64_t xs, int64_t R, int K, const float *Hin, int64_t hs,
                                   const float4 *packed, const float *b1, const float *bih, const float *bhh,
                                   const float *b2, int nout, int use_rnn, float *Hout, float *Q,
                                   const uint8_t *avail, int64_t a0, int64_t a1, int n, float epsilon, uint64_t seed,
                                   uint32_t counter, int64_t row_base, int64_t *out, int64_t o0, int64_t o1, int *err,
                                   hipStream_t s) {
    const SelectArgs sa{avail, a0, a1, n, epsilon, (uint32_t)seed, (uint32_t)(seed >> 32) ^ 0x5bd1e995u, counter,
                        row_base, out, o0, o1, err};
    return launch_rnn_agent_fwd(X, xs, R, K, Hin, hs, packed, b1, bih, bhh, b2, nout, use_rnn, Hout, Q, &sa, s);
}

}  // namespace asg

// 1: the GRU's products on split-bf16 MFMAs (the only form of the fallback kernel)
extern "C" int asg_rnn_agent_mfma_mode(void) { return 1; }
extern "C" int asg_rnn_agent_mode(int K, int hidden, int n_out, int use_rnn) {
    (void)use_rnn;
    if (hidden != 64) return -1;
    if (asg::h2_ok(K, n_out)) return 4;  // split-f16 (asg_h2.hip), GRU or Linear
    return asg_rnn_agent_mfma_mode();
}
