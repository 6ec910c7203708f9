// asg_unroll_mlp.hip -- the Linear RNNAgent (use_rnn = False: fc1 -> ReLU -> Linear(64, 64) ->
// ReLU -> fc2, the agent of mock_constellation_reda.yaml and mock_constellation_iql.yaml) over
// a whole sampled batch for the learners (gfx950, f32 MFMA).
//
// The agent has no recurrence, so the T1 = T + 1 rows of a batch are T1 * R independent agent
// rows (R = B * n).  Where the GRU kernels (asg_unroll.hip) can only spread R rows over the
// chip and walk t inside the wave, these spread the flattened N = T1 * R rows: a wave owns 16
// of them, a workgroup 64, and a tile may straddle a time boundary -- every lane derives its
// own (t, env, agent).
//
//   mlp_fwd_kernel : x1 = relu(W1 x + b1); h = relu(W_r x1 + b_r); q = W2 h + b2 per row.
//                    Writes q, h (h_all) and, for the backward pass, x1.  A second instance
//                    (asg_mlp_agent_unroll_ids) is the reference's ACCritic, whose input is
//                    [obs, eye(n)]: W1 is [64][K + n] and the one-hot block a column gather.
//   mlp_bwd_kernel : dh = dh_q . (h > 0); dx1 = (dh @ W_r) . (x1 > 0) per row.  The parameter
//                    gradients are plain GEMMs over the N rows and stay in PyTorch.
//
// Arithmetic as in asg_unroll.hip: v_mfma_f32_16x16x4_f32 in the transposed formulation
// (out^T = W . act^T): lane (r, q) = (lane & 15, lane >> 4) holds act[row r][16 t + 4 q + v] as
// one float4, both the C layout of output tile t and the B operand of k-chunk t of the next
// layer.  Exact fp32 products, fp32 accumulation in a fixed order, no atomics: two runs give
// identical bits.  The weights are read in their torch layouts (no packed copy to keep in step
// with the optimiser): W_r (16 KiB) is staged in LDS once per workgroup -- row-padded forward,
// transposed backward -- W1 and W2 come through L2.
#include "unroll_common.h"

namespace asg {
namespace {

constexpr int kWS = kHid + 4;  // LDS row stride (floats) of W_r [64][64] and of its transpose
constexpr int kWaves = 4;      // waves per workgroup, 16 rows each
constexpr int kFc1G = 2;       // fc1 k-chunks (of 16 inputs) per register buffer

struct MlpFwdArgs {
    const float *x;
    int64_t xs_t, xs_e, xs_a;
    int64_t R, N;
    int n, K;
    const float *W1, *b1, *Wr, *br, *W2, *b2;
    int nout;
    float *q, *h_all, *x1_save;
    int xvec, w1vec;
};

// kIds: the reference critics' agent-id inputs (modules/critics/ac.py:32-43) -- W1 is [64][K + n]
// and the one-hot block of row (t, env, agent) is the column gather W1[:, K + agent], added with
// the bias after the K observation inputs are accumulated; the concatenation is never read.
template <bool kIds>
__global__ void __launch_bounds__(64 * kWaves) mlp_fwd_kernel(MlpFwdArgs a) {
    __shared__ float sWr[kHid * kWS];
    for (int i = threadIdx.x; i < kHid * (kHid / 4); i += blockDim.x) {
        const int row = i >> 4, c = (i & 15) * 4;
        st4(sWr + row * kWS + c, ld4(a.Wr + row * kHid + c));
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, r = lane & 15, qd = lane >> 4;
    const int64_t row0 = ((int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6)) * 16;
    if (row0 >= a.N) return;  // whole wave idle
    const int64_t row = row0 + r;
    const bool ok = row < a.N;
    const int64_t rc = ok ? row : 0;  // rows past N compute row 0 again and store nothing
    // the flattened row is (t, env, agent) in the outputs' [T1][R] order
    const int64_t ts = rc / a.R;
    const int64_t rr = rc - ts * a.R;
    const int64_t env = rr / a.n;
    const int64_t ag = rr - env * a.n;
    const float *xr = a.x + ts * a.xs_t + env * a.xs_e + ag * a.xs_a;
    const int K = a.K, nk = (K + 15) / 16, nout = a.nout, nct = (nout + 15) / 16;
    const bool xvec = a.xvec != 0, w1vec = a.w1vec != 0, qvec = (nout & 3) == 0;
    const int64_t base = rc * kHid;
    const int64_t ldw = kIds ? (int64_t)K + a.n : (int64_t)K;  // W1 row stride

    // ---- fc1: x1^T = relu(W1 x^T + b1) ----
    f32x4 x1[4];
    {
        // the bias (kIds: and the id column) is added once, after the products: an accumulator
        // that starts from it is rounded at the bias's magnitude by every MFMA
        f32x4 acc[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        // two register buffers of kFc1G k-chunks each: one is refilled from L2 / HBM under the
        // MFMAs of the other; chunks past K load nothing (ldk) and are skipped
        f32x4 xa[kFc1G], wa[kFc1G][4], xb[kFc1G], wb[kFc1G][4];
        auto load = [&](int kc0, f32x4(&xv)[kFc1G], f32x4(&w)[kFc1G][4]) {
#pragma unroll
            for (int g = 0; g < kFc1G; ++g) {
                const int k = 16 * (kc0 + g) + 4 * qd;
                xv[g] = ldk(xr, k, K, xvec);
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) w[g][mt] = ldk(a.W1 + (int64_t)(16 * mt + r) * ldw, k, K, w1vec);
            }
            __builtin_amdgcn_sched_barrier(0);  // issue the loads here, not next to their use
        };
        auto mm = [&](int kc0, const f32x4(&xv)[kFc1G], const f32x4(&w)[kFc1G][4]) {
#pragma unroll
            for (int g = 0; g < kFc1G; ++g) {
                if (kc0 + g >= nk) break;  // wave-uniform
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt) acc[mt] = mfma4(w[g][mt][e], xv[g][e], acc[mt]);
            }
        };
        load(0, xa, wa);
        for (int kc = 0; kc < nk; kc += 2 * kFc1G) {
            load(kc + kFc1G, xb, wb);
            mm(kc, xa, wa);
            load(kc + 2 * kFc1G, xa, wa);
            mm(kc + kFc1G, xb, wb);
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            f32x4 b = ld4(a.b1 + 16 * mt + 4 * qd);
            if constexpr (kIds) {
                const float *wid = a.W1 + K + ag;  // column K + agent of every W1 row
#pragma unroll
                for (int v = 0; v < 4; ++v) b[v] += wid[(int64_t)(16 * mt + 4 * qd + v) * ldw];
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) x1[mt][v] = fmaxf(acc[mt][v] + b[v], 0.f);
        }
    }
    // ---- the middle layer: h^T = relu(W_r x1^T + b_r) ----
    f32x4 h[4];
#pragma unroll
    for (int hb = 0; hb < 4; ++hb) {
        const int u = 16 * hb + 4 * qd;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) {
            const f32x4 w = ld4(sWr + (16 * hb + r) * kWS + 16 * kc + 4 * qd);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = mfma4(w[e], x1[kc][e], acc);
        }
        const f32x4 b = ld4(a.br + u);  // after the products, as in fc1
#pragma unroll
        for (int v = 0; v < 4; ++v) h[hb][v] = fmaxf(acc[v] + b[v], 0.f);
        if (ok) {
            st4(a.h_all + base + u, h[hb]);
            if (a.x1_save) st4(a.x1_save + base + u, x1[hb]);
        }
    }
    // ---- fc2 one 16-output tile at a time: q^T = W2 h^T + b2 ----
    float *qrow = a.q + rc * nout;
    // W2 fragments one tile ahead (tiles past n_out load nothing)
    auto load_w2 = [&](int c, f32x4(&w)[4]) {
        const int wr = 16 * c + r;  // W2 row of this lane's A fragment
#pragma unroll
        for (int t = 0; t < 4; ++t)
            w[t] = wr < nout ? ld4(a.W2 + (int64_t)wr * kHid + 16 * t + 4 * qd) : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    f32x4 wn[4];
    load_w2(0, wn);
    for (int c = 0; c < nct; ++c) {
        const int j0 = 16 * c + 4 * qd;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f}, b;
#pragma unroll
        for (int v = 0; v < 4; ++v) b[v] = j0 + v < nout ? a.b2[j0 + v] : 0.f;
        f32x4 w[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) w[t] = wn[t];
        load_w2(c + 1, wn);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = mfma4(w[t][e], h[t][e], acc);
        acc = acc + b;
        if (ok) {
            if (qvec && j0 + 3 < nout) {
                st4(qrow + j0, acc);
            } else {
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    if (j0 + v < nout) qrow[j0 + v] = acc[v];
            }
        }
    }
}

struct MlpBwdArgs {
    const float *dhq, *h_all, *x1_save, *Wr;
    int64_t N;
    float *dh, *dx1;
};

__global__ void __launch_bounds__(64 * kWaves) mlp_bwd_kernel(MlpBwdArgs a) {
    // W_r^T [64][64]: the A operand of (dh @ W_r)^T = W_r^T dh^T is then a float4 of one LDS row
    __shared__ float sT[kHid * kWS];
    for (int i = threadIdx.x; i < kHid * kHid; i += blockDim.x) {
        const int k = i >> 6, j = i & 63;
        sT[j * kWS + k] = a.Wr[i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, r = lane & 15, qd = lane >> 4;
    const int64_t row0 = ((int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6)) * 16;
    if (row0 >= a.N) return;
    const int64_t row = row0 + r;
    const bool ok = row < a.N;
    const int64_t base = (ok ? row : 0) * kHid;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    f32x4 dh[4], x1[4];
#pragma unroll
    for (int hb = 0; hb < 4; ++hb) {
        const int u = 16 * hb + 4 * qd;
        const f32x4 d = ld4(a.dhq + base + u), hv = ld4(a.h_all + base + u);
        x1[hb] = ld4(a.x1_save + base + u);
#pragma unroll
        for (int v = 0; v < 4; ++v) dh[hb][v] = hv[v] > 0.f ? d[v] : 0.f;
        if (ok) st4(a.dh + base + u, dh[hb]);
    }
    // ---- dx1 = (dh @ W_r) . (x1 > 0) ----
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        f32x4 acc = zero;
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) {
            const f32x4 w = ld4(sT + (16 * mt + r) * kWS + 16 * kc + 4 * qd);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = mfma4(w[e], dh[kc][e], acc);
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[v] = x1[mt][v] > 0.f ? acc[v] : 0.f;
        if (ok) st4(a.dx1 + base + 16 * mt + 4 * qd, acc);
    }
}

constexpr int64_t kMaxRows = (int64_t)0x7fffffff * 16 * kWaves;  // the grid's x dimension

}  // namespace
}  // namespace asg

namespace asg {
namespace {

template <bool kIds>
int mlp_unroll(const char *who, const float *x, const int64_t x_strides[3], int T1, int64_t B, int n, int K,
               const float *W1, const float *W_r, const float *W2, const float *b1, const float *b_r,
               const float *b2, int hidden, int n_out, float *q, float *h_all, float *x1_save, void *hip_stream) {
    const std::string w(who);
    const int64_t R = (B > 0 && n > 0) ? B * n : 0;
    if (hidden != 64) return fail((w + ": hidden must be 64").c_str());
    if (n_out < 1 || n_out > 512) return fail((w + ": n_out must be in 1..512").c_str());
    if (T1 < 1) return fail((w + ": T1 must be >= 1").c_str());
    if (R < 1) return fail((w + ": needs at least one agent row").c_str());
    if (K < 1) return fail((w + ": K must be >= 1").c_str());
    if (R > kMaxRows / T1) return fail((w + ": too many rows").c_str());
    if (!x || !x_strides || !W1 || !W_r || !W2 || !b1 || !b_r || !b2 || !q || !h_all)
        return fail((w + ": NULL argument").c_str());
    if (!al(x, 4) || !al(W1, 4) || !al(b2, 4) || !al(W_r, 16) || !al(W2, 16) || !al(b1, 16) || !al(b_r, 16) ||
        !al(q, 16) || !al(h_all, 16) || !al(x1_save, 16))
        return fail((w + ": misaligned pointer (16 B for W_r, W2, b1, b_r, q, h_all, x1_save)").c_str());
    MlpFwdArgs a;
    a.x = x;
    a.xs_t = x_strides[0];
    a.xs_e = x_strides[1];
    a.xs_a = x_strides[2];
    a.R = R;
    a.N = (int64_t)T1 * R;
    a.n = n;
    a.K = K;
    a.W1 = W1;
    a.b1 = b1;
    a.Wr = W_r;
    a.br = b_r;
    a.W2 = W2;
    a.b2 = b2;
    a.nout = n_out;
    a.q = q;
    a.h_all = h_all;
    a.x1_save = x1_save;
    a.xvec = K % 4 == 0 && al(x, 16) && ((a.xs_t | a.xs_e | a.xs_a) & 3) == 0;
    // 16-B loads of a W1 row's first K entries: the row stride (K, or K + n with the id block)
    // and K are both multiples of 4
    a.w1vec = K % 4 == 0 && (!kIds || (K + n) % 4 == 0) && al(W1, 16);
    const unsigned grid = (unsigned)((a.N + 16 * kWaves - 1) / (16 * kWaves));
    hipLaunchKernelGGL(mlp_fwd_kernel<kIds>, dim3(grid), dim3(64 * kWaves), 0, static_cast<hipStream_t>(hip_stream),
                       a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? ASG_OK : hip_fail(e, who);
}

}  // namespace
}  // namespace asg

extern "C" int asg_mlp_agent_unroll(const float *x, const int64_t x_strides[3], int T1, int64_t B, int n, int K,
                                    const float *W1, const float *W_r, const float *W2, const float *b1,
                                    const float *b_r, const float *b2, int hidden, int n_out, float *q, float *h_all,
                                    float *x1_save, void *hip_stream) {
    return asg::mlp_unroll<false>("asg_mlp_agent_unroll", x, x_strides, T1, B, n, K, W1, W_r, W2, b1, b_r, b2, hidden,
                                  n_out, q, h_all, x1_save, hip_stream);
}

extern "C" int asg_mlp_agent_unroll_ids(const float *x, const int64_t x_strides[3], int T1, int64_t B, int n, int K,
                                        const float *W1, const float *W_r, const float *W2, const float *b1,
                                        const float *b_r, const float *b2, int hidden, int n_out, float *q,
                                        float *h_all, float *x1_save, void *hip_stream) {
    return asg::mlp_unroll<true>("asg_mlp_agent_unroll_ids", x, x_strides, T1, B, n, K, W1, W_r, W2, b1, b_r, b2,
                                 hidden, n_out, q, h_all, x1_save, hip_stream);
}

extern "C" int asg_mlp_agent_unroll_backward(const float *dh_q, const float *h_all, const float *x1_save,
                                             const float *W_r, int64_t N, int hidden, float *dh, float *dx1,
                                             void *hip_stream) {
    using namespace asg;
    if (hidden != 64) return fail("asg_mlp_agent_unroll_backward: hidden must be 64");
    if (N < 1) return fail("asg_mlp_agent_unroll_backward: needs at least one agent row");
    if (N > kMaxRows) return fail("asg_mlp_agent_unroll_backward: too many rows");
    if (!dh_q || !h_all || !x1_save || !W_r || !dh || !dx1)
        return fail("asg_mlp_agent_unroll_backward: NULL argument");
    if (!al(dh_q, 16) || !al(h_all, 16) || !al(x1_save, 16) || !al(W_r, 4) || !al(dh, 16) || !al(dx1, 16))
        return fail("asg_mlp_agent_unroll_backward: misaligned pointer (16 B)");
    MlpBwdArgs a;
    a.dhq = dh_q;
    a.h_all = h_all;
    a.x1_save = x1_save;
    a.Wr = W_r;
    a.N = N;
    a.dh = dh;
    a.dx1 = dx1;
    const unsigned grid = (unsigned)((N + 16 * kWaves - 1) / (16 * kWaves));
    hipLaunchKernelGGL(mlp_bwd_kernel, dim3(grid), dim3(64 * kWaves), 0, static_cast<hipStream_t>(hip_stream), a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? ASG_OK : hip_fail(e, "asg_mlp_agent_unroll_backward");
}
