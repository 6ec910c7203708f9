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
constexpr int kFc1G = 2;       // fc1 k-chunks (of 16 inputs) per register buffer

struct MlpFwdArgs {  // the entry fills it by position
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
    const WaveRows wv(a.N);
    if (wv.row0 >= a.N) return;  // whole wave idle
    const int r = wv.r, qd = wv.qd;
    const bool ok = wv.ok;
    const int64_t rc = wv.rc;
    // the flattened row is (t, env, agent) in the outputs' [T1][R] order
    const int64_t ts = rc / a.R;
    const int64_t rr = rc - ts * a.R;
    const int64_t env = rr / a.n;
    const int64_t ag = rr - env * a.n;
    const float *xr = a.x + ts * a.xs_t + env * a.xs_e + ag * a.xs_a;
    const int K = a.K;
    const int64_t base = rc * kHid;
    const int64_t ldw = kIds ? (int64_t)K + a.n : (int64_t)K;  // W1 row stride

    // ---- fc1: x1^T = relu(W1 x^T + b1) ----
    f32x4 x1[4];
    {
        // the bias (kIds: and the id column) is added once, after the products
        const Fc1Acc acc = fc1_products<kFc1G>(xr, a.W1, ldw, K, a.xvec != 0, a.w1vec != 0, r, qd);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            f32x4 b = ld4(a.b1 + 16 * mt + 4 * qd);
            if constexpr (kIds) {
                const float *wid = a.W1 + K + ag;  // column K + agent of every W1 row
#pragma unroll
                for (int v = 0; v < 4; ++v) b[v] += wid[(int64_t)(16 * mt + 4 * qd + v) * ldw];
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) x1[mt][v] = fmaxf(acc.t[mt][v] + b[v], 0.f);
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
    fc2_rows(a.W2, a.b2, a.nout, h, a.q + rc * a.nout, ok, r, qd);
}

struct MlpBwdArgs {  // the entry fills it by position
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
    const WaveRows wv(a.N);
    if (wv.row0 >= a.N) return;  // whole wave idle
    const int r = wv.r, qd = wv.qd;
    const bool ok = wv.ok;
    const int64_t base = wv.rc * kHid;
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

template <bool kIds>
int mlp_unroll(const char *who, const float *x, const int64_t x_strides[3], int T1, int64_t B, int n, int K,
               const float *W1, const float *W_r, const float *W2, const float *b1, const float *b_r,
               const float *b2, int hidden, int n_out, float *q, float *h_all, float *x1_save, void *hip_stream) {
    const int64_t R = (B > 0 && n > 0) ? B * n : 0;
    if (const char *m = seq_shape_error(hidden, 1, n_out, T1, R, K)) return fail(who, m);
    if (!x || !x_strides || !W1 || !W_r || !W2 || !b1 || !b_r || !b2 || !q || !h_all)
        return fail(who, "NULL argument");
    if (!al(x, 4) || !al(W1, 4) || !al(b2, 4) || !al(W_r, 16) || !al(W2, 16) || !al(b1, 16) || !al(b_r, 16) ||
        !al(q, 16) || !al(h_all, 16) || !al(x1_save, 16))
        return fail(who, "misaligned pointer (16 B for W_r, W2, b1, b_r, q, h_all, x1_save)");
    const int64_t *xs = x_strides, N = (int64_t)T1 * R;
    // W1's rows: the first K entries of a row of K (with the id block: K + n) floats
    const MlpFwdArgs a = {x, xs[0], xs[1], xs[2], R, N, n, K, W1, b1, W_r, b_r, W2, b2, n_out, q, h_all, x1_save,
                          vec_rows(x, K, xs[0], xs[1], xs[2]), vec_rows(W1, K, kIds ? K + n : K)};
    return launch_rows(who, mlp_fwd_kernel<kIds>, N, 0, hip_stream, a);
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
    const char *who = "asg_mlp_agent_unroll_backward";
    if (const char *m = seq_shape_error(hidden, 1, 1, 1, N, 1)) return fail(who, m);
    if (!dh_q || !h_all || !x1_save || !W_r || !dh || !dx1) return fail(who, "NULL argument");
    if (!al(dh_q, 16) || !al(h_all, 16) || !al(x1_save, 16) || !al(W_r, 4) || !al(dh, 16) || !al(dx1, 16))
        return fail(who, "misaligned pointer (16 B)");
    const MlpBwdArgs a = {dh_q, h_all, x1_save, W_r, N, dh, dx1};
    return launch_rows(who, mlp_bwd_kernel, N, 0, hip_stream, a);
}
