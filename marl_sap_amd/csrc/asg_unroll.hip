// asg_unroll.hip -- the GRU RNNAgent unrolled over time for the learner (gfx950, f32 MFMA).
//
// The SAP Q-learner runs the agent over all T1 = T + 1 rows of a sampled batch (reference
// learners/sap_q_learner.py:69-84: T1 calls of RNNAgent.forward) and backpropagates through
// that chain.  In PyTorch this is, per row, fc1, ReLU, two GRU GEMMs, the GRU cell and fc2 --
// and as many again backwards.  Here the whole chain is ONE launch each way:
//
//   unroll_fwd_kernel : for t = 0..T1-1: x1 = relu(W1 x_t + b1); h = GRUCell(x1, h);
//                       q_t = W2 h + b2.  A wave owns 16 agent rows and keeps their h in
//                       registers over all T1 steps; rows never interact, so there is no
//                       grid-wide synchronisation.  Optionally saves x1, r, z, n and
//                       gh_n = W_hn h + b_hn per step for the backward pass.
//   unroll_bwd_kernel : the sequential core of backpropagation through time, t = T1-1..0,
//                       with dh carried in registers (the recurrence in asg.h).  Emits the
//                       per-step gate gradients; the parameter gradients are plain GEMMs
//                       over the flattened T1 * R rows and stay in PyTorch.
//
// Arithmetic: v_mfma_f32_16x16x4_f32 in the transposed formulation of asg_agent.hip
// (out^T = W . act^T): lane (r, q) = (lane & 15, lane >> 4) holds act[row r][16 t + 4 q + v]
// as one float4, which is both the C layout of output tile t and the B operand of k-chunk
// t of the next layer.  Exact fp32 products, fp32 accumulation in a fixed order: no atomics,
// so two runs give identical bits.  The weights are read in their torch layouts (no packed
// copy to keep in step with the optimiser): W_ih and W_hh (48 KiB each) are staged in LDS
// once per workgroup -- row-padded forward, transposed backward -- W1 and W2 come through L2.
#include "unroll_common.h"

namespace asg {
namespace {

constexpr int kG = 3 * kHid;       // gate rows of W_ih / W_hh
constexpr int kWS = kHid + 4;      // LDS row stride (floats) of W [192][64], forward
constexpr int kWTS = kG + 4;       // LDS row stride (floats) of W^T [64][192], backward
constexpr int kFc1G = 4;           // fc1 k-chunks (of 16 inputs) per register buffer
constexpr size_t kFwdLds = 2 * (size_t)kG * kWS * sizeof(float);     // 104,448 B
constexpr size_t kBwdLds = 2 * (size_t)kHid * kWTS * sizeof(float);  // 100,352 B

__device__ __forceinline__ float sigmoid_(float x) { return 1.0f / (1.0f + expf(-x)); }

struct FwdArgs {  // the entry fills it by position
    const float *x;
    int64_t xs_t, xs_e, xs_a;
    int T1;
    int64_t R;
    int n, K;
    const float *h0;
    int64_t hs;
    const float *W1, *b1, *Wih, *bih, *Whh, *bhh, *W2, *b2;
    int nout;
    float *q, *h_all, *save;
    int xvec, w1vec;
};

__global__ void __launch_bounds__(64 * kWaves) unroll_fwd_kernel(FwdArgs a) {
    extern __shared__ float s_w[];
    float *sWih = s_w, *sWhh = s_w + kG * kWS;
    for (int i = threadIdx.x; i < kG * (kHid / 4); i += blockDim.x) {
        const int row = i >> 4, c = (i & 15) * 4;
        st4(sWih + row * kWS + c, ld4(a.Wih + row * kHid + c));
        st4(sWhh + row * kWS + c, ld4(a.Whh + row * kHid + c));
    }
    __syncthreads();
    const WaveRows wv(a.R);
    if (wv.row0 >= a.R) return;  // whole wave idle
    const int r = wv.r, qd = wv.qd;
    const bool ok = wv.ok;
    const int64_t rc = wv.rc;
    const int64_t env = rc / a.n;
    const int64_t ag = rc - env * a.n;
    const float *xrow = a.x + env * a.xs_e + ag * a.xs_a;
    const int64_t plane = (int64_t)a.T1 * a.R * kHid;

    f32x4 h[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) h[t] = a.h0 ? ld4(a.h0 + rc * a.hs + 16 * t + 4 * qd) : f32x4{0.f, 0.f, 0.f, 0.f};

    for (int ts = 0; ts < a.T1; ++ts) {
        const int64_t base = ((int64_t)ts * a.R + rc) * kHid;
        // ---- fc1: x1^T = relu(W1 x^T + b1) ----
        f32x4 x1[4];
        {
            const Fc1Acc acc = fc1_products<kFc1G>(xrow + (int64_t)ts * a.xs_t, a.W1, a.K, a.K, a.xvec != 0,
                                                   a.w1vec != 0, r, qd);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const f32x4 b = ld4(a.b1 + 16 * mt + 4 * qd);
#pragma unroll
                for (int v = 0; v < 4; ++v) x1[mt][v] = fmaxf(acc.t[mt][v] + b[v], 0.f);
            }
        }
        // ---- GRUCell: r and z sum the input and hidden products in one accumulator; the gate
        // accumulators start from their biases (the gates' absolute floor covers that rounding),
        // gh_n = W_hn h + b_hn, a plane of its own, gets its bias after the products ----
        f32x4 hn[4];
#pragma unroll
        for (int hb = 0; hb < 4; ++hb) {
            const int u = 16 * hb + 4 * qd;
            f32x4 gr = ld4(a.bih + u) + ld4(a.bhh + u);
            f32x4 gz = ld4(a.bih + kHid + u) + ld4(a.bhh + kHid + u);
            f32x4 gni = ld4(a.bih + 2 * kHid + u);
            f32x4 gnh = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kc = 0; kc < 4; ++kc) {
                // keep the LDS reads of later chunks from being hoisted here (register pressure)
                __builtin_amdgcn_sched_barrier(0);
                f32x4 wi[3], wh[3];
#pragma unroll
                for (int g = 0; g < 3; ++g) {
                    const int off = (g * kHid + 16 * hb + r) * kWS + 16 * kc + 4 * qd;
                    wi[g] = ld4(sWih + off);
                    wh[g] = ld4(sWhh + off);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    gr = mfma4(wi[0][e], x1[kc][e], gr);
                    gz = mfma4(wi[1][e], x1[kc][e], gz);
                    gni = mfma4(wi[2][e], x1[kc][e], gni);
                    gnh = mfma4(wh[2][e], h[kc][e], gnh);
                    gr = mfma4(wh[0][e], h[kc][e], gr);
                    gz = mfma4(wh[1][e], h[kc][e], gz);
                }
            }
            gnh = gnh + ld4(a.bhh + 2 * kHid + u);
            f32x4 rg, zg, ng;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                rg[v] = sigmoid_(gr[v]);
                zg[v] = sigmoid_(gz[v]);
                ng[v] = tanhf(gni[v] + rg[v] * gnh[v]);
                hn[hb][v] = ng[v] + zg[v] * (h[hb][v] - ng[v]);
            }
            if (ok) {
                st4(a.h_all + base + u, hn[hb]);
                if (a.save) {
                    st4(a.save + base + u, x1[hb]);
                    st4(a.save + plane + base + u, rg);
                    st4(a.save + 2 * plane + base + u, zg);
                    st4(a.save + 3 * plane + base + u, ng);
                    st4(a.save + 4 * plane + base + u, gnh);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) h[t] = hn[t];
        fc2_rows(a.W2, a.b2, a.nout, h, a.q + ((int64_t)ts * a.R + rc) * a.nout, ok, r, qd);
    }
}

struct BwdArgs {  // the entry fills it by position
    const float *dhq, *dh_last, *save, *h_all, *h0;
    int64_t hs;
    const float *Wih, *Whh;
    int T1;
    int64_t R;
    float *dgi, *dghn, *dx1, *dh0;
};

__global__ void __launch_bounds__(64 * kWaves) unroll_bwd_kernel(BwdArgs a) {
    extern __shared__ float s_w[];
    // W^T [64][192]: the A operand of (d @ W)^T = W^T d^T is then a float4 of one LDS row
    float *sTih = s_w, *sThh = s_w + kHid * kWTS;
    for (int i = threadIdx.x; i < kG * kHid; i += blockDim.x) {
        const int k = i >> 6, j = i & 63;
        sTih[j * kWTS + k] = a.Wih[i];
        sThh[j * kWTS + k] = a.Whh[i];
    }
    __syncthreads();
    const WaveRows wv(a.R);
    if (wv.row0 >= a.R) return;  // whole wave idle
    const int r = wv.r, qd = wv.qd;
    const bool ok = wv.ok;
    const int64_t rc = wv.rc;
    const int64_t plane = (int64_t)a.T1 * a.R * kHid;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    f32x4 dh[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) dh[t] = a.dh_last ? ld4(a.dh_last + rc * kHid + 16 * t + 4 * qd) : zero;

    for (int ts = a.T1 - 1; ts >= 0; --ts) {
        const int64_t rowt = (int64_t)ts * a.R + rc;
        const int64_t base = rowt * kHid;
        f32x4 di[12], dg[4], zz[4];  // dgi (k-chunks g * 4 + hb), the n part of dgh, z
#pragma unroll
        for (int hb = 0; hb < 4; ++hb) {
            const int u = 16 * hb + 4 * qd;
            const f32x4 rg = ld4(a.save + plane + base + u), zg = ld4(a.save + 2 * plane + base + u);
            const f32x4 ng = ld4(a.save + 3 * plane + base + u), gh = ld4(a.save + 4 * plane + base + u);
            const f32x4 hp = ts > 0 ? ld4(a.h_all + base - a.R * kHid + u) : (a.h0 ? ld4(a.h0 + rc * a.hs + u) : zero);
            const f32x4 d = dh[hb] + ld4(a.dhq + base + u);
            dh[hb] = d;
            f32x4 drp, dzp, dnp, dgn;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const float dn = d[v] * (1.0f - zg[v]);
                const float dz = d[v] * (hp[v] - ng[v]);
                dnp[v] = dn * (1.0f - ng[v] * ng[v]);
                drp[v] = dnp[v] * gh[v] * rg[v] * (1.0f - rg[v]);
                dzp[v] = dz * zg[v] * (1.0f - zg[v]);
                dgn[v] = dnp[v] * rg[v];
            }
            di[hb] = drp;
            di[4 + hb] = dzp;
            di[8 + hb] = dnp;
            dg[hb] = dgn;
            zz[hb] = zg;
            if (ok) {
                float *gi = a.dgi + rowt * kG + u;
                st4(gi, drp);
                st4(gi + kHid, dzp);
                st4(gi + 2 * kHid, dnp);
                st4(a.dghn + base + u, dgn);
            }
        }
        // ---- dx1 = (dgi @ W_ih) . (x1 > 0) ----
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            f32x4 ag[3] = {zero, zero, zero};  // one accumulator per gate: three independent chains
#pragma unroll
            for (int kc = 0; kc < 12; ++kc) {
                if ((kc & 3) == 0) __builtin_amdgcn_sched_barrier(0);  // bound the LDS reads in flight
                const f32x4 w = ld4(sTih + (16 * mt + r) * kWTS + 16 * kc + 4 * qd);
#pragma unroll
                for (int e = 0; e < 4; ++e) ag[kc >> 2] = mfma4(w[e], di[kc][e], ag[kc >> 2]);
            }
            f32x4 acc = (ag[0] + ag[1]) + ag[2];
            const int u = 16 * mt + 4 * qd;
            const f32x4 x1 = ld4(a.save + base + u);
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[v] = x1[v] > 0.f ? acc[v] : 0.f;
            if (ok) st4(a.dx1 + base + u, acc);
        }
        // ---- dh = dh . z + dgh @ W_hh ----
        f32x4 nd[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            // one accumulator per gate, started from zero and summed at the end: adding the
            // 192 small products one by one onto dh . z would round each at dh's magnitude
            f32x4 acc[3] = {zero, zero, zero};
#pragma unroll
            for (int kc = 0; kc < 12; ++kc) {
                if ((kc & 3) == 0) __builtin_amdgcn_sched_barrier(0);
                const f32x4 w = ld4(sThh + (16 * mt + r) * kWTS + 16 * kc + 4 * qd);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    acc[kc >> 2] = mfma4(w[e], kc < 8 ? di[kc][e] : dg[kc - 8][e], acc[kc >> 2]);
            }
            nd[mt] = dh[mt] * zz[mt] + ((acc[0] + acc[1]) + acc[2]);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) dh[t] = nd[t];
    }
    if (a.dh0 && ok) {
#pragma unroll
        for (int t = 0; t < 4; ++t) st4(a.dh0 + rc * kHid + 16 * t + 4 * qd, dh[t]);
    }
}

}  // namespace
}  // namespace asg

extern "C" int asg_rnn_agent_unroll(const float *x, const int64_t x_strides[3], int T1, int64_t B, int n, int K,
                                    const float *h0, int64_t h_stride, const float *W1, const float *W_ih,
                                    const float *W_hh, const float *W2, const float *b1, const float *b_ih,
                                    const float *b_hh, const float *b2, int hidden, int n_out, int use_rnn, float *q,
                                    float *h_all, float *save, void *hip_stream) {
    using namespace asg;
    const char *who = "asg_rnn_agent_unroll";
    const int64_t R = (B > 0 && n > 0) ? B * n : 0;
    if (const char *m = seq_shape_error(hidden, use_rnn, n_out, T1, R, K)) return fail(who, m);
    if (!x || !x_strides || !W1 || !W_ih || !W_hh || !W2 || !b1 || !b_ih || !b_hh || !b2 || !q || !h_all)
        return fail(who, "NULL argument");
    if (!al(x, 4) || !al(W1, 4) || !al(q, 16) || !al(b2, 4) || !al(h0, 16) || h_stride % 4 != 0 || h_stride < 0 ||
        !al(W_ih, 16) || !al(W_hh, 16) || !al(W2, 16) || !al(b1, 16) || !al(b_ih, 16) || !al(b_hh, 16) ||
        !al(h_all, 16) || !al(save, 16))
        return fail(who, "misaligned pointer (16 B for h0, W_ih, W_hh, W2, b1, b_ih, b_hh, q, h_all, save; "
                         "h_stride % 4 == 0)");
    const int64_t *xs = x_strides;
    const FwdArgs a = {x, xs[0], xs[1], xs[2], T1, R, n, K, h0, h_stride, W1, b1, W_ih, b_ih, W_hh, b_hh, W2, b2,
                       n_out, q, h_all, save, vec_rows(x, K, xs[0], xs[1], xs[2]), vec_rows(W1, K, K)};
    return launch_rows(who, unroll_fwd_kernel, R, kFwdLds, hip_stream, a);
}

extern "C" int asg_rnn_agent_unroll_backward(const float *dh_q, const float *dh_last, const float *save,
                                             const float *h_all, const float *h0, int64_t h_stride,
                                             const float *W_ih, const float *W_hh, int T1, int64_t R, int hidden,
                                             int n_out, int use_rnn, float *dgi, float *dgh_n, float *dx1, float *dh0,
                                             void *hip_stream) {
    using namespace asg;
    const char *who = "asg_rnn_agent_unroll_backward";
    if (const char *m = seq_shape_error(hidden, use_rnn, n_out, T1, R, 1)) return fail(who, m);
    if (!dh_q || !save || !h_all || !W_ih || !W_hh || !dgi || !dgh_n || !dx1)
        return fail(who, "NULL argument");
    if (!al(dh_q, 16) || !al(dh_last, 16) || !al(save, 16) || !al(h_all, 16) || !al(h0, 16) || h_stride % 4 != 0 ||
        h_stride < 0 || !al(W_ih, 4) || !al(W_hh, 4) || !al(dgi, 16) || !al(dgh_n, 16) || !al(dx1, 16) || !al(dh0, 16))
        return fail(who, "misaligned pointer (16 B; h_stride % 4 == 0)");
    const BwdArgs a = {dh_q, dh_last, save, h_all, h0, h_stride, W_ih, W_hh, T1, R, dgi, dgh_n, dx1, dh0};
    return launch_rows(who, unroll_bwd_kernel, R, kBwdLds, hip_stream, a);
}
