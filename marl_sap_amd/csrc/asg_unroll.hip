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
constexpr int kWaves = 4;          // waves per workgroup, 16 rows each
constexpr int kFc1G = 4;           // fc1 k-chunks (of 16 inputs) per register buffer
constexpr size_t kFwdLds = 2 * (size_t)kG * kWS * sizeof(float);     // 104,448 B
constexpr size_t kBwdLds = 2 * (size_t)kHid * kWTS * sizeof(float);  // 100,352 B

__device__ __forceinline__ float sigmoid_(float x) { return 1.0f / (1.0f + expf(-x)); }

struct FwdArgs {
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
    const int lane = threadIdx.x & 63, r = lane & 15, qd = lane >> 4;
    const int64_t row0 = ((int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6)) * 16;
    if (row0 >= a.R) return;  // whole wave idle
    const int64_t row = row0 + r;
    const bool ok = row < a.R;
    const int64_t rc = ok ? row : 0;  // rows past R compute row 0 again and store nothing
    const int64_t env = rc / a.n;
    const int64_t ag = rc - env * a.n;
    const float *xrow = a.x + env * a.xs_e + ag * a.xs_a;
    const int K = a.K, nk = (K + 15) / 16, nout = a.nout, nct = (nout + 15) / 16;
    const bool xvec = a.xvec != 0, w1vec = a.w1vec != 0, qvec = (nout & 3) == 0;
    const int64_t plane = (int64_t)a.T1 * a.R * kHid;

    f32x4 h[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) h[t] = a.h0 ? ld4(a.h0 + rc * a.hs + 16 * t + 4 * qd) : f32x4{0.f, 0.f, 0.f, 0.f};

    for (int ts = 0; ts < a.T1; ++ts) {
        const int64_t base = ((int64_t)ts * a.R + rc) * kHid;
        // ---- fc1: x1^T = relu(W1 x^T + b1) ----
        f32x4 x1[4];
        {
            const float *xr = xrow + (int64_t)ts * a.xs_t;
            // the bias is added once, after the products: an accumulator that starts from it is
            // rounded at the bias's magnitude by every MFMA (rows with |W1 x| << |b1|)
            f32x4 acc[4];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
            // two register buffers of kFc1G k-chunks each: one is refilled from L2 / HBM under the
            // MFMAs of the other (a single wave per SIMD has nothing else to hide that latency);
            // chunks past K load nothing (ldk) and are skipped
            f32x4 xa[kFc1G], wa[kFc1G][4], xb[kFc1G], wb[kFc1G][4];
            auto load = [&](int kc0, f32x4(&xv)[kFc1G], f32x4(&w)[kFc1G][4]) {
#pragma unroll
                for (int g = 0; g < kFc1G; ++g) {
                    const int k = 16 * (kc0 + g) + 4 * qd;
                    xv[g] = ldk(xr, k, K, xvec);
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt) w[g][mt] = ldk(a.W1 + (int64_t)(16 * mt + r) * K, k, K, w1vec);
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
                const f32x4 b = ld4(a.b1 + 16 * mt + 4 * qd);
#pragma unroll
                for (int v = 0; v < 4; ++v) x1[mt][v] = fmaxf(acc[mt][v] + b[v], 0.f);
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
        // ---- fc2 one 16-output tile at a time: q^T = W2 h^T + b2 ----
        float *qrow = a.q + ((int64_t)ts * a.R + rc) * nout;
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
            f32x4 acc = {0.f, 0.f, 0.f, 0.f}, b;  // the bias after the products, as in fc1
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
}

struct BwdArgs {
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
    const int lane = threadIdx.x & 63, r = lane & 15, qd = lane >> 4;
    const int64_t row0 = ((int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6)) * 16;
    if (row0 >= a.R) return;
    const int64_t row = row0 + r;
    const bool ok = row < a.R;
    const int64_t rc = ok ? row : 0;
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

// the shape both entries take: the GRU agent at hidden 64
const char *shape_error(int T1, int64_t R, int hidden, int n_out, int use_rnn) {
    if (hidden != 64) return "hidden must be 64";
    if (!use_rnn) return "use_rnn = 0 is not supported (the GRU agent only)";
    if (n_out < 1 || n_out > 512) return "n_out must be in 1..512";
    if (T1 < 1) return "T1 must be >= 1";
    if (R < 1) return "needs at least one agent row";
    return nullptr;
}

}  // namespace
}  // namespace asg

extern "C" int asg_rnn_agent_unroll(const float *x, const int64_t x_strides[3], int T1, int64_t B, int n, int K,
                                    const float *h0, int64_t h_stride, const float *W1, const float *W_ih,
                                    const float *W_hh, const float *W2, const float *b1, const float *b_ih,
                                    const float *b_hh, const float *b2, int hidden, int n_out, int use_rnn, float *q,
                                    float *h_all, float *save, void *hip_stream) {
    using namespace asg;
    const int64_t R = (B > 0 && n > 0) ? B * n : 0;
    if (const char *m = shape_error(T1, R, hidden, n_out, use_rnn))
        return fail((std::string("asg_rnn_agent_unroll: ") + m).c_str());
    if (K < 1) return fail("asg_rnn_agent_unroll: K must be >= 1");
    if (!x || !x_strides || !W1 || !W_ih || !W_hh || !W2 || !b1 || !b_ih || !b_hh || !b2 || !q || !h_all)
        return fail("asg_rnn_agent_unroll: NULL argument");
    if (!al(x, 4) || !al(W1, 4) || !al(q, 16) || !al(b2, 4) || !al(h0, 16) || h_stride % 4 != 0 || h_stride < 0 ||
        !al(W_ih, 16) || !al(W_hh, 16) || !al(W2, 16) || !al(b1, 16) || !al(b_ih, 16) || !al(b_hh, 16) ||
        !al(h_all, 16) || !al(save, 16))
        return fail("asg_rnn_agent_unroll: misaligned pointer (16 B for h0, W_ih, W_hh, W2, b1, b_ih, b_hh, q, h_all, "
                    "save; h_stride % 4 == 0)");
    FwdArgs a;
    a.x = x;
    a.xs_t = x_strides[0];
    a.xs_e = x_strides[1];
    a.xs_a = x_strides[2];
    a.T1 = T1;
    a.R = R;
    a.n = n;
    a.K = K;
    a.h0 = h0;
    a.hs = h_stride;
    a.W1 = W1;
    a.b1 = b1;
    a.Wih = W_ih;
    a.bih = b_ih;
    a.Whh = W_hh;
    a.bhh = b_hh;
    a.W2 = W2;
    a.b2 = b2;
    a.nout = n_out;
    a.q = q;
    a.h_all = h_all;
    a.save = save;
    a.xvec = K % 4 == 0 && al(x, 16) && ((a.xs_t | a.xs_e | a.xs_a) & 3) == 0;
    a.w1vec = K % 4 == 0 && al(W1, 16);
    const unsigned grid = (unsigned)((R + 16 * kWaves - 1) / (16 * kWaves));
    hipLaunchKernelGGL(unroll_fwd_kernel, dim3(grid), dim3(64 * kWaves), kFwdLds, static_cast<hipStream_t>(hip_stream),
                       a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? ASG_OK : hip_fail(e, "asg_rnn_agent_unroll");
}

extern "C" int asg_rnn_agent_unroll_backward(const float *dh_q, const float *dh_last, const float *save,
                                             const float *h_all, const float *h0, int64_t h_stride,
                                             const float *W_ih, const float *W_hh, int T1, int64_t R, int hidden,
                                             int n_out, int use_rnn, float *dgi, float *dgh_n, float *dx1, float *dh0,
                                             void *hip_stream) {
    using namespace asg;
    if (const char *m = shape_error(T1, R, hidden, n_out, use_rnn))
        return fail((std::string("asg_rnn_agent_unroll_backward: ") + m).c_str());
    if (!dh_q || !save || !h_all || !W_ih || !W_hh || !dgi || !dgh_n || !dx1)
        return fail("asg_rnn_agent_unroll_backward: NULL argument");
    if (!al(dh_q, 16) || !al(dh_last, 16) || !al(save, 16) || !al(h_all, 16) || !al(h0, 16) || h_stride % 4 != 0 ||
        h_stride < 0 || !al(W_ih, 4) || !al(W_hh, 4) || !al(dgi, 16) || !al(dgh_n, 16) || !al(dx1, 16) || !al(dh0, 16))
        return fail("asg_rnn_agent_unroll_backward: misaligned pointer (16 B; h_stride % 4 == 0)");
    BwdArgs a;
    a.dhq = dh_q;
    a.dh_last = dh_last;
    a.save = save;
    a.h_all = h_all;
    a.h0 = h0;
    a.hs = h_stride;
    a.Wih = W_ih;
    a.Whh = W_hh;
    a.T1 = T1;
    a.R = R;
    a.dgi = dgi;
    a.dghn = dgh_n;
    a.dx1 = dx1;
    a.dh0 = dh0;
    const unsigned grid = (unsigned)((R + 16 * kWaves - 1) / (16 * kWaves));
    hipLaunchKernelGGL(unroll_bwd_kernel, dim3(grid), dim3(64 * kWaves), kBwdLds, static_cast<hipStream_t>(hip_stream),
                       a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? ASG_OK : hip_fail(e, "asg_rnn_agent_unroll_backward");
}
