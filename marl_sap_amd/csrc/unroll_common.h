// unroll_common.h -- what the learner's sequence kernels share: the GRU agent's unroll
// (asg_unroll.hip) and the Linear agent's / critic's (asg_unroll_mlp.hip).  Device side: the
// wave-to-rows map, the fc1 product pipeline and the fc2 tile loop; host side: the entries'
// shape check, the vector-load rule and the launch.  (asg_ppo.hip takes fail / hip_fail / al.)
#pragma once
#include "asg_agent_common.h"

namespace asg {

constexpr int kWaves = 4;  // waves per workgroup, 16 rows each
constexpr int64_t kMaxSeqRows = (int64_t)0x7fffffff * 16 * kWaves;  // the grid's x dimension

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ void st4(float *p, f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }
// elements k .. k + 3 of a K-long row; vec: K % 4 == 0 and the row is 16-B aligned
__device__ __forceinline__ f32x4 ldk(const float *row, int k, int K, bool vec) {
    if (vec) return k < K ? ld4(row + k) : f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = k + e < K ? row[k + e] : 0.f;
    return v;
}

// The 16 rows of a wave: lane (r, qd) = (lane & 15, lane >> 4) works on row row0 + r.  A wave with
// row0 >= n_rows is idle and returns -- after its workgroup's LDS staging and __syncthreads().
struct WaveRows {
    int lane, r, qd;
    int64_t row0, row;
    bool ok;
    int64_t rc;  // rows past the end compute row 0 again and store nothing (!ok)
    __device__ __forceinline__ explicit WaveRows(int64_t n_rows)
        : lane(threadIdx.x & 63), r(lane & 15), qd(lane >> 4),
          row0(((int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6)) * 16), row(row0 + r), ok(row < n_rows),
          rc(ok ? row : 0) {}
};

// fc1's products W1[:, :K] x^T of a wave's rows as four 16x4 accumulators (output tile mt, C
// layout).  Bias, id column and ReLU are the caller's: the bias is added once, after the
// products -- an accumulator that starts from it is rounded at the bias's magnitude by every
// MFMA (rows with |W1 x| << |b1|).  The accumulators live here, start from zero and are returned by
// value: the callers compile to the registers they had with the stage written out in them.
struct Fc1Acc {
    f32x4 t[4];
};
// G: k-chunks (of 16 inputs) per register buffer; xr: this lane's x row; ldw: the W1 row stride
template <int G>
__device__ __forceinline__ Fc1Acc fc1_products(const float *xr, const float *W1, int64_t ldw, int K, bool xvec,
                                               bool w1vec, int r, int qd) {
    const int nk = (K + 15) / 16;
    Fc1Acc acc;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc.t[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // two register buffers of G k-chunks each: one is refilled from L2 / HBM under the MFMAs of
    // the other (a single wave per SIMD has nothing else to hide that latency); chunks past K
    // load nothing (ldk) and are skipped
    f32x4 xa[G], wa[G][4], xb[G], wb[G][4];
    auto load = [&](int kc0, f32x4(&xv)[G], f32x4(&w)[G][4]) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int k = 16 * (kc0 + g) + 4 * qd;
            xv[g] = ldk(xr, k, K, xvec);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) w[g][mt] = ldk(W1 + (int64_t)(16 * mt + r) * ldw, k, K, w1vec);
        }
        __builtin_amdgcn_sched_barrier(0);  // issue the loads here, not next to their use
    };
    auto mm = [&](int kc0, const f32x4(&xv)[G], const f32x4(&w)[G][4]) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (kc0 + g >= nk) break;  // wave-uniform
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) acc.t[mt] = mfma4(w[g][mt][e], xv[g][e], acc.t[mt]);
        }
    };
    load(0, xa, wa);
    for (int kc = 0; kc < nk; kc += 2 * G) {
        load(kc + G, xb, wb);
        mm(kc, xa, wa);
        load(kc + 2 * G, xa, wa);
        mm(kc + G, xb, wb);
    }
    return acc;
}

// fc2 one 16-output tile at a time: q^T = W2 h^T + b2 of a wave's rows, h as four k-chunk
// fragments, into the lane's q row (stored where ok).  The bias after the products, as in fc1.
__device__ __forceinline__ void fc2_rows(const float *W2, const float *b2, int nout, const f32x4 (&h)[4],
                                         float *qrow, bool ok, int r, int qd) {
    const int nct = (nout + 15) / 16;
    const bool qvec = (nout & 3) == 0;
    // W2 fragments one tile ahead (tiles past n_out load nothing)
    auto load_w2 = [&](int c, f32x4(&w)[4]) {
        const int wr = 16 * c + r;  // W2 row of this lane's A fragment
#pragma unroll
        for (int t = 0; t < 4; ++t)
            w[t] = wr < nout ? ld4(W2 + (int64_t)wr * kHid + 16 * t + 4 * qd) : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    f32x4 wn[4];
    load_w2(0, wn);
    for (int c = 0; c < nct; ++c) {
        const int j0 = 16 * c + 4 * qd;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f}, b;
#pragma unroll
        for (int v = 0; v < 4; ++v) b[v] = j0 + v < nout ? b2[j0 + v] : 0.f;
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

// ---- host side -----------------------------------------------------------------------------------
inline int fail(const char *msg) {
    set_last_error(msg);
    return ASG_E_INVALID_ARG;
}
inline int fail(const char *who, const char *msg) { return fail((std::string(who) + ": " + msg).c_str()); }
inline int hip_fail(hipError_t e, const char *what) {
    set_last_error(std::string(what) + ": " + hipGetErrorString(e));
    return ASG_E_HIP;
}
inline bool al(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// The shape the sequence entries take (an entry without one of the arguments passes 1), T1 * R
// rows in all; NULL where it is fine.
inline const char *seq_shape_error(int hidden, int use_rnn, int n_out, int T1, int64_t R, int K) {
    if (hidden != 64) return "hidden must be 64";
    if (!use_rnn) return "use_rnn = 0 is not supported (the GRU agent only)";
    if (n_out < 1 || n_out > 512) return "n_out must be in 1..512";
    if (T1 < 1) return "T1 must be >= 1";
    if (R < 1) return "needs at least one agent row";
    if (K < 1) return "K must be >= 1";
    if (R > kMaxSeqRows / T1) return "too many rows";
    return nullptr;
}

// ldk's vec for rows of K floats starting at p + (any sum of the strides): 16-B loads are aligned
inline int vec_rows(const void *p, int K, int64_t s0, int64_t s1 = 0, int64_t s2 = 0) {
    return K % 4 == 0 && al(p, 16) && ((s0 | s1 | s2) & 3) == 0;
}

// one wave per 16 rows, kWaves per workgroup
template <class Args>
int launch_rows(const char *who, void (*kernel)(Args), int64_t rows, size_t lds, void *hip_stream, const Args &a) {
    const unsigned grid = (unsigned)((rows + 16 * kWaves - 1) / (16 * kWaves));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * kWaves), lds, static_cast<hipStream_t>(hip_stream), a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? ASG_OK : hip_fail(e, who);
}

}  // namespace asg
