// asg_lsa.hip -- batched scipy-exact linear sum assignment, beta_hat and the fused HAA
// selector (gfx950).  One wave64 per problem; the working cost matrix sits in LDS when
// it fits (48 KiB budget per wave), otherwise it is read in place from global memory
// (L2-resident for the row sweeps); float32 problems of at most 64 columns stay in registers
// (lsa_reg64.h).  The runner's per-step selectors are asg_sap.hip.
// Reference call sites: sap_selectors.py:32,90 (SAP selectors on Q-values),
// non_rl_selectors.py:36-47 (HAA: beta_hat + LSA), mock_constellation_env.py:228-274.
#include <stdlib.h>

#include <type_traits>

#include "asg_device.h"
#include "asg_internal.h"
#include "lsa_reg64.h"
#include "lsa_wave.h"

namespace asg {

constexpr size_t kLdsCostBudget = 48 * 1024;

// working matrix read in place: transposed when nr0 > nc0, negated for maximize
template <typename IT>
struct GlobalCost {
    static constexpr bool kInMemory = true;
    const IT *C;
    int64_t rs, cs;
    bool tr, neg;
    __device__ double operator()(int i, int j) const {
        const double x = (double)(tr ? C[(int64_t)j * rs + (int64_t)i * cs] : C[(int64_t)i * rs + (int64_t)j * cs]);
        return neg ? -x : x;
    }
};

template <typename IT>
__device__ int lsa_check_wave(const IT *C, int64_t rs, int64_t cs, int nr0, int nc0, bool maximize) {
    const int lane = threadIdx.x & (kWave - 1);
    int bad = 0;
    for (int idx = lane; idx < nr0 * nc0; idx += kWave) {
        const int r = idx / nc0, c = idx - r * nc0;
        double x = (double)C[r * rs + c * cs];
        if (maximize) x = -x;
        bad |= (x != x) || (x == -__builtin_inf());
    }
    return wave_or_i32(bad) ? ASG_E_LSA_INVALID : ASG_OK;
}

// Solve with the smallest columns-per-lane that fits, then hand the register-resident
// assignment to `emit(col4row)` (a generic lambda taking int (&)[CPL]).
template <int CPL, class Acc, class Emit>
__device__ int solve_emit_cpl(const Acc &acc, int nr, int nc, Emit &emit) {
    int c4r[CPL];
    const int status = lsa_solve_wave<CPL>(acc, nr, nc, c4r);
    if (status == ASG_OK) emit(c4r);
    return status;
}

// columns per lane for a working matrix of nc columns (one kernel instantiation each,
// so the register budget of a 64-column problem is not that of a 1024-column one)
static int cpl_for(int nc) { return nc <= 64 ? 1 : nc <= 128 ? 2 : nc <= 256 ? 4 : nc <= 512 ? 8 : 16; }

#define ASG_DISPATCH_CPL(cpl, LAUNCH) \
    switch (cpl) {                    \
        case 1: LAUNCH(1); break;     \
        case 2: LAUNCH(2); break;     \
        case 4: LAUNCH(4); break;     \
        case 8: LAUNCH(8); break;     \
        default: LAUNCH(16); break;   \
    }

// The kernel instance a shape runs on, cpl | storage << 8 (asg_lsa_instance / asg_haa_instance /
// asg_bids_instance report it; the launchers below switch on nothing else).  Shapes are the
// entry points' own (validated there).
static int instance_code(int cpl, int storage) { return cpl | storage << 8; }

int lsa_instance(int dtype, int nr0, int nc0) {
    const int nr = nc0 < nr0 ? nc0 : nr0, nc = nc0 < nr0 ? nr0 : nc0;  // working orientation
    const size_t elem = dtype == ASG_F32 ? sizeof(float) : sizeof(double);
    const size_t cost_bytes = ((elem * (size_t)nr * nc + 15) / 16) * 16;
    if (dtype == ASG_F32 && nc <= 64) return instance_code(1, ASG_LSA_REGISTERS);
    return instance_code(cpl_for(nc), cost_bytes <= kLdsCostBudget ? ASG_LSA_LDS : ASG_LSA_GLOBAL);
}

int haa_instance(int n, int m) {
    const size_t cost = ((sizeof(float) * (size_t)n * m + 15) / 16) * 16;
    if (m <= 64) return instance_code(1, ASG_LSA_REGISTERS);
    return instance_code(cpl_for(m), cost <= kLdsCostBudget ? ASG_LSA_LDS : ASG_LSA_GLOBAL);
}

// LDS carve: [cost (optional)][mark: nr0 ints]
template <int CPL, typename IT, typename CT, bool LDS_COST>
__global__ void __launch_bounds__(64) lsa_batched_kernel(const IT *C, int64_t s0, int64_t s1, int64_t s2, int nr0,
                                                         int nc0, int maximize, int64_t *row_out, int64_t *col_out,
                                                         int32_t *status_out) {
    extern __shared__ double s_lsa[];
    const int64_t b = blockIdx.x;
    const IT *Cb = C + b * s0;
    const bool tr = nc0 < nr0;
    const int nr = tr ? nc0 : nr0, nc = tr ? nr0 : nc0;
    const int k = nr;
    char *p = reinterpret_cast<char *>(s_lsa);
    CT *cost = reinterpret_cast<CT *>(p);
    if (LDS_COST) p += ((sizeof(CT) * (size_t)nr * nc + 15) / 16) * 16;
    int *mark = reinterpret_cast<int *>(p);
    int64_t *ro = row_out ? row_out + b * k : nullptr;
    int64_t *co = col_out ? col_out + b * k : nullptr;
    auto emit = [&](const auto &c4r) { lsa_emit_wave(c4r, nr0, nc0, mark, ro, co, nullptr); };
    int status;
    if (LDS_COST) {
        status = lsa_stage_wave<IT, CT>(Cb, s1, s2, nr0, nc0, maximize != 0, cost);
        if (status == ASG_OK) status = solve_emit_cpl<CPL>(DenseCost<CT>{cost, nc}, nr, nc, emit);
    } else {
        status = lsa_check_wave<IT>(Cb, s1, s2, nr0, nc0, maximize != 0);
        if (status == ASG_OK)
            status = solve_emit_cpl<CPL>(GlobalCost<IT>{Cb, s1, s2, tr, maximize != 0}, nr, nc, emit);
    }
    const int lane = threadIdx.x;
    // (written out in both LSA kernels: a shared helper renumbered the registers of all 20 instances)
    if (status != ASG_OK) {
        for (int r = lane; r < k; r += kWave) {
            if (ro) ro[r] = -1;
            if (co) co[r] = -1;
        }
    }
    if (lane == 0 && status_out) status_out[b] = status;
}

static size_t lsa_scratch_bytes(int nr0) { return sizeof(int) * nr0 + 64; }

// float32 problems up to 64 x 64 (working orientation): the working matrix lives in the
// wave's registers (RegCostF32), so residency is set by registers alone (no LDS)
__global__ void __launch_bounds__(64 * kLsaWpb) __attribute__((amdgpu_waves_per_eu(kLsaRegWaves)))
lsa_reg_kernel(const float *C, int64_t s0, int64_t s1, int64_t s2, int nr0, int nc0, int maximize, int64_t *row_out,
               int64_t *col_out, int32_t *status_out, int64_t B) {
    __shared__ int s_mark[kLsaWpb][64];
    const int64_t b = lsa_reg_problem();
    if (b >= B) return;
    int *mark = s_mark[threadIdx.x >> 6];
    const bool tr = nc0 < nr0;
    const int nr = tr ? nc0 : nr0, nc = tr ? nr0 : nc0;
    const int k = nr;
    int64_t *ro = row_out ? row_out + b * k : nullptr;
    int64_t *co = col_out ? col_out + b * k : nullptr;
    RegCostF32 rc;
    int status = lsa_stage_regs<float>(C + b * s0, s1, s2, nr0, nc0, maximize != 0, rc);
    if (status == ASG_OK) {
        int c4r[1];
        status = lsa_solve_reg64(rc, nr, nc, c4r);
        if (status == ASG_OK) lsa_emit_wave(c4r, nr0, nc0, mark, ro, co, nullptr);
    }
    const int lane = threadIdx.x & (kWave - 1);
    // (written out in both LSA kernels: a shared helper renumbered the registers of all 20 instances)
    if (status != ASG_OK) {
        for (int r = lane; r < k; r += kWave) {
            if (ro) ro[r] = -1;
            if (co) co[r] = -1;
        }
    }
    if (lane == 0 && status_out) status_out[b] = status;
}

template <typename IT, typename CT>
static hipError_t launch_lsa_t(const IT *C, const int64_t st[3], int64_t B, int nr0, int nc0, int maximize,
                               int64_t *row_out, int64_t *col_out, int32_t *status_out, hipStream_t s) {
    const int nr = nc0 < nr0 ? nc0 : nr0, nc = nc0 < nr0 ? nr0 : nc0;
    const size_t cost_bytes = ((sizeof(CT) * (size_t)nr * nc + 15) / 16) * 16;
    const size_t scratch = lsa_scratch_bytes(nr0);
    const int inst = lsa_instance(std::is_same<IT, float>::value ? ASG_F32 : ASG_F64, nr0, nc0);
    const int cpl = inst & 0xff, storage = inst >> 8;
    if (storage == ASG_LSA_REGISTERS) {
        hipLaunchKernelGGL(lsa_reg_kernel, lsa_reg_grid(B), dim3(64 * kLsaWpb), 0, s, reinterpret_cast<const float *>(C),
                           st[0], st[1], st[2], nr0, nc0, maximize, row_out, col_out, status_out, B);
    } else if (storage == ASG_LSA_LDS) {
#define L_(CPL)                                                                                                   \
    hipLaunchKernelGGL((lsa_batched_kernel<CPL, IT, CT, true>), dim3(B), dim3(64), cost_bytes + scratch, s, C, \
                       st[0], st[1], st[2], nr0, nc0, maximize, row_out, col_out, status_out)
        ASG_DISPATCH_CPL(cpl, L_)
#undef L_
    } else {
#define L_(CPL)                                                                                                 \
    hipLaunchKernelGGL((lsa_batched_kernel<CPL, IT, CT, false>), dim3(B), dim3(64), scratch, s, C, st[0], st[1], \
                       st[2], nr0, nc0, maximize, row_out, col_out, status_out)
        ASG_DISPATCH_CPL(cpl, L_)
#undef L_
    }
    return hipGetLastError();
}

hipError_t launch_lsa_batched(const void *C, int dtype, const int64_t strides[3], int64_t B, int nr, int nc,
                              int maximize, int64_t *row_out, int64_t *col_out, int32_t *status_out,
                              hipStream_t s) {
    if (dtype == ASG_F32)
        return launch_lsa_t<float, float>(static_cast<const float *>(C), strides, B, nr, nc, maximize, row_out,
                                          col_out, status_out, s);
    return launch_lsa_t<double, double>(static_cast<const double *>(C), strides, B, nr, nc, maximize, row_out,
                                        col_out, status_out, s);
}

// ------------------------------------------------------------------------------------
// beta_hat = beta - lambda * T_trans[prev_i, j] * (beta > 1e-12)   (mock :250-270)
// ------------------------------------------------------------------------------------
template <typename BT>
__global__ void beta_hat_kernel(const BT *beta, int64_t b0, int64_t b1, int64_t b2, const int64_t *prev, int64_t p0,
                                int64_t p1, int64_t B, int n, int m, const double *T_trans, double lambda_,
                                double *out) {
    const int64_t total = B * n * m;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int j = (int)(idx % m);
        const int64_t bi = idx / m;
        const int i = (int)(bi % n);
        const int64_t b = bi / n;
        const double x = (double)beta[b * b0 + i * b1 + j * b2];
        const int64_t p = prev[b * p0 + i * p1];
        const double tt = T_trans ? T_trans[p * m + j] : (j == p ? 0.0 : 1.0);
        out[idx] = x - lambda_ * (tt * (x > 1e-12 ? 1.0 : 0.0));
    }
}

hipError_t launch_beta_hat(const void *beta, int dtype, const int64_t bs[3], const int64_t *prev,
                           const int64_t ps[2], int64_t B, int n, int m, const double *T_trans, double lambda_,
                           double *out, hipStream_t s) {
    const int64_t total = B * n * m;
    const int64_t blocks = total == 0 ? 1 : (total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192;
    if (dtype == ASG_F32)
        hipLaunchKernelGGL(beta_hat_kernel<float>, dim3(blocks), dim3(256), 0, s, static_cast<const float *>(beta),
                           bs[0], bs[1], bs[2], prev, ps[0], ps[1], B, n, m, T_trans, lambda_, out);
    else
        hipLaunchKernelGGL(beta_hat_kernel<double>, dim3(blocks), dim3(256), 0, s,
                           static_cast<const double *>(beta), bs[0], bs[1], bs[2], prev, ps[0], ps[1], B, n, m,
                           T_trans, lambda_, out);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// HAASelector (non_rl_selectors.py:19-50): col = LSA(beta_hat(beta, prev), maximize)[1]
// The working matrix -beta_hat is formed on the fly from the f32 beta staged in LDS, so
// a 64x64 problem needs 16 KiB of LDS instead of 32.
// ------------------------------------------------------------------------------------
struct HaaCost {
    static constexpr bool kInMemory = true;
    const float *beta;  // [n][m] in LDS (rs = m, cs = 1) or in place in global memory
    int64_t rs, cs;
    const int *prev;    // LDS [n]
    const double *T_trans;
    double lambda_;
    int m;
    __device__ double operator()(int i, int j) const {
        const double x = (double)beta[i * rs + j * cs];
        const int p = prev[i];
        const double tt = T_trans ? T_trans[(int64_t)p * m + j] : (j == p ? 0.0 : 1.0);
        return -(x - lambda_ * (tt * (x > 1e-12 ? 1.0 : 0.0)));
    }
};

template <int CPL, bool STAGE>
__global__ void __launch_bounds__(64) haa_select_kernel(const float *beta, int64_t b0, int64_t b1, int64_t b2,
                                                        const int64_t *prev, int64_t p0, int64_t p1, int n, int m,
                                                        const double *T_trans, double lambda_, float *col_out,
                                                        int32_t *status_out) {
    extern __shared__ double s_lsa[];
    const int64_t b = blockIdx.x;
    const int lane = threadIdx.x;
    char *p = reinterpret_cast<char *>(s_lsa);
    float *sb = reinterpret_cast<float *>(p);
    if (STAGE) p += ((sizeof(float) * (size_t)n * m + 15) / 16) * 16;
    int *sp = reinterpret_cast<int *>(p);
    int bad = 0;
    for (int idx = lane; idx < n * m; idx += kWave) {
        const int i = idx / m, j = idx - i * m;
        const float x = beta[b * b0 + i * b1 + j * b2];
        if (STAGE) sb[idx] = x;
        bad |= (x != x) || (x == __builtin_inff());  // -(+inf) = -inf is invalid
    }
    for (int i = lane; i < n; i += kWave) sp[i] = (int)prev[b * p0 + i * p1];
    wave_sync();
    float *co = col_out + b * n;
    auto emit = [&](const auto &c4r) { lsa_emit_wave(c4r, n, m, nullptr, nullptr, nullptr, co); };
    int status = wave_or_i32(bad) ? ASG_E_LSA_INVALID : ASG_OK;
    if (status == ASG_OK) {
        const HaaCost acc = STAGE ? HaaCost{sb, m, 1, sp, T_trans, lambda_, m}
                                  : HaaCost{beta + b * b0, b1, b2, sp, T_trans, lambda_, m};
        status = solve_emit_cpl<CPL>(acc, n, m, emit);
    }
    // (written out in both HAA kernels: a shared helper changed haa_reg_kernel's instructions)
    if (status != ASG_OK)
        for (int i = lane; i < n; i += kWave) co[i] = -1.0f;
    if (lane == 0 && status_out) status_out[b] = status;
}

// m <= 64: the beta column of the lane's task and prev_assigns of the lane's agent stay
// in registers; -beta_hat(i, j) is formed per relaxed entry
struct HaaRegCost {
    static constexpr bool kInMemory = false;  // T_trans reads are guarded below
    RegCostF32 beta;  // beta[i][lane], not sign-flipped
    int prev;         // prev_assigns[lane]
    const double *T_trans;
    double lambda_;
    int m;
    __device__ double operator()(int i, int j) const {
        const double x = (double)beta.get(i);
        const int p = __builtin_amdgcn_readlane(prev, i);
        const double tt = T_trans ? (j < m ? T_trans[(int64_t)p * m + j] : 0.0) : (j == p ? 0.0 : 1.0);
        return -(x - lambda_ * (tt * (x > 1e-12 ? 1.0 : 0.0)));
    }
    __device__ double col(int i) const { return (*this)(i, (int)(threadIdx.x & 63)); }
};

__global__ void __launch_bounds__(64 * kLsaWpb) __attribute__((amdgpu_waves_per_eu(kLsaRegWaves)))
haa_reg_kernel(const float *beta, int64_t b0, int64_t b1, int64_t b2, const int64_t *prev, int64_t p0, int64_t p1,
               int n, int m, const double *T_trans, double lambda_, float *col_out, int32_t *status_out, int64_t B) {
    const int64_t b = lsa_reg_problem();
    if (b >= B) return;
    const int lane = threadIdx.x & (kWave - 1);
    HaaRegCost acc;
    // beta_hat is not negated here (the accessor does it): stage with maximize = false,
    // which also rejects NaN; +inf beta (-inf cost) is rejected below
    int status = lsa_stage_regs<float>(beta + b * b0, b1, b2, n, m, false, acc.beta);
    int bad = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i)
        bad |= (acc.beta.lo[i] == __builtin_inff()) | (acc.beta.hi[i] == __builtin_inff());
    if (wave_or_i32(bad)) status = ASG_E_LSA_INVALID;
    acc.prev = lane < n ? (int)prev[b * p0 + lane * p1] : 0;
    acc.T_trans = T_trans;
    acc.lambda_ = lambda_;
    acc.m = m;
    float *co = col_out + b * n;
    if (status == ASG_OK) {
        int c4r[1];
        status = lsa_solve_reg64(acc, n, m, c4r);
        if (status == ASG_OK) lsa_emit_wave(c4r, n, m, nullptr, nullptr, nullptr, co);
    }
    // (written out in both HAA kernels: a shared helper changed haa_reg_kernel's instructions)
    if (status != ASG_OK)
        for (int i = lane; i < n; i += kWave) co[i] = -1.0f;
    if (lane == 0 && status_out) status_out[b] = status;
}

hipError_t launch_haa_select(const float *beta, const int64_t bs[3], const int64_t *prev, const int64_t ps[2],
                             int64_t B, int n, int m, const double *T_trans, double lambda_, float *col_out,
                             int32_t *status_out, hipStream_t s) {
    const size_t cost = ((sizeof(float) * (size_t)n * m + 15) / 16) * 16;
    const size_t rest = ((sizeof(int) * n + 15) / 16) * 16 + 64;
    const int inst = haa_instance(n, m);
    const int cpl = inst & 0xff, storage = inst >> 8;
    if (storage == ASG_LSA_REGISTERS) {
        hipLaunchKernelGGL(haa_reg_kernel, lsa_reg_grid(B), dim3(64 * kLsaWpb), 0, s, beta, bs[0], bs[1], bs[2], prev,
                           ps[0], ps[1], n, m, T_trans, lambda_, col_out, status_out, B);
    } else if (storage == ASG_LSA_LDS) {
#define L_(CPL)                                                                                                 \
    hipLaunchKernelGGL((haa_select_kernel<CPL, true>), dim3(B), dim3(64), cost + rest, s, beta, bs[0], bs[1], bs[2], \
                       prev, ps[0], ps[1], n, m, T_trans, lambda_, col_out, status_out)
        ASG_DISPATCH_CPL(cpl, L_)
#undef L_
    } else {
#define L_(CPL)                                                                                                  \
    hipLaunchKernelGGL((haa_select_kernel<CPL, false>), dim3(B), dim3(64), rest, s, beta, bs[0], bs[1], bs[2], prev, \
                       ps[0], ps[1], n, m, T_trans, lambda_, col_out, status_out)
        ASG_DISPATCH_CPL(cpl, L_)
#undef L_
    }
    return hipGetLastError();
}

}  // namespace asg
