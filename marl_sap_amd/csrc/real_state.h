// real_state.h -- what the real-env units share (asg_real.hip: the env's kernels and entry
// points; asg_real_haal.hip: the HAAL selector on the same handle): the device-visible state
// passed to the kernels by value, the typed field stores, the benefit and reward rules, and
// the host-side handle with its error plumbing.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/asg.h"
#include "asg_device.h"
#include "asg_internal.h"

namespace asg {

struct RealState {
    int64_t E;
    int n, m, T, L, N, M;
    double lambda_;
    const double *table;  // [E or 1][T][n][m]
    int64_t table_env_stride;
    const double *prios;    // [m]
    const double *T_trans;  // [m][m]
    int *prev;              // [E][n]
    double *returns;        // [E]
    float *totT;            // [E][m][n] L-summed totals of the current beta rounded to float32, task-major
    int *topA;              // [E][n][M]        each agent's top-M tasks, ties -> lower index
    int *topD;              // [E][n][M + M/2]  its top tasks, ties -> higher index
    int *err;
    int variant;            // asg_real_variant
    double *power;          // [E][n] power states (power / interference variants)
    const int *bands;       // [n] frequency band per satellite (interference)
    const double *nbr;      // [m][m] task neighbour matrix (interference)
    const int64_t *prev0;   // injected reset assignments [count][n] or nullptr (Philox)
    int64_t prev0_env_stride;
    uint64_t seed;
    int64_t env_base;
    uint32_t episode;
    int bids;                     // bids_as_actions: actions are float32 [n][m] bids
    const int64_t *assign;        // bids: LSA(bids row, maximize) assignments [E][n] of this step
    const int32_t *assign_status; // bids: their LSA status [E] (0, ASG_E_LSA_INVALID / _INFEASIBLE)
};

__device__ __forceinline__ void store_real(const asg_field &f, int64_t off, double v) {
    switch (f.dtype) {
        case ASG_F32: reinterpret_cast<float *>(f.ptr)[off] = (float)v; break;
        case ASG_F16: reinterpret_cast<__half *>(f.ptr)[off] = __float2half((float)v); break;
        case ASG_F64: reinterpret_cast<double *>(f.ptr)[off] = v; break;
        default: break;
    }
}
__device__ __forceinline__ void store_int(const asg_field &f, int64_t off, int64_t v) {
    switch (f.dtype) {
        case ASG_I64: reinterpret_cast<int64_t *>(f.ptr)[off] = v; break;
        case ASG_I32: reinterpret_cast<int32_t *>(f.ptr)[off] = (int32_t)v; break;
        case ASG_I16: reinterpret_cast<int16_t *>(f.ptr)[off] = (int16_t)v; break;
        case ASG_BOOL: reinterpret_cast<uint8_t *>(f.ptr)[off] = v != 0; break;
        default: break;
    }
}
__device__ __forceinline__ int64_t load_int(const asg_field &f, int64_t off) {
    switch (f.dtype) {
        case ASG_I64: return reinterpret_cast<const int64_t *>(f.ptr)[off];
        case ASG_I32: return reinterpret_cast<const int32_t *>(f.ptr)[off];
        case ASG_I16: return reinterpret_cast<const int16_t *>(f.ptr)[off];
        default: return 0;
    }
}
__device__ __forceinline__ int64_t foff(const asg_field &f, int64_t b, int64_t t, int64_t d2, int64_t d3) {
    return b * f.stride[0] + t * f.stride[1] + d2 * f.stride[2] + d3 * f.stride[3];
}

// beta value (i, j, l) at time k: table slice * task priority, zero past T
__device__ __forceinline__ double real_beta(const RealState &st, const double *tab, int k, int i, int j, int l) {
    const int kk = k + l;
    const double v = kk < st.T ? tab[((int64_t)kk * st.n + i) * st.m + j] : 0.0;
    return v * st.prios[j];
}

// ---- one step's rewards and power update of one env (block-wide; every thread calls) -----
// The variants' reward rules, shared by the transition kernel and HAAL's sequence values:
//   plain / power  beta_hat[i, a_i, 0] / count(a_i), or the full penalty when beta_hat <= 0
//                  (real_constellation_env.py:145-160); power: 0 for a dead satellite, beta_hat
//                  zeroed below 1e-12 power (real_power_constellation_env.py:150-165, :343-347)
//   interference   beta[i, a_i, 0] * 0.5 ** conflicts / count over applicable agents, minus
//                  lambda on a handover (interference_constellation_env.py:309-353)
// sa [n] this step's tasks, prevp(i) the previous task of agent i, pw [n] power (power
// variants), LDS scnt [m], sapp [n]; rewards into srew [n].
template <class PrevF>
__device__ __forceinline__ void real_step_rewards(const RealState &st, const double *tab, int k, const int *sa,
                                                  PrevF prevp, const double *pw, int *scnt, int *sapp,
                                                  double *srew) {
    const int n = st.n, m = st.m, L = st.L;
    for (int j = threadIdx.x; j < m; j += blockDim.x) scnt[j] = 0;
    __syncthreads();
    if (st.variant == ASG_REAL_INTERFERENCE) {
        // applicable = alive and on a meaningful task; counts over applicable agents only
        for (int i = threadIdx.x; i < n; i += blockDim.x)
            sapp[i] = (pw[i] <= 0 ? 0 : 1) * (real_beta(st, tab, k, i, sa[i], 0) < 1e-12 ? 0 : 1);
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += blockDim.x)
            if (sapp[i]) atomicAdd(&scnt[sa[i]], 1);
    } else {
        for (int i = threadIdx.x; i < n; i += blockDim.x) atomicAdd(&scnt[sa[i]], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int c = sa[i];
        const int pv = prevp(i);
        double r;
        if (st.variant == ASG_REAL_INTERFERENCE) {
            // conflicts = sum over the agents of i's band of nbr[a_i, a_j] * applicable_j - 1
            // (interference_constellation_env.py:327-331), then 0.5 ** conflicts
            double conf = 0.0;
            const int band = st.bands[i];
            for (int a = 0; a < n; ++a)
                if (st.bands[a] == band) conf = conf + st.nbr[(int64_t)c * m + sa[a]] * (double)sapp[a];
            conf = conf - 1.0;
            r = real_beta(st, tab, k, i, c, 0) * pow(0.5, conf);
            if (scnt[c] > 0) r = r / (double)scnt[c];
            if (sapp[i] && pv != c) r = r - st.lambda_;
        } else if (st.variant == ASG_REAL_POWER && !(pw[i] > 0)) {
            r = 0.0;  // dead satellite (real_power_constellation_env.py:161-162)
        } else {
            double bh;
            if (st.variant == ASG_REAL_POWER && pw[i] < 1e-12) {
                bh = 0.0;  // beta_hat zeroed below 1e-12 power (:343-347)
            } else {
                double s = real_beta(st, tab, k, i, c, 0);
                const double b0 = s;
                for (int l = 1; l < L; ++l) s = s + real_beta(st, tab, k, i, c, l);
                const double cond = s > 1e-12 ? 1.0 : 0.0;
                const double pen = st.T_trans[(int64_t)pv * m + c] * cond;
                bh = b0 - st.lambda_ * pen;
            }
            r = bh > 0 ? bh / (double)scnt[c] : bh;
        }
        srew[i] = r;
    }
}

// power update on the pre-step beta (real_power_constellation_env.py:170-178); the caller
// syncs before (every reader of the old power is done)
__device__ __forceinline__ void real_power_update(const RealState &st, const double *tab, int k, const int *sa,
                                                  double *pw) {
    for (int i = threadIdx.x; i < st.n; i += blockDim.x)
        if (pw[i] > 0) {
            if (real_beta(st, tab, k, i, sa[i], 0) > 1e-12) {
                pw[i] -= 0.2;
            } else {
                const double p = pw[i] + 0.1;
                pw[i] = p < 1.0 ? p : 1.0;
            }
        }
}

}  // namespace asg

// ---- host side ---------------------------------------------------------------------------
struct asg_real_handle {
    asg::RealState st{};
    hipStream_t stream = nullptr;
    int device = 0;
    int k = 0;
    bool has_reset = false;
    bool table_ready = false;
    double *table_buf = nullptr;
    void *haal_ws = nullptr;  // HAAL workspace (grown on demand)
    size_t haal_ws_bytes = 0;
    int64_t *bids_assign = nullptr;   // bids_as_actions: [E][n] assignments of the step's LSA
    int32_t *bids_status = nullptr;   // [E] its status
    std::string err;
};

inline int rfail(asg_real_handle *h, int code, const std::string &msg) {
    asg::set_last_error(msg);
    if (h) h->err = msg;
    return code;
}
inline int rhip(asg_real_handle *h, hipError_t e, const char *what) {
    return rfail(h, ASG_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
