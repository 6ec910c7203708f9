// asg_env.hip -- batched MockConstellationEnv kernels for gfx950.
//
// One workgroup advances one env.  The EpisodeBatch tensors (PyTorch-owned, any
// strides) are written in place: the next pre-transition row (obs, beta, avail_actions,
// prev_assigns, filled) and this step's post-transition row (rewards, terminated,
// actions_onehot).  Benefits come from one of three sources (env_src.h):
//   * BumpSrc  (Philox, native throughput mode): bump parameters are regenerated on the
//     fly from a counter-based key each step -- no benefit table in HBM at all;
//   * ParSrc   (MT19937 compat): the reset's recorded draws [E][m][n] (float64 values) and
//     their float32 table [E][T][n][m] (the rows);
//   * TableSrc (injected): float64 table [E][T][n][m].
// The MT19937 streams themselves (seeding, the reset's draws and table, the skip) are
// asg_env_mt.hip.
// Reference: envs/mock_constellation_env.py:94-175 (reset / step / pre-transition data),
// runners/episode_runner.py:60-100 and runners/parallel_runner.py:113-200 (which rows
// get which fields), components/transforms.py:12-22 (OneHot, int64).
#include "asg_device.h"
#include "asg_internal.h"
#include "env_src.h"
#include "lsa_reg64.h"
#include "lsa_wave.h"

namespace asg {

// ------------------------------------------------------------------------------------
// reset: prev_assigns = first n of a random permutation of m; row ts pre-transition data
// ------------------------------------------------------------------------------------
template <int VEC, class Src>
__global__ void __launch_bounds__(256) reset_kernel(Src src, asg_batch_view bv, EnvState st, int ts,
                                                    bool philox_perm) {
    extern __shared__ int s_dyn[];
    const int64_t e = blockIdx.x;
    const int n = st.n, m = st.m;
    int *perm = s_dyn;                                   // [m]
    float *s_scale = reinterpret_cast<float *>(s_dyn + m);  // [m]
    src.fill_scale(e, s_scale);
    if (philox_perm) {  // MT19937: mt_reset_kernel has drawn st.prev
        philox_perm_lds(perm, st, e);
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += blockDim.x) st.prev[e * n + i] = perm[i];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        if (bv.prev_assigns.ptr)
            *fptr<int64_t>(bv.prev_assigns, e, ts, i, 0) =
                (st.quirks & ASG_QUIRK_PREV_ASSIGNS_ZERO) ? 0 : st.prev[e * n + i];
    }
    if (threadIdx.x == 0) {
        st.returns[e] = 0.0;
        if (bv.filled.ptr) *fptr<int64_t>(bv.filled, e, ts, 0, 0) = 1;
    }
    write_pre_row<VEC>(src.bind(e, s_scale), bv, e, ts, 0, n, m, st.T, st.L, nullptr, -1);
}

// ------------------------------------------------------------------------------------
// bids_as_actions: assignments = LSA(bids, maximize)[1]  (mock :121-122), one wave per
// env, ahead of the step kernel; result in st.assign [E][n]
// ------------------------------------------------------------------------------------
template <int CPL>
__global__ void __launch_bounds__(64) bids_assign_kernel(asg_batch_view bv, EnvState st, int ts) {
    extern __shared__ double s_lsa[];
    const int64_t e = blockIdx.x;
    const int n = st.n, m = st.m;
    float *cost = reinterpret_cast<float *>(s_lsa);  // [n][m] (m > 64)
    const float *bids = fptr<float>(bv.actions, e, ts, 0, 0);
    int c4r[CPL];
    int status;
    if constexpr (CPL == 1) {  // m <= 64: the working matrix stays in registers
        RegCostF32 rc;
        status = lsa_stage_regs<float>(bids, bv.actions.stride[2], bv.actions.stride[3], n, m, true, rc);
        if (status == ASG_OK) status = lsa_solve_reg64(rc, n, m, c4r);
    } else {
        status = lsa_stage_wave<float, float>(bids, bv.actions.stride[2], bv.actions.stride[3], n, m, true, cost);
        if (status == ASG_OK) status = lsa_solve_wave<CPL>(DenseCost<float>{cost, m}, n, m, c4r);
    }
    if (status == ASG_OK) {
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int i = (int)threadIdx.x + kWave * c;
            if (i < n) st.assign[e * n + i] = c4r[c];
        }
    }
    if (status != ASG_OK) {
        for (int i = threadIdx.x; i < n; i += kWave) st.assign[e * n + i] = -1;
        if (threadIdx.x == 0) atomicCAS(st.err, 0, status);
    }
}

// ------------------------------------------------------------------------------------
// step (mock_constellation_env.py:116-162 plus the runner's batch updates)
// ------------------------------------------------------------------------------------
template <int VEC, class Src, bool BIDS>
__global__ void __launch_bounds__(256) step_kernel(Src src, asg_batch_view bv, EnvState st, int ts, int k) {
    extern __shared__ int s_dyn[];
    const int64_t e = blockIdx.x;
    const int n = st.n, m = st.m, T = st.T, L = st.L;
    int *s_act = s_dyn;                                                          // [n]
    int *s_cnt = s_act + n;                                                      // [m]
    float *s_scale = reinterpret_cast<float *>(s_cnt + m);                       // [m]
    double *s_rew = reinterpret_cast<double *>(s_scale + m + ((n + 2 * m) & 1));  // [n], 8-aligned
    __shared__ int s_err;

    if (threadIdx.x == 0) s_err = 0;
    for (int j = threadIdx.x; j < m; j += blockDim.x) s_cnt[j] = 0;
    src.fill_scale(e, s_scale);
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        int a;
        if (BIDS) {
            a = st.assign[e * n + i];
        } else {
            const int64_t a64 = *fptr<int64_t>(bv.actions, e, ts, i, 0);
            a = (a64 >= 0 && a64 < m) ? (int)a64 : -1;
            if (a < 0) s_err = ASG_E_ACTION_RANGE;
        }
        a = a < 0 ? 0 : a;
        s_act[i] = a;
        atomicAdd(&s_cnt[a], 1);
    }
    __syncthreads();
    const auto env = src.bind(e, s_scale);
    for (int i = threadIdx.x; i < n; i += blockDim.x)
        transition_reward(env, bv, st, e, ts, k, i, s_act[i], s_cnt, st.prev[e * n + i], s_rew);
    // next pre-transition row (mock :141-160) + this row's OneHot of the actions
    write_pre_row<VEC>(env, bv, e, ts + 1, k + 1, n, m, T, L, s_act, BIDS ? -1 : ts);
    __syncthreads();
    if (threadIdx.x == 0) {
        transition_tail(bv, st, e, ts, k, s_rew, st.returns[e]);
        if (s_err) atomicCAS(st.err, 0, s_err);
    }
}

// ------------------------------------------------------------------------------------
// uniform random actions (BASELINE config 2 random policy)
// ------------------------------------------------------------------------------------
__global__ void random_actions_kernel(asg_batch_view bv, EnvState st, int ts, int k) {
    const int64_t e = blockIdx.x;
    const EnvKey key = env_key(st.seed, st.env_base + e);
    for (int i = threadIdx.x; i < st.n; i += blockDim.x) {
        *fptr<int64_t>(bv.actions, e, ts, i, 0) = (int64_t)philox_action(key, st.episode, i, k, st.m);
    }
}

// ------------------------------------------------------------------------------------
// the random policy's whole episode in one launch (asg_random_rollout): for steps k0 ..
// k0 + steps - 1 of every env, the uniform actions of asg_random_actions (same Philox
// counters) and the transition of step_kernel, optionally after the reset of reset_kernel
// (same Fisher-Yates draws) -- one workgroup per env keeps prev_assigns, the actions, the
// task scales and the return in LDS across the steps; results are those of asg_reset +
// T x (asg_random_actions + asg_step), bit for bit.  Reference: mock_constellation_env.py:
// 94-162 (reset / step) driven by episode_runner.py:60-100 with a uniform policy.
// ------------------------------------------------------------------------------------
template <int VEC, class Src>
__global__ void __launch_bounds__(256) random_rollout_kernel(Src src, asg_batch_view bv, EnvState st, int ts0,
                                                             int k0, int steps, int reset) {
    extern __shared__ int s_dyn[];
    const int64_t e = blockIdx.x;
    const int n = st.n, m = st.m, T = st.T, L = st.L;
    int *s_act = s_dyn;                                                          // [n]
    int *s_cnt = s_act + n;                                                      // [m] (the reset's permutation)
    float *s_scale = reinterpret_cast<float *>(s_cnt + m);                       // [m]
    int *s_prev = reinterpret_cast<int *>(s_scale + m);                          // [n]
    double *s_rew = reinterpret_cast<double *>(s_prev + n + ((2 * n + 2 * m) & 1));  // [n], 8-aligned
    __shared__ double s_ret;
    src.fill_scale(e, s_scale);
    const auto env = src.bind(e, s_scale);
    const EnvKey key = env_key(st.seed, st.env_base + e);
    if (reset) {
        philox_perm_lds(s_cnt, st, e);
        if (threadIdx.x == 0) {
            s_ret = 0.0;
            if (bv.filled.ptr) *fptr<int64_t>(bv.filled, e, ts0, 0, 0) = 1;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            s_prev[i] = s_cnt[i];
            if (bv.prev_assigns.ptr)
                *fptr<int64_t>(bv.prev_assigns, e, ts0, i, 0) = (st.quirks & ASG_QUIRK_PREV_ASSIGNS_ZERO) ? 0 : s_cnt[i];
        }
        write_pre_row<VEC>(env, bv, e, ts0, 0, n, m, T, L, nullptr, -1);
    } else {
        for (int i = threadIdx.x; i < n; i += blockDim.x) s_prev[i] = st.prev[e * n + i];
        if (threadIdx.x == 0) s_ret = st.returns[e];
    }
    for (int it = 0; it < steps; ++it) {
        const int k = k0 + it, ts = ts0 + it;
        __syncthreads();  // the previous step's counts / actions are consumed
        for (int j = threadIdx.x; j < m; j += blockDim.x) s_cnt[j] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const int a = (int)philox_action(key, st.episode, i, k, m);
            if (bv.actions.ptr) *fptr<int64_t>(bv.actions, e, ts, i, 0) = a;
            s_act[i] = a;
            atomicAdd(&s_cnt[a], 1);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += blockDim.x)
            transition_reward(env, bv, st, e, ts, k, i, s_act[i], s_cnt, s_prev[i], s_rew);
        write_pre_row<VEC>(env, bv, e, ts + 1, k + 1, n, m, T, L, s_act, ts);
        __syncthreads();
        if (threadIdx.x == 0) transition_tail(bv, st, e, ts, k, s_rew, s_ret);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) st.prev[e * n + i] = s_prev[i];
    if (threadIdx.x == 0) st.returns[e] = s_ret;
}

// ------------------------------------------------------------------------------------
// table export (Philox bumps -> [E][n][m][T] float64, the reference layout)
// ------------------------------------------------------------------------------------
template <class Src>
__global__ void export_table_kernel(Src src, EnvState st, double *out) {
    extern __shared__ int s_dyn[];
    float *s_scale = reinterpret_cast<float *>(s_dyn);
    const int64_t e = blockIdx.x;
    const int n = st.n, m = st.m, T = st.T;
    src.fill_scale(e, s_scale);
    __syncthreads();
    const auto env = src.bind(e, s_scale);
    for (int p = threadIdx.x; p < n * m; p += blockDim.x) {
        const int i = p / m, j = p - i * m;
        const auto P = env.pair(i, j);
        for (int t = 0; t < T; ++t) out[((e * n + i) * (int64_t)m + j) * T + t] = P.at64(t);
    }
}

// Philox bump parameters [E][n][m][3] float32 = (scale (0: inactive pair), center, a2), the
// values every bump evaluation uses (value(t) = scale * 2^(-(t - center)^2 * a2))
__global__ void export_bump_params_kernel(BumpSrc src, EnvState st, float *out) {
    extern __shared__ int s_dyn[];
    float *s_scale = reinterpret_cast<float *>(s_dyn);
    const int64_t e = blockIdx.x;
    const int n = st.n, m = st.m;
    src.fill_scale(e, s_scale);
    __syncthreads();
    const auto env = src.bind(e, s_scale);
    for (int p = threadIdx.x; p < n * m; p += blockDim.x) {
        const Bump32 b = env.pair(p / m, p % m).b;
        float *o = out + (e * n * (int64_t)m + p) * 3;
        o[0] = b.scale;
        o[1] = b.center;
        o[2] = b.a2;
    }
}

// [E][n][m][T] (reference layout) -> [E][T][n][m] (kernel layout)
__global__ void import_table_kernel(const double *in, EnvState st, double *tab, int64_t src_envs) {
    const int64_t e = blockIdx.x;
    const int n = st.n, m = st.m, T = st.T;
    const int64_t se = src_envs == 1 ? 0 : e;
    for (int64_t p = threadIdx.x; p < (int64_t)n * m * T; p += blockDim.x) {
        const int t = (int)(p % T);
        const int64_t ij = p / T;
        const double x = in[se * (int64_t)n * m * T + p];
        tab[(e * T + t) * (int64_t)n * m + ij] = x;
        st.table32[(e * T + t) * (int64_t)n * m + ij] = (float)x;
    }
}

__global__ void export_prev_kernel(EnvState st, int64_t *out) {
    const int64_t e = blockIdx.x;
    for (int i = threadIdx.x; i < st.n; i += blockDim.x) out[e * st.n + i] = st.prev[e * st.n + i];
}

// ------------------------------------------------------------------------------------
// host launchers
// ------------------------------------------------------------------------------------
static size_t step_lds_bytes(const EnvState &st) {
    return sizeof(int) * (st.n + 2 * st.m + 1) + sizeof(double) * st.n + 16;
}

template <class Src, bool BIDS>
static void launch_step_t(const Src &src, const asg_batch_view &bv, const EnvState &st, int ts, int k,
                          hipStream_t s) {
    const size_t lds = step_lds_bytes(st);
    if (vec4_ok(bv, st.m))
        hipLaunchKernelGGL((step_kernel<4, Src, BIDS>), dim3(st.E), dim3(256), lds, s, src, bv, st, ts, k);
    else
        hipLaunchKernelGGL((step_kernel<1, Src, BIDS>), dim3(st.E), dim3(256), lds, s, src, bv, st, ts, k);
}

// cpl | storage << 8 of the bids_assign_kernel instance an (n, m) env runs (asg_bids_instance):
// registers at m <= 64, else the bid matrix staged in LDS (n * m <= 16384, checked at create)
int bids_instance(int n, int m) {
    if (m <= 64) return 1 | ASG_LSA_REGISTERS << 8;
    return (m <= 128 ? 2 : m <= 256 ? 4 : m <= 512 ? 8 : 16) | ASG_LSA_LDS << 8;
}

hipError_t launch_bids_assign(const asg_batch_view &bv, const EnvState &st, int ts, hipStream_t s) {
    const size_t lds = sizeof(float) * (size_t)st.n * st.m + 32;
    // bids matrices are at most 16384 entries (checked at create): m <= 16384 / n
    switch (bids_instance(st.n, st.m) & 0xff) {
        case 1: hipLaunchKernelGGL(bids_assign_kernel<1>, dim3(st.E), dim3(64), lds, s, bv, st, ts); break;
        case 2: hipLaunchKernelGGL(bids_assign_kernel<2>, dim3(st.E), dim3(64), lds, s, bv, st, ts); break;
        case 4: hipLaunchKernelGGL(bids_assign_kernel<4>, dim3(st.E), dim3(64), lds, s, bv, st, ts); break;
        case 8: hipLaunchKernelGGL(bids_assign_kernel<8>, dim3(st.E), dim3(64), lds, s, bv, st, ts); break;
        default: hipLaunchKernelGGL(bids_assign_kernel<16>, dim3(st.E), dim3(64), lds, s, bv, st, ts); break;
    }
    return hipGetLastError();
}

template <class Src>
static hipError_t launch_step_src(const Src &src, const asg_batch_view &bv, const EnvState &st, int ts, int k,
                                  hipStream_t s, bool assign_ready) {
    if (st.bids) {
        if (!assign_ready) {
            const hipError_t e = launch_bids_assign(bv, st, ts, s);
            if (e != hipSuccess) return e;
        }
        launch_step_t<Src, true>(src, bv, st, ts, k, s);
    } else {
        launch_step_t<Src, false>(src, bv, st, ts, k, s);
    }
    return hipGetLastError();
}

template <class Src>
static hipError_t launch_reset_src(const Src &src, const asg_batch_view &bv, const EnvState &st, int ts,
                                   bool philox_perm, hipStream_t s) {
    const size_t lds = sizeof(int) * 2 * st.m + 16;
    if (vec4_ok(bv, st.m))
        hipLaunchKernelGGL((reset_kernel<4, Src>), dim3(st.E), dim3(256), lds, s, src, bv, st, ts, philox_perm);
    else
        hipLaunchKernelGGL((reset_kernel<1, Src>), dim3(st.E), dim3(256), lds, s, src, bv, st, ts, philox_perm);
    return hipGetLastError();
}

hipError_t launch_reset(const asg_batch_view &bv, const EnvState &st, int ts, bool construct, hipStream_t s) {
    // MT19937: the stream's own kernels draw the permutation (and the table) first
    const bool philox_perm = st.rng_mode != ASG_RNG_MT19937;
    if (!philox_perm) {
        const hipError_t err = launch_reset_draws(st, construct, s);
        if (err != hipSuccess) return err;
    }
    return with_src(st, [&](const auto &src) { return launch_reset_src(src, bv, st, ts, philox_perm, s); });
}

hipError_t launch_step(const asg_batch_view &bv, const EnvState &st, int ts, int k, hipStream_t s, bool assign_ready) {
    return with_src(st, [&](const auto &src) { return launch_step_src(src, bv, st, ts, k, s, assign_ready); });
}

template <class Src>
static hipError_t launch_random_rollout_src(const Src &src, const asg_batch_view &bv, const EnvState &st, int ts,
                                            int k0, int steps, bool reset, hipStream_t s) {
    const size_t lds = sizeof(int) * (size_t)(2 * st.n + 2 * st.m + 2) + sizeof(double) * st.n + 16;
    // one wave per 64 work items of the row writer (VEC tasks each), at most 4 waves
    const int64_t items = (int64_t)st.n * ((st.m + 3) / 4);
    const int threads = items >= 256 ? 256 : (int)((items + 63) / 64 * 64);
    if (vec4_ok(bv, st.m))
        hipLaunchKernelGGL((random_rollout_kernel<4, Src>), dim3(st.E), dim3(threads), lds, s, src, bv, st, ts, k0, steps,
                           reset ? 1 : 0);
    else
        hipLaunchKernelGGL((random_rollout_kernel<1, Src>), dim3(st.E), dim3(threads), lds, s, src, bv, st, ts, k0, steps,
                           reset ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_random_rollout(const asg_batch_view &bv, const EnvState &st, int ts, int k0, int steps, bool reset,
                                 hipStream_t s) {
    return with_src(st, [&](const auto &src) {
        return launch_random_rollout_src(src, bv, st, ts, k0, steps, reset, s);
    });
}

hipError_t launch_random_actions(const asg_batch_view &bv, const EnvState &st, int ts, int k, hipStream_t s) {
    hipLaunchKernelGGL(random_actions_kernel, dim3(st.E), dim3(64), 0, s, bv, st, ts, k);
    return hipGetLastError();
}

hipError_t launch_export_bump_params(const EnvState &st, float *out, hipStream_t s) {
    hipLaunchKernelGGL(export_bump_params_kernel, dim3(st.E), dim3(256), sizeof(float) * st.m, s, bump_src(st), st,
                       out);
    return hipGetLastError();
}

hipError_t launch_export_table(const EnvState &st, double *out, hipStream_t s) {
    const size_t lds = sizeof(float) * st.m + 16;
    return with_src(st, [&](auto src) {
        hipLaunchKernelGGL((export_table_kernel<decltype(src)>), dim3(st.E), dim3(256), lds, s, src, st, out);
        return hipGetLastError();
    });
}

hipError_t launch_import_table(const double *in, int64_t src_envs, const EnvState &st, hipStream_t s) {
    hipLaunchKernelGGL(import_table_kernel, dim3(st.E), dim3(256), 0, s, in, st, st.table, src_envs);
    return hipGetLastError();
}

hipError_t launch_export_prev(const EnvState &st, int64_t *out, hipStream_t s) {
    hipLaunchKernelGGL(export_prev_kernel, dim3(st.E), dim3(64), 0, s, st, out);
    return hipGetLastError();
}

}  // namespace asg
