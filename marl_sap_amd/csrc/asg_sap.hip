// asg_sap.hip -- the runner's per-step selector kernels (gfx950), one wave64 per env on the
// register-resident solvers of lsa_reg64.h: the SAP selector on Q-values (sap_select_kernel, with
// its parity tool sap_noise_kernel) and bids_as_actions with the continuous selector
// (bids_select_kernel).  They are register-tight: 88 to 96 VGPRs at the 5-waves budget.
// Reference call sites: sap_selectors.py:52-98, bet_selectors.py:13-20,
// mock_constellation_env.py:121-122.
#include "asg_device.h"
#include "asg_internal.h"
#include "sap_stage.h"

namespace asg {

// ------------------------------------------------------------------------------------
// SequentialAssignmentProblemSelector (sap_selectors.py:52-98), n <= m <= 64, fused:
// noise of std mean|Q| * eps * 2 added in registers while the column is staged, then the
// register-resident LSA (maximize).  The reference runs, per env on the host: abs, mean,
// ones * avg * eps * 2, torch.normal, +=, scipy.
// ------------------------------------------------------------------------------------
// kWarm: `duals` [B][64] float64 holds each env's column duals from its previous selection --
// the fast path's warm start (lsa_fast_reg64) -- and receives this selection's (NaN when the
// fast path did not finish: the next call starts that env cold)
template <bool kCount, bool kDense64, bool kWarm>
__global__ void __launch_bounds__(64 * kLsaWpb) __attribute__((amdgpu_waves_per_eu(kLsaRegWaves)))
sap_select_kernel(const float *q, int64_t q0, int64_t q1, int64_t q2, int n, int m, float epsilon, uint64_t seed,
                  uint32_t counter, int64_t env_base, float *col_out, int64_t *act_out, int32_t *status_out,
                  int32_t *steps_out, int64_t B, double *duals, int warm) {
    __shared__ uint64_t s_slot[kLsaWpb][64];
    const int64_t b = lsa_reg_problem();
    if (b >= B) return;
    sap_select_one<kCount, kDense64, kWarm>(q, q0, q1, q2, n, m, epsilon, seed, counter, env_base, b, col_out, act_out,
                                            status_out, steps_out, duals, warm, s_slot[threadIdx.x >> 6]);
}

// the noisy Q the selector solves (Q + its noise, as sap_stage forms it): parity tooling,
// the SAP selection at epsilon > 0 is checked against scipy on exactly this matrix
__global__ void __launch_bounds__(64 * kLsaWpb) sap_noise_kernel(const float *q, int64_t q0, int64_t q1, int64_t q2,
                                                                 int n, int m, float epsilon, uint64_t seed,
                                                                 uint32_t counter, int64_t env_base, float *q_out,
                                                                 int32_t *status_out, int64_t B) {
    const int64_t b = lsa_reg_problem();
    if (b >= B) return;
    RegCostF32 rc;
    const int status = sap_stage<false>(q, q0, q1, q2, n, m, epsilon, seed, counter, env_base, b, rc);
    const int lane = threadIdx.x & (kWave - 1);
    float *o = q_out + b * n * m + lane;
    if (lane < m) {
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            if (i < n) o[i * m] = -rc.lo[i];
            if (i + 32 < n) o[(i + 32) * m] = -rc.hi[i];
        }
    }
    if (lane == 0 && status_out) status_out[b] = status;
}

hipError_t launch_sap_noise(const float *q, const int64_t qs[3], int64_t B, int n, int m, float epsilon, uint64_t seed,
                            uint32_t counter, int64_t env_base, float *q_out, int32_t *status_out, hipStream_t s) {
    hipLaunchKernelGGL(sap_noise_kernel, lsa_reg_grid(B), dim3(64 * kLsaWpb), 0, s, q, qs[0], qs[1], qs[2], n, m,
                       epsilon, seed, counter, env_base, q_out, status_out, B);
    return hipGetLastError();
}

hipError_t launch_sap_select(const float *q, const int64_t qs[3], int64_t B, int n, int m, float epsilon,
                             uint64_t seed, uint32_t counter, int64_t env_base, float *col_out, int32_t *status_out,
                             int32_t *steps_out, hipStream_t s, int64_t *act_out, double *duals, int warm) {
    // the rollout's Q rows ([B][64][64] contiguous): the unguarded staging instance
    const bool d64 = n == 64 && m == 64 && qs[2] == 1 && qs[1] == 64 && (reinterpret_cast<uintptr_t>(q) & 3) == 0;
    // [kWarm: duals given (square problems, the runner's selection)][kCount][kDense64]
    using Kernel = decltype(&sap_select_kernel<false, false, false>);
    static const Kernel kernels[2][2][2] = {
        {{sap_select_kernel<false, false, false>, sap_select_kernel<false, true, false>},
         {sap_select_kernel<true, false, false>, sap_select_kernel<true, true, false>}},
        {{sap_select_kernel<false, false, true>, sap_select_kernel<false, true, true>},
         {sap_select_kernel<true, false, true>, sap_select_kernel<true, true, true>}}};
    hipLaunchKernelGGL(kernels[duals != nullptr][steps_out != nullptr][d64], lsa_reg_grid(B), dim3(64 * kLsaWpb), 0, s,
                       q, qs[0], qs[1], qs[2], n, m, epsilon, seed, counter, env_base, col_out, act_out, status_out,
                       steps_out, B, duals, duals ? warm : 0);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// bids_as_actions with the ContinuousActionSelector (ippo_sap.yaml), n <= m <= 64, fused: env
// b's agent outputs (the rollout kernel's Q rows) -> softmax over the tasks (BasicMAC.forward
// with agent_output_type "pi_logits", basic_controller.py:37-46) -> softmax over the agents
// (softmax_agent_inputs, bet_selectors.py:13) -> th.normal(x, std) = x + std z (bet_selectors.py:
// 15-20; z from Philox keyed by (seed, global env, call)) -> the bids, stored as the batch's
// actions row -> LSA(bids, maximize) = the env's assignments for its next step
// (mock_constellation_env.py:121-122), kept in the handle for asg_step / asg_step_forward.
// ------------------------------------------------------------------------------------
// waves per SIMD the kernel is compiled for: 96 VGPRs with 26 spilled; the register allocator's
// own choice is 110 VGPRs at 4 waves (0.489 vs 0.498 ms, r5 A/B)
constexpr int kBidsWaves = 5;
// The row softmax's per-row max and sum over the 64 lanes, 16 rows at a time: rows 8g + j (a[j])
// and 8g + j + 32 (b[j]), j < 8, folded by a transposing butterfly -- v_permlane32_swap /
// v_permlane16_swap hand each lane its partner's copy of the rows it keeps (one instruction per
// pair), then row_mirror / row_half_mirror DPP, then a quad reduction -- 17 cross-lane steps for
// 16 rows instead of 16 wave reductions of 6 DPP steps and a broadcast each (one row-softmax pass
// priced at 0.076 ms of the kernel's 0.497, profiles/r6_bids_rowsm_s25.txt).  Lane l ends with
// row 8g + (l >> 2 & 7) + 32 (l >> 5) reduced over all lanes: row_lane16(r) is where row r is.
__device__ __forceinline__ float f_of(uint32_t u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ uint32_t u_of(float f) { return __builtin_bit_cast(uint32_t, f); }
template <class Op>
__device__ __forceinline__ float rows16_reduce(const float (&a)[8], const float (&b)[8], Op op) {
    const int lane = threadIdx.x & 63;
    float t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {  // lanes < 32 keep row 8g + j, lanes >= 32 row 8g + j + 32
        const auto r = __builtin_amdgcn_permlane32_swap(u_of(a[j]), u_of(b[j]), false, false);
        t[j] = op(f_of(r[0]), f_of(r[1]));
    }
    float u[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // + 4 (lane bit 4)
        const auto r = __builtin_amdgcn_permlane16_swap(u_of(t[j]), u_of(t[j + 4]), false, false);
        u[j] = op(f_of(r[0]), f_of(r[1]));
    }
    const bool b3 = (lane & 8) != 0, b2 = (lane & 4) != 0;
    float w[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {  // + 2 (lane bit 3): partner 15 - i in the 16-lane row
        const float keep = b3 ? u[j + 2] : u[j], send = b3 ? u[j] : u[j + 2];
        w[j] = op(keep, f_of((uint32_t)__builtin_amdgcn_update_dpp(0, (int)u_of(send), 0x140, 0xf, 0xf, false)));
    }
    // + 1 (lane bit 2): partner 7 - i in the 8-lane half row
    const float keep = b2 ? w[1] : w[0], send = b2 ? w[0] : w[1];
    float v = op(keep, f_of((uint32_t)__builtin_amdgcn_update_dpp(0, (int)u_of(send), 0x141, 0xf, 0xf, false)));
    // the quad holds four disjoint 16-lane partials of the same row
    v = op(v, f_of((uint32_t)__builtin_amdgcn_update_dpp(0, (int)u_of(v), 0x4e, 0xf, 0xf, false)));
    v = op(v, f_of((uint32_t)__builtin_amdgcn_update_dpp(0, (int)u_of(v), 0xb1, 0xf, 0xf, false)));
    return v;
}
// the lane holding row r (r mod 32 in [8g, 8g + 8)) after rows16_reduce of its group
__device__ __forceinline__ constexpr int row_lane16(int r) { return 32 * (r >> 5) + 4 * (r & 7); }

// kCount: the instrumented instance (bench.py's efficiency figure): steps_out[b] = the env's
// augmenting-path steps, fast path in bits 0..15, scipy-exact solver above (as asg_sap_select)
template <bool kCount>
__global__ void __launch_bounds__(64 * kLsaWpb) __attribute__((amdgpu_waves_per_eu(kBidsWaves)))
bids_select_kernel(const float *q, int64_t q0, int64_t q1, int64_t q2, int n, int m, int row_sm, int col_sm,
                   float stdv, uint64_t seed, uint32_t counter, int64_t env_base, float *bids, int64_t o0,
                   int64_t o1, int64_t o2, int *assign, int *env_err, int64_t B, int32_t *steps_out = nullptr) {
    __shared__ uint64_t s_slot[kLsaWpb][64];
    const int64_t b = lsa_reg_problem();
    if (b >= B) return;
    const int lane = threadIdx.x & (kWave - 1);
    const bool lv = lane < m;
    asm volatile("" : "+s"(q0), "+s"(q1), "+s"(q2), "+s"(o0), "+s"(o1), "+s"(o2));
    RegColPin rc;  // column `lane` of the env's matrix, rows 0..31 in lo, 32..63 in hi
    {
        const float *col = q + b * q0 + (int64_t)lane * q2;
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            rc.lo[i] = (lv && i < n) ? col[i * q1] : 0.0f;
            rc.hi[i] = (lv && i + 32 < n) ? col[(i + 32) * q1] : 0.0f;
        }
    }
    // f(x, i) applied to every row i < n of the column (rows at compile-time register slots)
    auto each_row = [&](auto f) {
#pragma unroll
        for (int i = 0; i < 32; ++i)
            if (i < n) rc.lo[i] = f(rc.lo[i], i);
#pragma unroll
        for (int i = 0; i < 32; ++i)
            if (i + 32 < n) rc.hi[i] = f(rc.hi[i], i + 32);
    };
    // exp as v_exp_f32 of x log2(e) (x = y - max <= 0: relative error <= |x| 2^-24 + 1 ulp; torch's
    // expf is within 1 ulp): the accurate expf unrolled over the 64 rows spilled at any budget
    if (row_sm) {  // softmax(dim = -1) of each agent's row: exp(x - max) / sum
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float a[8], bb[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                a[j] = lv ? rc.lo[8 * g + j] : -__builtin_inff();
                bb[j] = lv ? rc.hi[8 * g + j] : -__builtin_inff();
            }
            const float mx = rows16_reduce(a, bb, [](float x, float y) { return fmaxf(x, y); });
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float ma = f_of((uint32_t)__builtin_amdgcn_readlane((int)u_of(mx), row_lane16(8 * g + j)));
                const float mb = f_of((uint32_t)__builtin_amdgcn_readlane((int)u_of(mx), row_lane16(8 * g + j + 32)));
                a[j] = lv ? __expf(rc.lo[8 * g + j] - ma) : 0.0f;
                bb[j] = lv ? __expf(rc.hi[8 * g + j] - mb) : 0.0f;
            }
            const float sm = rows16_reduce(a, bb, [](float x, float y) { return x + y; });
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float sa = f_of((uint32_t)__builtin_amdgcn_readlane((int)u_of(sm), row_lane16(8 * g + j)));
                const float sb = f_of((uint32_t)__builtin_amdgcn_readlane((int)u_of(sm), row_lane16(8 * g + j + 32)));
                if (8 * g + j < n) rc.lo[8 * g + j] = a[j] / sa;
                if (8 * g + j + 32 < n) rc.hi[8 * g + j] = bb[j] / sb;
            }
        }
    }
    if (col_sm) {  // softmax(dim = 1): over the agents, lane-local
        float mx = -__builtin_inff(), sum = 0.0f;
        each_row([&](float x, int) {
            mx = fmaxf(mx, x);
            return x;
        });
        each_row([&](float x, int) {
            const float ex = __expf(x - mx);
            sum += ex;
            return ex;
        });
        each_row([&](float x, int) { return x / sum; });
    }
    // th.normal(mean, std): mean + std * z (std = 0 keeps the means exactly)
    if (stdv > 0.0f) add_normal_noise<kCtrBidsNoise>(rc, stdv, env_key(seed, env_base + b), counter);
    // the bids: the actions the batch stores (one 64-float row per store instruction); scipy
    // maximize on the float64 bids: NaN or +inf (-inf once negated) is invalid
    int bad = 0;
    {
        float *o = bids + b * o0 + (int64_t)lane * o2;
        each_row([&](float x, int i) {
            if (lv) o[i * o1] = x;
            bad |= lv & ((x != x) | (x == __builtin_inff()));
            return x;
        });
    }
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        rc.lo[i] = (lv && i < n) ? -rc.lo[i] : 0.0f;
        rc.hi[i] = (lv && i + 32 < n) ? -rc.hi[i] : 0.0f;
    }
    int status = __builtin_amdgcn_readfirstlane(wave_or_i32(bad)) ? ASG_E_LSA_INVALID : ASG_OK;
    int c4r[1] = {-1};
    int nfast = 0, nsteps = 0;
    bool done = false;
    if (status == ASG_OK && n == m)
        done = lsa_fast_reg64<decltype(rc), kCount>(rc, n, c4r, &nfast, s_slot[threadIdx.x >> 6]) == ASG_OK;
    if (status == ASG_OK && !done) status = lsa_solve_reg64<decltype(rc), kCount>(rc, n, m, c4r, &nsteps);
    if (lane < n) assign[b * n + lane] = status == ASG_OK ? c4r[0] : -1;
    if (status != ASG_OK && lane == 0) atomicCAS(env_err, 0, status);
    if (kCount && lane == 0 && steps_out) steps_out[b] = nfast | (nsteps << 16);
}

hipError_t launch_bids_select(const float *q, const int64_t qs[3], int64_t B, int n, int m, int row_sm, int col_sm,
                              float stdv, uint64_t seed, uint32_t counter, int64_t env_base, float *bids,
                              const int64_t os[3], int *assign, int *env_err, hipStream_t s, int32_t *steps_out) {
    if (steps_out)
        hipLaunchKernelGGL(bids_select_kernel<true>, lsa_reg_grid(B), dim3(64 * kLsaWpb), 0, s, q, qs[0], qs[1], qs[2],
                           n, m, row_sm, col_sm, stdv, seed, counter, env_base, bids, os[0], os[1], os[2], assign,
                           env_err, B, steps_out);
    else
        hipLaunchKernelGGL(bids_select_kernel<false>, lsa_reg_grid(B), dim3(64 * kLsaWpb), 0, s, q, qs[0], qs[1],
                           qs[2], n, m, row_sm, col_sm, stdv, seed, counter, env_base, bids, os[0], os[1], os[2],
                           assign, env_err, B, nullptr);
    return hipGetLastError();
}

}  // namespace asg
