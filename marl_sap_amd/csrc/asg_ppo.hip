// asg_ppo.hip -- the loss side of ContinuousPPOLearner.train (reference: learners/
// cont_ppo_learner.py:48-192, ippo_sap.yaml) on the unroll kernels' outputs (gfx950).
//
// Everything here works in the flattened time-major row order of asg_mlp_agent_unroll /
// asg_rnn_agent_unroll: row = t * R + env * n + agent, R = B * n, m contiguous values per row --
// the agent's logits, the critic's values, the advantages and the gradients are used as the
// unroll kernels wrote them, with no permute copy.  What lives in the EpisodeBatch (the bids in
// batch["actions"], the rewards, the (b, t) mask) is read through element strides {t, env, agent}.
//
//   bids_log_prob_kernel : logp = Normal(bids, sigma).log_prob(pi) per element, pi = softmax(logits)
//                          (row_softmax) or the logits, pi = 1 on masked rows (:66-75)
//   ppo_loss_kernel      : the clipped surrogate of one epoch (:91-101) and its gradient with
//                          respect to the logits in one pass; per-workgroup partial sums
//   nstep_kernel         : nstep_returns (:174-192), the reference's loop per element
//
// Lane mapping of the two row kernels: 16 lanes (one DPP row) own a row of m <= 512 values, lane
// l the float4 at columns 64 c + 4 l of chunk c, so a wave reads four consecutive rows -- 1 KiB
// contiguous at m = 64 -- and the row reductions (softmax max / sum, the softmax backward's dot
// product) are four DPP steps with no LDS.  The butterfly order makes every lane of a row hold
// the same bits.  No atomics, fixed reduction order: two runs give the same bits.
#include "unroll_common.h"

#include <cmath>

namespace asg {
namespace {

constexpr int kRowsWg = 16;   // rows per workgroup: 4 waves x 4 rows (ASG_PPO_ROWS_PER_GROUP)
constexpr int kMaxPow = 256;  // powers of gamma carried in the kernel arguments

template <int kCtrl>
__device__ __forceinline__ float dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), kCtrl, 0xf, 0xf, false));
}
// xor-butterfly over the 16 lanes of a DPP row: quad_perm [1,0,3,2], quad_perm [2,3,0,1], then
// row_half_mirror and row_mirror, which pair a lane with the other quad / half once those are uniform
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp<0xB1>(v);
    v += dpp<0x4E>(v);
    v += dpp<0x141>(v);
    v += dpp<0x140>(v);
    return v;
}
__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, dpp<0xB1>(v));
    v = fmaxf(v, dpp<0x4E>(v));
    v = fmaxf(v, dpp<0x141>(v));
    v = fmaxf(v, dpp<0x140>(v));
    return v;
}

__device__ __forceinline__ void strow(float *row, int j, int m, bool vec, f32x4 v) {
    if (vec) {
        if (j < m) st4(row + j, v);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (j + e < m) row[j + e] = v[e];
    }
}

struct RowArgs {
    const float *logits, *bids, *old_logp, *adv, *mask, *inv_count;
    int64_t bs_t, bs_e, bs_a, ms_t, ms_e, ms_a;
    int64_t R, N;
    int n, m;
    int softmax, vec, bvec;
    float two_var, var, log_sigma, half_log_2pi, lo, hi;
    float *logp, *dlogits, *partial, *row_max;
};

// the lane's row: (flattened row or 0 past N, whether it exists, its bids row and its mask)
struct Row {
    int64_t rc;
    bool ok;
    const float *bids;
    float mk;
};
__device__ __forceinline__ Row locate(const RowArgs &a) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kRowsWg + (threadIdx.x >> 6) * 4 + (lane >> 4);
    Row r;
    r.ok = row < a.N;
    r.rc = r.ok ? row : 0;  // rows past N compute row 0 again and store nothing
    const int64_t t = r.rc / a.R;
    const int64_t rr = r.rc - t * a.R;
    const int64_t env = rr / a.n;
    const int64_t ag = rr - env * a.n;
    r.bids = a.bids + t * a.bs_t + env * a.bs_e + ag * a.bs_a;
    r.mk = a.mask[t * a.ms_t + env * a.ms_e + ag * a.ms_a];
    return r;
}

// pi of the lane's row: softmax(logits) or the logits, 1 on a masked row (old_pi[mask == 0] = 1.0)
template <int NC>
__device__ __forceinline__ void row_pi(const RowArgs &a, const Row &r, int l, f32x4 (&pi)[NC]) {
    const int m = a.m;
    const float *lrow = a.logits + r.rc * m;
#pragma unroll
    for (int c = 0; c < NC; ++c)
        if (64 * c < m) pi[c] = ldk(lrow, 64 * c + 4 * l, m, a.vec != 0);
    if (a.softmax) {
        float mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < NC; ++c)
            if (64 * c < m)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (64 * c + 4 * l + e < m) mx = fmaxf(mx, pi[c][e]);
        mx = row16_max(mx);
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c)
            if (64 * c < m)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float ex = 64 * c + 4 * l + e < m ? expf(pi[c][e] - mx) : 0.f;
                    pi[c][e] = ex;
                    s += ex;
                }
        s = row16_sum(s);
#pragma unroll
        for (int c = 0; c < NC; ++c)
            if (64 * c < m)
#pragma unroll
                for (int e = 0; e < 4; ++e) pi[c][e] = pi[c][e] / s;
    }
    if (r.mk == 0.f) {
#pragma unroll
        for (int c = 0; c < NC; ++c)
            if (64 * c < m) pi[c] = f32x4{1.f, 1.f, 1.f, 1.f};
    }
}

template <int NC>
__global__ void __launch_bounds__(256) bids_log_prob_kernel(RowArgs a) {
    const int l = threadIdx.x & 15, m = a.m;
    const Row r = locate(a);
    f32x4 pi[NC];
    row_pi<NC>(a, r, l, pi);
    if (!r.ok) return;
    float *out = a.logp + r.rc * m;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        if (64 * c >= m) break;
        const int j = 64 * c + 4 * l;
        const f32x4 b = ldk(r.bids, j, m, a.bvec != 0);
        f32x4 lp;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d = pi[c][e] - b[e];
            lp[e] = -(d * d) / a.two_var - a.log_sigma - a.half_log_2pi;
        }
        strow(out, j, m, a.vec != 0, lp);
    }
}

template <int NC>
__global__ void __launch_bounds__(256) ppo_loss_kernel(RowArgs a) {
    __shared__ float s_part[4];
    const int lane = threadIdx.x & 63, l = lane & 15, m = a.m;
    const Row r = locate(a);
    f32x4 pi[NC];
    row_pi<NC>(a, r, l, pi);
    if (a.row_max) {  // the reference's "max bid" statistic: pi.max(dim=-1)
        float mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < NC; ++c)
            if (64 * c < m)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (64 * c + 4 * l + e < m) mx = fmaxf(mx, pi[c][e]);
        mx = row16_max(mx);
        if (r.ok && l == 0) a.row_max[r.rc] = mx;
    }
    const bool live = r.ok && r.mk != 0.f;
    const float scale = live ? -(r.mk * a.inv_count[0]) : 0.f;  // -mask * inv_count
    const float *orow = a.old_logp + r.rc * m, *arow = a.adv + r.rc * m;
    f32x4 g[NC];
    float part = 0.f, dot = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        if (64 * c >= m) break;
        const int j = 64 * c + 4 * l;
        const f32x4 b = ldk(r.bids, j, m, a.bvec != 0);
        const f32x4 olp = ldk(orow, j, m, a.vec != 0), A = ldk(arow, j, m, a.vec != 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d = pi[c][e] - b[e];
            const float lp = -(d * d) / a.two_var - a.log_sigma - a.half_log_2pi;
            const float ratio = expf(lp - olp[e]);
            const float s1 = ratio * A[e];
            const float s2 = fminf(fmaxf(ratio, a.lo), a.hi) * A[e];
            const bool valid = live && j + e < m;
            part += valid ? fminf(s1, s2) * r.mk : 0.f;
            // autograd through th.min / th.clamp: the gradient reaches the ratio when s1 <= s2
            const float ge = valid && s1 <= s2 ? scale * (A[e] * ratio * (-d / a.var)) : 0.f;
            g[c][e] = ge;
            dot += ge * pi[c][e];
        }
    }
    if (a.softmax) dot = row16_sum(dot);
    if (r.ok) {
        float *drow = a.dlogits + r.rc * m;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (64 * c >= m) break;
            f32x4 dl = g[c];
            if (a.softmax)
#pragma unroll
                for (int e = 0; e < 4; ++e) dl[e] = live ? pi[c][e] * (g[c][e] - dot) : 0.f;
            strow(drow, 64 * c + 4 * l, m, a.vec != 0, dl);
        }
    }
    // the workgroup's share of sum(obj * mask): row, wave, then the four waves in order
    part = row16_sum(part);
    part += __shfl_xor(part, 16);
    part += __shfl_xor(part, 32);
    if (lane == 0) s_part[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0) a.partial[blockIdx.x] = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
}

struct NstepArgs {
    const float *values, *rew, *mask;
    int64_t rs_t, rs_e, rs_a, ms_t, ms_e, ms_a;
    int64_t R, total;
    int T, n, m, mq, nsteps, add_last, vec;
    float *out;
    float gpow[kMaxPow];
};

// one thread per four consecutive columns of one output row; the reference's loop over `step`
// with its three branches, each product rounded as torch rounds it ((gamma^k x) mask)
__global__ void __launch_bounds__(256) nstep_kernel(NstepArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.total) return;
    const int64_t row = idx / a.mq;
    const int j = 4 * (int)(idx - row * a.mq), m = a.m, T = a.T;
    const int64_t t0 = row / a.R;
    const int64_t rr = row - t0 * a.R;
    const int64_t env = rr / a.n;
    const int64_t ag = rr - env * a.n;
    const float *rew = a.rew + env * a.rs_e + ag * a.rs_a;
    const float *mask = a.mask + env * a.ms_e + ag * a.ms_a;
    const bool vec = a.vec != 0;
    f32x4 ret = {0.f, 0.f, 0.f, 0.f};
    for (int step = 0; step <= a.nsteps; ++step) {
        const int64_t t = t0 + step;
        if (t >= T) break;
        const float mk = mask[t * a.ms_t], gs = a.gpow[step];
        if (step == a.nsteps) {
            const f32x4 v = ldk(a.values + (t * a.R + rr) * m, j, m, vec);
#pragma unroll
            for (int e = 0; e < 4; ++e) ret[e] += gs * v[e] * mk;
        } else {
            const float x = gs * rew[t * a.rs_t] * mk;
#pragma unroll
            for (int e = 0; e < 4; ++e) ret[e] += x;
            if (t == T - 1 && a.add_last) {
                const float g1 = a.gpow[step + 1];
                const f32x4 v = ldk(a.values + ((t + 1) * a.R + rr) * m, j, m, vec);
#pragma unroll
                for (int e = 0; e < 4; ++e) ret[e] += g1 * v[e];
            }
        }
    }
    strow(a.out + row * m, j, m, vec, ret);
}

constexpr int64_t kMaxRows = (int64_t)0x7fffffff * kRowsWg;

// the checks and arguments the two row kernels share
int row_args(const std::string &w, RowArgs &a, const float *logits, const float *bids, const int64_t *bs,
             const float *mask, const int64_t *ms, int T, int64_t B, int n, int m, double sigma, int row_softmax) {
    const int64_t R = (B > 0 && n > 0) ? B * n : 0;
    if (m < 1 || m > 512) return fail((w + ": m must be in 1..512").c_str());
    if (T < 1) return fail((w + ": T must be >= 1").c_str());
    if (R < 1) return fail((w + ": needs at least one agent row").c_str());
    if (R > kMaxRows / T) return fail((w + ": too many rows").c_str());
    if (!(sigma > 0.0) || !std::isfinite(sigma)) return fail((w + ": sigma must be positive").c_str());
    if (!logits || !bids || !bs || !mask || !ms) return fail((w + ": NULL argument").c_str());
    if (!al(logits, 16) || !al(bids, 4) || !al(mask, 4))
        return fail((w + ": misaligned pointer (16 B for logits, logp, old_logp, adv, dlogits)").c_str());
    a.logits = logits;
    a.bids = bids;
    a.mask = mask;
    a.bs_t = bs[0], a.bs_e = bs[1], a.bs_a = bs[2];
    a.ms_t = ms[0], a.ms_e = ms[1], a.ms_a = ms[2];
    a.R = R;
    a.N = (int64_t)T * R;
    a.n = n;
    a.m = m;
    a.softmax = row_softmax != 0;
    a.vec = m % 4 == 0;  // the contiguous [N][m] buffers are 16-B aligned: so is every row
    a.bvec = m % 4 == 0 && al(bids, 16) && ((a.bs_t | a.bs_e | a.bs_a) & 3) == 0;
    // Normal(loc, sigma).log_prob as torch evaluates it: -(d^2) / (2 var) - log(sigma) - log(sqrt(2 pi))
    const float s = (float)sigma, var = s * s;
    a.var = var;
    a.two_var = 2.f * var;
    a.log_sigma = std::log(s);
    a.half_log_2pi = (float)std::log(std::sqrt(2.0 * M_PI));
    a.old_logp = a.adv = a.inv_count = nullptr;
    a.logp = a.dlogits = a.partial = a.row_max = nullptr;
    a.lo = a.hi = 1.f;
    return ASG_OK;
}

template <template <int> class Launch>
void by_chunks(int m, const RowArgs &a, hipStream_t s) {
    const unsigned grid = (unsigned)((a.N + kRowsWg - 1) / kRowsWg);
    if (m <= 64) Launch<1>::go(grid, a, s);
    else if (m <= 128) Launch<2>::go(grid, a, s);
    else if (m <= 256) Launch<4>::go(grid, a, s);
    else Launch<8>::go(grid, a, s);
}
template <int NC>
struct LogProb {
    static void go(unsigned grid, const RowArgs &a, hipStream_t s) {
        hipLaunchKernelGGL(bids_log_prob_kernel<NC>, dim3(grid), dim3(256), 0, s, a);
    }
};
template <int NC>
struct Loss {
    static void go(unsigned grid, const RowArgs &a, hipStream_t s) {
        hipLaunchKernelGGL(ppo_loss_kernel<NC>, dim3(grid), dim3(256), 0, s, a);
    }
};

}  // namespace
}  // namespace asg

extern "C" int asg_bids_log_prob(const float *logits, const float *bids, const int64_t bid_strides[3],
                                 const float *mask, const int64_t mask_strides[3], int T, int64_t B, int n, int m,
                                 double sigma, int row_softmax, float *logp, void *hip_stream) {
    using namespace asg;
    RowArgs a;
    const int rc = row_args("asg_bids_log_prob", a, logits, bids, bid_strides, mask, mask_strides, T, B, n, m, sigma,
                            row_softmax);
    if (rc != ASG_OK) return rc;
    if (!logp) return fail("asg_bids_log_prob: NULL argument");
    if (!al(logp, 16)) return fail("asg_bids_log_prob: misaligned pointer (16 B for logits, logp)");
    a.logp = logp;
    by_chunks<LogProb>(m, a, static_cast<hipStream_t>(hip_stream));
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? ASG_OK : hip_fail(e, "asg_bids_log_prob");
}

extern "C" int asg_ppo_bids_loss(const float *logits, const float *bids, const int64_t bid_strides[3],
                                 const float *old_logp, const float *adv, const float *mask,
                                 const int64_t mask_strides[3], int T, int64_t B, int n, int m, double sigma,
                                 double eps_clip, const float *inv_count, int row_softmax, float *partial,
                                 float *dlogits, float *row_max, void *hip_stream) {
    using namespace asg;
    RowArgs a;
    const int rc = row_args("asg_ppo_bids_loss", a, logits, bids, bid_strides, mask, mask_strides, T, B, n, m, sigma,
                            row_softmax);
    if (rc != ASG_OK) return rc;
    if (!(eps_clip >= 0.0) || !std::isfinite(eps_clip)) return fail("asg_ppo_bids_loss: eps_clip must be >= 0");
    if (!old_logp || !adv || !inv_count || !partial || !dlogits) return fail("asg_ppo_bids_loss: NULL argument");
    if (!al(old_logp, 16) || !al(adv, 16) || !al(dlogits, 16) || !al(inv_count, 4) || !al(partial, 4) ||
        !al(row_max, 4))
        return fail("asg_ppo_bids_loss: misaligned pointer (16 B for logits, old_logp, adv, dlogits)");
    a.old_logp = old_logp;
    a.adv = adv;
    a.inv_count = inv_count;
    a.partial = partial;
    a.dlogits = dlogits;
    a.row_max = row_max;
    a.lo = (float)(1.0 - eps_clip);
    a.hi = (float)(1.0 + eps_clip);
    by_chunks<Loss>(m, a, static_cast<hipStream_t>(hip_stream));
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? ASG_OK : hip_fail(e, "asg_ppo_bids_loss");
}

extern "C" int asg_nstep_returns(const float *values, const float *rewards, const int64_t reward_strides[3],
                                 const float *mask, const int64_t mask_strides[3], int T, int64_t B, int n, int m,
                                 double gamma, int nsteps, int add_value_last_step, float *out, void *hip_stream) {
    using namespace asg;
    const int64_t R = (B > 0 && n > 0) ? B * n : 0;
    if (m < 1 || m > 512) return fail("asg_nstep_returns: m must be in 1..512");
    if (T < 1) return fail("asg_nstep_returns: T must be >= 1");
    if (R < 1) return fail("asg_nstep_returns: needs at least one agent row");
    if (nsteps < 1) return fail("asg_nstep_returns: nsteps must be >= 1");
    const int npow = (nsteps < T - 1 ? nsteps : T - 1) + 2;  // gamma^0 .. gamma^(min(nsteps, T - 1) + 1)
    if (npow > kMaxPow) return fail("asg_nstep_returns: min(nsteps, T - 1) must be at most 254");
    const int mq = (m + 3) / 4;
    if (R > ((int64_t)0x7fffffff * 256 / mq) / T) return fail("asg_nstep_returns: too many rows");
    if (!values || !rewards || !reward_strides || !mask || !mask_strides || !out)
        return fail("asg_nstep_returns: NULL argument");
    if (!al(values, 16) || !al(out, 16) || !al(rewards, 4) || !al(mask, 4))
        return fail("asg_nstep_returns: misaligned pointer (16 B for values, out)");
    NstepArgs a;
    a.values = values;
    a.rew = rewards;
    a.mask = mask;
    a.rs_t = reward_strides[0], a.rs_e = reward_strides[1], a.rs_a = reward_strides[2];
    a.ms_t = mask_strides[0], a.ms_e = mask_strides[1], a.ms_a = mask_strides[2];
    a.R = R;
    a.T = T;
    a.n = n;
    a.m = m;
    a.mq = mq;
    a.total = (int64_t)T * R * mq;
    a.nsteps = nsteps;
    a.add_last = add_value_last_step != 0;
    a.vec = m % 4 == 0;
    a.out = out;
    // gamma ** k as Python evaluates it (double), rounded to float32 as torch rounds a Python
    // scalar it applies to a float32 tensor
    for (int k = 0; k < kMaxPow; ++k) a.gpow[k] = k < npow ? (float)std::pow(gamma, (double)k) : 0.f;
    const unsigned grid = (unsigned)((a.total + 255) / 256);
    hipLaunchKernelGGL(nstep_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(hip_stream), a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? ASG_OK : hip_fail(e, "asg_nstep_returns");
}
