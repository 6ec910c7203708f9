// env_src.h -- the mock env's benefit sources, the pre-transition row writer and the pieces of
// the transition that step_kernel and random_rollout_kernel share (asg_env.hip).
#pragma once
#include "asg_device.h"
#include "asg_internal.h"

namespace asg {

// ------------------------------------------------------------------------------------
// benefit sources.  A source is bound to one env (`bind`) and yields per-pair evaluators.
// ------------------------------------------------------------------------------------
struct BumpSrc {  // Philox, float32 bumps regenerated on the fly (no table in HBM)
    uint64_t seed;
    int64_t env_base;
    uint32_t episode;
    int n, m, T;
    float wmin, wmax;
    bool dense;

    static constexpr bool kNeedsScale = true;
    struct Env {
        EnvKey key;
        uint32_t episode;
        int m, T;
        float wmin, wmax;
        bool dense;
        const float *scale;  // LDS [m]
        struct Pair {
            Bump32 b;
            __device__ float at(int t) const { return bump32_at(b, t); }
            __device__ double at64(int t) const { return bump64_at(b, t); }
        };
        __device__ Pair pair(int i, int j) const {
            return Pair{philox_bump32(key, episode, i * m + j, scale[j], T, wmin, wmax, dense)};
        }
        // pairs (i, j) .. (i, j + 3): one Philox call when they share one (pair index % 4 == 0)
        __device__ void pair4(int i, int j, Pair (&P)[4]) const {
            const int p = i * m + j;
            if ((p & 3) == 0) {
                const float sc[4] = {scale[j], scale[j + 1], scale[j + 2], scale[j + 3]};
                Bump32 b[4];
                philox_bump32x4(key, episode, p, sc, bump_shape(T, wmin, wmax), dense, b);
#pragma unroll
                for (int q = 0; q < 4; ++q) P[q].b = b[q];
                return;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) P[q] = pair(i, j + q);
        }
    };
    // fills scale[0..m) cooperatively (caller syncs)
    __device__ void fill_scale(int64_t e, float *scale) const {
        const EnvKey key = env_key(seed, env_base + e);
        for (int j = threadIdx.x; j < m; j += blockDim.x) scale[j] = philox_task_scale(key, episode, j);
    }
    __device__ Env bind(int64_t e, const float *scale) const {
        return Env{env_key(seed, env_base + e), episode, m, T, wmin, wmax, dense, scale};
    }
};

struct TableSrc {  // float64 table [E][T][n][m] (injected)
    const double *tab;
    int n, m, T;

    static constexpr bool kNeedsScale = false;
    struct Env {
        const double *p;  // &tab[e][0][0][0]
        int m;
        int64_t nm;
        struct Pair {
            const double *p;
            int64_t tstride;
            __device__ double at(int t) const { return p[t * tstride]; }
            __device__ double at64(int t) const { return p[t * tstride]; }
        };
        __device__ Pair pair(int i, int j) const { return Pair{p + (int64_t)i * m + j, nm}; }
        __device__ void pair4(int i, int j, Pair (&P)[4]) const {
#pragma unroll
            for (int q = 0; q < 4; ++q) P[q] = pair(i, j + q);
        }
    };
    __device__ void fill_scale(int64_t, float *) const {}
    __device__ Env bind(int64_t e, const float *) const {
        const int64_t nm = (int64_t)n * m;
        return Env{tab + e * (int64_t)T * nm, m, nm};
    }
};

// MT19937 compat mode: the rows' float32 benefits from the reset's compact float32 table (per
// (env, t) slice only the bump pairs, in (agent, task) order: tmask marks them, toff gives each
// mask word's first compact index -- every other pair is exactly 0), the float64 ones (rewards,
// export) evaluated from the recorded draws par [E][m][n] (mt_par_value, the function the table
// was written with): no float64 table in HBM
struct ParSrc {
    const float *tab32;
    const double2 *par;
    const uint64_t *tmask;
    const int *toff;
    int n, m, T;

    static constexpr bool kNeedsScale = false;
    struct Env {
        const float *p;  // &tab32[e][0][0] (slice 0; slices are n m floats apart)
        const double2 *q;  // &par[e][0][0]
        const uint64_t *mk;  // &tmask[e][0][0]
        const int *of;       // &toff[e][0][0]
        int n, m, W;
        int64_t nm;
        struct Pair {
            const float *p;  // the pair's slice-0 compact value, or nullptr: no bump (0 at every t)
            const double2 *q;
            int64_t tstride;
            __device__ float at(int t) const { return p ? p[t * tstride] : 0.0f; }
            __device__ double at64(int t) const { return mt_par_value(*q, t); }
        };
        __device__ Pair pair(int i, int j) const {
            const int w = j >> 6, b = j & 63;
            const uint64_t mw = mk[(int64_t)i * W + w];
            const float *v = nullptr;
            if ((mw >> b) & 1ull)
                v = p + of[(int64_t)i * W + w] + __popcll(mw & ((1ull << b) - 1ull));
            return Pair{v, q + (int64_t)j * n + i, nm};
        }
        __device__ void pair4(int i, int j, Pair (&P)[4]) const {
#pragma unroll
            for (int k = 0; k < 4; ++k) P[k] = pair(i, j + k);
        }
    };
    __device__ void fill_scale(int64_t, float *) const {}
    __device__ Env bind(int64_t e, const float *) const {
        const int64_t nm = (int64_t)n * m;
        const int W = (m + 63) >> 6;
        return Env{tab32 + e * (int64_t)T * nm, par + e * nm, tmask + e * n * W, toff + e * n * W, n, m, W, nm};
    }
};

// ------------------------------------------------------------------------------------
// pre-transition row writer: obs = [onehot(assign) | B(k) .. B(k+L-1)] (zeros past T),
// beta = B(k) (zeros when k >= T), avail_actions = 1; optionally actions_onehot of the
// post-transition row `ts_onehot`.  VEC consecutive tasks per work item; every store of
// a wave covers whole 128-B lines of one agent's rows.
// ------------------------------------------------------------------------------------
template <int VEC, class EnvB>
__device__ void write_pre_row(const EnvB &src, const asg_batch_view &bv, int64_t e, int ts, int k, int n, int m,
                              int T, int L, const int *s_assign, int ts_onehot) {
    const int groups = m / VEC;
    const int64_t os = bv.obs.stride[3];
    for (int idx = threadIdx.x; idx < n * groups; idx += blockDim.x) {
        const int i = idx / groups;
        const int j0 = (idx - i * groups) * VEC;
        const int a = s_assign ? s_assign[i] : -1;
        float oh[VEC];
        typename EnvB::Pair P[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) oh[q] = (a == j0 + q) ? 1.0f : 0.0f;
        if constexpr (VEC == 4) {
            src.pair4(i, j0, P);
        } else {
#pragma unroll
            for (int q = 0; q < VEC; ++q) P[q] = src.pair(i, j0 + q);
        }
        float *ob = fptr<float>(bv.obs, e, ts, i, j0);
        if (VEC == 4) {
            *reinterpret_cast<float4 *>(ob) = make_float4(oh[0], oh[1], oh[2], oh[3]);
        } else {
            for (int q = 0; q < VEC; ++q) ob[q * os] = oh[q];
        }
        float b0[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) b0[q] = 0.0f;
        for (int l = 0; l < L; ++l) {
            const int t = k + l;
            float val[VEC];
#pragma unroll
            for (int q = 0; q < VEC; ++q) val[q] = (t < T) ? (float)P[q].at(t) : 0.0f;
            if (l == 0) {
#pragma unroll
                for (int q = 0; q < VEC; ++q) b0[q] = val[q];
            }
            float *o = ob + (int64_t)m * (l + 1) * os;
            if (VEC == 4) {
                *reinterpret_cast<float4 *>(o) = make_float4(val[0], val[1], val[2], val[3]);
            } else {
                for (int q = 0; q < VEC; ++q) o[q * os] = val[q];
            }
        }
        if (L == 0 && k < T) {
#pragma unroll
            for (int q = 0; q < VEC; ++q) b0[q] = (float)P[q].at(k);
        }
        if (bv.beta.ptr) {
            float *bp = fptr<float>(bv.beta, e, ts, i, j0);
            if (VEC == 4) {
                *reinterpret_cast<float4 *>(bp) = make_float4(b0[0], b0[1], b0[2], b0[3]);
            } else {
                for (int q = 0; q < VEC; ++q) bp[q * bv.beta.stride[3]] = b0[q];
            }
        }
        if (bv.avail_actions.ptr) {
            uint8_t *ap = fptr<uint8_t>(bv.avail_actions, e, ts, i, j0);
            if (VEC == 4) {
                *reinterpret_cast<uint32_t *>(ap) = 0x01010101u;
            } else {
                for (int q = 0; q < VEC; ++q) ap[q * bv.avail_actions.stride[3]] = 1;
            }
        }
        if (ts_onehot >= 0 && bv.actions_onehot.ptr) {
            int64_t *hp = fptr<int64_t>(bv.actions_onehot, e, ts_onehot, i, j0);
            if (VEC == 4) {
                reinterpret_cast<longlong2 *>(hp)[0] = make_longlong2(a == j0, a == j0 + 1);
                reinterpret_cast<longlong2 *>(hp)[1] = make_longlong2(a == j0 + 2, a == j0 + 3);
            } else {
                for (int q = 0; q < VEC; ++q) hp[q * bv.actions_onehot.stride[3]] = (a == j0 + q);
            }
        }
    }
}

// ------------------------------------------------------------------------------------
// the pieces of reset and transition shared by the per-step kernels (reset_kernel, step_kernel,
// random_actions_kernel) and the episode launch (random_rollout_kernel).  The callers differ only
// in where an env's prev_assigns and return live -- st.prev / st.returns in HBM, or LDS across
// the steps of one launch -- so both are passed by reference: no mode flag.  The loops over the
// agents stay in the kernels: st.prev[e * n + i] formed inside the i < n loop lets the compiler
// use n > 0 for e * n, which a pointer or row index formed ahead of the loop does not (measured
// on step_kernel's code, profiles/env_split_ab.txt).
// ------------------------------------------------------------------------------------
// perm[0..m) (LDS) = Fisher-Yates from the top, Philox-drawn by one thread (distribution of
// choice(m, n, False)); the caller syncs before reading it
__device__ __forceinline__ void philox_perm_lds(int *perm, const EnvState &st, int64_t e) {
    const int m = st.m;
    for (int j = threadIdx.x; j < m; j += blockDim.x) perm[j] = j;
    __syncthreads();
    if (threadIdx.x == 0) {
        const EnvKey key = env_key(st.seed, st.env_base + e);
        for (int i = m - 1; i >= 1; --i) {
            const u32x4 r = philox4x32_10(u32x4{(uint32_t)i, 0u, kCtrPerm, st.episode}, key.k0, key.k1);
            const int jj = (int)(((uint64_t)r.x * (uint64_t)(i + 1)) >> 32);
            const int t = perm[i];
            perm[i] = perm[jj];
            perm[jj] = t;
        }
    }
}

// the uniform policy's action of agent i at step k
__device__ __forceinline__ uint32_t philox_action(const EnvKey &key, uint32_t episode, int i, int k, int m) {
    const u32x4 r = philox4x32_10(u32x4{(uint32_t)i, (uint32_t)k, kCtrAction, episode}, key.k0, key.k1);
    return (uint32_t)(((uint64_t)r.x * (uint64_t)m) >> 32);
}

// agent i's reward (mock :126-138) for its action j, with the per-task counts s_cnt [m]:
// only the chosen task's beta_hat is needed.  Writes s_rew[i], the reward of row ts and the
// prev_assigns of row ts + 1, and moves `prev`, the agent's previous assignment, to the action.
template <class EnvB>
__device__ __forceinline__ void transition_reward(const EnvB &env, const asg_batch_view &bv, const EnvState &st,
                                                  int64_t e, int ts, int k, int i, int j, const int *s_cnt, int &prev,
                                                  double *s_rew) {
    const int p = prev;
    const double beta = env.pair(i, j).at64(k);  // float64: mask and reward exact on the parameters
    const double tt = st.T_trans ? st.T_trans[(int64_t)p * st.m + j] : (j == p ? 0.0 : 1.0);
    const double pen = tt * (beta > 1e-12 ? 1.0 : 0.0);
    const double bh = beta - st.lambda_ * pen;
    const double r = bh > 0.0 ? bh / (double)s_cnt[j] : bh;
    s_rew[i] = r;
    if (bv.rewards.ptr) *fptr<float>(bv.rewards, e, ts, i, 0) = (float)r;
    prev = j;
    if (bv.prev_assigns.ptr)
        *fptr<int64_t>(bv.prev_assigns, e, ts + 1, i, 0) = (st.quirks & ASG_QUIRK_PREV_ASSIGNS_ZERO) ? 0 : j;
}

// the step's tail, by one thread after a sync: episode_return += sum(rewards) (Python sums the
// float64 list left to right), terminated of row ts, filled of row ts + 1
__device__ __forceinline__ void transition_tail(const asg_batch_view &bv, const EnvState &st, int64_t e, int ts, int k,
                                                const double *s_rew, double &ret) {
    double s = 0.0;
    for (int i = 0; i < st.n; ++i) s += s_rew[i];
    ret += s;
    bool term = k + 1 >= st.T;  // terminated = done != info.get("T", False)
    if (st.quirks & ASG_QUIRK_PARALLEL_TERMINATED) term = (e != 0);
    if (bv.terminated.ptr) *fptr<uint8_t>(bv.terminated, e, ts, 0, 0) = term;
    if (bv.filled.ptr) *fptr<int64_t>(bv.filled, e, ts + 1, 0, 0) = 1;
}

// ------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------
// float4 / uchar4 / 2x longlong2 row stores need unit inner stride, 4-element aligned
// outer strides and aligned base pointers
static bool vec4_ok(const asg_batch_view &b, int m) {
    auto al = [](const asg_field &f, uintptr_t bytes) {
        if (!f.ptr) return true;
        if (f.stride[3] != 1 || reinterpret_cast<uintptr_t>(f.ptr) % bytes) return false;
        return f.stride[0] % 4 == 0 && f.stride[1] % 4 == 0 && f.stride[2] % 4 == 0;
    };
    return m % 4 == 0 && al(b.obs, 16) && al(b.beta, 16) && al(b.avail_actions, 4) &&
           al(b.actions_onehot, 16);
}

static BumpSrc bump_src(const EnvState &st) {
    return BumpSrc{st.seed, st.env_base, st.episode, st.n, st.m, st.T, (float)st.wmin, (float)st.wmax,
                   st.benefit_mode == ASG_BENEFIT_DENSE};
}
static TableSrc table_src(const EnvState &st) { return TableSrc{st.table, st.n, st.m, st.T}; }
static ParSrc par_src(const EnvState &st) { return ParSrc{st.table32, st.mtpar, st.tmask, st.toff, st.n, st.m, st.T}; }

static bool uses_table(const EnvState &st) {
    return st.rng_mode == ASG_RNG_MT19937 || st.benefit_mode == ASG_BENEFIT_INJECTED;
}

// The one choice of benefit source, for every launcher: returns f(src) with the handle's ParSrc
// (MT19937 draws), TableSrc (injected table, under either generator) or BumpSrc (Philox).
// It rests on st.mtpar being non-null exactly when rng_mode is MT19937 and the table is not
// injected: asg_create allocates it under that condition alone (asg_abi.hip:176-181) and no
// other code assigns it.
template <class F>
static hipError_t with_src(const EnvState &st, F &&f) {
    if (st.mtpar) return f(par_src(st));
    if (uses_table(st)) return f(table_src(st));
    return f(bump_src(st));
}

}  // namespace asg
