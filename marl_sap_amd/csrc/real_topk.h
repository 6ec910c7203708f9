// real_topk.h -- wave-wide top-K of a short list in LDS, used by the real env's strip kernel
// (each agent's ranked task lists) and observation kernel (the strongest competitors).
//
// Contract of all three functions (one wave; vals[0..len) in LDS, V = double or float):
//   order   value descending; equal values go to the lower index (HIGHER_TIES = false:
//           np.argsort(-x) stable) or to the higher index (HIGHER_TIES = true: the tail of an
//           ascending stable argsort)
//   NaN     a NaN value (an injected NaN benefit) compares with nothing: NaNs rank last, by
//           the index rule, so every pick stays a valid index
//   CAP     candidates per lane held in registers: CAP > 0 serves len <= 64 * CAP (chosen per
//           kernel instance so each gets its own register budget); CAP = 0 is any len, by K
//           rescans over a [len] byte scratch row (`taken`)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "asg_device.h"

namespace asg {

// wave-wide selection of the best remaining candidate (the CAP = 0 rescan)
template <bool HIGHER_TIES, class V = double>
__device__ __forceinline__ int wave_select(const V *vals, unsigned char *taken, int len) {
    const int lane = threadIdx.x & 63;
    V bv = -INFINITY;
    int bj = -1;
    for (int j = lane; j < len; j += 64) {
        if (taken[j]) continue;
        const V v = vals[j];
        const bool better = bj < 0 || v > bv || (v == bv && (HIGHER_TIES ? j > bj : j < bj));
        if (better) {
            bv = v;
            bj = j;
        }
    }
    const V vmax = wave_allreduce(bj >= 0 ? bv : (V)-INFINITY, [](V a, V b) { return a > b ? a : b; });
    int key;
    if (HIGHER_TIES) {
        key = wave_max_i32(bj >= 0 && bv == vmax ? bj : -1);
    } else {
        key = -wave_max_i32(bj >= 0 && bv == vmax ? -bj : -0x7fffffff);
    }
    return key;
}

// Top-K of vals[0..len) in the same order as K successive wave_select calls, for short
// lists (len <= 64 * CAP): every lane sorts its own CAP candidates (j = lane + 64 c) once,
// then keeps only their indices.  Each pick reads the lanes' list heads back from LDS and
// reduces float32-rounded keys (one DPP-fused max): rounding is monotone, so a unique
// maximal key is the unique float64 maximum; equal keys take the exact path (float64
// compare against the first candidate, then the index rule).  The winning lane shifts its
// index list -- no rescans.  (V = float: the keys are the values.)
// The picks go out 64 at a time, lane k holding pick k (one store instead of one per pick);
// the return value is lane k's pick k for k < min(K, 64) (-1 past K).  (Keeping float32
// values in registers beside the indices instead of re-reading them measured no faster.)
template <int CAP, bool HIGHER_TIES, class V = double>
__device__ __forceinline__ int wave_topk_heads(const V *vals, int len, int K, int *out) {
    const int lane = threadIdx.x & 63;
    int id[CAP];
    {
        V v[CAP];
#pragma unroll
        for (int c = 0; c < CAP; ++c) {
            const int j = lane + 64 * c;
            v[c] = j < len ? vals[j] : -INFINITY;
            id[c] = j < len ? j : -1;  // -1: no candidate (sorts last, never wins)
        }
        auto before = [](V va, int ia, V vb, int ib) {
            if (ia < 0) return false;
            if (ib < 0) return true;
            return va > vb || (va == vb && (HIGHER_TIES ? ia > ib : ia < ib));
        };
        auto cswap = [&](int a, int b) {  // a < b: a gets the one that comes first
            if (before(v[b], id[b], v[a], id[a])) {
                const V tv = v[a];
                v[a] = v[b];
                v[b] = tv;
                const int ti = id[a];
                id[a] = id[b];
                id[b] = ti;
            }
        };
        if constexpr (CAP == 6) {  // the 12-comparator network for 6 inputs
            constexpr int kNet6[12][2] = {{0, 5}, {1, 3}, {2, 4}, {1, 2}, {3, 4}, {0, 3},
                                          {2, 5}, {0, 1}, {2, 3}, {4, 5}, {1, 2}, {3, 4}};
#pragma unroll
            for (int q = 0; q < 12; ++q) cswap(kNet6[q][0], kNet6[q][1]);
        } else if constexpr (CAP == 8) {
            // the 19-comparator sorting network for 8 inputs (depth 6) in place of the
            // 28-comparator odd-even transposition sort: same order (a total order on (value, index))
            constexpr int kNet[19][2] = {{0, 2}, {1, 3}, {4, 6}, {5, 7}, {0, 4}, {1, 5}, {2, 6}, {3, 7}, {0, 1}, {2, 3},
                                         {4, 5}, {6, 7}, {2, 4}, {3, 5}, {1, 4}, {3, 6}, {1, 2}, {3, 4}, {5, 6}};
#pragma unroll
            for (int q = 0; q < 19; ++q) cswap(kNet[q][0], kNet[q][1]);
        } else {
#pragma unroll
            for (int pass = 0; pass < CAP; ++pass)  // odd-even transposition sort, fully unrolled
#pragma unroll
                for (int c = pass & 1; c + 1 < CAP; c += 2) cswap(c, c + 1);
        }
    }
    int mine = -1, first = -1;
    for (int k = 0; k < K; ++k) {
        const bool has = id[0] >= 0;
        const V x = has ? vals[id[0]] : (V)-INFINITY;
        const float key = has ? (float)x : -INFINITY;
        const float kmax = wave_max_f32_nonan(key);
        uint64_t cm = __ballot(has && key == kmax);
        // NaN values match no key: rank them last, by index
        if (cm == 0) cm = __ballot(has);
        int wl = (int)__builtin_ctzll(cm);  // winning lane
        if (__popcll(cm) != 1) {
            // equal keys: exact float64 maximum among them, then the index rule
            V vmax;
            if constexpr (sizeof(V) == 8) {
                const uint64_t xb = __builtin_bit_cast(uint64_t, x);
                const uint32_t lo0 = __builtin_amdgcn_readlane((int)(uint32_t)xb, wl);
                const uint32_t hi0 = __builtin_amdgcn_readlane((int)(uint32_t)(xb >> 32), wl);
                vmax = __builtin_bit_cast(V, (uint64_t)lo0 | ((uint64_t)hi0 << 32));
            } else {
                vmax = __builtin_bit_cast(V, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), wl));
            }
            uint64_t cand = cm;
            if ((__ballot(x != vmax) & cm) != 0) {
                const bool in = __builtin_amdgcn_inverse_ballot_w64(cm);
                vmax = wave_allreduce(in ? x : (V)-INFINITY, [](V a, V b) { return a > b ? a : b; });
                cand = __ballot(x == vmax) & cm;
            }
            if (cand == 0) cand = cm;  // NaN maximum: the index rule over all candidates
            const bool cb = __builtin_amdgcn_inverse_ballot_w64(cand);
            const int win = HIGHER_TIES ? wave_max_i32(cb ? id[0] : -1) : -wave_max_i32(cb ? -id[0] : -0x7fffffff);
            wl = (int)__builtin_ctzll(__ballot(has && id[0] == win));
        }
        const int win = __builtin_amdgcn_readlane(id[0], wl);
        if (lane == (k & 63)) mine = win;
        if ((k & 63) == 63 || k == K - 1) {
            if (lane <= (k & 63)) out[(k & ~63) + lane] = mine;
            if (k < 64) first = mine;
        }
        if (lane == wl) {
#pragma unroll
            for (int c = 0; c + 1 < CAP; ++c) id[c] = id[c + 1];
            id[CAP - 1] = -1;
        }
    }
    return K > 0 ? first : -1;
}

// top-K into out[0..K): register heads (CAP > 0), else K rescans (CAP = 0; taken: [len] scratch)
template <int CAP, bool HIGHER_TIES, class V = double>
__device__ __forceinline__ void wave_topk(const V *vals, int len, int K, int *out, unsigned char *taken) {
    if constexpr (CAP > 0) {
        (void)wave_topk_heads<CAP, HIGHER_TIES, V>(vals, len, K, out);
    } else {
        const int lane = threadIdx.x & 63;
        for (int j = lane; j < len; j += 64) taken[j] = 0;
        wave_sync();
        for (int c = 0; c < K; ++c) {
            const int j = wave_select<HIGHER_TIES, V>(vals, taken, len);
            if (lane == 0) {
                out[c] = j;
                taken[j] = 1;
            }
            wave_sync();
        }
    }
    wave_sync();
}

}  // namespace asg
