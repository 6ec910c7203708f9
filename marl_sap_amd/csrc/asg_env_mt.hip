// asg_env_mt.hip -- the mock env's MT19937 compat mode: numpy's legacy stream per env (state
// [E][625] in HBM: key + pos), one wave per env.  Seeding, the reset's draws (benefit-table
// bumps and the permutation, in the reference's order), the compact float32 table written from
// them, and the stream skip.  Reference: envs/mock_constellation_env.py:32-37, :99-105 and
// :276-299 under np.random.seed(seed).
#include "asg_device.h"
#include "asg_internal.h"
#include "mt19937.h"

namespace asg {

__global__ void mt_seed_kernel(uint32_t *mt, int64_t E, uint64_t seed, int64_t base, bool replicate) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    uint32_t *key = mt + e * (kMtN + 1);
    uint32_t s = (uint32_t)(replicate ? seed : seed + (uint64_t)(base + e));
    key[0] = s;
    for (int i = 1; i < kMtN; ++i) {
        s = 1812433253u * (s ^ (s >> 30)) + (uint32_t)i;
        key[i] = s;
    }
    key[kMtN] = kMtN;  // pos
}

// generate_benefits_over_time + permutation in MT compat mode, the draws half: one wave per
// env consumes its MT19937 stream in the reference's order (mock :276-299, :105) and records
// each (agent, task) bump of the reset's table -- center and spread, the scale as the sign of spread,
// (0, 0) for no bump -- in par [E][m][n] (draw order: one coalesced 1 KiB store per 64 agents
// of a task); mt_table_kernel then writes the table from them with whole-row stores.
// construct: also replay the throwaway __init__ table draw (mock :34) first.
// bumps resolved per LDS round trip of the draw loop's bump search
constexpr int kMtBumps = 8;
// numpy's random_sample() from words (a, b) is ((a >> 5) 2^26 + (b >> 6)) 2^-53 exactly: r > 0.75
// (mock :283) is an integer test on the 53-bit numerator against 3 2^51
__device__ __forceinline__ bool mt_r_above_075(uint32_t a, uint32_t b) {
    const uint32_t hi = a >> 5, lo = b >> 6;
    return hi > (3u << 25) || (hi == (3u << 25) && lo != 0u);
}
__global__ void __launch_bounds__(64) mt_reset_kernel(uint32_t *mtstate, EnvState st, double2 *par, bool construct,
                                                       bool generate) {
    extern __shared__ uint32_t s_mt[];
    uint32_t *key = s_mt, *key2 = s_mt + kMtN, *out = s_mt + 2 * kMtN;
    int *perm = reinterpret_cast<int *>(out + 2 * kMtN);
    const int64_t e = blockIdx.x;
    const int lane = threadIdx.x;
    const int n = st.n, m = st.m, T = st.T;
    uint32_t *g = mtstate + e * (kMtN + 1);
    for (int i = lane; i < kMtN; i += kWave) key[i] = g[i];
    wave_sync();
    MtStream mt{key, key2, out, 0};
    mt.init((int)g[kMtN]);
    double2 *pe = par ? par + e * (int64_t)n * m : nullptr;
    for (int pass = construct ? 0 : 1; generate && pass < 2; ++pass) {
        const double wmin = pass == 0 ? st.wmin_init : st.wmin;
        const double wmax = pass == 0 ? st.wmax_init : st.wmax;
        for (int j = 0; j < m; ++j) {
            // benefit_scale = choice([1, 1, 1, 10]): one word (randint(0, 4), mask 3), read with the
            // first chunk's words (the chunk's offsets start after it: o0)
            const double scale = (mt.word(0) & 3u) == 3u ? 10.0 : 1.0;
            int o0 = 1;
            for (int c0 = 0; c0 < n; c0 += kWave) {
                const int rows = min(n, c0 + kWave) - c0;
                // 1. which agents of the chunk have a bump (r > 0.75): lane l tests agent a0 + l with
                //    its two r words at o + 2 l + 4 s, s = the bumps before it among a0.., s <
                //    kMtBumps -- all read in one LDS round trip, the first hit at s = 0 is exact, the
                //    first after it at s = 1, ... (integer tests, no float64); no stream advance yet
                uint64_t bumps = 0;
                int o = o0, a0 = 0;  // o0 + the words consumed by agents 0 .. a0 - 1 of the chunk
                while (a0 < rows) {
                    uint32_t rw[2 * kMtBumps];
#pragma unroll
                    for (int q = 0; q < 2 * kMtBumps; ++q) rw[q] = mt.word(o + 2 * lane + 4 * (q >> 1) + (q & 1));
                    int lo = 0, found = 0;
                    bool done = false;
#pragma unroll
                    for (int sb = 0; sb < kMtBumps; ++sb) {
                        const uint64_t act = __ballot(lane + a0 < rows && lane >= lo && mt_r_above_075(rw[2 * sb], rw[2 * sb + 1]));
                        if (act == 0) {
                            done = true;
                            break;
                        }
                        const int k = __builtin_amdgcn_readfirstlane(__builtin_ctzll(act));
                        bumps |= 1ull << (a0 + k);
                        lo = k + 1;
                        found = sb + 1;
                    }
                    if (done) {  // agents a0 .. rows - 1: two words each, four more per bump
                        o += 2 * (rows - a0) + 4 * found;
                        a0 = rows;
                    } else {
                        o += 2 * lo + 4 * found;
                        a0 += lo;
                    }
                }
                // 2. every bump's center and spread read by its own lane: agent l's words start at
                //    o0 + 2 l + 4 (bumps before l); center ~ U(0, T), spread ~ U(wmin, wmax) (numpy's
                //    uniform(lo, hi) = lo + (hi - lo) * random_sample(), the scaling of MtStream::dbl)
                double2 mine = make_double2(0.0, 0.0);  // agent c0 + lane's bump on task j
                if ((bumps >> lane) & 1) {
                    const int sl = __builtin_amdgcn_mbcnt_hi((uint32_t)(bumps >> 32),
                                                             __builtin_amdgcn_mbcnt_lo((uint32_t)bumps, 0u));
                    const int w = o0 + 2 * lane + 4 * sl + 2;
                    const double center = 0.0 + ((double)T - 0.0) * MtStream::dbl(mt.word(w), mt.word(w + 1));
                    const double spread = wmin + (wmax - wmin) * MtStream::dbl(mt.word(w + 2), mt.word(w + 3));
                    mine = make_double2(center, scale == 10.0 ? -spread : spread);  // s2 in mt_table_kernel
                }
                mt.advance(o);
                o0 = 0;
                if (pass == 1 && pe && c0 + lane < n) pe[(int64_t)j * n + c0 + lane] = mine;
            }
        }
    }
    // prev_assigns = choice(m, n, replace=False) = permutation(m)[:n]  (mock :105)
    for (int j = lane; j < m; j += kWave) perm[j] = j;
    wave_sync();
    for (int i = m - 1; i >= 1; --i) {
        const int jj = (int)mt.interval((uint32_t)i);
        if (lane == 0) {
            const int t = perm[i];
            perm[i] = perm[jj];
            perm[jj] = t;
        }
        wave_sync();
    }
    for (int i = lane; i < n; i += kWave) st.prev[e * n + i] = perm[i];
    for (int i = lane; i < kMtN; i += kWave) g[i] = key[i];
    if (lane == 0) g[kMtN] = (uint32_t)mt.pos;
}

// the reset's table B[e][t][i][j] = mt_par_value(draw, t) (the reference's zeros + bumps, mock
// :276-299) rounded to float32, the rows' dtype, stored COMPACT: per (env, t) slice only the
// bump pairs (about one in four; every other value is exactly 0), in (agent, task) order, with
// their masks tmask [E][n][W] and each mask word's first compact index toff [E][n][W] -- the
// episode kernel then reads ~1/4 of a dense slice per lookahead block.  Per chunk of `rows`
// agents (rows * m <= 1024): the draws staged transposed in LDS, the chunk's pair masks built
// (LDS 64-bit OR) and the compact order listed; then one thread per bump evaluates its T values
// (the float64 sigma_2 once, the exp / division per value: for bumps only) and stores them
// straight into the T slices -- consecutive threads, consecutive compact indices.  The float64
// values are not stored: their readers evaluate them from the draws (ParSrc).
constexpr int kTableRows = 16;  // agents per chunk, at most
static int mt_table_rows(int m) {
    return m >= 1024 ? 1 : (1024 / m < kTableRows ? 1024 / m : kTableRows);
}
static size_t mt_table_lds(int R, int m) {
    const size_t W = (m + 63) / 64;
    return (sizeof(double2) + sizeof(int)) * (size_t)R * m + 8 + (sizeof(uint64_t) + sizeof(int)) * (size_t)R * W;
}
__global__ void __launch_bounds__(256) mt_table_kernel(const double2 *par, EnvState st, int R) {
    extern __shared__ double2 s_par[];                               // [R agents][m tasks]
    int *s_list = reinterpret_cast<int *>(s_par + R * st.m);         // the chunk's bumps, compact order
    const int W = (st.m + 63) >> 6;
    unsigned long long *s_mask = reinterpret_cast<unsigned long long *>(s_list + R * st.m + ((R * st.m) & 1));
    int *s_off = reinterpret_cast<int *>(s_mask + R * W);           // [R][W] compact index (chunk-relative)
    __shared__ int s_cnt;
    const int64_t e = blockIdx.x;
    const int n = st.n, m = st.m, T = st.T;
    const int64_t nm = (int64_t)n * m;
    const double2 *pe = par + e * nm;
    float *te = st.table32 + e * T * nm;
    uint64_t *gm = st.tmask + e * n * W;
    int *go = st.toff + e * n * W;
    int base = 0;  // the env's compact index of the chunk's first bump
    for (int i0 = 0; i0 < n; i0 += R) {
        const int rows = min(R, n - i0), ne = rows * m;
        __syncthreads();
        // par is [task][agent]: `rows` consecutive agents of a task are contiguous
        for (int idx = threadIdx.x; idx < ne; idx += blockDim.x) {
            const int ii = idx % rows, j = idx / rows;
            s_par[ii * m + j] = pe[(int64_t)j * n + i0 + ii];
        }
        for (int x = threadIdx.x; x < rows * W; x += blockDim.x) s_mask[x] = 0ull;
        __syncthreads();
        for (int idx = threadIdx.x; idx < ne; idx += blockDim.x)
            if (s_par[idx].y != 0.0) {
                const int ii = idx / m, j = idx - ii * m;
                atomicOr(&s_mask[ii * W + (j >> 6)], 1ull << (j & 63));
            }
        __syncthreads();
        if (threadIdx.x == 0) {  // exclusive prefix over the chunk's mask words, (agent, word) order
            int c = 0;
            for (int x = 0; x < rows * W; ++x) {
                s_off[x] = c;
                c += __popcll(s_mask[x]);
            }
            s_cnt = c;
        }
        __syncthreads();
        for (int x = threadIdx.x; x < rows * W; x += blockDim.x) {
            gm[(int64_t)i0 * W + x] = s_mask[x];
            go[(int64_t)i0 * W + x] = base + s_off[x];
        }
        // each bump's slot in the compact order
        for (int idx = threadIdx.x; idx < ne; idx += blockDim.x)
            if (s_par[idx].y != 0.0) {
                const int ii = idx / m, j = idx - ii * m, w = ii * W + (j >> 6);
                s_list[s_off[w] + __popcll(s_mask[w] & ((1ull << (j & 63)) - 1ull))] = idx;
            }
        __syncthreads();
        const int cnt = s_cnt;
        float *o = te + base;
        for (int k = threadIdx.x; k < cnt; k += blockDim.x) {
            const double2 p = s_par[s_list[k]];
            // mt_par_value(p, t) for every t, sigma_2 hoisted (the same float64 operations)
            const double scale = p.y < 0.0 ? 10.0 : 1.0, s2 = bump_s2(__builtin_fabs(p.y));
            for (int t = 0; t < T; ++t) o[(int64_t)t * nm + k] = (float)bump_value(scale, p.x, s2, t);
        }
        base += cnt;
    }
}

// skip `words` draws of every stream (other consumers of numpy's global stream): only the raw
// state moves -- a twist each time pos reaches the block's end, no word is tempered
__global__ void __launch_bounds__(64) mt_advance_kernel(uint32_t *mtstate, int64_t words) {
    extern __shared__ uint32_t s_mt[];  // [624] raw state
    uint32_t *key = s_mt;
    const int64_t e = blockIdx.x;
    uint32_t *g = mtstate + e * (kMtN + 1);
    for (int i = threadIdx.x; i < kMtN; i += kWave) key[i] = g[i];
    wave_sync();
    int pos = (int)g[kMtN];
    int64_t left = words;
    while (left > 0) {
        if (pos >= kMtN) {
            mt_twist_inplace(key);
            pos = 0;
        }
        const int64_t take = min<int64_t>(left, kMtN - pos);
        pos += (int)take;
        left -= take;
    }
    for (int i = threadIdx.x; i < kMtN; i += kWave) g[i] = key[i];
    if (threadIdx.x == 0) g[kMtN] = (uint32_t)pos;
}

// The MT19937 mode's reset without its row write: the draws (and the float32 table) only --
// the episode launch that follows writes the reset row (asg_reset_rollout in the same-seed mode).
// Two launches on the caller's stream: the draws (one wave per env, latency-bound: the
// sequential MT19937 consumption), then the table writer (float64 bump evaluations,
// compute-bound), every env in one launch each.  With an injected table (sat_prox_mat=) neither
// __init__ nor reset draw a table: only the permutation consumes the stream (mock :32-37,
// :99-105).
hipError_t launch_reset_draws(const EnvState &st, bool construct, hipStream_t s) {
    if (st.rng_mode != ASG_RNG_MT19937) return hipErrorInvalidValue;
    // the two raw blocks, their tempered copies and the permutation: 10,240 B at m = 64, exactly
    // 16 workgroups in a CU's 160 KiB (LDS in 512-byte granules)
    const size_t lds = sizeof(uint32_t) * 4 * kMtN + sizeof(int) * st.m;
    const bool gen = st.benefit_mode != ASG_BENEFIT_INJECTED;
    const int R = mt_table_rows(st.m);
    hipLaunchKernelGGL(mt_reset_kernel, dim3(st.E), dim3(64), lds, s, st.mt, st, st.mtpar, construct && gen, gen);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess || !gen) return err;
    hipLaunchKernelGGL(mt_table_kernel, dim3(st.E), dim3(256), mt_table_lds(R, st.m), s, st.mtpar, st, R);
    return hipGetLastError();
}

hipError_t launch_mt_seed(const EnvState &st, hipStream_t s) {
    const int64_t blocks = (st.E + 63) / 64;
    hipLaunchKernelGGL(mt_seed_kernel, dim3(blocks), dim3(64), 0, s, st.mt, st.E, st.seed, st.env_base,
                       (st.quirks & ASG_QUIRK_REPLICATE_STREAM) != 0);
    return hipGetLastError();
}

hipError_t launch_mt_advance(const EnvState &st, int64_t words, hipStream_t s) {
    hipLaunchKernelGGL(mt_advance_kernel, dim3(st.E), dim3(64), sizeof(uint32_t) * kMtN, s, st.mt, words);
    return hipGetLastError();
}

}  // namespace asg
