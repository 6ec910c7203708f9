// lsa_wave.h -- one wave64 solves one rectangular linear sum assignment problem with
// exactly scipy's shortest-augmenting-path algorithm, tie rule and float64 operation
// order (scipy 1.15.3 `linear_sum_assignment`; restated in SURVEY.md Appendix B), so
// the assignments are bit-identical to the reference's scipy calls
// (mock_constellation_env.py:122, sap_selectors.py:32,90, non_rl_selectors.py:47).
//
// Parallelisation: lane l owns columns j = l + 64*c (c < CPL).  The serial scipy scan
// over `remaining` becomes: every lane relaxes its own columns, then one packed wave
// reduction picks the column the sequential scan would have picked:
//   lowest = min spc over remaining; candidates = remaining columns with spc == lowest;
//   if some candidate is unassigned: the candidate of LARGEST position in `remaining`
//   among the unassigned ones, else the candidate of SMALLEST position.
// `remaining` positions are tracked per column (pos), including scipy's
// swap-with-last removal, so ties resolve exactly as in the sequential code.
//
// The working matrix (already transposed so nr <= nc, and sign-flipped for maximize, as
// scipy does before solving) lives in registers for float32 problems up to 64 x 64
// (lsa_reg64.h, which has its own solver for them), else in LDS, else (large problems) is
// read in place from global memory.
#pragma once
#include "asg_device.h"

namespace asg {

// Row-major cost matrix in LDS (already transposed / sign-flipped)
template <typename CT>
struct DenseCost {
    static constexpr bool kInMemory = true;
    const CT *c;
    int nc;
    __device__ double operator()(int i, int j) const { return (double)c[(size_t)i * nc + j]; }
};

// Solve on the working matrix acc(i, j), i < nr <= nc <= 64*CPL (scipy's orientation).
// All per-row and per-column state lives in registers, distributed over the lanes
// (column j / row r in lane j%64, slot j/64); only the cost matrix may be in memory.
// Each augmenting-path step is: relax the lane's columns in float64 (scipy's operation
// order), one int32 min-reduction of the float32-rounded keys plus a ballot -- which
// settles the step whenever a single column attains the minimum key -- and otherwise the
// exact float64 minimum and scipy's tie rule by packed-key reduction.  Control flow is
// wave-uniform throughout (row, column and position indices are scalars).
// Returns 0 or ASG_E_LSA_INFEASIBLE; col4row[c] holds the column assigned to row
// lane + 64c.  All 64 lanes must call it with identical arguments.
template <int CPL, class Acc>
__device__ int lsa_solve_wave(const Acc &acc, int nr, int nc, int (&col4row)[CPL]) {
    const int lane = threadIdx.x & (kWave - 1);
    double v[CPL], u[CPL];
    int r4c[CPL], path[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        v[c] = 0.0;
        u[c] = 0.0;
        r4c[c] = -1;
        path[c] = -1;
        col4row[c] = -1;
    }
    for (int cur = 0; cur < nr; ++cur) {
        double spc[CPL];
        int pos[CPL];  // position in scipy's `remaining`, -1 once scanned (or absent)
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int j = lane + kWave * c;
            spc[c] = __builtin_inf();
            pos[c] = (j < nc) ? (nc - 1 - j) : -1;  // remaining[it] = nc - it - 1
        }
        int nrem = nc;
        double minv = 0.0;
        int i = cur, sink = -1;
        bool infeasible = false;
        do {
            i = __builtin_amdgcn_readfirstlane(i);
            const double ui = lane_get(u, i);
            float key[CPL];
            float kl = __builtin_inff();
#pragma unroll
            for (int c = 0; c < CPL; ++c) {
                const int j = lane + kWave * c;
                // branch-free over the lane's columns: scanned / absent ones are relaxed
                // too but neither updated nor keyed (+inf keys: a remaining column at
                // +inf ties with them and takes the exact path)
                const bool rem = pos[c] >= 0;
                // never read past a matrix in memory; register columns are always valid
                const double cij = (!Acc::kInMemory || j < nc) ? acc(i, j) : 0.0;
                const double r = ((minv + cij) - ui) - v[c];
                const bool upd = rem && r < spc[c];
                spc[c] = upd ? r : spc[c];
                path[c] = upd ? i : path[c];
                key[c] = rem ? (float)spc[c] : __builtin_inff();
                kl = c == 0 ? key[0] : __builtin_fminf(kl, key[c]);
            }
            const float kmin = wave_min_f32_nonan(kl);
            uint64_t cmsk[CPL];
            int total = 0;
#pragma unroll
            for (int c = 0; c < CPL; ++c) {
                cmsk[c] = __ballot(key[c] == kmin);
                total += __popcll(cmsk[c]);
            }
            if (total == 0) return ASG_E_LSA_INVALID;  // NaN keys (see lsa_solve_reg64)
            // first candidate (the selection when it is the only one)
            int src0 = 0, c0 = 0;
#pragma unroll
            for (int c = CPL - 1; c >= 0; --c) {
                if (cmsk[c] != 0) {
                    src0 = __builtin_ctzll(cmsk[c]);
                    c0 = c;
                }
            }
            double val0 = 0.0;
            int pos0 = 0;
#pragma unroll
            for (int c = 0; c < CPL; ++c) {
                if (c == c0) {
                    const uint64_t sb = __builtin_bit_cast(uint64_t, spc[c]);
                    const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)sb, src0);
                    const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(sb >> 32), src0);
                    val0 = __builtin_bit_cast(double, (uint64_t)lo | ((uint64_t)hi << 32));
                    pos0 = __builtin_amdgcn_readlane(pos[c], src0);
                }
            }
            double lowest = val0;
            int jsel = src0 + kWave * c0, psel = pos0;
            if (total != 1) {
                // Several columns share the minimum key.  Usually they hold exactly equal
                // float64 values (scipy's tie case: zero reduced costs, frequent with
                // correlated Q-values): check that against the first candidate's value,
                // then apply scipy's tie rule with one 32-bit max-reduction.  Otherwise
                // (distinct float64 values that round to one float32) take the exact
                // float64 minimum first.
                bool all_equal = true;
#pragma unroll
                for (int c = 0; c < CPL; ++c) all_equal &= (__ballot(spc[c] != val0) & cmsk[c]) == 0;
                if (!all_equal) {
                    double lo = __builtin_inf();
#pragma unroll
                    for (int c = 0; c < CPL; ++c)
                        if (pos[c] >= 0) lo = spc[c] < lo ? spc[c] : lo;
                    const uint64_t lb = __builtin_bit_cast(uint64_t, wave_min_f64(lo));  // uniform: pin to SGPRs
                    const uint32_t l0 = __builtin_amdgcn_readfirstlane((uint32_t)lb);
                    const uint32_t l1 = __builtin_amdgcn_readfirstlane((uint32_t)(lb >> 32));
                    lowest = __builtin_bit_cast(double, (uint64_t)l0 | ((uint64_t)l1 << 32));
                }
                // scipy's tie rule as a max-reduced 32-bit key over the candidates
                // (remaining columns at `lowest`):
                //   unassigned: 2^31 | pos        (the LARGEST position wins)
                //   assigned:   2^30 - pos        (else the SMALLEST position)
                uint32_t tk = 0;
#pragma unroll
                for (int c = 0; c < CPL; ++c) {
                    const bool cand = all_equal ? ((cmsk[c] >> lane) & 1) != 0 : (pos[c] >= 0 && spc[c] == lowest);
                    const uint32_t k = (r4c[c] == -1) ? (0x80000000u | (uint32_t)pos[c])
                                                      : ((1u << 30) - (uint32_t)pos[c]);
                    tk = (cand && k > tk) ? k : tk;
                }
                tk = __builtin_amdgcn_readfirstlane(wave_max_u32(tk));
                psel = (tk >> 31) ? (int)(tk & 0x7fffffffu) : (int)((1u << 30) - tk);
                // positions are distinct over the remaining columns: the owner is unique
#pragma unroll
                for (int c = 0; c < CPL; ++c) {
                    const uint64_t msk = __ballot(pos[c] == psel);
                    if (msk != 0) jsel = __builtin_ctzll(msk) + kWave * c;
                }
            }
            const int last = nrem - 1;
            // remaining[index] = remaining[--num_remaining]
#pragma unroll
            for (int c = 0; c < CPL; ++c)
                pos[c] = (lane + kWave * c == jsel) ? -1 : (pos[c] == last ? psel : pos[c]);
            --nrem;
            minv = lowest;
            const int owner = lane_get(r4c, jsel);
            // scipy: minVal == INFINITY (compared on the bits: a scalar compare)
            infeasible = __builtin_bit_cast(uint64_t, lowest) == 0x7ff0000000000000ull;
            if (owner == -1) sink = jsel;
            i = owner;
        } while (sink == -1 && !infeasible);
        if (infeasible) return ASG_E_LSA_INFEASIBLE;
        // dual update (scipy: u[cur] += minv; u[r] += minv - spc[col4row[r]] for the
        // other visited rows; v[j] -= minv - spc[j] for the scanned columns).  A row
        // r != cur was visited iff its matched column col4row[r] was scanned.
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int r = lane + kWave * c;
            const int jm = col4row[c];
            // gather (scanned, spc) of column jm from its owner lane; a column of the
            // matrix was scanned iff it left `remaining` (pos == -1)
            double spc_j = 0.0;
            int sc_j = 0;
#pragma unroll
            for (int c2 = 0; c2 < CPL; ++c2) {
                const double sv = __shfl(spc[c2], jm & 63, kWave);
                const int sb = __shfl(pos[c2], jm & 63, kWave) < 0;
                if (jm >= 0 && (jm >> 6) == c2) {
                    spc_j = sv;
                    sc_j = sb;
                }
            }
            if (r < nr) {
                if (r == cur) u[c] += minv;
                else if (jm >= 0 && sc_j) u[c] += minv - spc_j;
            }
        }
#pragma unroll
        for (int c = 0; c < CPL; ++c)
            if (pos[c] < 0 && lane + kWave * c < nc) v[c] -= minv - spc[c];
        // augment along path back to cur (uniform loop of lane reads/writes)
        int j = sink;
        while (true) {
            const int pi = lane_get(path, j);
            lane_set(r4c, j, pi);
            const int t = lane_get(col4row, pi);
            lane_set(col4row, pi, j);
            j = t;
            if (pi == cur) break;
        }
    }
    return ASG_OK;
}

// Stage C (input [nr0][nc0], strides in elements) into dst as scipy's working matrix:
// transposed when nr0 > nc0, negated for maximize.  Returns ASG_E_LSA_INVALID (wave
// uniform) when an entry is NaN or -inf after the sign flip.
template <typename IT, typename CT>
__device__ int lsa_stage_wave(const IT *C, int64_t rs, int64_t cs, int nr0, int nc0,
                              bool maximize, CT *dst) {
    const int lane = threadIdx.x & (kWave - 1);
    const bool tr = nc0 < nr0;
    const int nc = tr ? nr0 : nc0;
    int bad = 0;
    for (int idx = lane; idx < nr0 * nc0; idx += kWave) {
        const int r = idx / nc0, c = idx - r * nc0;
        CT x = (CT)C[r * rs + c * cs];
        if (maximize) x = -x;
        bad |= (x != x) || (x == -(CT)__builtin_inf());
        if (tr) dst[(size_t)c * nc + r] = x; else dst[(size_t)r * nc + c] = x;
    }
    wave_sync();
    return wave_or_i32(bad) ? ASG_E_LSA_INVALID : ASG_OK;
}

// scipy's output convention from the working solution: (arange(nr), col4row) or, when
// transposed, (col4row[argsort(col4row)], argsort(col4row)).  `mark` is LDS scratch of
// nr0 ints (only used when transposed).
template <int CPL>
__device__ void lsa_emit_wave(const int (&col4row)[CPL], int nr0, int nc0, int *mark, int64_t *row_out,
                              int64_t *col_out, float *colf_out) {
    const int lane = threadIdx.x & (kWave - 1);
    if (nc0 >= nr0) {
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int r = lane + kWave * c;
            if (r < nr0) {
                if (row_out) row_out[r] = r;
                if (col_out) col_out[r] = col4row[c];
                if (colf_out) colf_out[r] = (float)col4row[c];
            }
        }
        return;
    }
    // transposed: working rows are original columns (nc0 of them), col4row is the
    // original row matched to each original column; emit sorted by original row
    for (int r = lane; r < nr0; r += kWave) mark[r] = -1;
    wave_sync();
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        const int oc = lane + kWave * c;
        if (oc < nc0) mark[col4row[c]] = oc;
    }
    wave_sync();
    int base = 0;
    for (int r0 = 0; r0 < nr0; r0 += kWave) {
        const int r = r0 + lane;
        const bool has = r < nr0 && mark[r] >= 0;
        const uint64_t bal = __ballot(has);
        const int off = __popcll(bal & ((1ull << lane) - 1ull));
        if (has) {
            if (row_out) row_out[base + off] = r;
            if (col_out) col_out[base + off] = mark[r];
            if (colf_out) colf_out[base + off] = (float)mark[r];
        }
        base += __popcll(bal);
    }
}

}  // namespace asg
