// asg_real_haal.hip -- HAALSelector (action_selectors/non_rl_selectors.py:54-118) on a
// real-env handle's state (real_state.h; the env itself is asg_real.hip).
//
// The reference forks (deepcopy) every env once per time-interval sequence of the lookahead
// window, and per interval solves scipy's LSA on beta_hat summed over L and steps the fork
// interval-length times.  A fork's state is (step, previous assignment, and in the power /
// interference variants the power states, drained or recharged by every step the fork takes:
// real_power_constellation_env.py:137-191): the benefits are the constant table.  Sequences
// share prefixes, so the distinct LSA states form a tree of decision nodes (decision time t,
// the assignment in force before it = the parent node's, the power replayed along the
// ancestors' steps): 2^(eff-1) nodes, solved level by level as batched LSAs over all envs,
// then every sequence's value is the reference's sum of per-step reward sums (each variant's
// own reward rule, real_step_rewards).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <functional>
#include <vector>

#include "../../include/asg.h"
#include "asg_internal.h"
#include "real_state.h"

namespace asg {

constexpr int kHaalMaxL = 6;                     // 2^(6-1) = 32 nodes / sequences
struct HaalPlan {
    int nodes, seqs, eff;
    int8_t node_t[1 << (kHaalMaxL - 1)];         // decision time offset of each node
    int8_t node_parent[1 << (kHaalMaxL - 1)];    // parent node or -1 (root: the env's prev)
    int8_t seq_len[1 << (kHaalMaxL - 1)];        // intervals per sequence
    int8_t seq_node[1 << (kHaalMaxL - 1)][kHaalMaxL];  // the decision node of each interval
};
// host only (HaalPlan is a by-value kernel argument): nodes are numbered level by level
// (level = intervals up to and including the node's), level d is [start[d], start[d + 1])
struct HaalLevels {
    int count = 0;
    int start[kHaalMaxL + 1] = {};
};

// total beta_hat of one (node, env, agent) row: ((b0 - lambda * pen) + b1) + ... in numpy's
// order (real_constellation_env.py:309-326, then .sum(axis=-1) left to right).  Power variants
// (real_power_constellation_env.py:310-352, interference_constellation_env.py:355-406): the
// agent's power at the node's decision time, replayed from the env's along the ancestors'
// assignments; a row below 1e-12 power is all zeros; the interference variant's penalty mask is
// 1 - I whatever T_trans (interference_constellation_env.py:384).
__global__ void __launch_bounds__(256) haal_matrix_kernel(RealState st, int k, HaalPlan plan, int node0, int nodes,
                                                          const int64_t *assign, double *mats) {
    const int lane = threadIdx.x & 63;
    const int64_t gr = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // row over [nodes][E][n]
    const int n = st.n, m = st.m;
    if (gr >= (int64_t)nodes * st.E * n) return;
    const int i = (int)(gr % n);
    const int64_t ne = gr / n;
    const int64_t e = ne % st.E;
    const int node = node0 + (int)(ne / st.E);
    const int t = plan.node_t[node], par = plan.node_parent[node];
    const int prev = par < 0 ? st.prev[e * n + i] : (int)assign[((int64_t)par * st.E + e) * n + i];
    const double *tab = st.table + e * st.table_env_stride;
    double *row = mats + gr * m;
    bool poison = prev < 0 || prev >= m;
    bool dead = false;
    if (!poison && st.variant != ASG_REAL_PLAIN) {
        // the power this fork reaches at time t: the env's, then every step of the ancestors'
        // intervals (node chain root .. parent, each in force until its child's decision time)
        int chain[kHaalMaxL];
        int d = 0;
        for (int x = node; x >= 0 && d < kHaalMaxL; x = plan.node_parent[x]) chain[d++] = x;
        double p = st.power[e * n + i];
        for (int c = d - 1; c >= 1 && !poison; --c) {
            const int anc = chain[c];
            const int ai = (int)assign[((int64_t)anc * st.E + e) * n + i];
            if (ai < 0 || ai >= m) { poison = true; break; }
            for (int s2 = plan.node_t[anc]; s2 < plan.node_t[chain[c - 1]]; ++s2)
                if (p > 0) {  // real_power_update
                    if (real_beta(st, tab, k + s2, i, ai, 0) > 1e-12) {
                        p -= 0.2;
                    } else {
                        const double q = p + 0.1;
                        p = q < 1.0 ? q : 1.0;
                    }
                }
        }
        dead = p < 1e-12;  // np.where(sats_out_of_power, 0, beta_hat)
    }
    if (poison) {
        // the parent node's LSA failed (its assignment is -1 rows): poison this row so the
        // node's LSA reports invalid entries too, never index T_trans with it
        for (int j = lane; j < m; j += 64) row[j] = __builtin_nan("");
        return;
    }
    if (dead) {
        for (int j = lane; j < m; j += 64) row[j] = 0.0;
        return;
    }
    const bool eye = st.variant == ASG_REAL_INTERFERENCE;
    for (int j = lane; j < m; j += 64) {
        double s = real_beta(st, tab, k + t, i, j, 0);
        const double b0 = s;
        for (int l = 1; l < st.L; ++l) s = s + real_beta(st, tab, k + t, i, j, l);
        const double cond = s > 1e-12 ? 1.0 : 0.0;
        const double pen = (eye ? (prev != j ? 1.0 : 0.0) : st.T_trans[(int64_t)prev * m + j]) * cond;
        double tot = b0 - st.lambda_ * pen;
        for (int l = 1; l < st.L; ++l) tot = tot + real_beta(st, tab, k + t, i, j, l);
        row[j] = tot;
    }
}

// value of every (env, sequence): sum over its steps of Python's sum(rewards) (agent order,
// float64), one workgroup per (sequence, env), each step by the variant's own reward rule and,
// in the power variants, the fork's power carried from step to step; then (a second launch)
// the best sequence per env
__host__ __device__ __forceinline__ size_t haal_values_lds(int n, int m) {
    return (size_t)16 * n + (size_t)4 * (3 * n + m) + 16;  // rewards, power | tasks, prev, applicable, counts, flag
}

__global__ void __launch_bounds__(256) haal_values_kernel(RealState st, int k, HaalPlan plan, const int64_t *assign,
                                                          double *values) {
    extern __shared__ double s_rew[];  // [n] rewards, [n] power, then ints: [n] tasks, [n] prev, [n] applicable, [m] counts
    const int n = st.n, m = st.m;
    double *spw = s_rew + n;
    int *sa = reinterpret_cast<int *>(spw + n);
    int *sp = sa + n, *sapp = sp + n, *scnt = sapp + n;
    int *sbad = scnt + m;
    const int s = blockIdx.x % plan.seqs;
    const int64_t e = blockIdx.x / plan.seqs;
    const double *tab = st.table + e * st.table_env_stride;
    for (int i = threadIdx.x; i < n; i += blockDim.x) spw[i] = st.variant != ASG_REAL_PLAIN ? st.power[e * n + i] : 1.0;
    double tot = 0.0;
    bool bad = false;
    for (int iv = 0; iv < plan.seq_len[s] && !bad; ++iv) {
        const int node = plan.seq_node[s][iv];
        const int t0 = plan.node_t[node];
        const int t1 = iv + 1 < plan.seq_len[s] ? plan.node_t[plan.seq_node[s][iv + 1]] - 1 : plan.eff - 1;
        const int64_t *A = assign + ((int64_t)node * st.E + e) * n;
        const int par = plan.node_parent[node];
        for (int t = t0; t <= t1; ++t) {
            if (threadIdx.x == 0) *sbad = 0;
            __syncthreads();
            for (int i = threadIdx.x; i < n; i += blockDim.x) {
                // the previous assignment: the parent's on the interval's first step, then A
                const int p = t > t0 ? (int)A[i]
                                     : (par < 0 ? st.prev[e * n + i] : (int)assign[((int64_t)par * st.E + e) * n + i]);
                const int c = (int)A[i];
                sa[i] = c;
                sp[i] = p;
                if (c < 0 || c >= m || p < 0 || p >= m) *sbad = 1;
            }
            __syncthreads();
            if (*sbad) {
                // a failed LSA upstream (-1 assignment rows): the sequence's value is NaN and
                // the env's status carries the LSA error
                bad = true;
                break;
            }
            real_step_rewards(st, tab, k + t, sa, [&](int i) { return sp[i]; }, spw, scnt, sapp, s_rew);
            __syncthreads();
            if (threadIdx.x == 0) {
                double r = 0.0;
                for (int i = 0; i < n; ++i) r += s_rew[i];  // sum(rewards), left to right
                tot += r;                                   // total_tis_value += sum(rewards)
            }
            if (st.variant != ASG_REAL_PLAIN) real_power_update(st, tab, k + t, sa, spw);
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) values[e * plan.seqs + s] = bad ? __builtin_nan("") : tot;
}

// per env: the first sequence with the largest value (strict >), its first-interval
// assignment (the root node's: every sequence starts at the fork state) as float task ids
__global__ void haal_pick_kernel(int64_t E, int n, int seqs, const double *values, const int64_t *assign,
                                 const int32_t *lsa_status, float *col_out, int32_t *best_out, int32_t *status_out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    double best = -INFINITY;
    int bs = -1;
    for (int s = 0; s < seqs; ++s) {
        const double v = values[e * seqs + s];
        if (v > best) {
            best = v;
            bs = s;
        }
    }
    if (best_out) best_out[e] = bs;
    int32_t st = lsa_status ? lsa_status[e] : 0;
    if (st == 0 && bs < 0) st = ASG_E_INVALID_ARG;  // every value NaN: the reference's best_assignment is None
    if (status_out) status_out[e] = st;
    for (int i = 0; i < n; ++i) col_out[e * n + i] = (st == 0) ? (float)assign[e * n + i] : -1.0f;
}

// min over the levels' LSA status words of each env ([levels' B] -> [E])
__global__ void haal_status_kernel(const int32_t *st_all, int64_t rows, int64_t E, int32_t *st_env) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    int32_t v = 0;
    for (int64_t r = e; r < rows; r += E) v = st_all[r] < v ? st_all[r] : v;
    st_env[e] = v;
}

}  // namespace asg

// the decision tree and sequence list of HAALSelector's window (utils/methods.py:309-349:
// sequences depth first, the shorter first interval first)
static void haal_plan(int eff, asg::HaalPlan &p, asg::HaalLevels &lv) {
    std::vector<std::vector<int>> seqs;  // decision times of each sequence
    std::vector<int> cur;
    std::function<void(int)> rec = [&](int last) {
        if (last == eff - 1) {
            seqs.push_back(cur);
            return;
        }
        for (int j = last + 1; j < eff; ++j) {
            cur.push_back(last + 1);
            rec(j);
            cur.pop_back();
        }
    };
    rec(-1);
    // nodes = distinct decision-time prefixes, numbered level by level
    std::vector<std::vector<int>> nodes;
    lv.count = eff;
    for (int lev = 1; lev <= eff; ++lev) {
        lv.start[lev - 1] = (int)nodes.size();
        for (const auto &sq : seqs)
            if ((int)sq.size() >= lev) {
                std::vector<int> pre(sq.begin(), sq.begin() + lev);
                if (std::find(nodes.begin(), nodes.end(), pre) == nodes.end()) nodes.push_back(pre);
            }
    }
    lv.start[eff] = (int)nodes.size();
    p.eff = eff;
    p.nodes = (int)nodes.size();
    p.seqs = (int)seqs.size();
    for (int a = 0; a < p.nodes; ++a) {
        p.node_t[a] = (int8_t)nodes[a].back();
        std::vector<int> par(nodes[a].begin(), nodes[a].end() - 1);
        p.node_parent[a] = (int8_t)(par.empty() ? -1 : std::find(nodes.begin(), nodes.end(), par) - nodes.begin());
    }
    for (int s = 0; s < p.seqs; ++s) {
        p.seq_len[s] = (int8_t)seqs[s].size();
        for (size_t j = 0; j < seqs[s].size(); ++j) {
            std::vector<int> pre(seqs[s].begin(), seqs[s].begin() + j + 1);
            p.seq_node[s][j] = (int8_t)(std::find(nodes.begin(), nodes.end(), pre) - nodes.begin());
        }
    }
}

extern "C" {

int asg_real_haal_num_sequences(const asg_real_handle *h) {
    if (!h) return rfail(nullptr, ASG_E_INVALID_ARG, "NULL handle");
    const int eff = std::min(h->st.L, h->st.T - h->k);
    return eff > 0 ? 1 << (eff - 1) : 0;
}

int asg_real_haal_select(asg_real_handle *h, float *col_out, double *values_out, int32_t *best_out,
                         int32_t *status_out) {
    if (!h || !col_out) return rfail(h, ASG_E_INVALID_ARG, "NULL handle or output");
    if (!h->has_reset) return rfail(h, ASG_E_STATE, "asg_real_haal_select before asg_real_reset");
    const asg::RealState &st = h->st;
    const int eff = std::min(st.L, st.T - h->k);
    if (eff <= 0) return rfail(h, ASG_E_STATE, "asg_real_haal_select: the episode is done");
    if (eff > asg::kHaalMaxL) return rfail(h, ASG_E_INVALID_ARG, "asg_real_haal_select: lookahead window > 6");
    asg::HaalPlan plan{};
    asg::HaalLevels lv;
    haal_plan(eff, plan, lv);
    asg::DeviceGuard g(h->device);
    const int n = st.n, m = st.m;
    const int64_t E = st.E;
    int max_level = 0;  // nodes of the largest level
    for (int d = 0; d < lv.count; ++d) max_level = std::max(max_level, lv.start[d + 1] - lv.start[d]);
    // workspace: matrices of the largest level, all nodes' assignments, values, LSA status
    const size_t mats_b = sizeof(double) * (size_t)max_level * E * n * m;
    const size_t asg_b = sizeof(int64_t) * (size_t)plan.nodes * E * n;
    const size_t val_b = sizeof(double) * (size_t)E * plan.seqs;
    const size_t st_b = sizeof(int32_t) * (size_t)plan.nodes * E;
    const size_t need = mats_b + asg_b + val_b + st_b + 4 * 256;
    hipError_t e = hipSuccess;
    if (h->haal_ws_bytes < need) {
        e = hipStreamSynchronize(h->stream);
        (void)hipFree(h->haal_ws);
        h->haal_ws = nullptr;
        h->haal_ws_bytes = 0;
        if (e == hipSuccess) e = hipMalloc(&h->haal_ws, need);
        if (e != hipSuccess) return rhip(h, e, "asg_real_haal_select (workspace)");
        h->haal_ws_bytes = need;
    }
    auto align = [](size_t x) { return (x + 255) & ~(size_t)255; };
    char *base = static_cast<char *>(h->haal_ws);
    double *mats = reinterpret_cast<double *>(base);
    int64_t *assign = reinterpret_cast<int64_t *>(base + align(mats_b));
    double *values = reinterpret_cast<double *>(base + align(mats_b) + align(asg_b));
    int32_t *lsa_st = reinterpret_cast<int32_t *>(base + align(mats_b) + align(asg_b) + align(val_b));
    for (int d = 0; d < lv.count && e == hipSuccess; ++d) {  // one matrix launch + one batched LSA per level
        const int node0 = lv.start[d], cnt = lv.start[d + 1] - node0;
        const int64_t rows = (int64_t)cnt * E * n;
        hipLaunchKernelGGL(asg::haal_matrix_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, h->stream, st,
                           h->k, plan, node0, cnt, assign, mats);
        e = hipGetLastError();
        if (e == hipSuccess) {
            const int64_t strides[3] = {(int64_t)n * m, m, 1};
            e = asg::launch_lsa_batched(mats, ASG_F64, strides, (int64_t)cnt * E, n, m, 1, nullptr,
                                        assign + (int64_t)node0 * E * n, lsa_st + (int64_t)node0 * E, h->stream);
        }
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(asg::haal_values_kernel, dim3((unsigned)(E * plan.seqs)), dim3(256),
                           asg::haal_values_lds(n, m), h->stream, st, h->k, plan, assign, values);
        e = hipGetLastError();
    }
    int32_t *st_env = lsa_st;  // reduced in place into the first E words (row e is env e of level 0)
    if (e == hipSuccess) {
        hipLaunchKernelGGL(asg::haal_status_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, h->stream, lsa_st,
                           (int64_t)plan.nodes * E, E, st_env);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(asg::haal_pick_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, h->stream, E, n,
                           plan.seqs, values, assign, st_env, col_out, best_out, status_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess && values_out)
        e = hipMemcpyAsync(values_out, values, val_b, hipMemcpyDeviceToDevice, h->stream);
    return e == hipSuccess ? ASG_OK : rhip(h, e, "asg_real_haal_select");
}

}  // extern "C"
