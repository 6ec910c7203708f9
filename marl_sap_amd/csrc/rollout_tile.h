// rollout_tile.h -- one 32-agent tile of the fused rollout kernel: the observation row's
// stores, fc1 on the generated blocks, the recurrent layer, fc2 and the selection.  The env
// loops that call it are in rollout_kernel.h.
#pragma once
#include "rollout_env.h"
#include "rollout_rows.h"

#pragma clang fp contract(fast)

namespace asg {

// what a tile does for the next agent tile's h_t rows: loads them (HNext: one wave per env) ...
struct HNext {
    const float *src;
    int64_t stride, row0;
    int mode;
};
// ... or nothing (HKeep: a wave pair per env, rollout_envs_pair): a wave's next agent
// tile is the same 32 agents one step later, so hN takes h' in registers after the recurrent
// layer, and h' goes to Hout only when `store` says so (the launch's last agent pass).
struct HKeep {
    int store;
};

// One 32-agent tile of env e for observation row kk (batch row tsr): write the row (STORES:
// one-hot block and actions_onehot of the transition before it, avail, lookahead blocks,
// beta) and, AGENT, run fc1 on the generated blocks plus the recurrent layer, fc2 and the
// selection of row kk.  have_act: block 0 is onehot(s_act) (else zeros: the reset row).
// The agent tile's h_t rows (RNN): hN holds them on entry when the previous agent tile
// prefetched them (hpf), else they are loaded at the tile start; either way they are waited
// for with the one-hot gather, before the tile's stores (a wait after fc1 would drain every
// store of the tile: gfx9's vmcnt retires memory operations in order).  After the recurrent
// layer the tile issues the NEXT agent tile's h_t loads into hN (nx.src: its source rows, row
// nx.row0 on, stride nx.stride; NULL source = zeros; nx.mode 0 = no next agent tile in this env).
// With a wave pair per env (HKeep) hN instead takes this tile's h' in registers: hpf is true
// from the launch's second pass on and nothing is loaded.
// s_act: the env's tasks the row is built from; s_actw: where the selection puts the row's own
// (the same array with one wave per env; the next row of the task history with a wave pair).
// nx: HNext (run-time shapes), HKeep (SQ64).
//
// With W2 in LDS and an fc1 slice in L2 (64 x 64: 1 of 6; the SQ64 instances), that slice is
// the tile's first (w1_off = 1; as the last one its weights were read behind nearly all the
// tile's stores: 0.556-0.559 vs 0.575 ms/step; its rows stored after its MFMAs as well spilled
// 43 VGPRs and ran 0.65 ms).
template <bool RNN, bool W2L, bool GEN, int TAB, bool QOUT, bool AGENT, int SQ, class HX, class RA>
__device__ __forceinline__ void rollout_tile(RA &ra, int64_t e, int sub, int kk, int tsr, bool stores,
                                             bool have_act, int pass, const EnvKey &key, const uint64_t *s_scl,
                                             const uint16_t *s_act, uint16_t *s_actw, const u32x4v *Wl,
                                             const int (&sw)[4], f32x4 (&hN)[4][kH2NT], bool hpf, HX nx) {
    constexpr int NT = kH2NT;
    constexpr int RT = 16 * NT;  // rows per tile
    // opaque env / row indices and lane: addresses are formed here from them, not hoisted out
    // of the step and env loops (live across every tile they spill)
    asm volatile("" : "+s"(e), "+s"(tsr), "+s"(kk));
    int lane_ = threadIdx.x & 63;
    asm volatile("" : "+v"(lane_));
    const int lane = lane_, r = lane & 15, q = lane >> 4;
    const int n = rs_n<SQ>(ra), m = rs_m<SQ>(ra), T = ra.T, L = ra.L;
    const int K = m * (L + 1);
    const int Ub = rollout_mp(m) >> 5;
    const int64_t row0 = e * n + RT * sub;
    int64_t rows[NT];
    bool ok[NT];
    int ia[NT], act[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        ia[nt] = RT * sub + 16 * nt + r;
        ok[nt] = !GEN || ia[nt] < n;
        rows[nt] = e * n + ia[nt];
        act[nt] = (have_act && ok[nt]) ? (int)s_act[ia[nt]] : -1;
    }
    // the compact same-seed table's mask words / offsets of the lane's rows (chunk u's word is
    // u / 2): loaded here, with the gather, before the tile's stores -- once per tile when the
    // shape is compile-time 64 tasks (one word), per chunk otherwise
    constexpr bool cmp = TAB == 2;  // the compact same-seed table (MT19937 draws)
    uint64_t cmw[NT];
    int cof[NT];
    auto load_cm = [&](int w) {
        const int W = (m + 63) >> 6;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int64_t r = (e * n + (ok[nt] ? ia[nt] : 0)) * W + w;
            cmw[nt] = cmp ? ra.tmask[r] : 0ull;
            cof[nt] = cmp ? ra.toff[r] : 0;
        }
    };
    if (cmp && SQ == 64) load_cm(0);
    // The quad of tasks j0 .. j0 + 3 of the lane's row nt from the (env, t) slice `trow` of the
    // float32 table (the benefits rounded to the batch's dtype, as the separate step's rows: one
    // 16-byte load where the float64 table would take two behind the tile's stores): the 4 values
    // of the dense table, the packed bumps and their mask bits nb of the compact one
    // (compact_expand at the use)
    auto table_quad = [&](const float *trow, int j0, int nt, uint32_t &nb) {
        const float *tp = trow + (int64_t)ia[nt] * m + j0;
        if constexpr (cmp) {
            const f32x4 x = compact_quad_load(trow, cmw[nt], cof[nt], j0 & 63, ok[nt] && j0 < m, &nb);
            return make_float4(x.x, x.y, x.z, x.w);
        } else if (!GEN) {
            return *reinterpret_cast<const float4 *>(tp);
        } else {
            float v4[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) v4[v] = (ok[nt] && j0 + v < m) ? tp[v] : 0.f;
            return make_float4(v4[0], v4[1], v4[2], v4[3]);
        }
    };
    // row stores: batch row tsr (timing variant 32: row 1, env e & 7)
    const int tss = (ASG_ROLLOUT_XSKIP & 32) ? 1 : tsr;
    const int64_t sro = (ASG_ROLLOUT_XSKIP & 32) ? ((e & 7) - e) * n : 0;
    float *obs_r = ra.obs + ((int64_t)tss * ra.E * n + sro) * K;
    // fc1 accumulators start from the one-hot block's W1 columns, gathered (and consumed)
    // before the tile's stores (a load behind them would wait for their acknowledgements:
    // gfx9's vmcnt retires memory operations in order); a rescaled retry gathers again
    f32x4 acc[4][NT];
    int sx[NT];
    if (AGENT) {
        const float scS = pow2f(sw[0] + kH2SxInit);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            sx[nt] = kH2SxInit;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const float4 g = (act[nt] >= 0 && !(ASG_ROLLOUT_XSKIP & 2))
                                     ? *reinterpret_cast<const float4 *>(ra.W1T + act[nt] * kHid + 16 * mt + 4 * q)
                                     : make_float4(0.f, 0.f, 0.f, 0.f);
                acc[mt][nt] = f32x4{g.x, g.y, g.z, g.w} * scS;
            }
        }
    }
    if (AGENT && RNN) {
        if (!hpf) {
            const float *hin = pass == 0 ? ra.Hin : ra.Hout;
            const int64_t hs = pass == 0 ? ra.hs : kHid;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    hN[t][nt] = hin ? *reinterpret_cast<const f32x4 *>(hin + (ok[nt] ? rows[nt] : 0) * hs + 16 * t + 4 * q)
                                    : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        // waited for here, with the gather
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) asm volatile("" : "+v"(hN[t][nt]));
    }
    // w1_off (the SQ64 instances): the L2-resident fc1 slice is the tile's FIRST main slice, so
    // the wait for its weights covers only the prefix rows and the first block's rows of the
    // tile, not nearly all of its stores
    if (stores && !(ASG_ROLLOUT_XSKIP & 1)) {
        // obs block 0 = onehot(a) (row kk), actions_onehot (row kk - 1), avail = 1 (row kk)
        // actions_onehot of the transition before the row (none before the reset row)
        int64_t *oh_r = (ra.onehot && have_act) ? ra.onehot + ((int64_t)(tss - 1) * ra.E * n + sro) * m : nullptr;
        uint8_t *ab = ra.avail ? ra.avail + ((int64_t)tss * ra.E * n + sro + row0) * m : nullptr;
        // n = m = 64: the three as whole-line instructions; else in the generated blocks' layout
        if constexpr (SQ == 64)
            tile_action_rows64(obs_r + row0 * K, oh_r ? oh_r + row0 * m : nullptr, ab, K, s_act + RT * sub, have_act);
        for (int u = 0; u < (SQ == 64 ? 0 : Ub); ++u)
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int j0 = 32 * u + 16 * c + 4 * q;
                    const int aa = act[nt];
                    if (!GEN) {
                        st_f4(obs_r + rows[nt] * K + j0, aa == j0, aa == j0 + 1, aa == j0 + 2, aa == j0 + 3);
                        if (oh_r) {
                            st_i64x2(oh_r + rows[nt] * m + j0, aa == j0, aa == j0 + 1);
                            st_i64x2(oh_r + rows[nt] * m + j0 + 2, aa == j0 + 2, aa == j0 + 3);
                        }
                    } else if (ok[nt]) {
#pragma unroll
                        for (int v = 0; v < 4; ++v)
                            if (j0 + v < m) {
                                obs_r[rows[nt] * K + j0 + v] = aa == j0 + v ? 1.0f : 0.0f;
                                if (oh_r) oh_r[rows[nt] * m + j0 + v] = aa == j0 + v;
                            }
                    }
                }
        if (SQ != 64 && ab) {
            const int nrow = GEN ? min(RT, n - RT * sub) : RT;
            int off0 = (GEN ? 1 : 16) * lane;
            asm volatile("" : "+v"(off0));  // not hoisted: a per-lane 64-bit address kept across loops spilled
            if (!GEN) {
                // RT m = 1 KiB x Ub: a uniform trip count, 16 B per lane and whole lines per instruction
                for (int i = 0; i < Ub; ++i)
                    *reinterpret_cast<u32x4v *>(ab + 1024 * i + (uint32_t)off0) =
                        u32x4v{0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u};
            } else {
                for (int off = off0; off < nrow * m; off += 64) ab[off] = 1;
            }
        }
    }
    // ---- the lookahead blocks 1..L (times kk .. kk + L - 1), fc1 on them -------------------
    BumpShape bsh = bump_shape(T, ra.wmin, ra.wmax);
    bsh.q = __builtin_amdgcn_readfirstlane(bsh.q);  // uniform: keep the grid exponent scalar
    const lds_f4v Bs = (lds_f4v)(Wl + rec_f4(RNN));
    const u32x4v *W1g = ra.pk + 1;
    const int s0 = Ub, s_l2 = s0 + ra.w1_off + ra.w1_lds;
    float *beta_r = ra.beta ? ra.beta + ((int64_t)tss * ra.E * n + sro) * m : nullptr;
    const bool live = kk < T;  // rows past T are zeros: no bump parameters needed
    for (int attempt = 0;; ++attempt) {
        float scx[NT], rmax[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            scx[nt] = pow2f(AGENT ? sx[nt] : 0);
            rmax[nt] = 0.f;
        }
        if (AGENT && attempt > 0) {
            // a second copy of the gather above: merged (a lambda in any form), the retry keeps the
            // first attempt's values live and spills (the GRU pair instance: 0 -> 4 VGPRs)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const float scS = pow2f(sw[0] + sx[nt]);
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    const float4 g = act[nt] >= 0
                                         ? *reinterpret_cast<const float4 *>(ra.W1T + act[nt] * kHid + 16 * mt + 4 * q)
                                         : make_float4(0.f, 0.f, 0.f, 0.f);
                    acc[mt][nt] = f32x4{g.x, g.y, g.z, g.w} * scS;
                }
            }
        }
        const bool st_now = stores && attempt == 0 && !(ASG_ROLLOUT_XSKIP & 1);
        for (int u = 0; u < Ub; ++u) {
            // bump parameters of the lane's 16 (row, task) pairs of this chunk (Philox mode)
            Bump32 bp[2][4][NT];
            // table modes: the chunk's lookahead values of the first kTabPre blocks, loaded at
            // once at the chunk start (in place of the Philox parameters): one wait behind the
            // tile's stores per chunk instead of one per block (gfx9's in-order vmcnt)
            constexpr int kPre = TAB == 2 ? kTabPreCmp : kTabPre;
            float4 tv[kPre][2][NT];
            if (cmp && SQ != 64) load_cm(u >> 1);
            if constexpr (TAB != 0) {
#pragma unroll
                for (int l = 1; l <= kPre; ++l) {
                    const int t = kk + l - 1;
                    if (l > L || t >= T) continue;
                    const float *trow = ra.table32 + ((int64_t)e * T + t) * n * m;
#pragma unroll
                    for (int c = 0; c < 2; ++c)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) {
                            uint32_t nb;  // the compact table's packed bumps are expanded at their use
                            tv[l - 1][c][nt] = table_quad(trow, 32 * u + 16 * c + 4 * q, nt, nb);
                        }
                }
            }
            if constexpr (!TAB) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int jw = 32 * u + 16 * c + 4 * q;
                const uint64_t sbits = s_scl[jw >> 6];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    if (!live) {
#pragma unroll
                        for (int v = 0; v < 4; ++v) bp[c][v][nt] = Bump32{0.f, 0.f, 0.f};
                    } else if (ASG_ROLLOUT_XSKIP & 64) {
#pragma unroll
                        for (int v = 0; v < 4; ++v)
                            bp[c][v][nt] = Bump32{1.0f, (float)((jw + v + ia[nt]) & 15), 0.25f};
                    } else if (!GEN) {
                        // the lane's 4 pairs (j .. j + 3) are one Philox call (m % 4 == 0); their task
                        // scales from one 4-bit field of the scale bits (jw % 4 == 0: no wrap), each
                        // 1.0f or 10.0f as bits (0x3f800000 + b 0x01a00000)
                        float sv[4];
                        const uint32_t nib = (uint32_t)(sbits >> (jw & 63)) & 15u;
#pragma unroll
                        for (int v = 0; v < 4; ++v) sv[v] = __builtin_bit_cast(float, 0x3f800000u + ((nib >> v) & 1u) * 0x01a00000u);
                        Bump32 b4[4];
                        philox_bump32x4(key, ra.episode, ia[nt] * m + jw, sv, bsh, ra.dense != 0, b4);
#pragma unroll
                        for (int v = 0; v < 4; ++v) bp[c][v][nt] = b4[v];
                    } else {
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const int j = jw + v;
                            const bool in = j < m;
                            const float sv = ((sbits >> (j & 63)) & 1ull) ? 10.0f : 1.0f;
                            bp[c][v][nt] = philox_bump32(key, ra.episode, ia[nt] * m + (in ? j : 0), sv, bsh,
                                                         ra.dense != 0);
                            if (!in) bp[c][v][nt].scale = 0.f;
                        }
                    }
                }
            }
            }
            for (int l = 1; l <= L; ++l) {
                const int t = kk + l - 1;

                // the 2 x NT x 4 bump values, straight-line (one uniform branch per block: rows
                // past T are zeros)
                float4 xv[2][NT];
                if (TAB && t < T && l <= kPre) {
#pragma unroll
                    for (int c = 0; c < 2; ++c)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) {
                            // l is a loop variable: the preloaded block by a uniform select
                            float4 x = tv[0][c][nt];
#pragma unroll
                            for (int ll = 2; ll <= kPre; ++ll) x = l == ll ? tv[ll - 1][c][nt] : x;
                            if constexpr (cmp) {
                                const int j0 = 32 * u + 16 * c + 4 * q;
                                x = compact_expand(f32x4{x.x, x.y, x.z, x.w},
                                                   compact_nib(cmw[nt], j0 & 63, ok[nt] && j0 < m));
                            }
                            xv[c][nt] = x;
                        }
                } else if (TAB && t < T) {
                    const float *trow = ra.table32 + ((int64_t)e * T + t) * n * m;
#pragma unroll
                    for (int c = 0; c < 2; ++c)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) {
                            uint32_t nb;
                            const float4 x = table_quad(trow, 32 * u + 16 * c + 4 * q, nt, nb);
                            if constexpr (cmp) xv[c][nt] = compact_expand(f32x4{x.x, x.y, x.z, x.w}, nb);
                            else xv[c][nt] = x;
                        }
                } else if (!TAB && t < T) {
#pragma unroll
                    for (int c = 0; c < 2; ++c)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt)
                            xv[c][nt] = make_float4(bump32_at(bp[c][0][nt], t), bump32_at(bp[c][1][nt], t),
                                                    bump32_at(bp[c][2][nt], t), bump32_at(bp[c][3][nt], t));
                } else {
#pragma unroll
                    for (int c = 0; c < 2; ++c)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) xv[c][nt] = make_float4(0.f, 0.f, 0.f, 0.f);
                }
                auto store_rows = [&]() {
#pragma unroll
                    for (int c = 0; c < 2; ++c)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) {
                            const float vv[4] = {xv[c][nt].x, xv[c][nt].y, xv[c][nt].z, xv[c][nt].w};
                            const int j0 = 32 * u + 16 * c + 4 * q;
                            if (!GEN) {
                                st_f4(obs_r + rows[nt] * K + m * l + j0, vv[0], vv[1], vv[2], vv[3]);
                                if (l == 1 && beta_r) st_f4(beta_r + rows[nt] * m + j0, vv[0], vv[1], vv[2], vv[3]);
                            } else if (ok[nt]) {
#pragma unroll
                                for (int v = 0; v < 4; ++v)
                                    if (j0 + v < m) {
                                        obs_r[rows[nt] * K + m * l + j0 + v] = vv[v];
                                        if (l == 1 && beta_r) beta_r[rows[nt] * m + j0 + v] = vv[v];
                                    }
                            }
                        }
                };
                // an L2 weight slice (no W2 in LDS: the large shapes, 19 of 24 slices at 256 x 256):
                // its weights are loaded before this block's row stores and the stores follow the
                // MFMAs, so the loads wait for the previous block's stores only
                const bool late = !W2L && AGENT && l * Ub + u >= s_l2;
                if (st_now && !late) store_rows();
                if (AGENT) {
                    // the agent kernel's slice: abs-max, split, 4 output tiles x NT rows of MFMAs
                    const int sl = l * Ub + u;
                    u32x4v xp[NT][2];
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        rmax[nt] = absmax4(absmax4(rmax[nt], xv[0][nt]), xv[1][nt]);
                        const float x8[8] = {xv[0][nt].x, xv[0][nt].y, xv[0][nt].z, xv[0][nt].w,
                                             xv[1][nt].x, xv[1][nt].y, xv[1][nt].z, xv[1][nt].w};
                        split2s(x8, scx[nt], xp[nt][0], xp[nt][1]);
                    }
                    // two copies of the MFMA block: merged after an LDS-or-global select, the
                    // MFMAs would wait for vmcnt(0) -- every store of the tile -- each slice
                    auto mma = [&](bool lds) {
#pragma unroll
                        for (int mt = 0; mt < 4; ++mt) {
                            u32x4v w[2];
                            if (lds) {
                                const lds_u4p W1s = (lds_u4p)(Wl + lds_w1_off(RNN, (m + 15) / 16, W2L));
#pragma unroll
                                for (int pl = 0; pl < 2; ++pl)
                                    w[pl] = W1s[w1_idx((ASG_ROLLOUT_XSKIP & 4) && sl >= s_l2 ? 0 : sl - s0 - ra.w1_off, mt,
                                                       pl, lane)];
                            } else {
#pragma unroll
                                for (int pl = 0; pl < 2; ++pl) w[pl] = W1g[w1_idx(sl, mt, pl, lane)];
                            }
#pragma unroll
                            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = mfma_h2(w, xp[nt], acc[mt][nt]);
                        }
                    };
                    if ((sl >= s0 + ra.w1_off && sl < s_l2) || (ASG_ROLLOUT_XSKIP & 4))
                        mma(true);
                    else
                        mma(false);
                }
                if (st_now && late) store_rows();
            }
        }
        if (!AGENT) return;
        bool over[NT], any = false;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const float rm = row_max4(rmax[nt]);
            over[nt] = rm * scx[nt] >= 32768.f;
            any = any || over[nt];
            if (over[nt]) sx[nt] = h2_scale(rm, -90, 90 - sw[0]);
        }
        if (attempt > 0 || __ballot(any) == 0) break;
    }
    if constexpr (AGENT) {
        H2Args a = rollout_h2args<SQ>(ra);
        a.sel.counter = ra.counter + (uint32_t)pass;
        a.sel.out = ra.act + (int64_t)tsr * ra.E * n;
        if constexpr (QOUT) a.Q = ra.Q;
        float4 hB[4][NT];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                hB[t][nt] = (ASG_ROLLOUT_XSKIP & 8) ? make_float4(0.5f, 0.25f, -0.5f, 0.125f)
                            : RNN ? make_float4(hN[t][nt][0], hN[t][nt][1], hN[t][nt][2], hN[t][nt][3])
                                  : make_float4(0.f, 0.f, 0.f, 0.f);
        f32x4 xB[4][NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const float un = pow2f(-(sw[0] + sx[nt]));
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const f32x4 bb = Bs[4 * mt + q];
#pragma unroll
                for (int v = 0; v < 4; ++v) xB[mt][nt][v] = fmaxf(acc[mt][nt][v] * un + bb[v], 0.f);
            }
        }
        if constexpr (std::is_same<HX, HKeep>::value) {
            // the wave's next agent tile is this one a step later: its h_t is this h'
            auto keep = [&](const f32x4(&hp)[4][NT]) {
                if (!RNN) return;
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) hN[t][nt] = hp[t][nt];
            };
            h2_tail<NT, RNN, !QOUT, W2L, true, GEN, true>(a, Wl, sw, row0, rows, ok, hB, xB, s_actw, RT * sub, keep,
                                                          nx.store != 0);
        } else {
        // the next agent tile's h_t, issued once this tile's recurrent layer is done
        auto prefetch = [&](const auto &) {
            if (!RNN || nx.mode == 0) return;
            const int64_t nb = e * n + nx.row0;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int ni = (int)nx.row0 + 16 * nt + r;
                    const bool nok = !GEN || ni < n;
                    hN[t][nt] = nx.src ? *reinterpret_cast<const f32x4 *>(nx.src + (nok ? nb + 16 * nt + r : 0) * nx.stride +
                                                                        16 * t + 4 * q)
                                       : f32x4{0.f, 0.f, 0.f, 0.f};
                }
        };
        h2_tail<NT, RNN, !QOUT, W2L, true, GEN>(a, Wl, sw, row0, rows, ok, hB, xB, s_actw, RT * sub, prefetch);
        }
    }
}

}  // namespace asg
