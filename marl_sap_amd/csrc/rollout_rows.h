// rollout_rows.h -- how the fused rollout kernel's tiles move batch rows: the wide stores, the
// whole-line stores of the rows that depend on the actions alone, and the compact same-seed
// table's quads.
#pragma once
#include "rollout_args.h"

#pragma clang fp contract(fast)

namespace asg {

__device__ __forceinline__ void st_f4(float *p, float a, float b, float c, float d) {
    *reinterpret_cast<f32x4 *>(p) = f32x4{a, b, c, d};
}
__device__ __forceinline__ void st_i64x2(int64_t *p, long long a, long long b) {
    *reinterpret_cast<i64x2v *>(p) = i64x2v{a, b};
}

// The rows of a 32-agent tile that depend on nothing but the tile's actions, n = m = 64 (the
// SQ64 instances): obs block 0 = onehot(a), actions_onehot (oh, NULL = none) and avail = 1 (av,
// NULL = none), every store instruction 1 KiB of whole lines instead of the MFMA operand layout
// of the generated blocks (16 rows x 64 B per instruction for block 0, 16-B pieces at a 32-B
// stride for the int64 one-hot).  Any lane can read any row's action from the wave's LDS:
//   actions_onehot: the tile's 32 rows x 512 B are one 16 KiB span; instruction i writes rows
//     2 i and 2 i + 1 whole: lane l takes row 2 i + (l >> 5), columns 2 (l & 31) and the next
//   obs block 0: instruction i writes rows 4 i .. 4 i + 3, 256 B each: lane l takes row
//     4 i + (l >> 4), columns 4 (l & 15) .. + 3
//   avail: the tile's 2 KiB, two instructions
// ob / oh / av: the tile's first row (wave-uniform), K the obs row length; sa: the tile's
// actions; have_act false (the reset row): block 0 is zeros.  The lane index is laundered
// here and every address is a uniform base plus a 32-bit lane offset: no per-lane 64-bit
// pointer to keep across tiles.
__device__ __forceinline__ void tile_action_rows64(float *ob, int64_t *oh, uint8_t *av, int K, const uint16_t *sa,
                                                   bool have_act) {
    constexpr int RT = 16 * kH2NT, M = 64;
    int lane = threadIdx.x & 63;
    asm volatile("" : "+v"(lane));
    {
        const int rl = lane >> 4, c0 = 4 * (lane & 15);
        const uint32_t lo = (uint32_t)(rl * K + c0);
        // no action: a column no action reaches (one select per tile; the LDS reads stay
        // unconditional, a branch per instruction would wait for each read on its own)
        const int cc = have_act ? c0 : 0x10000;
#pragma unroll
        for (int i = 0; i < RT / 4; ++i) {
            const int d = (int)sa[4 * i + rl] - cc;
            st_f4(ob + (uint32_t)(4 * i * K) + lo, d == 0, d == 1, d == 2, d == 3);
        }
    }
    if (oh) {
        const int rl = lane >> 5, c0 = 2 * (lane & 31);
        const uint32_t lo = (uint32_t)(2 * lane);
#pragma unroll
        for (int i = 0; i < RT / 2; ++i) {
            const int d = (int)sa[2 * i + rl] - c0;
            st_i64x2(oh + 2 * M * i + lo, d == 0, d == 1);
        }
    }
    if (av) {
        const uint32_t lo = (uint32_t)(16 * lane);
#pragma unroll
        for (int i = 0; i < RT * M / 1024; ++i)
            *reinterpret_cast<u32x4v *>(av + 1024 * i + lo) = u32x4v{0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u};
    }
}

// The compact same-seed table (RolloutArgs::tmask): the 4 tasks j0 .. j0 + 3 of a row (j0 % 4 == 0,
// one mask word) are the set bits `nib` of the row's mask word at sh = j0 % 64, and their values
// sit at consecutive compact indices from pos = the word's first index + the bumps below sh.  One
// 16-byte load at pos (4-byte aligned; nib == 0: no load) then the expansion below
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ f32x4 compact_quad_load(const float *slice, uint64_t mw, int off, int sh, bool okrow,
                                                   uint32_t *nib_out) {
    const uint32_t nib = okrow ? (uint32_t)(mw >> sh) & 15u : 0u;
    *nib_out = nib;
    if (nib == 0u) return f32x4{0.f, 0.f, 0.f, 0.f};
    const int pos = off + (int)__popcll(mw & ((1ull << sh) - 1ull));
    if (ASG_ROLLOUT_XSKIP & 2048) return f32x4{0.5f, 0.25f, 0.125f, (float)pos};
    const f32x4u x = *reinterpret_cast<const f32x4u *>(slice + pos);
    return f32x4{x.x, x.y, x.z, x.w};
}
__device__ __forceinline__ uint32_t compact_nib(uint64_t mw, int sh, bool okrow) {
    return okrow ? (uint32_t)(mw >> sh) & 15u : 0u;
}
// the quad's 4 values from its packed bumps x (value v = the (rank of v)-th packed one, 0 off the mask)
__device__ __forceinline__ float4 compact_expand(f32x4 x, uint32_t nib) {
    if (ASG_ROLLOUT_XSKIP & 4096) return make_float4(x.x, x.y, x.z, x.w + (float)nib);
    const bool b0 = nib & 1u, b1 = nib & 2u, b2 = nib & 4u, b3 = nib & 8u;
    const float a01 = b0 ? x.y : x.x, a12 = b0 ? x.z : x.y, a23 = b0 ? x.w : x.z;  // rank shifted by b0
    const float r2 = b1 ? a12 : a01;                                               // rank b0 + b1
    const float r3 = b2 ? (b1 ? a23 : a12) : (b1 ? a12 : a01);                     // rank b0 + b1 + b2
    return make_float4(b0 ? x.x : 0.f, b1 ? a01 : 0.f, b2 ? r2 : 0.f, b3 ? r3 : 0.f);
}

// The table modes load each chunk's first lookahead blocks at the chunk start: kTabPre blocks
// of the dense table, kTabPreCmp of the compact one (MT19937 draws; SQ64 GRU instance: 0 VGPRs
// spilled with 1 block, 51 with 2, 84 with 3; the dense instance: 36 / 19 / 36)
constexpr int kTabPre = 2;
constexpr int kTabPreCmp = 1;

}  // namespace asg
