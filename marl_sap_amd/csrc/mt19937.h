// mt19937.h -- numpy's legacy MT19937 stream, wave-cooperative in LDS (the mock env's same-seed
// compat mode, asg_env_mt.hip): the recurrence, the tempering and the two-block stream view.
#pragma once
#include "asg_device.h"

namespace asg {

constexpr int kMtN = 624, kMtM = 397;

// the recurrence over one 624-word block k (LDS), in place, by one wave: 3 dependency phases
// plus the last word
__device__ __forceinline__ void mt_twist_inplace(uint32_t *k) {
    const int lane = threadIdx.x & (kWave - 1);
    auto gen = [&](uint32_t ki, uint32_t ki1, uint32_t kim) {
        const uint32_t y = (ki & 0x80000000u) | (ki1 & 0x7fffffffu);
        return kim ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    };
    const int phase_lo[3] = {0, kMtN - kMtM, 2 * (kMtN - kMtM)};
    const int phase_hi[3] = {kMtN - kMtM, 2 * (kMtN - kMtM), kMtN - 1};
    for (int ph = 0; ph < 3; ++ph) {
        uint32_t nv[4];
        int cnt = 0;
        for (int i = phase_lo[ph] + lane; i < phase_hi[ph]; i += kWave, ++cnt)
            nv[cnt] = gen(k[i], k[i + 1], k[(i + kMtM) % kMtN]);
        wave_sync();
        cnt = 0;
        for (int i = phase_lo[ph] + lane; i < phase_hi[ph]; i += kWave, ++cnt) k[i] = nv[cnt];
        wave_sync();
    }
    if (lane == 0) k[kMtN - 1] = gen(k[kMtN - 1], k[0], k[kMtM - 1]);
    wave_sync();
}

__device__ __forceinline__ uint32_t mt_temper_word(uint32_t y) {
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y;
}
// o[0..624) = the output words of block k
__device__ __forceinline__ void mt_temper(const uint32_t *k, uint32_t *o) {
    const int lane = threadIdx.x & (kWave - 1);
    for (int i = lane; i < kMtN; i += kWave) o[i] = mt_temper_word(k[i]);
    wave_sync();
}

// One stream over two LDS blocks: `out` holds the tempered words of the current block (numpy's
// state `key`, position `pos`) and of the next one (`key2`, twisted ahead), so any word up to
// 624 ahead of pos is readable without a twist in between -- what the speculative reads of
// mt_reset_kernel need.  The state handed back is (key, pos): numpy's.
struct MtStream {
    uint32_t *key, *key2;  // [624] raw states of the current and the next block (LDS)
    uint32_t *out;         // [1248] tempered words of both
    int pos;               // wave-uniform, < 624 between calls
    __device__ void init(int pos0) {
        const int lane = threadIdx.x & (kWave - 1);
        mt_temper(key, out);
        for (int i = lane; i < kMtN; i += kWave) key2[i] = key[i];
        wave_sync();
        mt_twist_inplace(key2);
        mt_temper(key2, out + kMtN);
        pos = pos0;
        if (pos >= kMtN) shift();
    }
    __device__ void shift() {  // the next block becomes the current one
        const int lane = threadIdx.x & (kWave - 1);
        for (int i = lane; i < kMtN; i += kWave) {
            key[i] = key2[i];
            out[i] = out[kMtN + i];
        }
        wave_sync();
        mt_twist_inplace(key2);
        mt_temper(key2, out + kMtN);
        pos -= kMtN;
    }
    __device__ uint32_t word(int k) const { return out[pos + k]; }  // k < 624 (per lane: the speculative reads)
    __device__ void advance(int c) {
        pos += c;
        if (pos >= kMtN) shift();
    }
    __device__ uint32_t next() {
        const uint32_t w = word(0);
        advance(1);
        return w;
    }
    __device__ static double dbl(uint32_t a, uint32_t b) {  // numpy's random_sample from two words
        return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) / 9007199254740992.0;
    }
    // numpy's rk_interval: a draw in [0, max] by masked rejection
    __device__ uint32_t interval(uint32_t max) {
        if (max == 0) return 0;
        uint32_t mask = max;
        mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
        uint32_t v;
        while ((v = (next() & mask)) > max) {}
        return v;
    }
};

}  // namespace asg
