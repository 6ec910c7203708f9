// unroll_common.h -- the small helpers shared by the learner's sequence kernels: the GRU
// agent's unroll (asg_unroll.hip) and the Linear agent's (asg_unroll_mlp.hip).
#pragma once
#include "asg_agent_common.h"

namespace asg {

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ void st4(float *p, f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }
// elements k .. k + 3 of a K-long row; vec: K % 4 == 0 and the row is 16-B aligned
__device__ __forceinline__ f32x4 ldk(const float *row, int k, int K, bool vec) {
    if (vec) return k < K ? ld4(row + k) : f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = k + e < K ? row[k + e] : 0.f;
    return v;
}

inline int fail(const char *msg) {
    set_last_error(msg);
    return ASG_E_INVALID_ARG;
}
inline int hip_fail(hipError_t e, const char *what) {
    set_last_error(std::string(what) + ": " + hipGetErrorString(e));
    return ASG_E_HIP;
}
inline bool al(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace asg
