// pt_bounds.h -- the f16 bounds arithmetic of the scene build, shared by the kernels that write BVH boxes
// (pt_kernels.hip: LBVH2 leaves and refit walk; pt_build.hip: BVH4 collapse and wide nodes; pt_refit.hip: refit in place).
// Host twins, the same expressions: pt_host.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ptk {

// f32 -> f16 is round-to-nearest-even (v_cvt_f16_f32)
__device__ __forceinline__ uint32_t f16_bits_rtne(float v) { return (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)v); }
__device__ __forceinline__ uint32_t step_f16(float v, bool up) {        // BVHBuilder.wgsl:63-81, returns f16 bits
    const uint32_t bits = f16_bits_rtne(v);
    uint32_t ord = (bits & 0x8000u) ? ((~bits) & 0xFFFFu) : (bits ^ 0x8000u);
    ord = up ? ord + 1u : ord - 1u;
    return ((ord & 0x8000u) ? (ord ^ 0x8000u) : ((~ord) & 0xFFFFu)) & 0xFFFFu;
}
// JS Math.min / Math.max on numbers (sign of zero ordered, first operand wins a tie otherwise): pt_host.cpp js_min_f / js_max_f
__device__ __forceinline__ float js_min_f(float a, float b) { if (a < b) return a; if (b < a) return b; return (__float_as_uint(a) >> 31) ? a : b; }
__device__ __forceinline__ float js_max_f(float a, float b) { if (a > b) return a; if (b > a) return b; return (__float_as_uint(a) >> 31) ? b : a; }
__device__ __forceinline__ float half_exact(uint32_t h) {        // PathTracer.js:16-40, integer form (exact for subnormals whatever the FP mode)
    const uint32_t sign = (h & 0x8000u) << 16, mag = h & 0x7fffu;
    if (mag >= 0x7c00u) return __uint_as_float(sign | 0x7f800000u | ((mag & 0x3ffu) << 13));
    if (mag >= 0x0400u) return __uint_as_float(sign | ((mag + (112u << 10)) << 13));
    const float v = (float)mag * 5.9604644775390625e-8f;
    return __uint_as_float(__float_as_uint(v) | sign);
}
__device__ __forceinline__ uint32_t half_trunc(float v) {        // PathTracer.js:42-51: truncate, flush below the normal range, saturate
    const uint32_t u = __float_as_uint(v);
    const uint32_t sign = (u >> 16) & 0x8000u;
    const int32_t e = (int32_t)((u >> 23) & 0xffu) - 112;
    if (e <= 0) return sign;
    if (e >= 31) return sign | 0x7c00u;
    return sign | ((uint32_t)e << 10) | ((u >> 13) & 0x3ffu);
}
__device__ __forceinline__ bool box_degenerate(uint32_t w0, uint32_t w1, uint32_t w2) {     // renderer.wgsl:244, 291: any(mn > mx)
    return half_exact(w0 & 0xffffu) > half_exact(w1 >> 16) || half_exact(w0 >> 16) > half_exact(w2 & 0xffffu) || half_exact(w1 & 0xffffu) > half_exact(w2 >> 16);
}

} // namespace ptk
