// pt_points.h -- the helpers the point-side batched queries hold in common, once: pt_pointquery.hip (pt_closest_points), pt_radius.hip
// (pt_radius_count, pt_radius_search) and pt_knn.hip (pt_nearest_k).  The three walks and their Qs stay in their files; what is here is
// the point record, the box bound and the triangle distance they all compute with the same instructions on the same operands.
// The point-triangle arithmetic itself is pt_closest.h, shared with the host twin.
// Records: PtPoint = one float4 (p.xyz, r_max).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_device.h"
#include "pt_closest.h"

namespace ptk {

constexpr uint32_t kInfBits = 0x7F800000u;

// p +- s, once per point: the box test subtracts them from the packed halves
struct PointSlack { F3 hi, lo; };
__device__ __forceinline__ PointSlack point_slack(F3 p) {
    PointSlack s;
    s.hi = f3(p.x + ptcp::kSlack, p.y + ptcp::kSlack, p.z + ptcp::kSlack);
    s.lo = f3(p.x - ptcp::kSlack, p.y - ptcp::kSlack, p.z - ptcp::kSlack);
    return s;
}
// o - float(low / high half of w) in one instruction: fma(h, -1.0, o), the f32 subtraction (one rounding of the exact difference)
__device__ __forceinline__ float minus_half_lo(float o, uint32_t w) { float r; asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(w), "v"(o)); return r; }
__device__ __forceinline__ float minus_half_hi(float o, uint32_t w) { float r; asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(w), "v"(o)); return r; }
// bound2 of one packed f16 box (w0 = mn.x | mn.y << 16, w1 = mn.z | mx.x << 16, w2 = mx.y | mx.z << 16): per axis
// g = max(mn - (p + s), (p - s) - mx, 0), three instructions straight from the packed halves (v_fma_mix_f32 twice, v_max3_f32).
// The inverted box of an empty or degenerate slot (mn = +inf) gives +inf, which is below no best2.  v_max ignores a NaN operand.
__device__ __forceinline__ float box_bound2(const PointSlack& s, uint32_t w0, uint32_t w1, uint32_t w2) {
    const float gx = wmax(wmax(half_lo_minus(w0, s.hi.x), minus_half_hi(s.lo.x, w1)), 0.0f);
    const float gy = wmax(wmax(half_hi_minus(w0, s.hi.y), minus_half_lo(s.lo.y, w2)), 0.0f);
    const float gz = wmax(wmax(half_lo_minus(w1, s.hi.z), minus_half_hi(s.lo.z, w2)), 0.0f);
    return (gx * gx + gy * gy) + gz * gz;
}

__device__ __forceinline__ void load_point(const float4* __restrict__ pts, uint32_t i, F3& p, float& rmax) {
    const float4 a = pts[i];
    p = f3(a.x, a.y, a.z); rmax = a.w;
}
// d2 of one triangle record (three axis-major pieces: v0[a], e1[a], e2[a]), with or without the u, v it was computed from
__device__ __forceinline__ float tri_d2(F3 p, const float4 a, const float4 b, const float4 c, float& u, float& v) {
    const float ax = p.x - a.x, ay = p.y - b.x, az = p.z - c.x;
    ptcp::closest_uv(ax, ay, az, a.y, b.y, c.y, a.z, b.z, c.z, u, v);
    return ptcp::closest_d2(ax, ay, az, a.y, b.y, c.y, a.z, b.z, c.z, u, v);
}
__device__ __forceinline__ float tri_d2(F3 p, const float4 a, const float4 b, const float4 c) { float u, v; return tri_d2(p, a, b, c, u, v); }
__device__ __forceinline__ uint4 as_uint4(const float4 f) { return make_uint4(__float_as_uint(f.x), __float_as_uint(f.y), __float_as_uint(f.z), __float_as_uint(f.w)); }
__device__ __forceinline__ float4 as_float4(const uint4 u) { return make_float4(__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w)); }

} // namespace ptk
