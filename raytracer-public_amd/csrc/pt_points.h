// pt_points.h -- what the point-side batched queries hold in common, once: pt_pointquery.hip (pt_closest_points), pt_radius.hip
// (pt_radius_count, pt_radius_search), pt_knn.hip (pt_nearest_k) and pt_overlap.hip (pt_box_count, pt_box_search).  Here are the point
// record, the box bound and the triangle distance they compute with the same instructions on the same operands, and key_traverse, the
// one-item-per-thread walk of all their simple kernels.  The persistent Qs stay in their files; the radius and box queries share the frame of
// their simple and brute-force kernels (pt_region.h).  The point-triangle arithmetic itself is pt_closest.h, shared with the host twin.
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

// One item (a point, a box) per thread with a private 64-entry stack: the walk of every simple kernel of the point side, and the
// counters of their *_STATS flags by the rules of pt_device.h::traverse<..., STATS>.  child(w0, w1, w2, key) is persistent_walk's
// Q::child (pt_walk.h) on a packed f16 box: whether the child is visited -- its key is below `bound` -- and the key; the visited
// children are ordered by pt_device.h::order_children (the first minimum is entered next, the others are pushed far -> near, a push at
// 64 entries is dropped), a stacked child is re-validated at pop against `bound`.  A query whose keys are all one constant (box) says so
// in child(), and the ordering folds away.
// leaf(cur, a, b, c) gets the triangle record of leaf reference `cur`; it may lower what `bound` refers to (closest point, k-nearest) or
// leave it alone (radius, box).  The ray side's counterpart is pt_rays.h::cross_traverse.
template <bool STATS, class Child, class Leaf>
__device__ __forceinline__ void key_traverse(const RenderArgs& A, Child child, const float& bound, uint2* __restrict__ stk, Counters& cnt, Leaf leaf) {
    if (A.root_ref == kInvalidRef || A.num_tris == 0u) return;
    if (STATS) { cnt.nodes += 1; if (cnt.maxstack < 1u) cnt.maxstack = 1u; }      // the root record is fetched before its degenerate check
    if (A.root_degenerate) return;
    float troot;
    if (!child(A.root_box[0], A.root_box[1], A.root_box[2], troot)) return;
    uint32_t cur = A.root_ref;
    int sp = 0;
    for (;;) {
        bool need_pop = false;
        if (cur & kLeaf) {
            if ((cur & 0x7fffffffu) < 4u * A.num_tris) {          // an out-of-range leaf points at the record behind the last triangle: skipped
                const float4* tp = (const float4*)arena_record(A, cur);
                if (STATS) cnt.tris += 1;
                leaf(cur, tp[0], tp[1], tp[2]);
            }
            need_pop = true;
        } else {
            const uint4* np = arena_record(A, cur);
            const uint4 n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3];
            const uint32_t r0 = n0.w, r1 = n1.w, r2 = n2.w, r3 = n3.w;
            float t0, t1, t2, t3;
            const bool h0 = child(n0.x, n0.y, n0.z, t0), h1 = child(n1.x, n1.y, n1.z, t1), h2 = child(n2.x, n2.y, n2.z, t2), h3 = child(n3.x, n3.y, n3.z, t3);
            if (STATS) cnt.nodes += (r0 != kInvalidRef) + (r1 != kInvalidRef) + (r2 != kInvalidRef) + (r3 != kInvalidRef);
            uint32_t enter;
            const int before = sp;
            const bool any = h0 | h1 | h2 | h3;
            const uint32_t wanted = (uint32_t)h0 + (uint32_t)h1 + (uint32_t)h2 + (uint32_t)h3;      // one entered, the others pushed
            const bool go = order_children(h0, h1, h2, h3, t0, t1, t2, t3, r0, r1, r2, r3, 0.0f, sp, enter, [&](int at, uint32_t ref, float k) __attribute__((always_inline)) {
                stk[at] = make_uint2(ref, __float_as_uint(k));
            });
            if (STATS && any) {
                // pushes that did not fit, and the nearest child's own when the stack is full (pt_device.h::traverse)
                cnt.drops += (wanted - 1u) - (uint32_t)(sp - before) + (go ? 0u : 1u);
                const uint32_t depth = (uint32_t)sp + (go ? 1u : 0u);
                if (depth > cnt.maxstack) cnt.maxstack = depth;
            }
            if (go) cur = enter; else need_pop = true;
        }
        if (need_pop) {
            bool found = false;
            while (sp > 0) {
                --sp;
                const uint2 e = stk[sp];
                if (__uint_as_float(e.y) < bound) { cur = e.x; found = true; break; }
            }
            if (!found) break;
        }
    }
}

} // namespace ptk
