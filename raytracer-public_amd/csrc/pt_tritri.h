// pt_tritri.h -- the arithmetic of the triangle-overlap queries (include/mi355pt.h: pt_tri_count, pt_tri_search),
// ONE text for the kernels (pt_tritri.hip) and the host twin (pt_host.cpp): plain f32 operations in a fixed order, each rounded once
// (both sides are compiled with -ffp-contract=off), and comparisons that a NaN operand fails, so both give the same booleans.  The walk
// holds the caller triangle's exact bounding box as a ptov::Box and enters a child iff ptov::node_overlaps: the node test of the box
// query, whose completeness proof therefore carries over.
// COPLANAR PAIRS ARE NOT LISTED: every det below is 0 for them.  A caller who needs them runs a 2-D test on the candidates of
// pt_box_search.
#pragma once
#include <stdint.h>

#include "pt_closest.h"
#include "pt_overlap.h"
#include "pt_raymath.h"

namespace pttt {

// The caller triangle as given: q0, q1, q2.
struct Tri { float q0x, q0y, q0z, q1x, q1y, q1z, q2x, q2y, q2z; };

// a triangle that is walked at all: nine finite coordinates (a NaN fails every comparison).  A degenerate triangle is walked.
PT_CP_FN bool tri_walked(const Tri& q) {
    return (__builtin_fabsf(q.q0x) <= ptov::kFltMax) & (__builtin_fabsf(q.q0y) <= ptov::kFltMax) & (__builtin_fabsf(q.q0z) <= ptov::kFltMax) &
           (__builtin_fabsf(q.q1x) <= ptov::kFltMax) & (__builtin_fabsf(q.q1y) <= ptov::kFltMax) & (__builtin_fabsf(q.q1z) <= ptov::kFltMax) &
           (__builtin_fabsf(q.q2x) <= ptov::kFltMax) & (__builtin_fabsf(q.q2y) <= ptov::kFltMax) & (__builtin_fabsf(q.q2z) <= ptov::kFltMax);
}

// min / max of three finite values by comparisons alone (exact)
PT_CP_FN float min3(float a, float b, float c) { const float m = b < a ? b : a; return c < m ? c : m; }
PT_CP_FN float max3(float a, float b, float c) { const float m = b > a ? b : a; return c > m ? c : m; }
// the exact bounding box of a walked caller triangle, with the corners moved out by the slack for the node test
PT_CP_FN ptov::Box tri_box(const Tri& q) {
    return ptov::make_box(min3(q.q0x, q.q1x, q.q2x), min3(q.q0y, q.q1y, q.q2y), min3(q.q0z, q.q1z, q.q2z),
                          max3(q.q0x, q.q1x, q.q2x), max3(q.q0y, q.q1y, q.q2y), max3(q.q0z, q.q1z, q.q2z));
}

// Stage (a) of pt_overlap.h::tri_overlaps, restated (it is not reachable on its own there): the three vertices of a record against the
// corners as given.  Per axis k some v_ik <= hi[k] and some v_ik >= lo[k] -- min <= hi and max >= lo -- and every v_ik passes at least one
// of its two comparisons, which only a NaN fails (lo <= hi).
PT_CP_FN bool axis_stage(float v0, float v1, float v2, float lo, float hi) {
    const bool l0 = v0 <= hi, l1 = v1 <= hi, l2 = v2 <= hi, g0 = v0 >= lo, g1 = v1 >= lo, g2 = v2 >= lo;
    return (l0 | l1 | l2) & (g0 | g1 | g2) & (l0 | g0) & (l1 | g1) & (l2 | g2);
}
// v1 = v0 + e1, v2 = v0 + e2 per component, one rounding each
PT_CP_FN bool box_stage(const ptov::Box& b, float v0x, float v0y, float v0z, float e1x, float e1y, float e1z, float e2x, float e2y, float e2z) {
    const bool ax = axis_stage(v0x, v0x + e1x, v0x + e2x, b.lox, b.hix), ay = axis_stage(v0y, v0y + e1y, v0y + e2y, b.loy, b.hiy);
    const bool az = axis_stage(v0z, v0z + e1z, v0z + e2z, b.loz, b.hiz);
    return ax & ay & az;
}

// The segment (p, d) -- from p to p + d -- against the triangle (a, f1, f2): a division-free, scale-free Moeller-Trumbore.
//   pv = cross(d, f2), det = dot(f1, pv), sv = p - a, U = dot(sv, pv), qv = cross(sv, f1), V = dot(d, qv), T = dot(f2, qv)
//   crosses iff det > 0 and U >= 0, V >= 0, U + V <= det, T >= 0, T <= det, or det < 0 and the same five mirrored.
// det == 0 (parallel, coplanar, a zero-length segment, a zero-area triangle) and a NaN cross nothing.  There is no epsilon: touching
// counts wherever the rounded values say so.
PT_CP_FN bool seg_crosses(float px, float py, float pz, float dx, float dy, float dz, float ax, float ay, float az,
                          float f1x, float f1y, float f1z, float f2x, float f2y, float f2z) {
    float pvx, pvy, pvz, qvx, qvy, qvz;
    ptry::cross(dx, dy, dz, f2x, f2y, f2z, pvx, pvy, pvz);
    const float det = ptcp::dot(f1x, f1y, f1z, pvx, pvy, pvz);
    const float svx = px - ax, svy = py - ay, svz = pz - az;
    const float U = ptcp::dot(svx, svy, svz, pvx, pvy, pvz);
    ptry::cross(svx, svy, svz, f1x, f1y, f1z, qvx, qvy, qvz);
    const float V = ptcp::dot(dx, dy, dz, qvx, qvy, qvz);
    const float T = ptcp::dot(f2x, f2y, f2z, qvx, qvy, qvz);
    const float W = U + V;
    const bool pos = (det > 0.0f) & (U >= 0.0f) & (V >= 0.0f) & (W <= det) & (T >= 0.0f) & (T <= det);
    const bool neg = (det < 0.0f) & (U <= 0.0f) & (V <= 0.0f) & (W >= det) & (T <= 0.0f) & (T >= det);
    return pos | neg;
}

// The six segment tests of the caller triangle q against a record as stored (v0, e1, e2).  Bits 0-2: the caller's edges (q0, q1 - q0),
// (q1, q2 - q1), (q2, q0 - q2) against (v0, e1, e2).  Bits 3-5: the mesh triangle's edges (v0, e1), (v1, e2 - e1), (v0, e2), with
// v1 = v0 + e1, against (q0, q1 - q0, q2 - q0).  Every difference and sum per component, with one rounding.  ALL = false may stop at the
// first set bit: the result is then nonzero exactly where the full word is.
template <bool ALL>
PT_CP_FN uint32_t edge_bits(const Tri& q, float v0x, float v0y, float v0z, float e1x, float e1y, float e1z, float e2x, float e2y, float e2z) {
    const float ax = q.q1x - q.q0x, ay = q.q1y - q.q0y, az = q.q1z - q.q0z;          // q0 -> q1
    uint32_t edges = seg_crosses(q.q0x, q.q0y, q.q0z, ax, ay, az, v0x, v0y, v0z, e1x, e1y, e1z, e2x, e2y, e2z) ? 1u : 0u;
    if (!ALL && edges) return edges;
    if (seg_crosses(q.q1x, q.q1y, q.q1z, q.q2x - q.q1x, q.q2y - q.q1y, q.q2z - q.q1z, v0x, v0y, v0z, e1x, e1y, e1z, e2x, e2y, e2z)) edges |= 2u;
    if (!ALL && edges) return edges;
    if (seg_crosses(q.q2x, q.q2y, q.q2z, q.q0x - q.q2x, q.q0y - q.q2y, q.q0z - q.q2z, v0x, v0y, v0z, e1x, e1y, e1z, e2x, e2y, e2z)) edges |= 4u;
    if (!ALL && edges) return edges;
    const float cx = q.q2x - q.q0x, cy = q.q2y - q.q0y, cz = q.q2z - q.q0z;          // q0 -> q2
    if (seg_crosses(v0x, v0y, v0z, e1x, e1y, e1z, q.q0x, q.q0y, q.q0z, ax, ay, az, cx, cy, cz)) edges |= 8u;
    if (!ALL && edges) return edges;
    if (seg_crosses(v0x + e1x, v0y + e1y, v0z + e1z, e2x - e1x, e2y - e1y, e2z - e1z, q.q0x, q.q0y, q.q0z, ax, ay, az, cx, cy, cz)) edges |= 16u;
    if (!ALL && edges) return edges;
    if (seg_crosses(v0x, v0y, v0z, e2x, e2y, e2z, q.q0x, q.q0y, q.q0z, ax, ay, az, cx, cy, cz)) edges |= 32u;
    return edges;
}

// The leaf test on a record (v0, e1, e2): accepted iff (a) the box stage passes against the caller triangle's exact bounding box and
// (b) edges != 0.  Returns edges, 0 for a triangle that is not accepted.
template <bool ALL>
PT_CP_FN uint32_t tri_crosses(const ptov::Box& b, const Tri& q, float v0x, float v0y, float v0z, float e1x, float e1y, float e1z,
                              float e2x, float e2y, float e2z) {
    if (!box_stage(b, v0x, v0y, v0z, e1x, e1y, e1z, e2x, e2y, e2z)) return 0u;
    return edge_bits<ALL>(q, v0x, v0y, v0z, e1x, e1y, e1z, e2x, e2y, e2z);
}

} // namespace pttt
