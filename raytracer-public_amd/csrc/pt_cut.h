// pt_cut.h -- the arithmetic of the plane-cut queries (include/mi355pt.h: pt_cut_count, pt_cut_search), ONE text
// for the kernels (pt_cut.hip) and the host twin (pt_host.cpp): plain f32 operations in a fixed order, each rounded once (both sides are
// compiled with -ffp-contract=off; there is no fmaf), and comparisons that a NaN operand fails, so both give the same booleans and the
// same bits of t0 and t1.  The walk enters a child iff ptov::node_overlaps of the window passes AND the plane separates two corners of
// the child's grown box (node_cut).  Completeness rests on the monotonicity of rounded arithmetic, not on an error budget of the dot
// product: DESIGN.md section 24.
#pragma once
#include <stdint.h>

#include "pt_closest.h"
#include "pt_overlap.h"
#include "pt_tritri.h"

namespace ptct {

// The plane n.x = d as given.  n need not be normalised.
struct Plane { float nx, ny, nz, d; };

// the plane function: six operations in this order, each rounded once
PT_CP_FN float side(const Plane& p, float x, float y, float z) { return ((p.nx * x + p.ny * y) + p.nz * z) - p.d; }

// a record that is walked at all: n and d finite, n not the zero vector, and the window a walked box (ptov::box_walked)
PT_CP_FN bool plane_walked(const Plane& p) {
    const bool finite = (__builtin_fabsf(p.nx) <= ptov::kFltMax) & (__builtin_fabsf(p.ny) <= ptov::kFltMax) &
                        (__builtin_fabsf(p.nz) <= ptov::kFltMax) & (__builtin_fabsf(p.d) <= ptov::kFltMax);
    return finite & ((p.nx != 0.0f) | (p.ny != 0.0f) | (p.nz != 0.0f));
}

// The plane half of the node test on the GROWN corners of a child box, gl = fl(mn - s), gh = fl(mx + s) with s = ptcp::kSlack: the
// p-corner takes gh where n_k >= 0 and gl otherwise, the n-corner the opposite; passes iff side(p-corner) >= 0 and side(n-corner) < 0.
// side is monotone in each coordinate in the rounded values, so every point between the grown corners lies between the two sides.  The
// inverted box of an empty slot gives -inf or a NaN at the p-corner and fails.
PT_CP_FN bool corners_cut(const Plane& p, float glx, float gly, float glz, float ghx, float ghy, float ghz) {
    const bool ux = p.nx >= 0.0f, uy = p.ny >= 0.0f, uz = p.nz >= 0.0f;
    const float sp = side(p, ux ? ghx : glx, uy ? ghy : gly, uz ? ghz : glz);
    const float sn = side(p, ux ? glx : ghx, uy ? gly : ghy, uz ? glz : ghz);
    return (sp >= 0.0f) & (sn < 0.0f);
}
// the same on a decoded child box (the host twin; the kernels take the grown values straight from the packed halves, which are the same
// values: fl(h * 1 - s))
PT_CP_FN bool node_cut(const Plane& p, float mnx, float mny, float mnz, float mxx, float mxy, float mxz) {
    return corners_cut(p, mnx - ptcp::kSlack, mny - ptcp::kSlack, mnz - ptcp::kSlack, mxx + ptcp::kSlack, mxy + ptcp::kSlack, mxz + ptcp::kSlack);
}

// One accepted triangle: code and, from the fill walk, where the plane crosses its two crossing edges.
struct Cut { uint32_t code; float t0, t1; };

// t of one crossing edge, measured from its vertex a with s_a < 0 towards b with s_b >= 0: one subtraction, one division, in [0, 1]
PT_CP_FN float edge_t(float sa, float sb) { return sa / (sa - sb); }
// the edge (i, j) with i < j, whichever end is below
PT_CP_FN float cross_t(float si, float sj) { return si < 0.0f ? edge_t(si, sj) : edge_t(sj, si); }

// The leaf test on a record as stored (v0, e1, e2), with v1 = v0 + e1, v2 = v0 + e2 per component, one rounding each:
//   (a) pttt::box_stage against the window as given;
//   (b) s_i = side(v_i): every s_i passes >= 0 or < 0 (a NaN fails), some s_i >= 0 and some s_i < 0.
// The half-open rule of slicers: a triangle in the plane, or touching it from the >= 0 side, is not accepted; one touching from below
// with one vertex is, as a zero-length segment.  code: bits 0-2 the crossing edges v0-v1, v1-v2, v0-v2 (exactly two), bits 3-5 the
// classes s_0 >= 0, s_1 >= 0, s_2 >= 0.  t0 belongs to the lowest set edge bit, t1 to the highest.  FILL = false classifies only and never
// divides.  Returns whether the triangle is accepted.
template <bool FILL>
PT_CP_FN bool tri_cut(const ptov::Box& w, const Plane& p, float v0x, float v0y, float v0z, float e1x, float e1y, float e1z,
                      float e2x, float e2y, float e2z, Cut& out) {
    if (!pttt::box_stage(w, v0x, v0y, v0z, e1x, e1y, e1z, e2x, e2y, e2z)) return false;
    const float s0 = side(p, v0x, v0y, v0z), s1 = side(p, v0x + e1x, v0y + e1y, v0z + e1z), s2 = side(p, v0x + e2x, v0y + e2y, v0z + e2z);
    const bool u0 = s0 >= 0.0f, u1 = s1 >= 0.0f, u2 = s2 >= 0.0f, l0 = s0 < 0.0f, l1 = s1 < 0.0f, l2 = s2 < 0.0f;
    if (!((u0 | l0) & (u1 | l1) & (u2 | l2) & (u0 | u1 | u2) & (l0 | l1 | l2))) return false;
    const bool c01 = u0 != u1, c12 = u1 != u2, c02 = u0 != u2;
    out.code = (c01 ? 1u : 0u) | (c12 ? 2u : 0u) | (c02 ? 4u : 0u) | (u0 ? 8u : 0u) | (u1 ? 16u : 0u) | (u2 ? 32u : 0u);
    if (FILL) {
        // two of the three edges cross: the lowest is v0-v1 unless that one does not cross, the highest v0-v2 unless that one does not
        out.t0 = c01 ? cross_t(s0, s1) : cross_t(s1, s2);
        out.t1 = c02 ? cross_t(s0, s2) : cross_t(s1, s2);
    }
    return true;
}

} // namespace ptct
