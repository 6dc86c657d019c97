// pt_overlap.h -- the box arithmetic of the box-overlap queries (include/mi355pt.h: pt_box_count, pt_box_search),
// ONE text for the kernels (pt_overlap.hip) and the host twin (pt_host.cpp): plain f32 operations in a fixed order, each rounded once
// (both sides are compiled with -ffp-contract=off), and comparisons that a NaN operand fails, so both give the same booleans.
#pragma once
#include <stdint.h>

#include "pt_closest.h"

namespace ptov {

constexpr float kFltMax = 3.402823466e+38f;

// a box that is walked at all: six finite coordinates, lo <= hi on every axis (a NaN fails every comparison)
PT_CP_FN bool box_walked(float lox, float loy, float loz, float hix, float hiy, float hiz) {
    const bool finite = (__builtin_fabsf(lox) <= kFltMax) & (__builtin_fabsf(loy) <= kFltMax) & (__builtin_fabsf(loz) <= kFltMax) &
                        (__builtin_fabsf(hix) <= kFltMax) & (__builtin_fabsf(hiy) <= kFltMax) & (__builtin_fabsf(hiz) <= kFltMax);
    return finite & (lox <= hix) & (loy <= hiy) & (loz <= hiz);
}

// What a walk holds per box: the corners themselves for (a) and the corners moved out by the slack, computed once, for the node test.
// Centre and half-extent are computed where (b) and (c) need them (tri_overlaps): six operations at a leaf that got that far, against six
// more live registers for the whole walk.
struct Box {
    float lox, loy, loz, hix, hiy, hiz;       // the corners as given
    float slx, sly, slz, shx, shy, shz;       // lo - s, hi + s with s = ptcp::kSlack
};
struct Half { float hx, hy, hz; };            // h = (hi - lo) * 0.5f
PT_CP_FN Box make_box(float lox, float loy, float loz, float hix, float hiy, float hiz) {
    Box b;
    b.lox = lox; b.loy = loy; b.loz = loz; b.hix = hix; b.hiy = hiy; b.hiz = hiz;
    b.slx = lox - ptcp::kSlack; b.sly = loy - ptcp::kSlack; b.slz = loz - ptcp::kSlack;
    b.shx = hix + ptcp::kSlack; b.shy = hiy + ptcp::kSlack; b.shz = hiz + ptcp::kSlack;
    return b;
}

// The node test on a decoded child box: entered iff mn[k] <= hi[k] + s and mx[k] >= lo[k] - s on every axis, written as the six
// differences mn - (hi + s), (lo - s) - mx, each rounded once (a rounded difference has the sign of the exact one), none above 0.  The
// inverted box of an empty slot (mn = +inf, mx = -inf) gives +inf and fails by itself.  The kernels compute the same six differences
// straight from the packed halves (pt_overlap.hip::node_overlaps).
PT_CP_FN bool node_overlaps(const Box& b, float mnx, float mny, float mnz, float mxx, float mxy, float mxz) {
    const float dx0 = mnx - b.shx, dx1 = b.slx - mxx, dy0 = mny - b.shy, dy1 = b.sly - mxy, dz0 = mnz - b.shz, dz1 = b.slz - mxz;
    return (dx0 <= 0.0f) & (dx1 <= 0.0f) & (dy0 <= 0.0f) & (dy1 <= 0.0f) & (dz0 <= 0.0f) & (dz1 <= 0.0f);
}

// one of the nine edge axes: the projections p0, p1, p2 of a0, a1, a2 and the box radius r; passes iff min p <= r and max p >= -r,
// written per projection so that a NaN fails
PT_CP_FN bool axis_pass(float p0, float p1, float p2, float r) {
    const float m = -r;
    return ((p0 <= r) | (p1 <= r) | (p2 <= r)) & ((p0 >= m) | (p1 >= m) | (p2 >= m));
}
// the three coordinate axes crossed with one edge f, in the order x, y, z:
//   x: p_i = a_i.z * f.y - a_i.y * f.z,  r = h.y * |f.z| + h.z * |f.y|
//   y: p_i = a_i.x * f.z - a_i.z * f.x,  r = h.x * |f.z| + h.z * |f.x|
//   z: p_i = a_i.y * f.x - a_i.x * f.y,  r = h.x * |f.y| + h.y * |f.x|
// every product rounded, then the difference or the sum
PT_CP_FN bool edge_pass(const Half& b, float fx, float fy, float fz, float a0x, float a0y, float a0z, float a1x, float a1y, float a1z,
                        float a2x, float a2y, float a2z) {
    const float gx = __builtin_fabsf(fx), gy = __builtin_fabsf(fy), gz = __builtin_fabsf(fz);
    if (!axis_pass(a0z * fy - a0y * fz, a1z * fy - a1y * fz, a2z * fy - a2y * fz, b.hy * gz + b.hz * gy)) return false;
    if (!axis_pass(a0x * fz - a0z * fx, a1x * fz - a1z * fx, a2x * fz - a2z * fx, b.hx * gz + b.hz * gx)) return false;
    return axis_pass(a0y * fx - a0x * fy, a1y * fx - a1x * fy, a2y * fx - a2x * fy, b.hx * gy + b.hy * gx);
}

// The triangle test on a record as stored (v0, e1, e2), against a walked box.  Returns whether the triangle is accepted; verts_inside gets
// bit i set when vertex i lies in the closed box (meaningful only when accepted).
//   vertices: v1 = v0 + e1, v2 = v0 + e2 per component, one rounding each
//   (a) the box axes, on the corners as given: per axis k, some v_ik <= hi[k] and some v_ik >= lo[k] -- min <= hi and max >= lo -- and
//       every v_ik passes at least one of its two comparisons, which only a NaN fails (lo <= hi).  The same eighteen comparisons give
//       verts_inside.
//   c = (lo + hi) * 0.5f, h = (hi - lo) * 0.5f, a_i = v_i - c
//   (b) the plane: n = e1 x e2 (each product rounded, then the difference), a0 = v0 - c,
//       |(n.x * a0.x + n.y * a0.y) + n.z * a0.z| <= (|n.x| * h.x + |n.y| * h.y) + |n.z| * h.z
//   (c) the nine edge axes: edge_pass for f = e1, e2 - e1 (per component, one rounding), e2, in that order, with a_i = v_i - c
//   accepted iff (a) and (verts_inside != 0 or ((b) and (c))): a vertex in the closed box is an overlap that no rounding touches.
// Touching counts.  A NaN anywhere in the record fails (a).
PT_CP_FN bool tri_overlaps(const Box& b, float v0x, float v0y, float v0z, float e1x, float e1y, float e1z, float e2x, float e2y, float e2z,
                           uint32_t& verts_inside) {
    const float v1x = v0x + e1x, v1y = v0y + e1y, v1z = v0z + e1z;
    const float v2x = v0x + e2x, v2y = v0y + e2y, v2z = v0z + e2z;
    const bool l0x = v0x <= b.hix, l1x = v1x <= b.hix, l2x = v2x <= b.hix, g0x = v0x >= b.lox, g1x = v1x >= b.lox, g2x = v2x >= b.lox;
    const bool l0y = v0y <= b.hiy, l1y = v1y <= b.hiy, l2y = v2y <= b.hiy, g0y = v0y >= b.loy, g1y = v1y >= b.loy, g2y = v2y >= b.loy;
    const bool l0z = v0z <= b.hiz, l1z = v1z <= b.hiz, l2z = v2z <= b.hiz, g0z = v0z >= b.loz, g1z = v1z >= b.loz, g2z = v2z >= b.loz;
    const bool ax = (l0x | l1x | l2x) & (g0x | g1x | g2x) & (l0x | g0x) & (l1x | g1x) & (l2x | g2x);
    const bool ay = (l0y | l1y | l2y) & (g0y | g1y | g2y) & (l0y | g0y) & (l1y | g1y) & (l2y | g2y);
    const bool az = (l0z | l1z | l2z) & (g0z | g1z | g2z) & (l0z | g0z) & (l1z | g1z) & (l2z | g2z);
    const bool in0 = l0x & g0x & l0y & g0y & l0z & g0z, in1 = l1x & g1x & l1y & g1y & l1z & g1z, in2 = l2x & g2x & l2y & g2y & l2z & g2z;
    verts_inside = (in0 ? 1u : 0u) | (in1 ? 2u : 0u) | (in2 ? 4u : 0u);
    if (!(ax & ay & az)) return false;
    if (verts_inside != 0u) return true;
    const float cx = (b.lox + b.hix) * 0.5f, cy = (b.loy + b.hiy) * 0.5f, cz = (b.loz + b.hiz) * 0.5f;
    const Half h = {(b.hix - b.lox) * 0.5f, (b.hiy - b.loy) * 0.5f, (b.hiz - b.loz) * 0.5f};
    const float a0x = v0x - cx, a0y = v0y - cy, a0z = v0z - cz;
    const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const float d = (nx * a0x + ny * a0y) + nz * a0z;
    const float r = (__builtin_fabsf(nx) * h.hx + __builtin_fabsf(ny) * h.hy) + __builtin_fabsf(nz) * h.hz;
    if (!(__builtin_fabsf(d) <= r)) return false;
    const float a1x = v1x - cx, a1y = v1y - cy, a1z = v1z - cz;
    const float a2x = v2x - cx, a2y = v2y - cy, a2z = v2z - cz;
    if (!edge_pass(h, e1x, e1y, e1z, a0x, a0y, a0z, a1x, a1y, a1z, a2x, a2y, a2z)) return false;
    if (!edge_pass(h, e2x - e1x, e2y - e1y, e2z - e1z, a0x, a0y, a0z, a1x, a1y, a1z, a2x, a2y, a2z)) return false;
    return edge_pass(h, e2x, e2y, e2z, a0x, a0y, a0z, a1x, a1y, a1z, a2x, a2y, a2z);
}

} // namespace ptov
