// pt_sweep.h -- the swept-sphere arithmetic of the sphere-cast queries (include/mi355pt.h: pt_sweep_spheres), ONE text
// for the kernels (pt_sweep.hip) and the host twin (pt_host.cpp): plain f32 operations in a fixed order, each rounded once (both sides are
// compiled with -ffp-contract=off; the device's f32 division and square root are the correctly rounded ones), and comparisons that a NaN
// operand fails, so both give the same bits.  dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z (ptcp::dot), cross(a, b) = (a.y*b.z - a.z*b.y,
// a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x), every product rounded, then the difference.
//
// A sweep is (o, t_max, d, r): the centre o + t*d, 0 <= t < t_max, of a sphere of radius r.  Per sweep, once: inv = safe_inv(d) (1 / d_k,
// or 1e30 where |d_k| <= 1e-8: pt_raymath.h), best = t_max.  Per triangle record (v0, e1, e2), in this order (tri_sweep):
//   1. own box.  v1 = v0 + e1, v2 = v0 + e2 per component; mn_k, mx_k = the smallest and largest of v0_k, v1_k, v2_k; the origin moved
//      by the radius, op_k = o_k + r, om_k = o_k - r; a_k = (mn_k - op_k) * inv_k, b_k = (mx_k - om_k) * inv_k; near_k, far_k = a_k, b_k
//      for inv_k >= 0 and b_k, a_k for inv_k < 0; tmin = max(near), tmax = min(far); t_in = tmin > 0 ? tmin : 0.  The triangle is
//      rejected unless tmax >= t_in and tmin < best (pt_device.h::slab on the box grown by r, the growth taken on the origin's side).
//   2. overlap at the start.  s = o - v0; (u, v) = ptcp::closest_uv(s, e1, e2), d2 = ptcp::closest_d2(s, e1, e2, u, v); rr = r * r;
//      d2 <= rr: t_c = 0.
//   3. otherwise t_c = the smallest valid candidate, +inf when there is none, of
//      face      n = cross(e1, e2), nn = dot(n, n), h = dot(n, s), nd = dot(n, d), rn = r * sqrt(nn); t = ((h >= 0 ? rn : -rn) - h) / nd;
//                w = s + d * t per component; uq, vq of w by the Gram-Schmidt step of pt_closest.h (a = dot(e1, e1), b = dot(e1, e2),
//                ra = 1 / a, k = b * ra, f = e2 - e1 * k, rf = 1 / dot(f, f), vq = dot(f, w) * rf, uq = (dot(e1, w) - vq * b) * ra);
//                valid iff t >= 0, uq >= 0, vq >= 0 and uq + vq <= 1
//      edges     (v0, e1) with m = s; (v0, e2) with m = s; (v1, e2 - e1) with m = o - v1: the line as a cylinder, in cross products:
//                p = cross(m, e), q = cross(d, e), ee = dot(e, e); rA = 1 / dot(q, q); t0 = -(dot(p, q) * rA), the time of the closest
//                approach to the line; w = p + q * t0 per component, what is left of p there; t = t0 - sqrt((rr * ee - dot(w, w)) * rA);
//                g = dot(m, e) + t * dot(d, e); valid iff t >= 0, g >= 0 and g <= ee (the foot of the contact lies on the edge)
//      vertices  v0 with m = s, v1 with m = o - v1, v2 with m = o - v2: rdd = 1 / dot(d, d); t0 = -(dot(m, d) * rdd); w = m + d * t0;
//                t = t0 - sqrt((rr - dot(w, w)) * rdd); valid iff t >= 0
//      Both are the smaller root of A t^2 + 2 B t + C = 0 taken from the closest approach: the discriminant B^2 - A C cancels to
//      sqrt(eps) of the scene where r is small (a moving point passing 2.4e-4 from an edge was reported as touching it), the vector w
//      cancels linearly.  A sphere that never comes within r gives NaN (the square root of a negative), a receding one a negative t.
//   4. clamp.  t_T = t_c > t_in ? t_c : t_in; the caller accepts the triangle iff t_T < best, strictly.
// After an accepted t_T the bound is bound_after(t_T): t_T itself, or -inf behind a contact at t_T = 0 -- t_T is never negative and
// acceptance is strict, so nothing can be accepted any more, every box test and every re-validation fails and the walk ends there instead
// of visiting every node whose grown box holds the origin.  The reported time is time_of(bound): the bound, or 0 for -inf.
// A NaN fails every comparison above and is never accepted.  A triangle collapsed to a segment or a point keeps its vertex candidates.
// After the walk the contact point is c = o + t * d per component (the product rounded, then the sum), and u, v = ptcp::closest_uv(c - v0,
// e1, e2) on the winning record (contact_uv).
#pragma once
#include <stdint.h>

#include "pt_bounds.h"

namespace ptsw {

constexpr float kNoContact = __builtin_inff();

// a sweep that is walked at all: no NaN in o, d, t_max or r, t_max > 0, r >= 0, d != (0, 0, 0)
PT_CP_FN bool sweep_walked(float ox, float oy, float oz, float tmax, float dx, float dy, float dz, float r) {
    const bool nan = (ox != ox) | (oy != oy) | (oz != oz) | (dx != dx) | (dy != dy) | (dz != dz);
    return !nan & (tmax > 0.0f) & (r >= 0.0f) & ((dx != 0.0f) | (dy != 0.0f) | (dz != 0.0f));
}
PT_CP_FN float bound_after(float t) { return t > 0.0f ? t : -kNoContact; }
PT_CP_FN float time_of(float bound) { return bound > 0.0f ? bound : 0.0f; }

using ptbd::sel_min;       // b < a ? b : a, the select flavour of pt_bounds.h
using ptbd::sel_max;

// one axis of a slab test with the growth g on the origin's side: op = o + g, om = o - g
PT_CP_FN void axis_slab(float mn, float mx, float op, float om, float inv, float& near, float& far) {
    const float a = (mn - op) * inv, b = (mx - om) * inv;
    const bool neg = inv < 0.0f;
    near = neg ? b : a; far = neg ? a : b;
}

// The node test on a decoded child box, for the twin: the slab test on the box grown by R = r + s (s = ptcp::kSlack), op = o + R and
// om = o - R computed once per sweep.  max and min ignore a NaN operand, as v_max_f32 and v_min_f32 do (the inverted box of an empty slot
// gives near = +inf, far = -inf and fails by itself).  The kernels form the same differences straight from the packed halves behind
// the sign selection (pt_sweep.hip::sweep_slab_sel): the same values, so the same booleans and the same key.
PT_CP_FN float nan_max(float a, float b) { return a != a ? b : (b != b ? a : (b > a ? b : a)); }
PT_CP_FN float nan_min(float a, float b) { return a != a ? b : (b != b ? a : (b < a ? b : a)); }
PT_CP_FN bool node_pass(float mnx, float mny, float mnz, float mxx, float mxy, float mxz, float opx, float opy, float opz,
                        float omx, float omy, float omz, float ix, float iy, float iz, float best, float& tmin_out) {
    float nx, ny, nz, fx, fy, fz;
    axis_slab(mnx, mxx, opx, omx, ix, nx, fx); axis_slab(mny, mxy, opy, omy, iy, ny, fy); axis_slab(mnz, mxz, opz, omz, iz, nz, fz);
    const float tmin = nan_max(nan_max(nx, ny), nz), tmax = nan_min(nan_min(fx, fy), fz);
    tmin_out = tmin;
    return (tmax >= nan_max(tmin, 0.0f)) & (tmin < best);
}

// an edge (a, e) with m = o - a, folded into the running minimum tc
PT_CP_FN float edge_contact(float tc, float mx, float my, float mz, float ex, float ey, float ez, float dx, float dy, float dz, float rr) {
    const float px = my * ez - mz * ey, py = mz * ex - mx * ez, pz = mx * ey - my * ex;
    const float qx = dy * ez - dz * ey, qy = dz * ex - dx * ez, qz = dx * ey - dy * ex;
    const float ee = ptcp::dot(ex, ey, ez, ex, ey, ez);
    const float rA = 1.0f / ptcp::dot(qx, qy, qz, qx, qy, qz);
    const float t0 = -(ptcp::dot(px, py, pz, qx, qy, qz) * rA);
    const float wx = px + qx * t0, wy = py + qy * t0, wz = pz + qz * t0;
    const float t = t0 - __builtin_sqrtf((rr * ee - ptcp::dot(wx, wy, wz, wx, wy, wz)) * rA);
    const float g = ptcp::dot(mx, my, mz, ex, ey, ez) + t * ptcp::dot(dx, dy, dz, ex, ey, ez);
    return ((t >= 0.0f) & (g >= 0.0f) & (g <= ee) & (t < tc)) ? t : tc;
}
// a vertex a with m = o - a
PT_CP_FN float vertex_contact(float tc, float mx, float my, float mz, float dx, float dy, float dz, float rdd, float rr) {
    const float t0 = -(ptcp::dot(mx, my, mz, dx, dy, dz) * rdd);
    const float wx = mx + dx * t0, wy = my + dy * t0, wz = mz + dz * t0;
    const float t = t0 - __builtin_sqrtf((rr - ptcp::dot(wx, wy, wz, wx, wy, wz)) * rdd);
    return ((t >= 0.0f) & (t < tc)) ? t : tc;
}

// t_T of one record against a walked sweep, kNoContact when the triangle is rejected; the caller accepts iff the result is < best
PT_CP_FN float tri_sweep(float ox, float oy, float oz, float dx, float dy, float dz, float ix, float iy, float iz, float r, float best,
                         float v0x, float v0y, float v0z, float e1x, float e1y, float e1z, float e2x, float e2y, float e2z) {
    // 1. own box
    const float v1x = v0x + e1x, v1y = v0y + e1y, v1z = v0z + e1z;
    const float v2x = v0x + e2x, v2y = v0y + e2y, v2z = v0z + e2z;
    float nx, ny, nz, fx, fy, fz;
    axis_slab(sel_min(sel_min(v0x, v1x), v2x), sel_max(sel_max(v0x, v1x), v2x), ox + r, ox - r, ix, nx, fx);
    axis_slab(sel_min(sel_min(v0y, v1y), v2y), sel_max(sel_max(v0y, v1y), v2y), oy + r, oy - r, iy, ny, fy);
    axis_slab(sel_min(sel_min(v0z, v1z), v2z), sel_max(sel_max(v0z, v1z), v2z), oz + r, oz - r, iz, nz, fz);
    const float tmin = sel_max(sel_max(nx, ny), nz), tmax = sel_min(sel_min(fx, fy), fz);
    const float t_in = tmin > 0.0f ? tmin : 0.0f;
    if (!((tmax >= t_in) & (tmin < best))) return kNoContact;
    // 2. overlap at the start
    const float sx = ox - v0x, sy = oy - v0y, sz = oz - v0z;
    float u, v;
    ptcp::closest_uv(sx, sy, sz, e1x, e1y, e1z, e2x, e2y, e2z, u, v);
    const float d2 = ptcp::closest_d2(sx, sy, sz, e1x, e1y, e1z, e2x, e2y, e2z, u, v);
    const float rr = r * r;
    float tc = kNoContact;
    if (d2 <= rr) {
        tc = 0.0f;
    } else {
        // 3. the face, the three edges, the three vertices
        const float nnx = e1y * e2z - e1z * e2y, nny = e1z * e2x - e1x * e2z, nnz = e1x * e2y - e1y * e2x;
        const float nn = ptcp::dot(nnx, nny, nnz, nnx, nny, nnz), h = ptcp::dot(nnx, nny, nnz, sx, sy, sz), nd = ptcp::dot(nnx, nny, nnz, dx, dy, dz);
        const float rn = r * __builtin_sqrtf(nn);
        const float tf = ((h >= 0.0f ? rn : -rn) - h) / nd;
        const float wx = sx + dx * tf, wy = sy + dy * tf, wz = sz + dz * tf;
        const float a = ptcp::dot(e1x, e1y, e1z, e1x, e1y, e1z), b = ptcp::dot(e1x, e1y, e1z, e2x, e2y, e2z);
        const float ra = 1.0f / a, k = b * ra;
        const float gx = e2x - e1x * k, gy = e2y - e1y * k, gz = e2z - e1z * k;
        const float rf = 1.0f / ptcp::dot(gx, gy, gz, gx, gy, gz);
        const float vq = ptcp::dot(gx, gy, gz, wx, wy, wz) * rf, uq = (ptcp::dot(e1x, e1y, e1z, wx, wy, wz) - vq * b) * ra;
        if ((tf >= 0.0f) & (uq >= 0.0f) & (vq >= 0.0f) & (uq + vq <= 1.0f)) tc = tf;
        const float m1x = ox - v1x, m1y = oy - v1y, m1z = oz - v1z;
        const float m2x = ox - v2x, m2y = oy - v2y, m2z = oz - v2z;
        tc = edge_contact(tc, sx, sy, sz, e1x, e1y, e1z, dx, dy, dz, rr);
        tc = edge_contact(tc, sx, sy, sz, e2x, e2y, e2z, dx, dy, dz, rr);
        tc = edge_contact(tc, m1x, m1y, m1z, e2x - e1x, e2y - e1y, e2z - e1z, dx, dy, dz, rr);
        const float rdd = 1.0f / ptcp::dot(dx, dy, dz, dx, dy, dz);
        tc = vertex_contact(tc, sx, sy, sz, dx, dy, dz, rdd, rr);
        tc = vertex_contact(tc, m1x, m1y, m1z, dx, dy, dz, rdd, rr);
        tc = vertex_contact(tc, m2x, m2y, m2z, dx, dy, dz, rdd, rr);
    }
    // 4. clamp
    return tc > t_in ? tc : t_in;
}

// u, v of the contact point c = o + t * d on the winning record
PT_CP_FN void contact_uv(float ox, float oy, float oz, float dx, float dy, float dz, float t,
                         float v0x, float v0y, float v0z, float e1x, float e1y, float e1z, float e2x, float e2y, float e2z, float& u, float& v) {
    const float cx = ox + t * dx, cy = oy + t * dy, cz = oz + t * dz;
    ptcp::closest_uv(cx - v0x, cy - v0y, cz - v0z, e1x, e1y, e1z, e2x, e2y, e2z, u, v);
}

} // namespace ptsw
