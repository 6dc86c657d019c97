// pt_closest.h -- the point-triangle arithmetic of the closest-point queries (include/mi355pt.h: pt_closest_points),
// ONE text for the kernels (pt_pointquery.hip) and the host twin (pt_host.cpp): plain f32 operations in a fixed order, each rounded once
// (both sides are compiled with -ffp-contract=off; the device's f32 division is the correctly rounded one), so both give the same bits.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define PT_CP_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define PT_CP_FN inline
#endif

namespace ptcp {

constexpr float kSlack = 0x1p-12f;       // the s of bound2 (the f16 subnormal flush plus every rounding of bound2 and d2)

PT_CP_FN float dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// Closest point of the triangle (v0, v0 + e1, v0 + e2) to p as v0 + u*e1 + v*e2, from ap = p - v0.
// 1. The unconstrained minimum of |ap - u*e1 - v*e2|^2 by one Gram-Schmidt step, not by Cramer's rule on the Gram matrix (whose
//    determinant squares the condition of a thin triangle): f = e2 - (b / a) e1 is the part of e2 orthogonal to e1, vq = (f . ap) / (f . f),
//    uq = (d1 - vq * b) / a.
// 2. The signs of uq, vq and 1 - (uq + vq) name one of seven regions of the plane (Eberly, "Distance between point and triangle in 3D"):
//    the face, or one or two edges on which the minimum then lies; where two edges are possible, his comparisons of the d's choose.
// 3. On an edge the point is a clamped quotient num / den (exactly 0 below, exactly 1 above).
// Three reciprocals in all: 1 / a, 1 / (f . f), and 1 / den of the edges v0 v2 and v1 v2.
// NaN operands fail every comparison and reach the edge v1 v2.  A triangle collapsed to a segment still gets a point of that segment (a
// distance that is never too small); one collapsed to a point gets NaN (0 / 0) unless p projects onto v0 itself.
PT_CP_FN void closest_uv(float ax, float ay, float az, float e1x, float e1y, float e1z, float e2x, float e2y, float e2z, float& u, float& v) {
    const float a = dot(e1x, e1y, e1z, e1x, e1y, e1z), b = dot(e1x, e1y, e1z, e2x, e2y, e2z), c = dot(e2x, e2y, e2z, e2x, e2y, e2z);
    const float d1 = dot(e1x, e1y, e1z, ax, ay, az), d2 = dot(e2x, e2y, e2z, ax, ay, az);
    const float ra = 1.0f / a, k = b * ra;
    const float fx = e2x - e1x * k, fy = e2y - e1y * k, fz = e2z - e1z * k;
    const float rf = 1.0f / dot(fx, fy, fz, fx, fy, fz);
    const float vq = dot(fx, fy, fz, ax, ay, az) * rf, uq = (d1 - vq * b) * ra;
    const float cd = c - d2, bd = b - d1, ad = a - d1, be = b - d2;
    // 0: the edge v0 v1 (v = 0, u = clamp(d1 / a)); 1: the edge v0 v2 (u = 0, v = clamp(d2 / c)); 2: the edge v1 v2 (u = clamp(((c - d2) -
    // (b - d1)) / ((a - 2b) + c)), v = 1 - u); 3: the face
    int where;
    if (uq + vq <= 1.0f) where = uq < 0.0f ? (vq < 0.0f ? (d1 > 0.0f ? 0 : 1) : 1) : (vq < 0.0f ? 0 : 3);
    else where = uq < 0.0f ? (cd > bd ? 2 : 1) : (vq < 0.0f ? (ad > be ? 2 : 0) : 2);
    const float num = where == 0 ? d1 : where == 1 ? d2 : cd - bd;
    const float den = where == 0 ? a : where == 1 ? c : (a - (b + b)) + c;
    const float r = 1.0f / den;
    float x = where == 0 ? d1 * ra : num * r;              // along the edge; NaN stays NaN
    x = num <= 0.0f ? 0.0f : (num >= den ? 1.0f : x);
    u = where == 3 ? uq : where == 1 ? 0.0f : x;
    v = where == 3 ? vq : where == 0 ? 0.0f : where == 1 ? x : 1.0f - x;
}

// squared distance from p to that point: diff = ap - (e1*u + e2*v), d2 = dot(diff, diff)
PT_CP_FN float closest_d2(float ax, float ay, float az, float e1x, float e1y, float e1z, float e2x, float e2y, float e2z, float u, float v) {
    const float dx = ax - (e1x * u + e2x * v), dy = ay - (e1y * u + e2y * v), dz = az - (e1z * u + e2z * v);
    return dot(dx, dy, dz, dx, dy, dz);
}

// a point that is walked at all: no NaN in p or r_max, r_max > 0
PT_CP_FN bool point_walked(float px, float py, float pz, float r_max) {
    return !((px != px) | (py != py) | (pz != pz)) & (r_max > 0.0f);
}

} // namespace ptcp
