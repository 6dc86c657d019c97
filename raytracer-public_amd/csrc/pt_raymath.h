// pt_raymath.h -- the ray arithmetic of the ray-side batched queries (include/mi355pt.h: pt_trace_rays, pt_occlusion, pt_occlusion_rays,
// pt_count_hits, pt_contains, pt_list_hits; DESIGN.md sections 4, 13, 16, 17 and 20), ONE text for the kernels (through the forwarders of
// pt_device.h and pt_rays.h) and the host twin (pt_host.cpp): plain f32 and u32 operations in a fixed order, each rounded once (both
// sides are compiled with -ffp-contract=off; the device's f32 division and square root are the correctly rounded ones), fmaf exactly
// where it is written, and comparisons that a NaN operand fails, so both give the same bits.  dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z,
// cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x), every product rounded, then the difference.
//
// A ray is (o, t_max, d).  Per ray, once: it is walked iff no component of o or d is a NaN and t_max > 0 (ray_walked); inv_k =
// safe_inv(d_k) = 1 / d_k, or 1e30 where |d_k| <= 1e-8.  Per triangle record (v0, e1, e2), in this order (tri_hit; renderer.wgsl:185-205
// with the rejections combined at the end):
//   pv = cross(d, e2); det = dot(e1, pv); inv_det = 1 / det; sv = o - v0; u = inv_det * dot(sv, pv); q = cross(sv, e1);
//   v = inv_det * dot(d, q); t = inv_det * dot(e2, q);
//   hit iff !(|det| < 1e-7), !(u < 0 or u > 1), !(v < 0 or u + v > 1) and t > 1e-7.  The caller compares t with its bound.
// hit_uv is the same u and v by the same operations on the same operands: the u, v of a record are those of the accepted test.
//
// A sample ray of a surfel (p, r_max, n) -- traced iff no component of p or n is a NaN and r_max > 0 (surfel_walked) -- is the
// build-defined sampling of DESIGN.md section 4: key = sample_key(seed, pixel, s), three rounds of the integer hash mix32;
// u1 = rnd(key, 0, 2), u2 = rnd(key, 0, 3), the top 24 bits of a hash times 2^-24; (c, s) = sincos_2pi(u2), the quadrant by
// floor(4 u2 + 0.5) and two fixed fmaf polynomials; l = (sqrt(u1) c, sqrt(u1) s, sqrt(1 - u1)) (cosine_local); d = (t l.x + bt l.y) + n l.z
// per component in the branch-free orthonormal basis (t, bt, n) of Duff et al. (cosine_world); o_k = p_k + n_k * bias (offset_origin).
#pragma once
#include <stdint.h>

#include "pt_closest.h"

namespace ptry {

constexpr float kInfT = 1e30f;          // renderer.wgsl:64
constexpr float kTriEps = 1e-7f;        // renderer.wgsl:178

using ptcp::dot;
PT_CP_FN void cross(float ax, float ay, float az, float bx, float by, float bz, float& cx, float& cy, float& cz) {
    cx = ay * bz - az * by; cy = az * bx - ax * bz; cz = ax * by - ay * bx;
}

PT_CP_FN float safe_inv(float d) { return __builtin_fabsf(d) > 1e-8f ? 1.0f / d : kInfT; }      // renderer.wgsl:74-80, per component

// a ray with a NaN anywhere, or with t_max <= 0, is a miss and is not walked (a NaN t_max fails the comparison as well)
PT_CP_FN bool ray_walked(float ox, float oy, float oz, float dx, float dy, float dz, float tmax) {
    const bool nan = __builtin_isnan(ox) | __builtin_isnan(oy) | __builtin_isnan(oz) | __builtin_isnan(dx) | __builtin_isnan(dy) | __builtin_isnan(dz);
    return !nan & (tmax > 0.0f);
}
// a surfel with a NaN in p, n or r_max, or with r_max <= 0, is not traced (a NaN r_max fails the comparison as well)
PT_CP_FN bool surfel_walked(float px, float py, float pz, float nx, float ny, float nz, float r_max) {
    const bool nan = __builtin_isnan(px) | __builtin_isnan(py) | __builtin_isnan(pz) | __builtin_isnan(nx) | __builtin_isnan(ny) | __builtin_isnan(nz);
    return !nan & (r_max > 0.0f);
}

// Whether the ray hits the triangle at t > kTriEps.  The all-zero record behind the last triangle is rejected: |det| < eps.
PT_CP_FN bool tri_hit(float ox, float oy, float oz, float dx, float dy, float dz, float v0x, float v0y, float v0z,
                      float e1x, float e1y, float e1z, float e2x, float e2y, float e2z, float& t) {
    float pvx, pvy, pvz; cross(dx, dy, dz, e2x, e2y, e2z, pvx, pvy, pvz);
    const float det = dot(e1x, e1y, e1z, pvx, pvy, pvz);
    const bool ok_det = !(__builtin_fabsf(det) < kTriEps);
    const float inv_det = 1.0f / det;
    const float svx = ox - v0x, svy = oy - v0y, svz = oz - v0z;
    const float u = inv_det * dot(svx, svy, svz, pvx, pvy, pvz);
    const bool ok_u = !((u < 0.0f) | (u > 1.0f));
    float qx, qy, qz; cross(svx, svy, svz, e1x, e1y, e1z, qx, qy, qz);
    const float v = inv_det * dot(dx, dy, dz, qx, qy, qz);
    const bool ok_v = !((v < 0.0f) | ((u + v) > 1.0f));
    t = inv_det * dot(e2x, e2y, e2z, qx, qy, qz);
    return ok_det & ok_u & ok_v & (t > kTriEps);
}
// (u, v of tri_hit, written out again: on one shared body the comparisons move behind t, and the ray kernels compile to other code)
PT_CP_FN void hit_uv(float ox, float oy, float oz, float dx, float dy, float dz, float v0x, float v0y, float v0z,
                     float e1x, float e1y, float e1z, float e2x, float e2y, float e2z, float& u, float& v) {
    float pvx, pvy, pvz; cross(dx, dy, dz, e2x, e2y, e2z, pvx, pvy, pvz);
    const float det = dot(e1x, e1y, e1z, pvx, pvy, pvz);
    const float inv_det = 1.0f / det;
    const float svx = ox - v0x, svy = oy - v0y, svz = oz - v0z;
    u = inv_det * dot(svx, svy, svz, pvx, pvy, pvz);
    float qx, qy, qz; cross(svx, svy, svz, e1x, e1y, e1z, qx, qy, qz);
    v = inv_det * dot(dx, dy, dz, qx, qy, qz);
}

PT_CP_FN uint32_t mix32(uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }
PT_CP_FN uint32_t sample_key(uint32_t seed, uint32_t pixel, uint32_t sidx) {
    uint32_t h = mix32(seed + 0x9E3779B9u);
    h = mix32(h ^ pixel);
    return mix32(h ^ sidx);
}
PT_CP_FN float rnd(uint32_t key, uint32_t bounce, uint32_t dim) {
    const uint32_t h = mix32(key ^ (bounce * 8u + dim + 1u) * 0x9E3779B1u);
    return (float)(h >> 8) * (1.0f / 16777216.0f);
}
PT_CP_FN void sincos_2pi(float u, float& c, float& s) {
    const float q = u * 4.0f;
    const float kf = __builtin_floorf(q + 0.5f);
    const float y = (q - kf) * 1.57079632679489662f;
    const float y2 = y * y;
    float sp = __builtin_fmaf(y2, 2.7557319e-6f, -1.9841270e-4f);
    sp = __builtin_fmaf(y2, sp, 8.3333333e-3f);
    sp = __builtin_fmaf(y2, sp, -1.6666667e-1f);
    sp = __builtin_fmaf(y2, sp, 1.0f);
    const float sy = y * sp;
    float cp = __builtin_fmaf(y2, -2.7557319e-7f, 2.4801587e-5f);
    cp = __builtin_fmaf(y2, cp, -1.3888889e-3f);
    cp = __builtin_fmaf(y2, cp, 4.1666667e-2f);
    cp = __builtin_fmaf(y2, cp, -0.5f);
    const float cy = __builtin_fmaf(y2, cp, 1.0f);
    const int k = (int)kf & 3;
    c = (k == 0) ? cy : (k == 1) ? -sy : (k == 2) ? -cy : sy;
    s = (k == 0) ? sy : (k == 1) ? cy : (k == 2) ? -sy : -cy;
}
// cosine-weighted direction around n in two halves: the sample in the local frame (independent of n) and its transfer into the
// branch-free orthonormal basis of n (Duff et al.)
PT_CP_FN void cosine_local(float u1, float u2, float& lx, float& ly, float& lz) {
    float c, s; sincos_2pi(u2, c, s);
    const float r = __builtin_sqrtf(u1);
    lx = r * c; ly = r * s; lz = __builtin_sqrtf(1.0f - u1);
}
PT_CP_FN void cosine_world(float nx, float ny, float nz, float lx, float ly, float lz, float& wx, float& wy, float& wz) {
    const float sign = __builtin_copysignf(1.0f, nz);
    const float a = -1.0f / (sign + nz);
    const float b = nx * ny * a;
    const float tx = 1.0f + sign * nx * nx * a, ty = sign * b, tz = -sign * nx;
    const float bx = b, by = sign + ny * ny * a, bz = -ny;
    // the nine products and six sums in the order of the vector expression (t * l.x + bt * l.y) + n * l.z
    const float tlx = tx * lx, tly = ty * lx, tlz = tz * lx;
    const float blx = bx * ly, bly = by * ly, blz = bz * ly;
    const float sx = tlx + blx, sy = tly + bly, sz = tlz + blz;
    const float nlx = nx * lz, nly = ny * lz, nlz = nz * lz;
    wx = sx + nlx; wy = sy + nly; wz = sz + nlz;
}
// a sample ray's origin, p + n * bias per component
PT_CP_FN void offset_origin(float px, float py, float pz, float nx, float ny, float nz, float bias, float& ox, float& oy, float& oz) {
    const float bx = nx * bias, by = ny * bias, bz = nz * bias;
    ox = px + bx; oy = py + by; oz = pz + bz;
}

} // namespace ptry
