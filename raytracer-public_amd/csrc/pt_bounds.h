// pt_bounds.h -- the box and build arithmetic of the scene build and the refit (DESIGN.md sections 3, 5, 12 and 14), ONE text for the
// kernels (pt_kernels.hip: LBVH2 leaves and refit walk; pt_build.hip: Morton codes, collapse, PLOC, records, wide nodes; pt_refit.hip;
// pt_cover.hip; pt_expose.hip) and the host twin (pt_host.cpp, pt_api.cpp): plain f32, f64 and u32 operations in a fixed order, each
// rounded once (both sides are compiled with -ffp-contract=off; the device's f32 division and square root are the correctly rounded
// ones), so both give the same bits.  No HIP header: pt_host.cpp is also built by a plain host compiler.
//
// A packed box is three words of six f16: w0 = mn.x | mn.y << 16, w1 = mn.z | mx.x << 16, w2 = mx.y | mx.z << 16 (renderer.wgsl:94-99).
//   decode      half_exact, the integer form of PathTracer.js:16-40: exact, subnormals included, whatever the FP mode (unpack_box)
//   encode      two rules.  store_bounds2 (BVHBuilder.wgsl:63-102): RTNE to f16, then one f16 step outwards in the
//               order of the patterns (step_f16) -- every LBVH2 / PLOC BVH2 box, and every leaf box of a refit.  pack_trunc
//               (PathTracer.js:42-51): truncate, flush below the normal range to the signed zero, saturate -- the internal BVH4 boxes
//               of the collapse (PathTracer.js:640-661) and of the BVH4 refit
//   min / max   three flavours, and every site keeps its own:
//               js_min_f / js_max_f   JS Math.min / Math.max on numbers: -0 below +0, a NaN operand loses every comparison and the
//                                     second operand is returned -- collapse and BVH4 refit unions, on both sides; on the host also
//                                     the PLOC leaf words and the PLOC BVH2 refit
//               wmin / wmax           v_min_f32 / v_max_f32: the non-NaN operand, -0 below +0 -- the leaf box of a triangle
//                                     (leaf_box_words: BVHBuilder.wgsl:278-306) and propagateUp (BVHBuilder.wgsl:242-275) on the device,
//                                     refit_bvh2 and the leaf rule of the refits on the host
//               sel_min / sel_max     b < a ? b : a, the f32 cluster boxes of PLOC, on both sides
//   Host and device do not use the same flavour at every corresponding site: the PLOC BVH2's leaf words and refit are js_min_f /
//   js_max_f over (a, b), c on the host and wmin / wmax over a, (b, c) in lbvh2_leaves_kernel.  The two agree except on NaN operands.
//   degenerate  any(mn > mx) on the decoded halves (renderer.wgsl:133, 244, 291), false where a NaN is involved
//   areas       node_area2: ((dx*dy) + (dy*dz)) + (dz*dx) in f32 from the decoded words, the key of the area-guided collapse;
//               union_extent + ploc_area: the same sum over the union of two f32 cluster boxes, NaN as +inf, the key of PLOC;
//               half_area: the f64 sum of pt_bvh_cost, 0 for a degenerate box, a NaN bound or inf * 0
//   Morton      centroid_axis = ((a + b) + c) / 3 in f64 (PathTracer.js:419-421), quantize1023 = max(0, min(1023, (x * 1023) | 0)),
//               spread10 (PathTracer.js:440-447)
//
// Two primitives have a body per side, the only #if blocks over __HIP_DEVICE_COMPILE__ in here:
//   f16_bits_rtne   the device has the conversion as one instruction (v_cvt_f16_f32, the (_Float16) cast); a plain host compiler
//                   need not have the type, so the host rounds in integers
//   wmin / wmax     on the device __builtin_fminf / __builtin_fmaxf ARE v_min_f32 / v_max_f32; the host builtin leaves the order
//                   of -0 and +0 open, so the host spells the instruction's rule out
// Everything above them (step_f16, the packers, the leaf box) is shared.
//
// Three short pieces stay written on each side, from the primitives in here, because the kernels compile to other code (the same
// instructions, other registers or another order) once they go through a shared function -- the yardstick is the device assembly of
// every file, profiles/boundsmath_asm_identity.txt:
//   the union of a BVH4 node's children   six js_min_f / js_max_f over half_exact of the child's halves, per child in slot order
//                                         (collapse_up_kernel, pt_refit.hip::finish_node; pt_host.cpp::union_children4): a shared
//                                         function takes the address of bounds a kernel carries round a loop
//   the Morton code                       (spread10(x) << 2) | (spread10(y) << 1) | spread10(z) (morton_kernel, morton_codes_sorted):
//                                         behind a call the operands of the two ors change places
//   the triangle record                   e1 = v1 - v0, e2 = v2 - v0, n = cross(e1, e2) * (1 / sqrt((c.x*c.x + c.y*c.y) + c.z*c.z))
//                                         (renderer.wgsl:179-180, 269; tri_records_kernel, build_tri_records): the kernel scales the
//                                         normal behind its first three stores
// For the same reason a kernel never hands a packer pointers to bounds it accumulates in a loop: store_bounds2 takes a Box of its own,
// pack_trunc_word six floats by value.
#pragma once
#include <stdint.h>

#include "pt_closest.h"

namespace ptbd {

// ---- layouts ---------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kNode2Stride = 6;            // BVHBuilder.wgsl:5
constexpr uint32_t kNode4Stride = 8;            // renderer.wgsl:10
constexpr uint32_t kLeafFlag    = 0x80000000u;  // renderer.wgsl:11
constexpr uint32_t kInvalid     = 0xFFFFFFFFu;  // renderer.wgsl:12
constexpr uint32_t kDegenerate  = 0xFFFFFFFEu;  // wide layout only: a child the reference fetches and then rejects for every ray (renderer.wgsl:289-291): counted, never entered
constexpr uint32_t kPlocRadius  = 16;           // PLOC's search radius in clusters
constexpr uint32_t kEmptyBox0 = 0x7C007C00u, kEmptyBox1 = 0xFC007C00u, kEmptyBox2 = 0xFC00FC00u;   // wide layout: box words of an empty or degenerate child slot, mn = +inf, mx = -inf (f16)

// Packed references: the traversal gathers triangle records (64 B) and wide nodes (64 B) from ONE arena, so a child reference
// is the record's position in it in 16-byte units -- `ref << 4` is the byte offset, and the shift drops the leaf flag:
//   leaf        kLeafFlag | 4 * tri                 (triangle record `tri` at byte 64 * tri)
//   wide node   node_base16 + 4 * index             (node `index` at byte 16 * node_base16 + 64 * index)
// A leaf whose triangle index is >= num_tris (the reference enters such a leaf and tests nothing, renderer.wgsl:262) points at
// the all-zero record behind the last triangle (index num_tris: never hit, |det| < eps).
PT_CP_FN uint32_t packed_leaf_ref(uint32_t tri, uint32_t num_tris) { return kLeafFlag | (4u * (tri < num_tris ? tri : num_tris)); }

// ---- f16 -------------------------------------------------------------------------------------------------------------------------
PT_CP_FN uint32_t bits_of(float f) { return __builtin_bit_cast(uint32_t, f); }
PT_CP_FN float float_of(uint32_t u) { return __builtin_bit_cast(float, u); }

PT_CP_FN float half_exact(uint32_t h) {
    const uint32_t sign = (h & 0x8000u) << 16, mag = h & 0x7fffu;
    if (mag >= 0x7c00u) return float_of(sign | 0x7f800000u | ((mag & 0x3ffu) << 13));    // inf / nan
    if (mag >= 0x0400u) return float_of(sign | ((mag + (112u << 10)) << 13));             // normal: rebias 15 -> 127
    const float v = (float)mag * 5.9604644775390625e-8f;                                  // zero / subnormal: mag * 2^-24, exact in f32
    return float_of(bits_of(v) | sign);
}
PT_CP_FN uint32_t half_trunc(float v) {
    const uint32_t u = bits_of(v);
    const uint32_t sign = (u >> 16) & 0x8000u;
    const int32_t e = (int32_t)((u >> 23) & 0xffu) - 112;
    if (e <= 0) return sign;                       // below the f16 normal range -> signed zero
    if (e >= 31) return sign | 0x7c00u;            // saturate (also inf / nan)
    return sign | ((uint32_t)e << 10) | ((u >> 13) & 0x3ffu);
}
#if defined(__HIP_DEVICE_COMPILE__)
PT_CP_FN uint32_t f16_bits_rtne(float v) { return (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)v); }
#else
PT_CP_FN uint32_t f16_bits_rtne(float v) {
    const uint32_t u = bits_of(v);
    const uint32_t sign = (u >> 16) & 0x8000u;
    uint32_t a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return sign | 0x7e00u;    // nan
    if (a >= 0x477ff000u) return sign | 0x7c00u;   // rounds to / is infinity
    if (a < 0x38800000u) {                         // below 2^-14: subnormal half
        if (a < 0x33000000u) return sign;          // < 2^-25
        // align the 24-bit significand so that bit 0 of the result is 2^-24
        const uint32_t sig = (a & 0x007fffffu) | 0x00800000u;
        const uint32_t shift = 126u - (a >> 23);   // 14..24
        const uint32_t q = sig >> shift;
        const uint32_t rest = sig & ((1u << shift) - 1u);
        const uint32_t halfway = 1u << (shift - 1u);
        return sign | (q + ((rest > halfway) || (rest == halfway && (q & 1u)) ? 1u : 0u));
    }
    // normal: add rounding bias in the f32 domain, then rebias the exponent
    const uint32_t lsb = (a >> 13) & 1u;
    a += 0x0fffu + lsb;
    return sign | ((a - (112u << 23)) >> 13);
}
#endif
PT_CP_FN uint32_t step_f16(float v, bool up) {        // BVHBuilder.wgsl:63-81, returns f16 bits
    const uint32_t bits = f16_bits_rtne(v);
    uint32_t ord = (bits & 0x8000u) ? ((~bits) & 0xFFFFu) : (bits ^ 0x8000u);
    ord = up ? ord + 1u : ord - 1u;
    return ((ord & 0x8000u) ? (ord ^ 0x8000u) : ((~ord) & 0xFFFFu)) & 0xFFFFu;
}

// ---- min / max -------------------------------------------------------------------------------------------------------------------
PT_CP_FN float js_min_f(float a, float b) { if (a < b) return a; if (b < a) return b; return (bits_of(a) >> 31) ? a : b; }
PT_CP_FN float js_max_f(float a, float b) { if (a > b) return a; if (b > a) return b; return (bits_of(a) >> 31) ? b : a; }
#if defined(__HIP_DEVICE_COMPILE__)
PT_CP_FN float wmin(float a, float b) { return __builtin_fminf(a, b); }
PT_CP_FN float wmax(float a, float b) { return __builtin_fmaxf(a, b); }
#else
PT_CP_FN float wmin(float a, float b) { if (a != a) return b; if (b != b) return a; return js_min_f(a, b); }
PT_CP_FN float wmax(float a, float b) { if (a != a) return b; if (b != b) return a; return js_max_f(a, b); }
#endif
PT_CP_FN float sel_min(float a, float b) { return b < a ? b : a; }
PT_CP_FN float sel_max(float a, float b) { return b > a ? b : a; }

// ---- boxes -----------------------------------------------------------------------------------------------------------------------
struct Box { float mn[3], mx[3]; };
// the six halves of a packed box, as f32 or widened to f64
template <class T> PT_CP_FN void unpack_box(uint32_t w0, uint32_t w1, uint32_t w2, T mn[3], T mx[3]) {
    mn[0] = half_exact(w0 & 0xffffu); mn[1] = half_exact(w0 >> 16); mn[2] = half_exact(w1 & 0xffffu);
    mx[0] = half_exact(w1 >> 16); mx[1] = half_exact(w2 & 0xffffu); mx[2] = half_exact(w2 >> 16);
}
PT_CP_FN Box unpack_box(const uint32_t w[3]) { Box b; unpack_box(w[0], w[1], w[2], b.mn, b.mx); return b; }
PT_CP_FN bool box_degenerate(uint32_t w0, uint32_t w1, uint32_t w2) {
    return half_exact(w0 & 0xffffu) > half_exact(w1 >> 16) || half_exact(w0 >> 16) > half_exact(w2 & 0xffffu) || half_exact(w1 & 0xffffu) > half_exact(w2 >> 16);
}
// The header computes the words; the caller decides how and when they reach memory.  A kernel that stores each word as it comes
// keeps its stores between the conversions: store_bounds2 hands word k to put(k, word) as soon as it is computed, pack_trunc_word
// computes word k alone.
template <class Put> PT_CP_FN void store_bounds2(const Box& b, Put put) {
    put(0, step_f16(b.mn[0], false) | (step_f16(b.mn[1], false) << 16));
    put(1, step_f16(b.mn[2], false) | (step_f16(b.mx[0], true) << 16));
    put(2, step_f16(b.mx[1], true) | (step_f16(b.mx[2], true) << 16));
}
PT_CP_FN uint32_t pack_trunc_word(float mn0, float mn1, float mn2, float mx0, float mx1, float mx2, int k) {
    return k == 0 ? half_trunc(mn0) | (half_trunc(mn1) << 16) : k == 1 ? half_trunc(mn2) | (half_trunc(mx0) << 16) : half_trunc(mx1) | (half_trunc(mx2) << 16);
}
PT_CP_FN void store_bounds2(const Box& b, uint32_t w[3]) { store_bounds2(b, [&](int k, uint32_t v) { w[k] = v; }); }
PT_CP_FN void pack_trunc(const Box& b, uint32_t w[3]) { for (int k = 0; k < 3; ++k) w[k] = pack_trunc_word(b.mn[0], b.mn[1], b.mn[2], b.mx[0], b.mx[1], b.mx[2], k); }
// the leaf box of the triangle t[0..8]: min / max of the three vertices as a, (b, c), stepped outwards
PT_CP_FN void leaf_box_words(const float* t, uint32_t w[3]) {
    const float v0x = t[0], v0y = t[1], v0z = t[2], v1x = t[3], v1y = t[4], v1z = t[5], v2x = t[6], v2y = t[7], v2z = t[8];
    const Box b = {{wmin(v0x, wmin(v1x, v2x)), wmin(v0y, wmin(v1y, v2y)), wmin(v0z, wmin(v1z, v2z))},
                   {wmax(v0x, wmax(v1x, v2x)), wmax(v0y, wmax(v1y, v2y)), wmax(v0z, wmax(v1z, v2z))}};
    store_bounds2(b, w);
}

// ---- areas -----------------------------------------------------------------------------------------------------------------------
PT_CP_FN float node_area2(uint32_t w0, uint32_t w1, uint32_t w2) {
    const float dx = half_exact(w1 >> 16) - half_exact(w0 & 0xffffu);
    const float dy = half_exact(w2 & 0xffffu) - half_exact(w0 >> 16);
    const float dz = half_exact(w2 >> 16) - half_exact(w1 & 0xffffu);
    return ((dx * dy) + (dy * dz)) + (dz * dx);
}
// PLOC: the extent of the union of two clusters along one axis (a = the cluster at the lower position), and the key from the three
PT_CP_FN float union_extent(float amx, float bmx, float amn, float bmn) { return sel_max(amx, bmx) - sel_min(amn, bmn); }
PT_CP_FN float ploc_area(float dx, float dy, float dz) {
    const float d = ((dx * dy) + (dy * dz)) + (dz * dx);
    return d == d ? d : float_of(0x7f800000u);
}
PT_CP_FN double half_area(uint32_t w0, uint32_t w1, uint32_t w2) {
    double mn[3], mx[3]; unpack_box(w0, w1, w2, mn, mx);
    if (!(mn[0] <= mx[0] && mn[1] <= mx[1] && mn[2] <= mx[2])) return 0.0;      // degenerate, or a NaN
    const double dx = mx[0] - mn[0], dy = mx[1] - mn[1], dz = mx[2] - mn[2];
    const double a = (dx * dy + dy * dz) + dz * dx;
    return a == a ? a : 0.0;                                                    // inf * 0
}

// ---- Morton codes (PathTracer.js:411-456), doubles throughout, like the JS -----------------------------------------------------
PT_CP_FN double centroid_axis(const float* p, int k) { return (((double)p[k] + (double)p[3 + k]) + (double)p[6 + k]) / 3; }
PT_CP_FN uint32_t spread10(uint32_t v) {
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
PT_CP_FN uint32_t quantize1023(double x) {
    const double s = x * 1023;
    if (!(s == s)) return 0u;                      // NaN | 0 == 0
    if (s >= 1023.0) return 1023u;
    if (s <= 0.0) return 0u;
    return (uint32_t)(int32_t)s;                   // truncation toward zero
}

} // namespace ptbd
