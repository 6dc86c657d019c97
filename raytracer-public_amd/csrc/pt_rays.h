// pt_rays.h -- what the ray-side batched queries hold in common, once: pt_rayquery.hip (pt_trace_rays), pt_occlusion.hip (pt_occlusion),
// pt_crossings.hip (pt_count_hits, pt_contains) and pt_hitlist.hip (pt_list_hits).  The bit-for-bit contract between them -- a hit-list
// entry equals the pt_trace_rays record of its triangle, count >= 1 exactly where any-hit hits, a sample ray of pt_contains equals the
// pt_occlusion_rays record -- holds because each of these is one function here and not a copy per file; the arithmetic among them
// (ray_traced, hit_entry's u and v, surfel_traced, sample_ray) forwards to pt_raymath.h, the text the host twin compiles as well:
//   * load_ray, ray_traced                        a PtRay record and whether it is walked
//   * hit_entry                                   t, triangle, u, v of an accepted hit
//   * Surfel, load_surfel, surfel_traced, sample_ray
//   * count_same                                  one atomic per distinct id among the finishing lanes
//   * magic_of                                    the host's floor(2^32 / d) for divmod_magic
//   * RayState                                    the lane state of a persistent_walk Q (pt_walk.h) that walks a ray
//   * cross_traverse<STATS>                       the one-ray-per-thread walk whose `best` never moves, over a leaf functor
// Records: PtRay = two float4 (org.xyz, t_max | dir.xyz, reserved), PtSurfel = two float4 (p.xyz, r_max | n.xyz, reserved),
// PtHit = one uint4 (t bits, prim, u bits, v bits).
// The LDS streaming loop of the brute-force kernels (brute_records) and the list sink (ListSink) are pt_walk.h's, shared with the point side.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_kernels.h"
#include "pt_device.h"

namespace ptk {

__device__ __forceinline__ void load_ray(const float4* __restrict__ rays, uint32_t i, F3& o, F3& d, float& tmax) {
    const float4 a = rays[(size_t)i * 2], b = rays[(size_t)i * 2 + 1];
    o = f3(a.x, a.y, a.z); tmax = a.w; d = f3(b.x, b.y, b.z);
}
// a ray with a NaN anywhere, or with t_max <= 0, is a miss and is not traversed (a NaN t_max fails the comparison as well)
__device__ __forceinline__ bool ray_traced(F3 o, F3 d, float tmax) {
    return ptry::ray_walked(o.x, o.y, o.z, d.x, d.y, d.z, tmax);
}
// The 16-byte record of a hit at t on a fetched triangle record (three axis-major pieces: v0[a], e1[a], e2[a]; pt_host.h::TriRecord).
// u, v are recomputed with the arithmetic of the accepted test (renderer.wgsl:185-205, pt_device.h::traverse and pt_raymath.h::tri_hit;
// pt_raymath.h::hit_uv): the same operations on the same operands, so the same bits, and the traversal step keeps no registers for them.
__device__ __forceinline__ uint4 hit_entry(F3 o, F3 d, float t, uint32_t tri, const uint4 n0, const uint4 n1, const uint4 n2) {
    float u, v;
    ptry::hit_uv(o.x, o.y, o.z, d.x, d.y, d.z, __uint_as_float(n0.x), __uint_as_float(n1.x), __uint_as_float(n2.x),
                 __uint_as_float(n0.y), __uint_as_float(n1.y), __uint_as_float(n2.y),
                 __uint_as_float(n0.z), __uint_as_float(n1.z), __uint_as_float(n2.z), u, v);
    return make_uint4(__float_as_uint(t), tri, __float_as_uint(u), __float_as_uint(v));
}

struct Surfel { F3 p, n; float r_max; };
__device__ __forceinline__ Surfel load_surfel(const float4* __restrict__ surfels, uint32_t i) {
    const float4 a = surfels[(size_t)i * 2], b = surfels[(size_t)i * 2 + 1];
    Surfel s; s.p = f3(a.x, a.y, a.z); s.r_max = a.w; s.n = f3(b.x, b.y, b.z);
    return s;
}
// a surfel with a NaN in p, n or r_max, or with r_max <= 0, is not traced (a NaN r_max fails the comparison as well)
__device__ __forceinline__ bool surfel_traced(const Surfel& s) {
    return ptry::surfel_walked(s.p.x, s.p.y, s.p.z, s.n.x, s.n.y, s.n.z, s.r_max);
}
// sample ray s of the surfel with sample index `pixel` = index_base + i (mod 2^32): DESIGN.md section 4's cosine sampling around n as given
__device__ __forceinline__ void sample_ray(const Surfel& sf, uint32_t seed, uint32_t pixel, uint32_t s, float bias, F3& o, F3& d) {
    const uint32_t key = sample_key(seed, pixel, s);
    const float u1 = rnd(key, 0u, 2u), u2 = rnd(key, 0u, 3u);
    d = cosine_dir(sf.n, u1, u2);
    ptry::offset_origin(sf.p.x, sf.p.y, sf.p.z, sf.n.x, sf.n.y, sf.n.z, bias, o.x, o.y, o.z);
}

// The lanes of `flag` that hold the same id add their number to word 1 of out[id] with ONE atomic (the first of them issues it): the
// lanes of a chunk share a surfel or a point, and one same-address atomic per ray would serialise in the L2.  Wave-uniform loop over the
// distinct ids among the finishing lanes (one or two in practice).  Integer sums: any order gives the same bits.
__device__ __forceinline__ void count_same(uint4* __restrict__ out, bool flag, uint32_t id, uint32_t lane) {
    unsigned long long m = __ballot(flag);
    while (m != 0ull) {
        const int leader = __builtin_ctzll(m);
        const uint32_t i0 = (uint32_t)__shfl((int)id, leader, 64);
        const unsigned long long same = __ballot(flag && id == i0);
        if (lane == (uint32_t)leader) atomicAdd(&((uint32_t*)(out + i0))[1], (uint32_t)__popcll(same));
        m &= ~same;
    }
}

// floor(2^32 / d), saturated for d = 1 (divmod_magic's one correction covers the difference)
inline uint32_t magic_of(uint32_t d) { return d == 1u ? 0xFFFFFFFFu : (uint32_t)((1ull << 32) / d); }

// What persistent_walk's Q (pt_walk.h) of a ray holds whichever record the ray comes from and whatever becomes of its hits: the key of a
// child is tmin of its slab test, a stacked key is re-validated against `best`.  A Q derives from this and adds start(), leaf(),
// kWaveHooks and the hooks it uses.  A leaf whose triangle index is out of range points at the all-zero record behind the last
// triangle, which tri_hit rejects.
struct RayState {
    static constexpr float kKeyInit = kInfT;      // pt_device.h::order_children
    float best = 0.0f;
    F3 o = f3(0, 0, 0), d = o, inv = o; RaySel sel = ray_selectors(inv);

    // o, d and best are set: whether the ray enters the root
    __device__ __forceinline__ bool enter_root(const RenderArgs& A, bool scene_ok, bool walked) {
        inv = safe_inv(d); sel = ray_selectors(inv);
        Ray r; r.o = o; r.d = d; r.inv = inv;
        float troot;
        return scene_ok && walked && slab(r, A.root_box[0], A.root_box[1], A.root_box[2], best, troot);
    }
    __device__ __forceinline__ bool child(uint32_t w0, uint32_t w1, uint32_t w2, float& tmin) const { return lane_of(slab_sel(o, inv, sel, w0, w1, w2, best, tmin)); }
    __device__ __forceinline__ float bound() const { return best; }      // entries whose box the ray no longer reaches (tmin >= best) are skipped
    __device__ __forceinline__ void finish(const RenderArgs&) {}
    __device__ __forceinline__ void after_refill(uint32_t) {}
    __device__ __forceinline__ void after_step(bool, uint32_t) {}
};

// One ray per thread with a private 64-entry stack, `best` constant and no hit ending the ray: pt_device.h::traverse (the same visit
// order, cap and counters) with leaf(triangle, n0, n1, n2) called on every triangle record reached.
template <bool STATS, class Leaf>
__device__ __forceinline__ void cross_traverse(const RenderArgs& A, const Ray& r, uint2* __restrict__ stk, Counters& cnt, float best, Leaf leaf) {
    if (A.root_ref == kInvalidRef || A.num_tris == 0u) return;
    if (STATS) { cnt.nodes += 1; if (cnt.maxstack < 1u) cnt.maxstack = 1u; }
    if (A.root_degenerate) return;
    float troot;
    if (!slab(r, A.root_box[0], A.root_box[1], A.root_box[2], best, troot)) return;
    uint32_t cur = A.root_ref;
    int sp = 0;
    for (;;) {
        bool need_pop = false;
        if (cur & kLeaf) {
            const uint32_t ti4 = cur & 0x7fffffffu;
            if (ti4 < 4u * A.num_tris) {                          // an out-of-range leaf is skipped
                const uint4* tp = arena_record(A, cur);
                const uint4 n0 = tp[0], n1 = tp[1], n2 = tp[2];
                if (STATS) cnt.tris += 1;
                leaf(ti4 >> 2, n0, n1, n2);
            }
            need_pop = true;
        } else {
            const uint4* np = arena_record(A, cur);
            const uint4 n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3];
            float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f, t3 = 0.0f;
            const uint32_t r0 = n0.w, r1 = n1.w, r2 = n2.w, r3 = n3.w;
            const bool h0 = (r0 < kDegenerateRef) && slab(r, n0.x, n0.y, n0.z, best, t0);
            const bool h1 = (r1 < kDegenerateRef) && slab(r, n1.x, n1.y, n1.z, best, t1);
            const bool h2 = (r2 < kDegenerateRef) && slab(r, n2.x, n2.y, n2.z, best, t2);
            const bool h3 = (r3 < kDegenerateRef) && slab(r, n3.x, n3.y, n3.z, best, t3);
            if (STATS) cnt.nodes += (r0 != kInvalidRef) + (r1 != kInvalidRef) + (r2 != kInvalidRef) + (r3 != kInvalidRef);
            uint32_t enter;
            const int before = sp;
            const bool any = h0 | h1 | h2 | h3;
            const uint32_t wanted = (uint32_t)h0 + (uint32_t)h1 + (uint32_t)h2 + (uint32_t)h3;      // one entered, the others pushed
            const bool go = order_children(h0, h1, h2, h3, t0, t1, t2, t3, r0, r1, r2, r3, kInfT, sp, enter, [&](int at, uint32_t ref, float key) __attribute__((always_inline)) {
                stk[at] = make_uint2(ref, __float_as_uint(key));
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
                if (__uint_as_float(e.y) < best) { cur = e.x; found = true; break; }      // always passes: `best` never moves
            }
            if (!found) break;
        }
    }
}

} // namespace ptk
