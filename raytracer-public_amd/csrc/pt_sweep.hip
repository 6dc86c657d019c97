// pt_sweep.hip -- sphere-cast queries over the context's tree: the first contact of a sphere of radius r that moves from o along d
// (include/mi355pt.h: pt_sweep_spheres):
//   * sweep_kernel                 the default: persistent wavefronts, one sweep per lane, a lane whose sweep is answered takes the next
//                                  sweep of its wavefront's chunk (64 sweeps per queue claim)
//   * sweep_simple_kernel<STATS>   one sweep per thread with a private 64-entry stack: PT_SWEEP_SIMPLE_KERNEL, PT_SWEEP_STATS
//   * sweep_brute_kernel<STATS>    every triangle in index order, the records streamed through LDS: PT_SWEEP_BRUTE_FORCE
//
// The walk is the ray queries' (pt_walk.h::persistent_walk): a child is entered iff the sign-selected slab test passes on its packed f16
// box grown by R = r + s (s = ptcp::kSlack) and its key tmin is below `best`; passing children keep slot order, the first minimum trades
// places with the first of them and is entered next, the others are pushed far -> near, a push at 64 entries is dropped, a stacked child is
// re-validated at pop.  `best` starts at t_max and shrinks to each accepted t_T (to -inf behind a contact at 0, which ends the walk:
// ptsw::bound_after).  The growth is taken on the origin's side: the lane keeps
// o + R and o - R per axis, sorted once by the sign of inv into the origin that goes with the near bound and the one that goes with the
// far bound, so a node costs what a ray's node costs.  The triangle arithmetic is pt_sweep.h, shared with the host twin
// (pt_host.cpp::sweep_spheres), which gives the same bits.
// Records: PtSweep = two float4 (org.xyz, t_max | dir.xyz, radius), PtHit = one uint4 (t bits, prim, u bits, v bits).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_kernels.h"
#include "pt_device.h"
#include "pt_sweep.h"
#include "pt_points.h"
#include "pt_rays.h"
#include "pt_walk.h"

namespace ptk {

// pt_device.h::slab_sel with an origin of its own for the near and for the far bound of every axis: on = o + R where inv >= 0 (the near
// bound is mn) and o - R where inv < 0 (the near bound is mx), of the other one.  (mn - (o + R)) * inv and (mx - (o - R)) * inv are
// ptsw::node_pass's a and b; the selection by sign is its near / far.  Returns the hit mask of the wavefront's active lanes.
__device__ __forceinline__ unsigned long long sweep_slab_sel(const F3& on, const F3& of, const F3& inv, const RaySel& sel, uint32_t w0, uint32_t w1, uint32_t w2,
                                                             float best, float& tmin_out) {
    const uint32_t bx = __builtin_amdgcn_perm(w1, w0, sel.x), by = __builtin_amdgcn_perm(w2, w0, sel.y), bz = __builtin_amdgcn_perm(w2, w1, sel.z);
    const float nx = half_lo_minus(bx, on.x) * inv.x, ny = half_lo_minus(by, on.y) * inv.y, nz = half_lo_minus(bz, on.z) * inv.z;
    const float fx = half_hi_minus(bx, of.x) * inv.x, fy = half_hi_minus(by, of.y) * inv.y, fz = half_hi_minus(bz, of.z) * inv.z;
    const float tmin = wmax(wmax(nx, ny), nz);
    const float tmax = wmin(wmin(fx, fy), fz);
    tmin_out = tmin;
    return __builtin_amdgcn_ballot_w64(tmax >= wmax(tmin, 0.0f)) & __builtin_amdgcn_ballot_w64(tmin < best);
}

// What a sweep holds for the walk besides RayState's o, d, inv, sel and best
struct SweepItem {
    float r = 0.0f; F3 on = f3(0, 0, 0), of = on;

    // o and d are set: inv, sel and the two origins
    __device__ __forceinline__ void setup(const F3& o, const F3& d, F3& inv, RaySel& sel) {
        inv = safe_inv(d); sel = ray_selectors(inv);
        const float R = r + ptcp::kSlack;
        const F3 op = f3(o.x + R, o.y + R, o.z + R), om = f3(o.x - R, o.y - R, o.z - R);
        on = f3(inv.x < 0.0f ? om.x : op.x, inv.y < 0.0f ? om.y : op.y, inv.z < 0.0f ? om.z : op.z);
        of = f3(inv.x < 0.0f ? op.x : om.x, inv.y < 0.0f ? op.y : om.y, inv.z < 0.0f ? op.z : om.z);
    }
};
__device__ __forceinline__ bool load_sweep(const float4* __restrict__ sweeps, uint32_t i, F3& o, F3& d, float& tmax, float& r) {
    const float4 a = sweeps[(size_t)i * 2], b = sweeps[(size_t)i * 2 + 1];
    o = f3(a.x, a.y, a.z); tmax = a.w; d = f3(b.x, b.y, b.z); r = b.w;
    return ptsw::sweep_walked(a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w);
}
// t_T of one triangle record (three axis-major pieces: v0[a], e1[a], e2[a])
__device__ __forceinline__ float tri_sweep(const F3& o, const F3& d, const F3& inv, float r, float best, const float4 a, const float4 b, const float4 c) {
    return ptsw::tri_sweep(o.x, o.y, o.z, d.x, d.y, d.z, inv.x, inv.y, inv.z, r, best, a.x, b.x, c.x, a.y, b.y, c.y, a.z, b.z, c.z);
}
// The 16-byte result: t, the triangle, and u, v of the contact point recomputed from the winning record; or the miss
__device__ __forceinline__ uint4 sweep_record(const float4* __restrict__ tris, const F3& o, const F3& d, float t, uint32_t tri) {
    if (tri == kInvalidRef) return make_uint4(kInfBits, kInvalidRef, 0u, 0u);
    const float4* tp = tris + (size_t)tri * 4;
    const float4 a = tp[0], b = tp[1], c = tp[2];
    float u, v;
    ptsw::contact_uv(o.x, o.y, o.z, d.x, d.y, d.z, t, a.x, b.x, c.x, a.y, b.y, c.y, a.z, b.z, c.z, u, v);
    return make_uint4(__float_as_uint(t), tri, __float_as_uint(u), __float_as_uint(v));
}

// ------------------------------------------------------------------------------------
// simple kernel: one sweep per thread, a private 64-entry stack (pt_points.h::key_traverse, whose bound the leaves lower); the counters
// of PT_SWEEP_STATS by the rules of traverse<..., STATS>
// ------------------------------------------------------------------------------------
template <bool STATS>
__global__ __launch_bounds__(256) void sweep_simple_kernel(const RenderArgs A, const float4* __restrict__ sweeps, uint4* __restrict__ hits, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    Counters cnt; cnt.nodes = cnt.tris = cnt.drops = cnt.maxstack = 0;
    uint32_t n_items = 0;
    if (i < n) {
        F3 o, d; float best; SweepItem s;
        const bool walked = load_sweep(sweeps, i, o, d, best, s.r);
        uint32_t tri = kInvalidRef;
        n_items = 1;
        if (walked) {
            F3 inv; RaySel sel;
            s.setup(o, d, inv, sel);
            uint2 stk[kStackMax];
            key_traverse<STATS>(A, [&](uint32_t w0, uint32_t w1, uint32_t w2, float& key) __attribute__((always_inline)) {
                return lane_of(sweep_slab_sel(s.on, s.of, inv, sel, w0, w1, w2, best, key));
            }, best, stk, cnt, [&](uint32_t cur, const float4 a, const float4 b, const float4 c) __attribute__((always_inline)) {
                const float t = tri_sweep(o, d, inv, s.r, best, a, b, c);
                if (t < best) { best = ptsw::bound_after(t); tri = (cur & 0x7fffffffu) >> 2; }
            });
        }
        hits[i] = sweep_record(A.tris, o, d, ptsw::time_of(best), tri);
    }
    if (STATS) add_stats(A, 0, n_items, cnt);
}

// ------------------------------------------------------------------------------------
// persistent kernel: one wavefront per workgroup, one sweep per lane, lanes refilled from the wavefront's chunk
// ------------------------------------------------------------------------------------
// persistent_walk's Q (pt_walk.h) of a sweep: RayState (pt_rays.h) with the grown-box test in place of the ray's, the radius and the
// triangle touched first so far.  A leaf is gated on leaf_end: an out-of-range leaf points at the all-zero record behind the last
// triangle, whose vertex at the origin must not count.
struct SweepWalk : RayState {
    static constexpr bool kWaveHooks = false;
    const float4* __restrict__ sweeps; uint4* __restrict__ hits; const float4* __restrict__ tris; uint32_t leaf_end;
    uint32_t rid = 0, btri = kInvalidRef;
    SweepItem s;

    __device__ __forceinline__ bool start(const RenderArgs& A, uint32_t item, bool scene_ok) {
        rid = item;
        const bool walked = load_sweep(sweeps, rid, o, d, best, s.r);
        btri = kInvalidRef;
        s.setup(o, d, inv, sel);
        float troot;
        const bool in = lane_of(sweep_slab_sel(s.on, s.of, inv, sel, A.root_box[0], A.root_box[1], A.root_box[2], best, troot));
        if (scene_ok && walked && in) return true;
        hits[rid] = make_uint4(kInfBits, kInvalidRef, 0u, 0u);
        return false;
    }
    __device__ __forceinline__ bool child(uint32_t w0, uint32_t w1, uint32_t w2, float& tmin) const {
        return lane_of(sweep_slab_sel(s.on, s.of, inv, sel, w0, w1, w2, best, tmin));
    }
    __device__ __forceinline__ bool leaf(uint32_t cur, const uint4 n0, const uint4 n1, const uint4 n2) {
        const float t = tri_sweep(o, d, inv, s.r, best, as_float4(n0), as_float4(n1), as_float4(n2));
        if (((cur & 0x7fffffffu) < leaf_end) & (t < best)) { best = ptsw::bound_after(t); btri = cur; }
        return false;
    }
    __device__ __forceinline__ void finish(const RenderArgs&) { hits[rid] = sweep_record(tris, o, d, ptsw::time_of(best), btri == kInvalidRef ? kInvalidRef : (btri & 0x7fffffffu) >> 2); }
};
// amdgpu_waves_per_eu: left alone the allocator took 84 VGPRs (5 waves per SIMD); asked for PT_SW_WAVES_PER_SIMD it stays within 80 with
// no scratch and no spills, which is what tests/test_sweep_resources.py pins
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(PT_SW_WAVES_PER_SIMD, PT_SW_WAVES_PER_SIMD))) void sweep_kernel(const RenderArgs A, const float4* __restrict__ sweeps, uint4* __restrict__ hits, uint32_t n,
                                                   unsigned long long* __restrict__ queue, unsigned long long* __restrict__ spill, uint32_t fill) {
    SweepWalk q; q.sweeps = sweeps; q.hits = hits; q.tris = A.tris; q.leaf_end = 4u * A.num_tris;
    persistent_walk<PT_SW_SHORT_STACK>(A, n, queue, spill, fill, q);
}

// ------------------------------------------------------------------------------------
// brute force: one sweep per thread, every triangle in index order (pt_walk.h::brute_records)
// ------------------------------------------------------------------------------------
template <bool STATS>
__global__ __launch_bounds__(256) void sweep_brute_kernel(const RenderArgs A, const float4* __restrict__ sweeps, uint4* __restrict__ hits, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    F3 o = f3(0, 0, 0), d = o; float best = 0.0f, r = 0.0f;
    const bool walked = (i < n) && load_sweep(sweeps, i, o, d, best, r);
    const F3 inv = safe_inv(d);
    uint32_t tri = kInvalidRef;
    brute_records(A, walked, [&](uint32_t t, const uint4 n0, const uint4 n1, const uint4 n2) __attribute__((always_inline)) {
        const float tt = tri_sweep(o, d, inv, r, best, as_float4(n0), as_float4(n1), as_float4(n2));
        if (tt < best) { best = ptsw::bound_after(tt); tri = t; }
    });
    if (i < n) hits[i] = sweep_record(A.tris, o, d, ptsw::time_of(best), tri);
    if (STATS) {
        Counters cnt; cnt.nodes = cnt.drops = cnt.maxstack = 0;
        cnt.tris = walked ? A.num_tris : 0u;                              // a walked sweep tests every record
        add_stats(A, 0, i < n ? 1u : 0u, cnt);
    }
}

hipError_t launch_sweep(const RenderArgs& A, const void* sweeps, void* hits, uint32_t n, bool simple, bool stats, bool brute,
                        unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    const float4* s = (const float4*)sweeps; uint4* h = (uint4*)hits;
    const dim3 g256((n + 255u) / 256u);
    if (brute) {
        if (stats) sweep_brute_kernel<true><<<g256, 256, 0, stream>>>(A, s, h, n);
        else sweep_brute_kernel<false><<<g256, 256, 0, stream>>>(A, s, h, n);
        return hipGetLastError();
    }
    if (simple || stats) {
        if (stats) sweep_simple_kernel<true><<<g256, 256, 0, stream>>>(A, s, h, n);
        else sweep_simple_kernel<false><<<g256, 256, 0, stream>>>(A, s, h, n);
        return hipGetLastError();
    }
    hipError_t e = walk_begin(queue, n, grid, stream);
    if (e != hipSuccess) return e;
    sweep_kernel<<<grid, 64, 0, stream>>>(A, s, h, n, queue, spill, PT_SW_FILL);
    return hipGetLastError();
}

} // namespace ptk
