// pt_rayquery.hip -- batched ray queries over the context's scene (include/mi355pt.h: pt_trace_rays, pt_camera_rays):
//   * trace_rays_kernel<ANYHIT>              the default: persistent wavefronts, one ray per lane, a lane whose ray has ended takes the
//                                            next ray of its wavefront's chunk (64 rays per queue claim)
//   * trace_rays_simple_kernel<ANYHIT,STATS> one ray per thread over the renderer's traverse() (pt_device.h): PT_TRACE_SIMPLE_KERNEL, PT_TRACE_STATS
//   * camera_rays_kernel                     the primary rays of PT_MODE_REFERENCE, written out as PtRay records
//
// Both trace kernels walk the tree exactly as render_rays_kernel does (visit order, first-minimum ties, pushes far -> near, the silent drop at
// 64 entries, re-validation at pop) with `best` starting at min(t_max, kInfT), so with t_max = +inf a result is the oracle's orc_trace_ray, bit for bit.
// Records: PtRay = two float4 (org.xyz, t_max | dir.xyz, reserved), PtHit = one uint4 (t bits, prim, u bits, v bits).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_kernels.h"
#include "pt_device.h"
#include "pt_walk.h"

namespace ptk {

__device__ __forceinline__ void load_ray(const float4* __restrict__ rays, uint32_t i, F3& o, F3& d, float& tmax) {
    const float4 a = rays[(size_t)i * 2], b = rays[(size_t)i * 2 + 1];
    o = f3(a.x, a.y, a.z); tmax = a.w; d = f3(b.x, b.y, b.z);
}
// a ray with a NaN anywhere, or with t_max <= 0, is a miss and is not traversed (a NaN t_max fails the comparison as well)
__device__ __forceinline__ bool ray_traced(F3 o, F3 d, float tmax) {
    const bool nan = __builtin_isnan(o.x) | __builtin_isnan(o.y) | __builtin_isnan(o.z) | __builtin_isnan(d.x) | __builtin_isnan(d.y) | __builtin_isnan(d.z);
    return !nan & (tmax > 0.0f);
}
// The 16-byte result.  u, v are recomputed from the winning triangle's record with the arithmetic of the accepted test
// (renderer.wgsl:185-205, pt_device.h::traverse): the same operations on the same operands, so the same bits, and the traversal
// step keeps no registers for them.
__device__ __forceinline__ uint4 hit_record(const RenderArgs& A, F3 o, F3 d, float t, uint32_t tri) {
    if (tri == kInvalidRef) return make_uint4(0x7F800000u, kInvalidRef, 0u, 0u);      // +inf, no triangle, u = v = 0
    const float4* tp = A.tris + (size_t)tri * 4;
    const float4 a = tp[0], b = tp[1], c = tp[2];
    const F3 v0 = f3(a.x, b.x, c.x), e1 = f3(a.y, b.y, c.y), e2 = f3(a.z, b.z, c.z);   // axis-major record (pt_host.h::TriRecord)
    const F3 p = cross3(d, e2);
    const float det = dot3(e1, p);
    const float inv_det = 1.0f / det;
    const F3 s = o - v0;
    const float u = inv_det * dot3(s, p);
    const F3 q = cross3(s, e1);
    const float v = inv_det * dot3(d, q);
    return make_uint4(__float_as_uint(t), tri, __float_as_uint(u), __float_as_uint(v));
}

// ------------------------------------------------------------------------------------
// simple kernel: one ray per thread, the renderer's traversal with its 64-entry private stack
// ------------------------------------------------------------------------------------
template <bool ANYHIT, bool STATS>
__global__ __launch_bounds__(256) void trace_rays_simple_kernel(const RenderArgs A, const float4* __restrict__ rays, uint4* __restrict__ hits, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    Counters cnt; cnt.nodes = cnt.tris = cnt.drops = cnt.maxstack = 0;
    uint32_t n_rays = 0;
    if (i < n) {
        F3 o, d; float tmax;
        load_ray(rays, i, o, d, tmax);
        float t = __uint_as_float(0x7F800000u); uint32_t tri = kInvalidRef;
        n_rays = 1;
        if (ray_traced(o, d, tmax)) {
            Ray r; r.o = o; r.d = d; r.inv = safe_inv(d);
            uint2 stk[kStackMax];
            float bt; uint32_t bi;
            if (traverse<ANYHIT, STATS>(A, r, bt, bi, stk, cnt, wmin(tmax, kInfT))) { t = bt; tri = bi; }
        }
        hits[i] = hit_record(A, o, d, t, tri);
    }
    if (STATS) add_stats(A, ANYHIT ? 1 : 0, n_rays, cnt);
}

// ------------------------------------------------------------------------------------
// persistent kernel: one wavefront per workgroup, one ray per lane, lanes refilled from the wavefront's chunk
// ------------------------------------------------------------------------------------
// persistent_walk's Q (pt_walk.h) of a ray: the key of a child is tmin of its slab test, `best` starts at min(t_max, kInfT).  A leaf whose
// triangle index is out of range points at the all-zero record behind the last triangle, which tri_hit rejects.
template <bool ANYHIT>
struct RayWalk {
    static constexpr bool kWaveHooks = false;
    static constexpr float kKeyInit = kInfT;      // pt_device.h::order_children
    const float4* __restrict__ rays; uint4* __restrict__ hits;
    uint32_t rid = 0, btri = kInvalidRef; float best = 0.0f;
    F3 o = f3(0, 0, 0), d = o, inv = o; RaySel sel = ray_selectors(inv);

    __device__ __forceinline__ bool start(const RenderArgs& A, uint32_t item, bool scene_ok) {
        rid = item;
        float tmax;
        load_ray(rays, rid, o, d, tmax);
        best = wmin(tmax, kInfT); btri = kInvalidRef;
        inv = safe_inv(d); sel = ray_selectors(inv);
        Ray r; r.o = o; r.d = d; r.inv = inv;
        float troot;
        if (scene_ok && ray_traced(o, d, tmax) && slab(r, A.root_box[0], A.root_box[1], A.root_box[2], best, troot)) return true;
        hits[rid] = hit_record(A, o, d, 0.0f, kInvalidRef);
        return false;
    }
    __device__ __forceinline__ bool child(uint32_t w0, uint32_t w1, uint32_t w2, float& tmin) const { return lane_of(slab_sel(o, inv, sel, w0, w1, w2, best, tmin)); }
    __device__ __forceinline__ bool leaf(uint32_t cur, const uint4 n0, const uint4 n1, const uint4 n2) {
        float t;
        if (tri_hit(o, d, n0, n1, n2, t) & (t < best)) { best = t; btri = cur; return ANYHIT; }
        return false;
    }
    __device__ __forceinline__ float bound() const { return best; }      // entries whose box the ray no longer reaches (tmin >= best) are skipped
    __device__ __forceinline__ void finish(const RenderArgs& A) { hits[rid] = hit_record(A, o, d, best, btri == kInvalidRef ? kInvalidRef : (btri & 0x7fffffffu) >> 2); }
    __device__ __forceinline__ void after_refill(uint32_t) {}
    __device__ __forceinline__ void after_step(bool, uint32_t) {}
};
template <bool ANYHIT>
__global__ __launch_bounds__(64) void trace_rays_kernel(const RenderArgs A, const float4* __restrict__ rays, uint4* __restrict__ hits, uint32_t n,
                                                        unsigned long long* __restrict__ queue, unsigned long long* __restrict__ spill, uint32_t fill) {
    RayWalk<ANYHIT> q{rays, hits};
    persistent_walk<PT_RQ_SHORT_STACK>(A, n, queue, spill, fill, q);
}

// the camera rays of PT_MODE_REFERENCE: one through each pixel centre (renderer.wgsl:387-395), row-major, t_max = +inf
__global__ __launch_bounds__(256) void camera_rays_kernel(const RenderArgs A, float4* __restrict__ rays) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.width * A.height) return;
    const uint32_t px = i % A.width, py = i / A.width;
    const Ray r = primary_ray(A, (float)px + 0.5f, (float)py + 0.5f);
    rays[(size_t)i * 2] = make_float4(r.o.x, r.o.y, r.o.z, __uint_as_float(0x7F800000u));
    rays[(size_t)i * 2 + 1] = make_float4(r.d.x, r.d.y, r.d.z, 0.0f);
}

hipError_t launch_trace_rays(const RenderArgs& A, const void* rays, void* hits, uint32_t n, bool anyhit, bool simple, bool stats,
                             unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    const float4* r = (const float4*)rays; uint4* h = (uint4*)hits;
    if (simple || stats) {
        const dim3 g((n + 255u) / 256u);
        if (stats) {
            if (anyhit) trace_rays_simple_kernel<true, true><<<g, 256, 0, stream>>>(A, r, h, n);
            else trace_rays_simple_kernel<false, true><<<g, 256, 0, stream>>>(A, r, h, n);
        } else {
            if (anyhit) trace_rays_simple_kernel<true, false><<<g, 256, 0, stream>>>(A, r, h, n);
            else trace_rays_simple_kernel<false, false><<<g, 256, 0, stream>>>(A, r, h, n);
        }
        return hipGetLastError();
    }
    hipError_t e = walk_begin(queue, n, grid, stream);
    if (e != hipSuccess) return e;
    if (anyhit) trace_rays_kernel<true><<<grid, 64, 0, stream>>>(A, r, h, n, queue, spill, PT_RQ_FILL);
    else trace_rays_kernel<false><<<grid, 64, 0, stream>>>(A, r, h, n, queue, spill, PT_RQ_FILL);
    return hipGetLastError();
}

hipError_t launch_camera_rays(const RenderArgs& A, void* rays, hipStream_t stream) {
    const uint32_t n = A.width * A.height;
    camera_rays_kernel<<<dim3((n + 255u) / 256u), 256, 0, stream>>>(A, (float4*)rays);
    return hipGetLastError();
}

} // namespace ptk
