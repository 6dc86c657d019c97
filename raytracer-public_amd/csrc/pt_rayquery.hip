// pt_rayquery.hip -- batched ray queries over the context's scene (include/mi355pt.h: pt_trace_rays, pt_camera_rays):
//   * trace_rays_kernel<ANYHIT>              the default: persistent wavefronts, one ray per lane, a lane whose ray has ended takes the
//                                            next ray of its wavefront's chunk (64 rays per queue claim)
//   * trace_rays_simple_kernel<ANYHIT,STATS> one ray per thread over the renderer's traverse() (pt_device.h): PT_TRACE_SIMPLE_KERNEL, PT_TRACE_STATS
//   * camera_rays_kernel                     the primary rays of PT_MODE_REFERENCE, written out as PtRay records
//
// Both trace kernels walk the tree exactly as render_rays_kernel does (visit order, first-minimum ties, pushes far -> near, the silent drop at
// 64 entries, re-validation at pop) with `best` starting at min(t_max, kInfT), so with t_max = +inf a result is the oracle's orc_trace_ray, bit for bit.
// Records: PtRay = two float4 (org.xyz, t_max | dir.xyz, reserved), PtHit = one uint4 (t bits, prim, u bits, v bits).
// The ray record, the hit record and the lane state of the walk are pt_rays.h's, shared with the occlusion, crossing and hit-list queries.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_kernels.h"
#include "pt_device.h"
#include "pt_rays.h"
#include "pt_walk.h"

namespace ptk {

// The 16-byte result: pt_rays.h::hit_entry on the winning triangle's record, or the miss
__device__ __forceinline__ uint4 hit_record(const RenderArgs& A, F3 o, F3 d, float t, uint32_t tri) {
    if (tri == kInvalidRef) return make_uint4(0x7F800000u, kInvalidRef, 0u, 0u);      // +inf, no triangle, u = v = 0
    const uint4* tp = (const uint4*)A.tris + (size_t)tri * 4;
    return hit_entry(o, d, t, tri, tp[0], tp[1], tp[2]);
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
// persistent_walk's Q (pt_walk.h) of a traced ray: RayState (pt_rays.h) with the closest triangle so far; `best` starts at
// min(t_max, kInfT) and shrinks to each accepted hit.
template <bool ANYHIT>
struct RayWalk : RayState {
    static constexpr bool kWaveHooks = false;
    const float4* __restrict__ rays; uint4* __restrict__ hits;
    uint32_t rid = 0, btri = kInvalidRef;

    __device__ __forceinline__ bool start(const RenderArgs& A, uint32_t item, bool scene_ok) {
        rid = item;
        float tmax;
        load_ray(rays, rid, o, d, tmax);
        best = wmin(tmax, kInfT); btri = kInvalidRef;
        if (enter_root(A, scene_ok, ray_traced(o, d, tmax))) return true;
        hits[rid] = hit_record(A, o, d, 0.0f, kInvalidRef);
        return false;
    }
    __device__ __forceinline__ bool leaf(uint32_t cur, const uint4 n0, const uint4 n1, const uint4 n2) {
        float t;
        if (tri_hit(o, d, n0, n1, n2, t) & (t < best)) { best = t; btri = cur; return ANYHIT; }
        return false;
    }
    __device__ __forceinline__ void finish(const RenderArgs& A) { hits[rid] = hit_record(A, o, d, best, btri == kInvalidRef ? kInvalidRef : (btri & 0x7fffffffu) >> 2); }
};
template <bool ANYHIT>
__global__ __launch_bounds__(64) void trace_rays_kernel(const RenderArgs A, const float4* __restrict__ rays, uint4* __restrict__ hits, uint32_t n,
                                                        unsigned long long* __restrict__ queue, unsigned long long* __restrict__ spill, uint32_t fill) {
    RayWalk<ANYHIT> q; q.rays = rays; q.hits = hits;
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
