// pt_pointquery.hip -- batched closest-point queries over the context's tree (include/mi355pt.h: pt_closest_points):
//   * closest_points_kernel               the default: persistent wavefronts, one point per lane, a lane whose point is answered takes the
//                                         next point of its wavefront's chunk (64 points per queue claim)
//   * closest_points_simple_kernel<STATS> one point per thread with a private 64-entry stack: PT_CLOSEST_SIMPLE_KERNEL, PT_CLOSEST_STATS
//   * closest_points_brute_kernel         every triangle in index order, the records streamed through LDS: PT_CLOSEST_BRUTE_FORCE
//
// The walk is the ray queries' (pt_walk.h::persistent_walk, pt_device.h::traverse) with bound2, a squared lower bound of the distance from the point to
// a child's box, in place of tmin: children with bound2 < best2 keep slot order, the first minimum trades places with the first of them and is
// entered next, the others are pushed far -> near, a push at 64 entries is dropped, a stacked child is re-validated at pop.  The
// point-triangle arithmetic is pt_closest.h, shared with the host twin (pt_host.cpp::closest_points), which gives the same bits.
// The point record, the slack, box_bound2, tri_d2 and the one-point-per-thread walk (key_traverse) are pt_points.h's, shared with
// pt_radius.hip, pt_knn.hip and pt_overlap.hip; the LDS streaming loop (brute_records) is pt_walk.h's.
// Records: PtPoint = one float4 (p.xyz, r_max), PtClosest = one uint4 (dist bits, prim, u bits, v bits).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_kernels.h"
#include "pt_device.h"
#include "pt_closest.h"
#include "pt_points.h"
#include "pt_walk.h"

namespace ptk {

// The 16-byte result: dist = sqrtf(best2), u and v recomputed from the winning triangle's record with the operations of the accepted test
__device__ __forceinline__ uint4 closest_record(const float4* __restrict__ tris, F3 p, float best2, uint32_t tri) {
    if (tri == kInvalidRef) return make_uint4(kInfBits, kInvalidRef, 0u, 0u);
    const float4* tp = tris + (size_t)tri * 4;
    const float4 a = tp[0], b = tp[1], c = tp[2];
    float u, v;
    ptcp::closest_uv(p.x - a.x, p.y - b.x, p.z - c.x, a.y, b.y, c.y, a.z, b.z, c.z, u, v);
    return make_uint4(__float_as_uint(sqrtf(best2)), tri, __float_as_uint(u), __float_as_uint(v));
}

// ------------------------------------------------------------------------------------
// simple kernel: one point per thread, a private 64-entry stack (pt_points.h::key_traverse, whose bound the leaves lower); the counters
// of PT_CLOSEST_STATS by the rules of traverse<..., STATS>
// ------------------------------------------------------------------------------------
template <bool STATS>
__device__ __forceinline__ void walk_point(const RenderArgs& A, F3 p, float& best2, uint32_t& best_tri, uint2* __restrict__ stk, Counters& cnt) {
    best_tri = kInvalidRef;
    const PointSlack s = point_slack(p);
    key_traverse<STATS>(A, [&](uint32_t w0, uint32_t w1, uint32_t w2, float& key) __attribute__((always_inline)) { key = box_bound2(s, w0, w1, w2); return key < best2; }, best2, stk, cnt,
                        [&](uint32_t cur, const float4 a, const float4 b, const float4 c) __attribute__((always_inline)) {
        const float d2 = tri_d2(p, a, b, c);
        if (d2 < best2) { best2 = d2; best_tri = (cur & 0x7fffffffu) >> 2; }
    });
}

template <bool STATS>
__global__ __launch_bounds__(256) void closest_points_simple_kernel(const RenderArgs A, const float4* __restrict__ pts, uint4* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    Counters cnt; cnt.nodes = cnt.tris = cnt.drops = cnt.maxstack = 0;
    uint32_t n_pts = 0;
    if (i < n) {
        F3 p; float rmax;
        load_point(pts, i, p, rmax);
        float best2 = rmax * rmax; uint32_t tri = kInvalidRef;
        n_pts = 1;
        if (ptcp::point_walked(p.x, p.y, p.z, rmax)) {
            uint2 stk[kStackMax];
            walk_point<STATS>(A, p, best2, tri, stk, cnt);
        }
        out[i] = closest_record(A.tris, p, best2, tri);
    }
    if (STATS) add_stats(A, 0, n_pts, cnt);
}

// ------------------------------------------------------------------------------------
// persistent kernel: one wavefront per workgroup, one point per lane, lanes refilled from the wavefront's chunk
// ------------------------------------------------------------------------------------
// persistent_walk's Q (pt_walk.h) of a point: the key of a child is bound2 of its box, compared with best2, which starts at r_max^2.
// A leaf is gated on leaf_end: an out-of-range leaf points at the record behind the last triangle, whose distance must not count.
struct PointWalk {
    static constexpr bool kWaveHooks = false;
    static constexpr float kKeyInit = 0.0f;       // pt_device.h::order_children
    const float4* __restrict__ pts; uint4* __restrict__ out; const float4* __restrict__ tris; uint32_t leaf_end;
    uint32_t rid = 0, btri = kInvalidRef; float best2 = 0.0f;
    F3 p = f3(0, 0, 0); PointSlack s = point_slack(p);

    __device__ __forceinline__ bool start(const RenderArgs& A, uint32_t item, bool scene_ok) {
        rid = item;
        float rmax;
        load_point(pts, rid, p, rmax);
        best2 = rmax * rmax; btri = kInvalidRef;
        s = point_slack(p);
        if (scene_ok && ptcp::point_walked(p.x, p.y, p.z, rmax) && box_bound2(s, A.root_box[0], A.root_box[1], A.root_box[2]) < best2) return true;
        out[rid] = make_uint4(kInfBits, kInvalidRef, 0u, 0u);
        return false;
    }
    __device__ __forceinline__ bool child(uint32_t w0, uint32_t w1, uint32_t w2, float& bound2) const { bound2 = box_bound2(s, w0, w1, w2); return bound2 < best2; }
    __device__ __forceinline__ bool leaf(uint32_t cur, const uint4 n0, const uint4 n1, const uint4 n2) {
        const float d2 = tri_d2(p, as_float4(n0), as_float4(n1), as_float4(n2));
        if (((cur & 0x7fffffffu) < leaf_end) & (d2 < best2)) { best2 = d2; btri = cur; }
        return false;
    }
    __device__ __forceinline__ float bound() const { return best2; }
    __device__ __forceinline__ void finish(const RenderArgs&) { out[rid] = closest_record(tris, p, best2, btri == kInvalidRef ? kInvalidRef : (btri & 0x7fffffffu) >> 2); }
    __device__ __forceinline__ void after_refill(uint32_t) {}
    __device__ __forceinline__ void after_step(bool, uint32_t) {}
};
__global__ __launch_bounds__(64) void closest_points_kernel(const RenderArgs A, const float4* __restrict__ pts, uint4* __restrict__ out, uint32_t n,
                                                            unsigned long long* __restrict__ queue, unsigned long long* __restrict__ spill, uint32_t fill) {
    PointWalk q{pts, out, A.tris, 4u * A.num_tris};
    persistent_walk<PT_PQ_SHORT_STACK>(A, n, queue, spill, fill, q);
}

// ------------------------------------------------------------------------------------
// brute force: one point per thread, every triangle in index order (pt_walk.h::brute_records)
// ------------------------------------------------------------------------------------
template <bool STATS>
__global__ __launch_bounds__(256) void closest_points_brute_kernel(const RenderArgs A, const float4* __restrict__ pts, uint4* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    F3 p = f3(0, 0, 0); float rmax = 0.0f;
    if (i < n) load_point(pts, i, p, rmax);
    const bool walked = (i < n) && ptcp::point_walked(p.x, p.y, p.z, rmax);
    float best2 = rmax * rmax; uint32_t tri = kInvalidRef;
    brute_records(A, walked, [&](uint32_t t, const uint4 n0, const uint4 n1, const uint4 n2) __attribute__((always_inline)) {
        const float d2 = tri_d2(p, as_float4(n0), as_float4(n1), as_float4(n2));
        if (d2 < best2) { best2 = d2; tri = t; }
    });
    if (i < n) out[i] = closest_record(A.tris, p, best2, tri);
    if (STATS) {
        Counters cnt; cnt.nodes = cnt.drops = cnt.maxstack = 0;
        cnt.tris = walked ? A.num_tris : 0u;                              // a walked point tests every record
        add_stats(A, 0, i < n ? 1u : 0u, cnt);
    }
}

hipError_t launch_closest_points(const RenderArgs& A, const void* points, void* out, uint32_t n, bool simple, bool stats, bool brute,
                                 unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    const float4* p = (const float4*)points; uint4* o = (uint4*)out;
    const dim3 g256((n + 255u) / 256u);
    if (brute) {
        if (stats) closest_points_brute_kernel<true><<<g256, 256, 0, stream>>>(A, p, o, n);
        else closest_points_brute_kernel<false><<<g256, 256, 0, stream>>>(A, p, o, n);
        return hipGetLastError();
    }
    if (simple || stats) {
        if (stats) closest_points_simple_kernel<true><<<g256, 256, 0, stream>>>(A, p, o, n);
        else closest_points_simple_kernel<false><<<g256, 256, 0, stream>>>(A, p, o, n);
        return hipGetLastError();
    }
    hipError_t e = walk_begin(queue, n, grid, stream);
    if (e != hipSuccess) return e;
    closest_points_kernel<<<grid, 64, 0, stream>>>(A, p, o, n, queue, spill, PT_PQ_FILL);
    return hipGetLastError();
}

} // namespace ptk
