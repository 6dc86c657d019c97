// pt_radius.hip -- radius queries over the context's tree: every triangle within r_max of a point, counted and listed (include/mi355pt.h:
// pt_radius_count, pt_radius_search):
//   * radius_kernel<FILL>                 the default: persistent wavefronts, one point per lane, a lane whose point is answered takes the
//                                         next point of its wavefront's chunk.  FILL = false counts the accepted leaves of a point;
//                                         FILL = true walks the same walk again and stores entry k of point i at offsets[i] + k
//   * radius_simple_kernel<FILL, STATS>   one point per thread with a private 64-entry stack: PT_RADIUS_SIMPLE_KERNEL, PT_RADIUS_STATS
//   * radius_brute_kernel<FILL, STATS>    every triangle in index order, the records streamed through LDS: PT_RADIUS_BRUTE_FORCE
//   * launch_radius_scan                  offsets = the exclusive prefix sums of the counts in 64 bits (hipcub::DeviceScan)
//
// The walk is the closest-point walk (pt_pointquery.hip, pt_walk.h::persistent_walk) with best2 held at r2 = r_max * r_max: a child is
// entered if bound2 < r2, a leaf is accepted if d2 < r2, nothing shrinks r2, so every stacked entry passes its re-validation.  The list of
// a point is its accepted leaves in visit order, which depends on the point and the tree alone: the count walk and the fill walk of a
// point take the same steps whichever lane, wavefront or kernel runs them, so entry k lands at offsets[i] + k without an atomic.
// The point-triangle arithmetic is pt_closest.h, shared with the host twin (pt_host.cpp::radius_search), which gives the same bits.
// The point record, the slack, box_bound2 and tri_d2 are pt_points.h's, shared with pt_pointquery.hip and pt_knn.hip.  The bodies of the
// simple and the brute-force kernel and the dispatch are pt_region.h's, shared with the box query (pt_overlap.hip): this file holds the
// sphere and the persistent kernel's Q.
// Records: PtPoint = one float4 (p.xyz, r_max), an entry = PtClosest = one uint4 (dist bits, prim, u bits, v bits).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <hipcub/hipcub.hpp>

#include "pt_kernels.h"
#include "pt_device.h"
#include "pt_closest.h"
#include "pt_points.h"
#include "pt_region.h"
#include "pt_walk.h"

namespace ptk {

// The region of a radius query (pt_region.h): the sphere of r_max around p.  The key of a child is bound2 of its box, the bound is
// r2 = r_max * r_max, and a leaf is accepted if d2 < r2.  An entry is pt_pointquery.hip::closest_record's: dist = sqrtf(d2), u and v of
// the accepted test.
struct SphereRegion {
    float rmax = 0.0f, r2 = 0.0f;
    F3 p = f3(0, 0, 0); PointSlack s = point_slack(p);

    __device__ __forceinline__ void load(const float4* __restrict__ pts, uint32_t i) {
        load_point(pts, i, p, rmax);
        r2 = rmax * rmax;
        s = point_slack(p);
    }
    __device__ __forceinline__ bool walked() const { return ptcp::point_walked(p.x, p.y, p.z, rmax); }
    __device__ __forceinline__ bool child(uint32_t w0, uint32_t w1, uint32_t w2, float& key) const { key = box_bound2(s, w0, w1, w2); return key < r2; }
    __device__ __forceinline__ float bound() const { return r2; }
    template <class Sink>
    __device__ __forceinline__ void leaf(uint32_t tri, const float4 a, const float4 b, const float4 c, Sink& sink) const {
        float u, v;
        const float d2 = tri_d2(p, a, b, c, u, v);
        if (d2 < r2) sink.accept([&]() __attribute__((always_inline)) { return make_uint4(__float_as_uint(sqrtf(d2)), tri, __float_as_uint(u), __float_as_uint(v)); });
    }
};

#define PT_REGION_ARGS const RenderArgs A, const float4* __restrict__ pts, uint32_t* __restrict__ counts, const unsigned long long* __restrict__ offsets, \
                       uint4* __restrict__ entries, unsigned long long capacity, uint32_t n
template <bool FILL, bool STATS>
__global__ __launch_bounds__(256) void radius_simple_kernel(PT_REGION_ARGS) { region_simple<SphereRegion, FILL, STATS>(A, pts, counts, offsets, entries, capacity, n); }
template <bool FILL, bool STATS>
__global__ __launch_bounds__(256) void radius_brute_kernel(PT_REGION_ARGS) { region_brute<SphereRegion, FILL, STATS>(A, pts, counts, offsets, entries, capacity, n); }
// persistent_walk's Q (pt_walk.h) of a radius query: pt_pointquery.hip::PointWalk with a best2 that never moves.  It keeps its own lines
// (the exact registers and speed of a persistent kernel are required properties).  A leaf is gated on leaf_end: an
// out-of-range leaf points at the record behind the last triangle, whose distance must not count.
template <bool FILL>
struct RadiusWalk {
    static constexpr bool kWaveHooks = false;
    static constexpr float kKeyInit = 0.0f;       // pt_device.h::order_children
    const float4* __restrict__ pts; uint32_t* __restrict__ counts; const unsigned long long* __restrict__ offsets; uint32_t leaf_end;
    ListSink<FILL> sink;
    uint32_t rid = 0; float r2 = 0.0f;
    F3 p = f3(0, 0, 0); PointSlack s = point_slack(p);

    __device__ __forceinline__ bool start(const RenderArgs& A, uint32_t item, bool scene_ok) {
        rid = item;
        float rmax;
        load_point(pts, rid, p, rmax);
        r2 = rmax * rmax; sink.count = 0u;
        s = point_slack(p);
        if (scene_ok && ptcp::point_walked(p.x, p.y, p.z, rmax) && box_bound2(s, A.root_box[0], A.root_box[1], A.root_box[2]) < r2) {
            if (FILL) sink.base = offsets[rid];
            return true;
        }
        if (!FILL) counts[rid] = 0u;
        return false;
    }
    __device__ __forceinline__ bool child(uint32_t w0, uint32_t w1, uint32_t w2, float& bound2) const { bound2 = box_bound2(s, w0, w1, w2); return bound2 < r2; }
    __device__ __forceinline__ bool leaf(uint32_t cur, const uint4 n0, const uint4 n1, const uint4 n2) {
        float u, v;
        const float d2 = tri_d2(p, as_float4(n0), as_float4(n1), as_float4(n2), u, v);
        if (((cur & 0x7fffffffu) < leaf_end) & (d2 < r2)) {
            const uint32_t tri = (cur & 0x7fffffffu) >> 2;
            sink.accept([&]() __attribute__((always_inline)) { return make_uint4(__float_as_uint(sqrtf(d2)), tri, __float_as_uint(u), __float_as_uint(v)); });
        }
        return false;                                                     // no leaf ends the point
    }
    __device__ __forceinline__ float bound() const { return r2; }         // r2 never moves: every stacked entry is walked
    __device__ __forceinline__ void finish(const RenderArgs&) { if (!FILL) counts[rid] = sink.count; }
    __device__ __forceinline__ void after_refill(uint32_t) {}
    __device__ __forceinline__ void after_step(bool, uint32_t) {}
};
template <bool FILL>
__global__ __launch_bounds__(64) void radius_kernel(PT_REGION_ARGS, unsigned long long* __restrict__ queue, unsigned long long* __restrict__ spill, uint32_t fill) {
    RadiusWalk<FILL> q{pts, counts, offsets, 4u * A.num_tris, ListSink<FILL>{entries, capacity}};
    persistent_walk<PT_RD_SHORT_STACK>(A, n, queue, spill, fill, q);
}
#undef PT_REGION_ARGS

hipError_t launch_radius(const RenderArgs& A, const void* points, uint32_t n, void* counts, const unsigned long long* offsets, void* entries,
                         unsigned long long capacity, bool simple, bool stats, bool brute,
                         unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream) {
    static const RegionKernels K = {{radius_brute_kernel<true, false>, radius_brute_kernel<false, true>, radius_brute_kernel<false, false>},
                                    {radius_simple_kernel<true, false>, radius_simple_kernel<false, true>, radius_simple_kernel<false, false>},
                                    {radius_kernel<true>, radius_kernel<false>}, PT_RD_FILL};
    return launch_region(K, A, points, n, counts, offsets, entries, capacity, simple, stats, brute, queue, spill, grid, stream);
}

// ------------------------------------------------------------------------------------
// the scan between the two walks: n + 1 items, item n read as 0, so that offsets[n] is the total
// ------------------------------------------------------------------------------------
struct RdCountAt {
    const uint32_t* counts; uint32_t n;
    __host__ __device__ __forceinline__ unsigned long long operator()(unsigned long long i) const { return i < n ? (unsigned long long)counts[i] : 0ull; }
};
using RdCountIter = hipcub::TransformInputIterator<unsigned long long, RdCountAt, hipcub::CountingInputIterator<unsigned long long>>;

size_t radius_scan_temp_bytes(uint32_t n) {
    size_t bytes = 0;
    RdCountIter in(hipcub::CountingInputIterator<unsigned long long>(0ull), RdCountAt{nullptr, n});
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, (unsigned long long*)nullptr, (size_t)n + 1u);
    return bytes;
}

hipError_t launch_radius_scan(const void* counts, uint32_t n, unsigned long long* offsets, void* temp, size_t temp_bytes, hipStream_t stream) {
    RdCountIter in(hipcub::CountingInputIterator<unsigned long long>(0ull), RdCountAt{(const uint32_t*)counts, n});
    return hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, in, offsets, (size_t)n + 1u, stream);
}

} // namespace ptk
