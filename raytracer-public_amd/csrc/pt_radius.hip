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
// The point record, the slack, box_bound2 and tri_d2 are pt_points.h's, shared with pt_pointquery.hip and pt_knn.hip.
// Records: PtPoint = one float4 (p.xyz, r_max), an entry = PtClosest = one uint4 (dist bits, prim, u bits, v bits).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <hipcub/hipcub.hpp>

#include "pt_kernels.h"
#include "pt_device.h"
#include "pt_closest.h"
#include "pt_points.h"
#include "pt_walk.h"

namespace ptk {

// What the three kernels do with an accepted leaf: count it, and with FILL store its entry (one plain 16-byte vector store) when its
// global index is below the capacity.  base + k is 64-bit: the total of a batch may pass 2^32.
template <bool FILL>
struct RdSink {
    uint4* __restrict__ entries; unsigned long long capacity;
    unsigned long long base = 0; uint32_t count = 0;
    __device__ __forceinline__ void accept(float d2, uint32_t tri, float u, float v) {
        if (FILL) {
            const unsigned long long g = base + count;
            if (g < capacity) entries[g] = make_uint4(__float_as_uint(sqrtf(d2)), tri, __float_as_uint(u), __float_as_uint(v));
        }
        ++count;
    }
};

// ------------------------------------------------------------------------------------
// simple kernel: one point per thread, a private 64-entry stack; the counters of PT_RADIUS_STATS by the rules of PT_CLOSEST_STATS
// (pt_pointquery.hip::walk_point with a constant best2)
// ------------------------------------------------------------------------------------
template <bool FILL, bool STATS>
__device__ __forceinline__ void radius_walk_point(const RenderArgs& A, F3 p, float r2, uint2* __restrict__ stk, Counters& cnt, RdSink<FILL>& sink) {
    if (A.root_ref == kInvalidRef || A.num_tris == 0u) return;
    if (STATS) { cnt.nodes += 1; if (cnt.maxstack < 1u) cnt.maxstack = 1u; }      // the root record is fetched before its degenerate check
    if (A.root_degenerate) return;
    const PointSlack s = point_slack(p);
    if (!(box_bound2(s, A.root_box[0], A.root_box[1], A.root_box[2]) < r2)) return;
    uint32_t cur = A.root_ref;
    int sp = 0;
    for (;;) {
        bool need_pop = false;
        if (cur & kLeaf) {
            const uint32_t ti4 = cur & 0x7fffffffu;
            if (ti4 < 4u * A.num_tris) {                          // an out-of-range leaf points at the record behind the last triangle: skipped
                const float4* tp = (const float4*)arena_record(A, cur);
                if (STATS) cnt.tris += 1;
                float u, v;
                const float d2 = tri_d2(p, tp[0], tp[1], tp[2], u, v);
                if (d2 < r2) sink.accept(d2, ti4 >> 2, u, v);
            }
            need_pop = true;
        } else {
            const uint4* np = arena_record(A, cur);
            const uint4 n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3];
            const uint32_t r0 = n0.w, r1 = n1.w, r2r = n2.w, r3 = n3.w;
            const float t0 = box_bound2(s, n0.x, n0.y, n0.z), t1 = box_bound2(s, n1.x, n1.y, n1.z);
            const float t2 = box_bound2(s, n2.x, n2.y, n2.z), t3 = box_bound2(s, n3.x, n3.y, n3.z);
            const bool h0 = t0 < r2, h1 = t1 < r2, h2 = t2 < r2, h3 = t3 < r2;
            if (STATS) cnt.nodes += (r0 != kInvalidRef) + (r1 != kInvalidRef) + (r2r != kInvalidRef) + (r3 != kInvalidRef);
            uint32_t enter;
            const int before = sp;
            const bool any = h0 | h1 | h2 | h3;
            const uint32_t wanted = (uint32_t)h0 + (uint32_t)h1 + (uint32_t)h2 + (uint32_t)h3;      // one entered, the others pushed
            const bool go = order_children(h0, h1, h2, h3, t0, t1, t2, t3, r0, r1, r2r, r3, 0.0f, sp, enter, [&](int at, uint32_t ref, float key) __attribute__((always_inline)) {
                stk[at] = make_uint2(ref, __float_as_uint(key));
            });
            if (STATS && any) {
                // pushes that did not fit, and the nearest child's own when the stack is full (pt_pointquery.hip::walk_point)
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
                if (__uint_as_float(e.y) < r2) { cur = e.x; found = true; break; }      // always passes: r2 never moves
            }
            if (!found) break;
        }
    }
}

template <bool FILL, bool STATS>
__global__ __launch_bounds__(256) void radius_simple_kernel(const RenderArgs A, const float4* __restrict__ pts, uint32_t* __restrict__ counts,
                                                            const unsigned long long* __restrict__ offsets, uint4* __restrict__ entries,
                                                            unsigned long long capacity, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    Counters cnt; cnt.nodes = cnt.tris = cnt.drops = cnt.maxstack = 0;
    if (i < n) {
        F3 p; float rmax;
        load_point(pts, i, p, rmax);
        RdSink<FILL> sink{entries, capacity};
        if (FILL) sink.base = offsets[i];
        if (ptcp::point_walked(p.x, p.y, p.z, rmax)) {
            uint2 stk[kStackMax];
            radius_walk_point<FILL, STATS>(A, p, rmax * rmax, stk, cnt, sink);
        }
        if (!FILL) counts[i] = sink.count;
    }
    if (STATS) add_stats(A, 0, i < n ? 1u : 0u, cnt);
}

// ------------------------------------------------------------------------------------
// persistent kernel: one wavefront per workgroup, one point per lane, lanes refilled from the wavefront's chunk
// ------------------------------------------------------------------------------------
// persistent_walk's Q (pt_walk.h) of a radius query: pt_pointquery.hip::PointWalk with a best2 that never moves.  A leaf is gated on
// leaf_end: an out-of-range leaf points at the record behind the last triangle, whose distance must not count.
template <bool FILL>
struct RadiusWalk {
    static constexpr bool kWaveHooks = false;
    static constexpr float kKeyInit = 0.0f;       // pt_device.h::order_children
    const float4* __restrict__ pts; uint32_t* __restrict__ counts; const unsigned long long* __restrict__ offsets; uint32_t leaf_end;
    RdSink<FILL> sink;
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
        if (((cur & 0x7fffffffu) < leaf_end) & (d2 < r2)) sink.accept(d2, (cur & 0x7fffffffu) >> 2, u, v);
        return false;                                                     // no leaf ends the point
    }
    __device__ __forceinline__ float bound() const { return r2; }         // r2 never moves: every stacked entry is walked
    __device__ __forceinline__ void finish(const RenderArgs&) { if (!FILL) counts[rid] = sink.count; }
    __device__ __forceinline__ void after_refill(uint32_t) {}
    __device__ __forceinline__ void after_step(bool, uint32_t) {}
};
template <bool FILL>
__global__ __launch_bounds__(64) void radius_kernel(const RenderArgs A, const float4* __restrict__ pts, uint32_t* __restrict__ counts,
                                                    const unsigned long long* __restrict__ offsets, uint4* __restrict__ entries, unsigned long long capacity,
                                                    uint32_t n, unsigned long long* __restrict__ queue, unsigned long long* __restrict__ spill, uint32_t fill) {
    RadiusWalk<FILL> q{pts, counts, offsets, 4u * A.num_tris, RdSink<FILL>{entries, capacity}};
    persistent_walk<PT_RD_SHORT_STACK>(A, n, queue, spill, fill, q);
}

// ------------------------------------------------------------------------------------
// brute force: one point per thread, every triangle in index order; a workgroup streams the records through LDS, kRdBruteTile at a time
// ------------------------------------------------------------------------------------
constexpr uint32_t kRdBruteTile = 256;
template <bool FILL, bool STATS>
__global__ __launch_bounds__(256) void radius_brute_kernel(const RenderArgs A, const float4* __restrict__ pts, uint32_t* __restrict__ counts,
                                                           const unsigned long long* __restrict__ offsets, uint4* __restrict__ entries,
                                                           unsigned long long capacity, uint32_t n) {
    __shared__ float4 rec[kRdBruteTile][3];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    F3 p = f3(0, 0, 0); float rmax = 0.0f;
    if (i < n) load_point(pts, i, p, rmax);
    const bool walked = (i < n) && ptcp::point_walked(p.x, p.y, p.z, rmax);
    const float r2 = rmax * rmax;
    RdSink<FILL> sink{entries, capacity};
    if (FILL && i < n) sink.base = offsets[i];
    Counters cnt; cnt.nodes = cnt.tris = cnt.drops = cnt.maxstack = 0;
    for (uint32_t base = 0; base < A.num_tris; base += kRdBruteTile) {
        const uint32_t tile = min(kRdBruteTile, A.num_tris - base);
        __syncthreads();
        if (threadIdx.x < tile) {
            const float4* tp = A.tris + (size_t)(base + threadIdx.x) * 4;
            rec[threadIdx.x][0] = tp[0]; rec[threadIdx.x][1] = tp[1]; rec[threadIdx.x][2] = tp[2];
        }
        __syncthreads();
        if (walked) {
            for (uint32_t k = 0; k < tile; ++k) {
                float u, v;
                const float d2 = tri_d2(p, rec[k][0], rec[k][1], rec[k][2], u, v);
                if (d2 < r2) sink.accept(d2, base + k, u, v);
            }
            if (STATS) cnt.tris += tile;
        }
    }
    if (!FILL && i < n) counts[i] = sink.count;
    if (STATS) add_stats(A, 0, i < n ? 1u : 0u, cnt);
}

hipError_t launch_radius(const RenderArgs& A, const void* points, uint32_t n, void* counts, const unsigned long long* offsets, void* entries,
                         unsigned long long capacity, bool simple, bool stats, bool brute,
                         unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    const float4* p = (const float4*)points; uint32_t* c = (uint32_t*)counts; uint4* e = (uint4*)entries;
    const bool fill = offsets != nullptr;
    const dim3 g256((n + 255u) / 256u);
    if (brute) {
        if (fill) radius_brute_kernel<true, false><<<g256, 256, 0, stream>>>(A, p, c, offsets, e, capacity, n);
        else if (stats) radius_brute_kernel<false, true><<<g256, 256, 0, stream>>>(A, p, c, offsets, e, capacity, n);
        else radius_brute_kernel<false, false><<<g256, 256, 0, stream>>>(A, p, c, offsets, e, capacity, n);
        return hipGetLastError();
    }
    if (simple || stats) {
        if (fill) radius_simple_kernel<true, false><<<g256, 256, 0, stream>>>(A, p, c, offsets, e, capacity, n);
        else if (stats) radius_simple_kernel<false, true><<<g256, 256, 0, stream>>>(A, p, c, offsets, e, capacity, n);
        else radius_simple_kernel<false, false><<<g256, 256, 0, stream>>>(A, p, c, offsets, e, capacity, n);
        return hipGetLastError();
    }
    hipError_t err = walk_begin(queue, n, grid, stream);
    if (err != hipSuccess) return err;
    if (fill) radius_kernel<true><<<grid, 64, 0, stream>>>(A, p, c, offsets, e, capacity, n, queue, spill, PT_RD_FILL);
    else radius_kernel<false><<<grid, 64, 0, stream>>>(A, p, c, offsets, e, capacity, n, queue, spill, PT_RD_FILL);
    return hipGetLastError();
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
