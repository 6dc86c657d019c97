// pt_overlap.hip -- box-overlap queries over the context's tree: every triangle that overlaps an axis-aligned box, counted and listed
// (include/mi355pt.h: pt_box_count, pt_box_search):
//   * box_kernel<FILL>                 the default: persistent wavefronts, one box per lane, a lane whose box is answered takes the next
//                                      box of its wavefront's chunk.  FILL = false counts the accepted leaves of a box; FILL = true walks
//                                      the same walk again and stores entry k of box i at offsets[i] + k
//   * box_simple_kernel<FILL, STATS>   one box per thread with a private 64-entry stack: PT_BOX_SIMPLE_KERNEL, PT_BOX_STATS
//   * box_brute_kernel<FILL, STATS>    every triangle in index order, the records streamed through LDS: PT_BOX_BRUTE_FORCE
// The scan between the two walks is pt_radius.hip::launch_radius_scan.
//
// The walk is pt_walk.h::persistent_walk with every key equal: a child is entered iff its packed f16 box meets the query box moved out by
// the slack, its key is 0 and bound() is 1, so the first passing child in slot order is entered, the others pop in slot order (depth-first
// slot order) and every stacked entry passes its re-validation.  The list of a box is its accepted leaves in visit order, which depends on
// the box and the tree alone: the count walk and the fill walk of a box take the same steps whichever lane, wavefront or kernel runs them,
// so entry k lands at offsets[i] + k without an atomic.  The box arithmetic is pt_overlap.h, shared with the host twin
// (pt_host.cpp::box_search), which gives the same booleans.  The bodies of the simple and the brute-force kernel and the dispatch are
// pt_region.h's, shared with the radius query (pt_radius.hip): this file holds the box and the persistent kernel's Q.
// Records: PtBox = two float4 (lo.xyz, pad; hi.xyz, pad), an entry = PtOverlap = one uint4 (prim, verts_inside, 0, 0).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_kernels.h"
#include "pt_device.h"
#include "pt_overlap.h"
#include "pt_points.h"
#include "pt_region.h"
#include "pt_walk.h"

namespace ptk {

// ptov::node_overlaps on one packed f16 box (w0 = mn.x | mn.y << 16, w1 = mn.z | mx.x << 16, w2 = mx.y | mx.z << 16): the six differences
// straight from the packed halves (v_fma_mix_f32), their maximum (v_max3_f32) not above 0.  No operand is a NaN: the halves are finite or
// the +-inf of an inverted box, the box corners finite.
__device__ __forceinline__ bool node_overlaps(const ptov::Box& b, uint32_t w0, uint32_t w1, uint32_t w2) {
    const float gx = wmax(half_lo_minus(w0, b.shx), minus_half_hi(b.slx, w1));
    const float gy = wmax(half_hi_minus(w0, b.shy), minus_half_lo(b.sly, w2));
    const float gz = wmax(half_lo_minus(w1, b.shz), minus_half_hi(b.slz, w2));
    return wmax(wmax(gx, gy), gz) <= 0.0f;
}
// the triangle test of one record (three axis-major pieces: v0[a], e1[a], e2[a])
__device__ __forceinline__ bool tri_overlaps(const ptov::Box& b, const float4 a, const float4 c, const float4 d, uint32_t& verts_inside) {
    return ptov::tri_overlaps(b, a.x, c.x, d.x, a.y, c.y, d.y, a.z, c.z, d.z, verts_inside);
}

// The region of a box query (pt_region.h).  Every key is equal: 0 for a child whose packed f16 box meets the query box moved out by the
// slack, and the bound is 1, so the first passing child in slot order is entered and the others pop in slot order (depth-first slot
// order); a child that does not overlap is not entered.  An entry is (prim, verts_inside, 0, 0).
struct BoxRegion {
    ptov::Box b = ptov::make_box(0, 0, 0, 0, 0, 0);

    __device__ __forceinline__ void load(const float4* __restrict__ boxes, uint32_t i) {
        const float4 lo = boxes[2 * (size_t)i], hi = boxes[2 * (size_t)i + 1];
        b = ptov::make_box(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z);
    }
    __device__ __forceinline__ bool walked() const { return ptov::box_walked(b.lox, b.loy, b.loz, b.hix, b.hiy, b.hiz); }
    __device__ __forceinline__ bool child(uint32_t w0, uint32_t w1, uint32_t w2, float& key) const { key = 0.0f; return node_overlaps(b, w0, w1, w2); }
    __device__ __forceinline__ float bound() const { return 1.0f; }
    template <class Sink>
    __device__ __forceinline__ void leaf(uint32_t tri, const float4 a, const float4 c, const float4 d, Sink& sink) const {
        uint32_t in;
        const bool hit = tri_overlaps(b, a, c, d, in);
        if (hit) sink.accept([&]() __attribute__((always_inline)) { return make_uint4(tri, in, 0u, 0u); });
    }
};

#define PT_REGION_ARGS const RenderArgs A, const float4* __restrict__ boxes, uint32_t* __restrict__ counts, const unsigned long long* __restrict__ offsets, \
                       uint4* __restrict__ entries, unsigned long long capacity, uint32_t n
template <bool FILL, bool STATS>
__global__ __launch_bounds__(256) void box_simple_kernel(PT_REGION_ARGS) { region_simple<BoxRegion, FILL, STATS>(A, boxes, counts, offsets, entries, capacity, n); }
template <bool FILL, bool STATS>
__global__ __launch_bounds__(256) void box_brute_kernel(PT_REGION_ARGS) { region_brute<BoxRegion, FILL, STATS>(A, boxes, counts, offsets, entries, capacity, n); }
// persistent_walk's Q (pt_walk.h) of a box query.  It keeps its own lines (the exact registers and speed of a persistent kernel are
// required properties).  A leaf is gated on leaf_end: an out-of-range leaf points at the record behind the last
// triangle, which must not count.
template <bool FILL>
struct BoxWalk {
    static constexpr bool kWaveHooks = false;
    static constexpr float kKeyInit = 0.0f;       // pt_device.h::order_children
    const float4* __restrict__ boxes; uint32_t* __restrict__ counts; const unsigned long long* __restrict__ offsets; uint32_t leaf_end;
    ListSink<FILL> sink;
    uint32_t rid = 0;
    ptov::Box b = ptov::make_box(0, 0, 0, 0, 0, 0);

    __device__ __forceinline__ bool start(const RenderArgs& A, uint32_t item, bool scene_ok) {
        rid = item;
        const float4 lo = boxes[2 * (size_t)rid], hi = boxes[2 * (size_t)rid + 1];
        b = ptov::make_box(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z);
        const bool walked = ptov::box_walked(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z);
        sink.count = 0u;
        if (scene_ok && walked && node_overlaps(b, A.root_box[0], A.root_box[1], A.root_box[2])) {
            if (FILL) sink.base = offsets[rid];
            return true;
        }
        if (!FILL) counts[rid] = 0u;
        return false;
    }
    __device__ __forceinline__ bool child(uint32_t w0, uint32_t w1, uint32_t w2, float& key) const { key = 0.0f; return node_overlaps(b, w0, w1, w2); }
    __device__ __forceinline__ bool leaf(uint32_t cur, const uint4 n0, const uint4 n1, const uint4 n2) {
        uint32_t in;
        const bool hit = tri_overlaps(b, as_float4(n0), as_float4(n1), as_float4(n2), in);
        if (((cur & 0x7fffffffu) < leaf_end) & hit) {
            const uint32_t tri = (cur & 0x7fffffffu) >> 2;
            sink.accept([&]() __attribute__((always_inline)) { return make_uint4(tri, in, 0u, 0u); });
        }
        return false;                                                     // no leaf ends the box
    }
    __device__ __forceinline__ float bound() const { return 1.0f; }       // above every key: every stacked entry is walked
    __device__ __forceinline__ void finish(const RenderArgs&) { if (!FILL) counts[rid] = sink.count; }
    __device__ __forceinline__ void after_refill(uint32_t) {}
    __device__ __forceinline__ void after_step(bool, uint32_t) {}
};
template <bool FILL>
__global__ __launch_bounds__(64) void box_kernel(PT_REGION_ARGS, unsigned long long* __restrict__ queue, unsigned long long* __restrict__ spill, uint32_t fill) {
    BoxWalk<FILL> q{boxes, counts, offsets, 4u * A.num_tris, ListSink<FILL>{entries, capacity}};
    persistent_walk<PT_BX_SHORT_STACK>(A, n, queue, spill, fill, q);
}
#undef PT_REGION_ARGS

hipError_t launch_box(const RenderArgs& A, const void* boxes, uint32_t n, void* counts, const unsigned long long* offsets, void* entries,
                      unsigned long long capacity, bool simple, bool stats, bool brute,
                      unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream) {
    static const RegionKernels K = {{box_brute_kernel<true, false>, box_brute_kernel<false, true>, box_brute_kernel<false, false>},
                                    {box_simple_kernel<true, false>, box_simple_kernel<false, true>, box_simple_kernel<false, false>},
                                    {box_kernel<true>, box_kernel<false>}, PT_BX_FILL};
    return launch_region(K, A, boxes, n, counts, offsets, entries, capacity, simple, stats, brute, queue, spill, grid, stream);
}

} // namespace ptk
