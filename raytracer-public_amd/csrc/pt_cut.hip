// pt_cut.hip -- plane-cut queries over the context's tree: every mesh triangle that a plane cuts inside a window, counted and listed with
// where the plane crosses its two crossing edges (include/mi355pt.h: pt_cut_count, pt_cut_search):
//   * cut_kernel<FILL>                 the default: persistent wavefronts, one plane per lane, a lane whose plane is answered takes the
//                                      next plane of its wavefront's chunk.  FILL = false counts the accepted leaves of a plane (it
//                                      classifies only and never divides); FILL = true walks the same walk again and stores entry k of
//                                      plane i at offsets[i] + k
//   * cut_simple_kernel<FILL, STATS>   one plane per thread with a private 64-entry stack: PT_CUT_SIMPLE_KERNEL, PT_CUT_STATS
//   * cut_brute_kernel<FILL, STATS>    every mesh triangle in index order, the records streamed through LDS: PT_CUT_BRUTE_FORCE
// The scan between the two walks is pt_radius.hip::launch_radius_scan.
//
// The walk is the box query's (pt_overlap.hip) on the window, with the plane test added to the node test: every key 0, bound() 1,
// depth-first slot order, so the list of a plane is its accepted leaves in visit order, which depends on the record and the tree alone,
// and entry k lands at offsets[i] + k without an atomic.  The arithmetic is pt_cut.h, shared with the host twin (pt_host.cpp::cut_search),
// which gives the same booleans and the same bits of t0 and t1.  The bodies of the simple and the brute-force kernel and the dispatch
// are pt_region.h's.
// Records: PtCutPlane = three float4 (n.xyz, d; lo.xyz, pad; hi.xyz, pad), an entry = PtCut = one uint4 (prim, code, t0 bits, t1 bits).
//
// A lane holds the window's twelve values, n and d for the whole walk and derives the corner selectors from the sign of n_k at each node
// (pt_cut.h::corners_cut, the text the twin compiles).  DESIGN.md section 24 has the registers of this form and of the one that holds the
// selectors; no GPU run has compared them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_kernels.h"
#include "pt_device.h"
#include "pt_overlap.h"
#include "pt_tritri.h"
#include "pt_cut.h"
#include "pt_points.h"
#include "pt_region.h"
#include "pt_walk.h"

namespace ptk {

// The node test on one packed f16 box (w0 = mn.x | mn.y, w1 = mn.z | mx.x, w2 = mx.y | mx.z): ptov::node_overlaps of the window, restated
// from pt_overlap.hip as pt_tritri.hip does (the six differences straight from the packed halves, v_fma_mix_f32), AND ptct::corners_cut
// on the grown corners fl(mn - s), fl(mx + s), taken from the packed halves by the same instruction: fl(h * 1 - s) is the value the twin
// computes from the decoded half.  side() stays pt_cut.h's six separately rounded operations.
__device__ __forceinline__ bool cut_node(const ptov::Box& b, const ptct::Plane& p, uint32_t w0, uint32_t w1, uint32_t w2) {
    const float gx = wmax(half_lo_minus(w0, b.shx), minus_half_hi(b.slx, w1));
    const float gy = wmax(half_hi_minus(w0, b.shy), minus_half_lo(b.sly, w2));
    const float gz = wmax(half_lo_minus(w1, b.shz), minus_half_hi(b.slz, w2));
    const float s = ptcp::kSlack, m = -ptcp::kSlack;
    const bool cut = ptct::corners_cut(p, half_lo_minus(w0, s), half_hi_minus(w0, s), half_lo_minus(w1, s),
                                       half_hi_minus(w1, m), half_lo_minus(w2, m), half_hi_minus(w2, m));
    return (wmax(wmax(gx, gy), gz) <= 0.0f) & cut;
}
// one record: the plane, the window, and whether it is walked
__device__ __forceinline__ bool load_cut(const float4* __restrict__ planes, uint32_t i, ptct::Plane& p, ptov::Box& b) {
    const float4 a = planes[3 * (size_t)i], lo = planes[3 * (size_t)i + 1], hi = planes[3 * (size_t)i + 2];
    p = ptct::Plane{a.x, a.y, a.z, a.w};
    b = ptov::make_box(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z);
    const bool plane_ok = ptct::plane_walked(p), window_ok = ptov::box_walked(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z);
    return plane_ok & window_ok;
}
__device__ __forceinline__ uint4 cut_entry(uint32_t tri, const ptct::Cut& c) { return make_uint4(tri, c.code, __float_as_uint(c.t0), __float_as_uint(c.t1)); }

// The region of a plane-cut query (pt_region.h): the node test above and the leaf test of pt_cut.h.  An entry is (prim, code, t0, t1).
template <bool FILL>
struct CutRegion {
    ptct::Plane p = {0, 0, 0, 0};
    ptov::Box b = ptov::make_box(0, 0, 0, 0, 0, 0);
    bool ok = false;

    __device__ __forceinline__ void load(const float4* __restrict__ planes, uint32_t i) { ok = load_cut(planes, i, p, b); }
    __device__ __forceinline__ bool walked() const { return ok; }
    __device__ __forceinline__ bool child(uint32_t w0, uint32_t w1, uint32_t w2, float& key) const { key = 0.0f; return cut_node(b, p, w0, w1, w2); }
    __device__ __forceinline__ float bound() const { return 1.0f; }
    template <class Sink>
    __device__ __forceinline__ void leaf(uint32_t tri, const float4 a, const float4 c, const float4 d, Sink& sink) const {
        ptct::Cut cut = {0u, 0.0f, 0.0f};
        if (ptct::tri_cut<FILL>(b, p, a.x, c.x, d.x, a.y, c.y, d.y, a.z, c.z, d.z, cut))
            sink.accept([&]() __attribute__((always_inline)) { return cut_entry(tri, cut); });
    }
};

#define PT_REGION_ARGS const RenderArgs A, const float4* __restrict__ planes, uint32_t* __restrict__ counts, const unsigned long long* __restrict__ offsets, \
                       uint4* __restrict__ entries, unsigned long long capacity, uint32_t n
template <bool FILL, bool STATS>
__global__ __launch_bounds__(256) void cut_simple_kernel(PT_REGION_ARGS) { region_simple<CutRegion<FILL>, FILL, STATS>(A, planes, counts, offsets, entries, capacity, n); }
template <bool FILL, bool STATS>
__global__ __launch_bounds__(256) void cut_brute_kernel(PT_REGION_ARGS) { region_brute<CutRegion<FILL>, FILL, STATS>(A, planes, counts, offsets, entries, capacity, n); }
// persistent_walk's Q (pt_walk.h) of a plane-cut query.  A leaf is gated on leaf_end: an out-of-range leaf points at the record behind
// the last triangle, which must not count.
template <bool FILL>
struct CutWalk {
    static constexpr bool kWaveHooks = false;
    static constexpr float kKeyInit = 0.0f;       // pt_device.h::order_children
    const float4* __restrict__ planes; uint32_t* __restrict__ counts; const unsigned long long* __restrict__ offsets; uint32_t leaf_end;
    ListSink<FILL> sink;
    uint32_t rid = 0;
    ptov::Box b = ptov::make_box(0, 0, 0, 0, 0, 0);
    ptct::Plane p = {0, 0, 0, 0};

    __device__ __forceinline__ bool start(const RenderArgs& A, uint32_t item, bool scene_ok) {
        rid = item;
        const bool walked = load_cut(planes, rid, p, b);
        sink.count = 0u;
        if (scene_ok && walked && cut_node(b, p, A.root_box[0], A.root_box[1], A.root_box[2])) {
            if (FILL) sink.base = offsets[rid];
            return true;
        }
        if (!FILL) counts[rid] = 0u;
        return false;
    }
    __device__ __forceinline__ bool child(uint32_t w0, uint32_t w1, uint32_t w2, float& key) const { key = 0.0f; return cut_node(b, p, w0, w1, w2); }
    __device__ __forceinline__ bool leaf(uint32_t cur, const uint4 n0, const uint4 n1, const uint4 n2) {
        const float4 a = as_float4(n0), c = as_float4(n1), d = as_float4(n2);
        if ((cur & 0x7fffffffu) < leaf_end) {
            ptct::Cut cut = {0u, 0.0f, 0.0f};
            if (ptct::tri_cut<FILL>(b, p, a.x, c.x, d.x, a.y, c.y, d.y, a.z, c.z, d.z, cut)) {
                const uint32_t tri = (cur & 0x7fffffffu) >> 2;
                sink.accept([&]() __attribute__((always_inline)) { return cut_entry(tri, cut); });
            }
        }
        return false;                                                     // no leaf ends the plane
    }
    __device__ __forceinline__ float bound() const { return 1.0f; }       // above every key: every stacked entry is walked
    __device__ __forceinline__ void finish(const RenderArgs&) { if (!FILL) counts[rid] = sink.count; }
    __device__ __forceinline__ void after_refill(uint32_t) {}
    __device__ __forceinline__ void after_step(bool, uint32_t) {}
};
template <bool FILL>
__global__ __launch_bounds__(64) void cut_kernel(PT_REGION_ARGS, unsigned long long* __restrict__ queue, unsigned long long* __restrict__ spill, uint32_t fill) {
    CutWalk<FILL> q{planes, counts, offsets, 4u * A.num_tris, ListSink<FILL>{entries, capacity}};
    persistent_walk<PT_CT_SHORT_STACK>(A, n, queue, spill, fill, q);
}
#undef PT_REGION_ARGS

hipError_t launch_cut(const RenderArgs& A, const void* planes, uint32_t n, void* counts, const unsigned long long* offsets, void* entries,
                      unsigned long long capacity, bool simple, bool stats, bool brute,
                      unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream) {
    static const RegionKernels K = {{cut_brute_kernel<true, false>, cut_brute_kernel<false, true>, cut_brute_kernel<false, false>},
                                    {cut_simple_kernel<true, false>, cut_simple_kernel<false, true>, cut_simple_kernel<false, false>},
                                    {cut_kernel<true>, cut_kernel<false>}, PT_CT_FILL};
    return launch_region(K, A, planes, n, counts, offsets, entries, capacity, simple, stats, brute, queue, spill, grid, stream);
}

} // namespace ptk
