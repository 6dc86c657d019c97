// pt_tritri.hip -- triangle-overlap queries over the context's tree: every mesh triangle that a caller triangle cuts, counted and listed
// (include/mi355pt.h: pt_tri_count, pt_tri_search):
//   * tri_kernel<FILL>                 the default: persistent wavefronts, one caller triangle per lane, a lane whose triangle is answered
//                                      takes the next triangle of its wavefront's chunk.  FILL = false counts the accepted leaves of a
//                                      triangle; FILL = true walks the same walk again and stores entry k of triangle i at offsets[i] + k
//   * tri_simple_kernel<FILL, STATS>   one caller triangle per thread with a private 64-entry stack: PT_TRI_SIMPLE_KERNEL, PT_TRI_STATS
//   * tri_brute_kernel<FILL, STATS>    every mesh triangle in index order, the records streamed through LDS: PT_TRI_BRUTE_FORCE
// The scan between the two walks is pt_radius.hip::launch_radius_scan.
//
// The walk is the box query's (pt_overlap.hip) on the caller triangle's exact bounding box: every key 0, bound() 1, depth-first slot
// order, so the list of a triangle is its accepted leaves in visit order, which depends on the triangle and the tree alone, and entry k
// lands at offsets[i] + k without an atomic.  The leaf arithmetic is pt_tritri.h, shared with the host twin (pt_host.cpp::tri_search),
// which gives the same booleans.  The bodies of the simple and the brute-force kernel and the dispatch are pt_region.h's.
// Records: PtTri = three float4 (q0.xyz, pad; q1.xyz, pad; q2.xyz, pad), an entry = PtCross = one uint4 (prim, edges, 0, 0).
//
// The persistent kernel holds the twelve values of the box AND the caller's nine coordinates per lane for the whole walk: that form
// compiled to fewer registers (66 / 69 VGPRs, 7 waves per SIMD) than the one that reads the 48-byte record again at each leaf that passed
// the box stage (68 / 81 VGPRs, 5 waves per SIMD for the fill walk).  DESIGN.md section 23 has both rows; no GPU run has compared them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_kernels.h"
#include "pt_device.h"
#include "pt_overlap.h"
#include "pt_tritri.h"
#include "pt_points.h"
#include "pt_region.h"
#include "pt_walk.h"

namespace ptk {

// ptov::node_overlaps on one packed f16 box, restated from pt_overlap.hip (a definition of that translation unit): the six differences
// straight from the packed halves (v_fma_mix_f32), their maximum (v_max3_f32) not above 0.  No operand is a NaN: the halves are finite
// or the +-inf of an inverted box, the box corners finite.
__device__ __forceinline__ bool tri_node_overlaps(const ptov::Box& b, uint32_t w0, uint32_t w1, uint32_t w2) {
    const float gx = wmax(half_lo_minus(w0, b.shx), minus_half_hi(b.slx, w1));
    const float gy = wmax(half_hi_minus(w0, b.shy), minus_half_lo(b.sly, w2));
    const float gz = wmax(half_lo_minus(w1, b.shz), minus_half_hi(b.slz, w2));
    return wmax(wmax(gx, gy), gz) <= 0.0f;
}
__device__ __forceinline__ pttt::Tri load_tri(const float4* __restrict__ tris_in, uint32_t i) {
    const float4 a = tris_in[3 * (size_t)i], b = tris_in[3 * (size_t)i + 1], c = tris_in[3 * (size_t)i + 2];
    return pttt::Tri{a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z};
}

// The region of a triangle query (pt_region.h): the box query's node test on the caller triangle's bounding box, and the leaf test of
// pt_tritri.h.  An entry is (prim, edges, 0, 0).  FILL computes all six bits; the count walk stops at the first.
template <bool FILL>
struct TriRegion {
    pttt::Tri q = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    ptov::Box b = ptov::make_box(0, 0, 0, 0, 0, 0);
    bool ok = false;

    __device__ __forceinline__ void load(const float4* __restrict__ tris_in, uint32_t i) {
        q = load_tri(tris_in, i);
        ok = pttt::tri_walked(q);
        b = pttt::tri_box(q);
    }
    __device__ __forceinline__ bool walked() const { return ok; }
    __device__ __forceinline__ bool child(uint32_t w0, uint32_t w1, uint32_t w2, float& key) const { key = 0.0f; return tri_node_overlaps(b, w0, w1, w2); }
    __device__ __forceinline__ float bound() const { return 1.0f; }
    template <class Sink>
    __device__ __forceinline__ void leaf(uint32_t tri, const float4 a, const float4 c, const float4 d, Sink& sink) const {
        const uint32_t edges = pttt::tri_crosses<FILL>(b, q, a.x, c.x, d.x, a.y, c.y, d.y, a.z, c.z, d.z);
        if (edges) sink.accept([&]() __attribute__((always_inline)) { return make_uint4(tri, edges, 0u, 0u); });
    }
};

#define PT_REGION_ARGS const RenderArgs A, const float4* __restrict__ tris_in, uint32_t* __restrict__ counts, const unsigned long long* __restrict__ offsets, \
                       uint4* __restrict__ entries, unsigned long long capacity, uint32_t n
template <bool FILL, bool STATS>
__global__ __launch_bounds__(256) void tri_simple_kernel(PT_REGION_ARGS) { region_simple<TriRegion<FILL>, FILL, STATS>(A, tris_in, counts, offsets, entries, capacity, n); }
template <bool FILL, bool STATS>
__global__ __launch_bounds__(256) void tri_brute_kernel(PT_REGION_ARGS) { region_brute<TriRegion<FILL>, FILL, STATS>(A, tris_in, counts, offsets, entries, capacity, n); }
// persistent_walk's Q (pt_walk.h) of a triangle query.  A leaf is gated on leaf_end: an out-of-range leaf points at the record behind
// the last triangle, which must not count.
template <bool FILL>
struct TriWalk {
    static constexpr bool kWaveHooks = false;
    static constexpr float kKeyInit = 0.0f;       // pt_device.h::order_children
    const float4* __restrict__ tris_in; uint32_t* __restrict__ counts; const unsigned long long* __restrict__ offsets; uint32_t leaf_end;
    ListSink<FILL> sink;
    uint32_t rid = 0;
    ptov::Box b = ptov::make_box(0, 0, 0, 0, 0, 0);
    pttt::Tri q = {0, 0, 0, 0, 0, 0, 0, 0, 0};

    __device__ __forceinline__ bool start(const RenderArgs& A, uint32_t item, bool scene_ok) {
        rid = item;
        q = load_tri(tris_in, rid);
        const bool walked = pttt::tri_walked(q);
        b = pttt::tri_box(q);
        sink.count = 0u;
        if (scene_ok && walked && tri_node_overlaps(b, A.root_box[0], A.root_box[1], A.root_box[2])) {
            if (FILL) sink.base = offsets[rid];
            return true;
        }
        if (!FILL) counts[rid] = 0u;
        return false;
    }
    __device__ __forceinline__ bool child(uint32_t w0, uint32_t w1, uint32_t w2, float& key) const { key = 0.0f; return tri_node_overlaps(b, w0, w1, w2); }
    __device__ __forceinline__ bool leaf(uint32_t cur, const uint4 n0, const uint4 n1, const uint4 n2) {
        const float4 a = as_float4(n0), c = as_float4(n1), d = as_float4(n2);
        if ((cur & 0x7fffffffu) < leaf_end) {
            const uint32_t edges = pttt::tri_crosses<FILL>(b, q, a.x, c.x, d.x, a.y, c.y, d.y, a.z, c.z, d.z);
            if (edges) {
                const uint32_t tri = (cur & 0x7fffffffu) >> 2;
                sink.accept([&]() __attribute__((always_inline)) { return make_uint4(tri, edges, 0u, 0u); });
            }
        }
        return false;                                                     // no leaf ends the triangle
    }
    __device__ __forceinline__ float bound() const { return 1.0f; }       // above every key: every stacked entry is walked
    __device__ __forceinline__ void finish(const RenderArgs&) { if (!FILL) counts[rid] = sink.count; }
    __device__ __forceinline__ void after_refill(uint32_t) {}
    __device__ __forceinline__ void after_step(bool, uint32_t) {}
};
template <bool FILL>
__global__ __launch_bounds__(64) void tri_kernel(PT_REGION_ARGS, unsigned long long* __restrict__ queue, unsigned long long* __restrict__ spill, uint32_t fill) {
    TriWalk<FILL> q{tris_in, counts, offsets, 4u * A.num_tris, ListSink<FILL>{entries, capacity}};
    persistent_walk<PT_TT_SHORT_STACK>(A, n, queue, spill, fill, q);
}
#undef PT_REGION_ARGS

hipError_t launch_tri(const RenderArgs& A, const void* tris_in, uint32_t n, void* counts, const unsigned long long* offsets, void* entries,
                      unsigned long long capacity, bool simple, bool stats, bool brute,
                      unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream) {
    static const RegionKernels K = {{tri_brute_kernel<true, false>, tri_brute_kernel<false, true>, tri_brute_kernel<false, false>},
                                    {tri_simple_kernel<true, false>, tri_simple_kernel<false, true>, tri_simple_kernel<false, false>},
                                    {tri_kernel<true>, tri_kernel<false>}, PT_TT_FILL};
    return launch_region(K, A, tris_in, n, counts, offsets, entries, capacity, simple, stats, brute, queue, spill, grid, stream);
}

} // namespace ptk
