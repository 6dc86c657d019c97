// pt_knn.hip -- k-nearest-triangle queries over the context's tree: the k closest triangles to each point, sorted by distance
// (include/mi355pt.h: pt_nearest_k):
//   * nearest_k_kernel<KCAP>              the default: persistent wavefronts, one point per lane, a lane whose point is answered takes the
//                                         next point of its wavefront's chunk.  The lane's list is a column of LDS, list[j][lane]; KCAP is
//                                         the capacity tier (4, 16, 64), the smallest one >= k is launched
//   * nearest_k_simple_kernel<STATS>      one point per thread with a private 64-entry stack and a private list: PT_NEAREST_SIMPLE_KERNEL,
//                                         PT_NEAREST_STATS
//   * nearest_k_brute_kernel<STATS>       every triangle in index order, the records streamed through LDS: PT_NEAREST_BRUTE_FORCE
//
// The walk is the closest-point walk (pt_pointquery.hip, pt_walk.h::persistent_walk) with worst2 in the place of best2: r_max^2 while the
// list holds fewer than k pairs, the d2 of its last pair after that.  A child is entered if bound2 < worst2, a leaf is accepted if
// d2 < worst2 (strictly), a stacked child is re-validated at pop against worst2, which only falls.  An accepted pair (d2, leaf reference)
// goes behind every pair with d2' <= d2, so equal distances keep visit order, and the pair behind the k-th falls off.  The visit order
// depends on the point and the tree alone, so the three kernels' walks and the host twin (pt_host.cpp::nearest_k) give the same rows, ties
// included.  The point-triangle arithmetic is pt_closest.h, shared with the twin.
// The point record, the slack, box_bound2, tri_d2 and the one-point-per-thread walk (key_traverse) are pt_points.h's, shared with
// pt_pointquery.hip, pt_radius.hip and pt_overlap.hip; the LDS streaming loop (brute_records) is pt_walk.h's.
// Records: PtPoint = one float4 (p.xyz, r_max), an entry = PtClosest = one uint4 (dist bits, prim, u bits, v bits); row i is
// out[i * k .. i * k + k - 1], padded with (+inf, 0xFFFFFFFF, 0, 0).  Plain vector stores only; the one atomic is the walk's queue claim.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_kernels.h"
#include "pt_device.h"
#include "pt_closest.h"
#include "pt_points.h"
#include "pt_walk.h"

namespace ptk {

// ------------------------------------------------------------------------------------
// the list: at most k pairs (d2 bits << 32 | tag), ascending by d2, entry j at lst[j * STRIDE].  STRIDE = 64 is a lane's column of LDS
// (list[j][lane]: a lane touching row j hits the same banks whatever j is, so divergent insert positions do not conflict), STRIDE = 1 a
// private array.  The tag is the leaf reference in the walks and the triangle index in brute force.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ float nk_pair_d2(unsigned long long e) { return __uint_as_float((uint32_t)(e >> 32)); }

// d2 < worst2 holds: the pair goes behind every pair with d2' <= d2, shifting the tail down one row from the end; with k pairs held the
// last one falls off.  Returns the new worst2.
template <int STRIDE>
__device__ __forceinline__ float nk_insert(unsigned long long* lst, uint32_t& count, uint32_t k, float worst2, float d2, uint32_t tag) {
    uint32_t j = count < k ? count : k - 1u;
    while (j > 0u) {
        const unsigned long long e = lst[(j - 1u) * STRIDE];
        if (!(nk_pair_d2(e) > d2)) break;
        lst[j * STRIDE] = e;
        --j;
    }
    lst[j * STRIDE] = ((unsigned long long)__float_as_uint(d2) << 32) | tag;
    if (count < k) ++count;
    return count == k ? nk_pair_d2(lst[(k - 1u) * STRIDE]) : worst2;
}

// Row `row` of the output: entry j < count is pt_pointquery.hip::closest_record of the pair's triangle (dist = sqrtf(d2), u and v recomputed
// from the record with the operations of the accepted test), the entries behind them are the padding.  TAG_SHIFT turns a tag into a
// triangle index: 2 for a leaf reference (whose leaf bit is masked), 0 for an index.
template <int STRIDE, int TAG_SHIFT>
__device__ __forceinline__ void nk_write_row(uint4* __restrict__ out, const float4* __restrict__ tris, F3 p, const unsigned long long* lst,
                                             uint32_t count, uint32_t k, uint32_t row) {
    uint4* o = out + (size_t)row * k;
    for (uint32_t j = 0; j < count; ++j) {
        const unsigned long long e = lst[j * STRIDE];
        const uint32_t tri = ((uint32_t)e & 0x7fffffffu) >> TAG_SHIFT;
        const float4* tp = tris + (size_t)tri * 4;
        const float4 a = tp[0], b = tp[1], c = tp[2];
        float u, v;
        ptcp::closest_uv(p.x - a.x, p.y - b.x, p.z - c.x, a.y, b.y, c.y, a.z, b.z, c.z, u, v);
        o[j] = make_uint4(__float_as_uint(sqrtf(nk_pair_d2(e))), tri, __float_as_uint(u), __float_as_uint(v));
    }
    for (uint32_t j = count; j < k; ++j) o[j] = make_uint4(kInfBits, kInvalidRef, 0u, 0u);
}

// ------------------------------------------------------------------------------------
// simple kernel: one point per thread, a private 64-entry stack and a private list; the walk and the counters of PT_NEAREST_STATS are
// pt_pointquery.hip::walk_point's (pt_points.h::key_traverse) with worst2 for best2
// ------------------------------------------------------------------------------------
template <bool STATS>
__device__ __forceinline__ void nearest_walk_point(const RenderArgs& A, F3 p, float worst2, uint32_t k, unsigned long long* lst, uint32_t& count,
                                                   uint2* __restrict__ stk, Counters& cnt) {
    const PointSlack s = point_slack(p);
    key_traverse<STATS>(A, [&](uint32_t w0, uint32_t w1, uint32_t w2, float& key) __attribute__((always_inline)) { key = box_bound2(s, w0, w1, w2); return key < worst2; }, worst2, stk, cnt,
                        [&](uint32_t cur, const float4 a, const float4 b, const float4 c) __attribute__((always_inline)) {
        const float d2 = tri_d2(p, a, b, c);
        if (d2 < worst2) worst2 = nk_insert<1>(lst, count, k, worst2, d2, cur);
    });
}

template <bool STATS>
__global__ __launch_bounds__(256) void nearest_k_simple_kernel(const RenderArgs A, const float4* __restrict__ pts, uint4* __restrict__ out,
                                                               uint32_t n, uint32_t k) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    Counters cnt; cnt.nodes = cnt.tris = cnt.drops = cnt.maxstack = 0;
    if (i < n) {
        F3 p; float rmax;
        load_point(pts, i, p, rmax);
        unsigned long long lst[kNearestMaxK];
        uint32_t count = 0;
        if (ptcp::point_walked(p.x, p.y, p.z, rmax)) {
            uint2 stk[kStackMax];
            nearest_walk_point<STATS>(A, p, rmax * rmax, k, lst, count, stk, cnt);
        }
        nk_write_row<1, 2>(out, A.tris, p, lst, count, k, i);
    }
    if (STATS) add_stats(A, 0, i < n ? 1u : 0u, cnt);
}

// ------------------------------------------------------------------------------------
// persistent kernel: one wavefront per workgroup, one point per lane, lanes refilled from the wavefront's chunk
// ------------------------------------------------------------------------------------
// persistent_walk's Q (pt_walk.h) of a k-nearest query: pt_pointquery.hip::PointWalk with worst2 for best2 and the list for the best
// triangle.  worst2 is the register copy of what the list says; `lst` is the lane's column of the kernel's LDS list.  A leaf is gated on
// leaf_end: an out-of-range leaf points at the record behind the last triangle, whose distance must not count.
struct NearestWalk {
    static constexpr bool kWaveHooks = false;
    static constexpr float kKeyInit = 0.0f;       // pt_device.h::order_children
    const float4* __restrict__ pts; uint4* __restrict__ out; const float4* __restrict__ tris; uint32_t leaf_end, k;
    unsigned long long* lst;
    uint32_t rid = 0, count = 0; float worst2 = 0.0f;
    F3 p = f3(0, 0, 0); PointSlack s = point_slack(p);

    __device__ __forceinline__ bool start(const RenderArgs& A, uint32_t item, bool scene_ok) {
        rid = item;
        float rmax;
        load_point(pts, rid, p, rmax);
        worst2 = rmax * rmax; count = 0u;
        s = point_slack(p);
        if (scene_ok && ptcp::point_walked(p.x, p.y, p.z, rmax) && box_bound2(s, A.root_box[0], A.root_box[1], A.root_box[2]) < worst2) return true;
        nk_write_row<64, 2>(out, tris, p, lst, 0u, k, rid);
        return false;
    }
    __device__ __forceinline__ bool child(uint32_t w0, uint32_t w1, uint32_t w2, float& bound2) const { bound2 = box_bound2(s, w0, w1, w2); return bound2 < worst2; }
    __device__ __forceinline__ bool leaf(uint32_t cur, const uint4 n0, const uint4 n1, const uint4 n2) {
        const float d2 = tri_d2(p, as_float4(n0), as_float4(n1), as_float4(n2));
        if (((cur & 0x7fffffffu) < leaf_end) & (d2 < worst2)) worst2 = nk_insert<64>(lst, count, k, worst2, d2, cur);
        return false;                                                     // no leaf ends the point
    }
    __device__ __forceinline__ float bound() const { return worst2; }
    __device__ __forceinline__ void finish(const RenderArgs&) { nk_write_row<64, 2>(out, tris, p, lst, count, k, rid); }
    __device__ __forceinline__ void after_refill(uint32_t) {}
    __device__ __forceinline__ void after_step(bool, uint32_t) {}
};
// k <= KCAP (launch_nearest_k picks the tier): the list rows k .. KCAP-1 are never touched
template <int KCAP>
__global__ __launch_bounds__(64) void nearest_k_kernel(const RenderArgs A, const float4* __restrict__ pts, uint4* __restrict__ out, uint32_t n, uint32_t k,
                                                       unsigned long long* __restrict__ queue, unsigned long long* __restrict__ spill, uint32_t fill) {
    __shared__ unsigned long long list[KCAP][64];
    NearestWalk q{pts, out, A.tris, 4u * A.num_tris, k, &list[0][threadIdx.x]};
    persistent_walk<PT_NK_SHORT_STACK>(A, n, queue, spill, fill, q);
}

// ------------------------------------------------------------------------------------
// brute force: one point per thread, every triangle in index order with the same list rule (pt_walk.h::brute_records)
// ------------------------------------------------------------------------------------
template <bool STATS>
__global__ __launch_bounds__(256) void nearest_k_brute_kernel(const RenderArgs A, const float4* __restrict__ pts, uint4* __restrict__ out,
                                                              uint32_t n, uint32_t k) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    F3 p = f3(0, 0, 0); float rmax = 0.0f;
    if (i < n) load_point(pts, i, p, rmax);
    const bool walked = (i < n) && ptcp::point_walked(p.x, p.y, p.z, rmax);
    float worst2 = rmax * rmax;
    unsigned long long lst[kNearestMaxK];
    uint32_t count = 0;
    brute_records(A, walked, [&](uint32_t t, const uint4 n0, const uint4 n1, const uint4 n2) __attribute__((always_inline)) {
        const float d2 = tri_d2(p, as_float4(n0), as_float4(n1), as_float4(n2));
        if (d2 < worst2) worst2 = nk_insert<1>(lst, count, k, worst2, d2, t);
    });
    if (i < n) nk_write_row<1, 0>(out, A.tris, p, lst, count, k, i);
    if (STATS) {
        Counters cnt; cnt.nodes = cnt.drops = cnt.maxstack = 0;
        cnt.tris = walked ? A.num_tris : 0u;                              // a walked point tests every record
        add_stats(A, 0, i < n ? 1u : 0u, cnt);
    }
}

uint32_t nearest_k_waves_per_simd(uint32_t k) { return k <= 4u ? PT_NK_WAVES_PER_SIMD_4 : k <= 16u ? PT_NK_WAVES_PER_SIMD_16 : PT_NK_WAVES_PER_SIMD_64; }

hipError_t launch_nearest_k(const RenderArgs& A, const void* points, void* out, uint32_t n, uint32_t k, bool simple, bool stats, bool brute,
                            unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    if (k == 0u || k > kNearestMaxK) return hipErrorInvalidValue;
    const float4* p = (const float4*)points; uint4* o = (uint4*)out;
    const dim3 g256((n + 255u) / 256u);
    if (brute) {
        if (stats) nearest_k_brute_kernel<true><<<g256, 256, 0, stream>>>(A, p, o, n, k);
        else nearest_k_brute_kernel<false><<<g256, 256, 0, stream>>>(A, p, o, n, k);
        return hipGetLastError();
    }
    if (simple || stats) {
        if (stats) nearest_k_simple_kernel<true><<<g256, 256, 0, stream>>>(A, p, o, n, k);
        else nearest_k_simple_kernel<false><<<g256, 256, 0, stream>>>(A, p, o, n, k);
        return hipGetLastError();
    }
    hipError_t e = walk_begin(queue, n, grid, stream);
    if (e != hipSuccess) return e;
    if (k <= 4u) nearest_k_kernel<4><<<grid, 64, 0, stream>>>(A, p, o, n, k, queue, spill, PT_NK_FILL);
    else if (k <= 16u) nearest_k_kernel<16><<<grid, 64, 0, stream>>>(A, p, o, n, k, queue, spill, PT_NK_FILL);
    else nearest_k_kernel<64><<<grid, 64, 0, stream>>>(A, p, o, n, k, queue, spill, PT_NK_FILL);
    return hipGetLastError();
}

} // namespace ptk
