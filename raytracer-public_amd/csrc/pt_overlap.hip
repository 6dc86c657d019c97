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
// (pt_host.cpp::box_search), which gives the same booleans.
// Records: PtBox = two float4 (lo.xyz, pad; hi.xyz, pad), an entry = PtOverlap = one uint4 (prim, verts_inside, 0, 0).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_kernels.h"
#include "pt_device.h"
#include "pt_overlap.h"
#include "pt_points.h"
#include "pt_walk.h"

namespace ptk {

// What the three kernels do with an accepted leaf: count it, and with FILL store its entry (one plain 16-byte vector store) when its
// global index is below the capacity.  base + k is 64-bit: the total of a batch may pass 2^32.
template <bool FILL>
struct BxSink {
    uint4* __restrict__ entries; unsigned long long capacity;
    unsigned long long base = 0; uint32_t count = 0;
    __device__ __forceinline__ void accept(uint32_t tri, uint32_t verts_inside) {
        if (FILL) {
            const unsigned long long g = base + count;
            if (g < capacity) entries[g] = make_uint4(tri, verts_inside, 0u, 0u);
        }
        ++count;
    }
};

__device__ __forceinline__ bool load_box(const float4* __restrict__ boxes, uint32_t i, ptov::Box& b) {
    const float4 lo = boxes[2 * (size_t)i], hi = boxes[2 * (size_t)i + 1];
    b = ptov::make_box(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z);
    return ptov::box_walked(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z);
}
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

// ------------------------------------------------------------------------------------
// simple kernel: one box per thread, a private 64-entry stack; the counters of PT_BOX_STATS by the rules of PT_RADIUS_STATS
// (pt_radius.hip::radius_walk_point with every key 0)
// ------------------------------------------------------------------------------------
template <bool FILL, bool STATS>
__device__ __forceinline__ void box_walk_one(const RenderArgs& A, const ptov::Box& b, uint2* __restrict__ stk, Counters& cnt, BxSink<FILL>& sink) {
    if (A.root_ref == kInvalidRef || A.num_tris == 0u) return;
    if (STATS) { cnt.nodes += 1; if (cnt.maxstack < 1u) cnt.maxstack = 1u; }      // the root record is fetched before its degenerate check
    if (A.root_degenerate) return;
    if (!node_overlaps(b, A.root_box[0], A.root_box[1], A.root_box[2])) return;
    uint32_t cur = A.root_ref;
    int sp = 0;
    for (;;) {
        bool need_pop = false;
        if (cur & kLeaf) {
            const uint32_t ti4 = cur & 0x7fffffffu;
            if (ti4 < 4u * A.num_tris) {                          // an out-of-range leaf points at the record behind the last triangle: skipped
                const float4* tp = (const float4*)arena_record(A, cur);
                if (STATS) cnt.tris += 1;
                uint32_t in;
                if (tri_overlaps(b, tp[0], tp[1], tp[2], in)) sink.accept(ti4 >> 2, in);
            }
            need_pop = true;
        } else {
            const uint4* np = arena_record(A, cur);
            const uint4 n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3];
            const uint32_t r0 = n0.w, r1 = n1.w, r2 = n2.w, r3 = n3.w;
            const bool h0 = node_overlaps(b, n0.x, n0.y, n0.z), h1 = node_overlaps(b, n1.x, n1.y, n1.z);
            const bool h2 = node_overlaps(b, n2.x, n2.y, n2.z), h3 = node_overlaps(b, n3.x, n3.y, n3.z);
            if (STATS) cnt.nodes += (r0 != kInvalidRef) + (r1 != kInvalidRef) + (r2 != kInvalidRef) + (r3 != kInvalidRef);
            uint32_t enter;
            const int before = sp;
            const bool any = h0 | h1 | h2 | h3;
            const uint32_t wanted = (uint32_t)h0 + (uint32_t)h1 + (uint32_t)h2 + (uint32_t)h3;      // one entered, the others pushed
            const bool go = order_children(h0, h1, h2, h3, 0.0f, 0.0f, 0.0f, 0.0f, r0, r1, r2, r3, 0.0f, sp, enter, [&](int at, uint32_t ref, float) __attribute__((always_inline)) {
                stk[at] = make_uint2(ref, 0u);
            });
            if (STATS && any) {
                // pushes that did not fit, and the entered child's own when the stack is full (pt_radius.hip::radius_walk_point)
                cnt.drops += (wanted - 1u) - (uint32_t)(sp - before) + (go ? 0u : 1u);
                const uint32_t depth = (uint32_t)sp + (go ? 1u : 0u);
                if (depth > cnt.maxstack) cnt.maxstack = depth;
            }
            if (go) cur = enter; else need_pop = true;
        }
        if (need_pop) {
            if (sp == 0) break;
            cur = stk[--sp].x;                                    // every stacked entry is walked: nothing shrinks the box
        }
    }
}

template <bool FILL, bool STATS>
__global__ __launch_bounds__(256) void box_simple_kernel(const RenderArgs A, const float4* __restrict__ boxes, uint32_t* __restrict__ counts,
                                                         const unsigned long long* __restrict__ offsets, uint4* __restrict__ entries,
                                                         unsigned long long capacity, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    Counters cnt; cnt.nodes = cnt.tris = cnt.drops = cnt.maxstack = 0;
    if (i < n) {
        ptov::Box b;
        const bool walked = load_box(boxes, i, b);
        BxSink<FILL> sink{entries, capacity};
        if (FILL) sink.base = offsets[i];
        if (walked) {
            uint2 stk[kStackMax];
            box_walk_one<FILL, STATS>(A, b, stk, cnt, sink);
        }
        if (!FILL) counts[i] = sink.count;
    }
    if (STATS) add_stats(A, 0, i < n ? 1u : 0u, cnt);
}

// ------------------------------------------------------------------------------------
// persistent kernel: one wavefront per workgroup, one box per lane, lanes refilled from the wavefront's chunk
// ------------------------------------------------------------------------------------
// persistent_walk's Q (pt_walk.h) of a box query.  A leaf is gated on leaf_end: an out-of-range leaf points at the record behind the last
// triangle, which must not count.
template <bool FILL>
struct BoxWalk {
    static constexpr bool kWaveHooks = false;
    static constexpr float kKeyInit = 0.0f;       // pt_device.h::order_children
    const float4* __restrict__ boxes; uint32_t* __restrict__ counts; const unsigned long long* __restrict__ offsets; uint32_t leaf_end;
    BxSink<FILL> sink;
    uint32_t rid = 0;
    ptov::Box b = ptov::make_box(0, 0, 0, 0, 0, 0);

    __device__ __forceinline__ bool start(const RenderArgs& A, uint32_t item, bool scene_ok) {
        rid = item;
        const bool walked = load_box(boxes, rid, b);
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
        if (((cur & 0x7fffffffu) < leaf_end) & hit) sink.accept((cur & 0x7fffffffu) >> 2, in);
        return false;                                                     // no leaf ends the box
    }
    __device__ __forceinline__ float bound() const { return 1.0f; }       // above every key: every stacked entry is walked
    __device__ __forceinline__ void finish(const RenderArgs&) { if (!FILL) counts[rid] = sink.count; }
    __device__ __forceinline__ void after_refill(uint32_t) {}
    __device__ __forceinline__ void after_step(bool, uint32_t) {}
};
template <bool FILL>
__global__ __launch_bounds__(64) void box_kernel(const RenderArgs A, const float4* __restrict__ boxes, uint32_t* __restrict__ counts,
                                                 const unsigned long long* __restrict__ offsets, uint4* __restrict__ entries, unsigned long long capacity,
                                                 uint32_t n, unsigned long long* __restrict__ queue, unsigned long long* __restrict__ spill, uint32_t fill) {
    BoxWalk<FILL> q{boxes, counts, offsets, 4u * A.num_tris, BxSink<FILL>{entries, capacity}};
    persistent_walk<PT_BX_SHORT_STACK>(A, n, queue, spill, fill, q);
}

// ------------------------------------------------------------------------------------
// brute force: one box per thread, every triangle in index order; a workgroup streams the records through LDS, kBxBruteTile at a time
// ------------------------------------------------------------------------------------
constexpr uint32_t kBxBruteTile = 256;
template <bool FILL, bool STATS>
__global__ __launch_bounds__(256) void box_brute_kernel(const RenderArgs A, const float4* __restrict__ boxes, uint32_t* __restrict__ counts,
                                                        const unsigned long long* __restrict__ offsets, uint4* __restrict__ entries,
                                                        unsigned long long capacity, uint32_t n) {
    __shared__ float4 rec[kBxBruteTile][3];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    ptov::Box b = ptov::make_box(0, 0, 0, 0, 0, 0);
    const bool walked = (i < n) && load_box(boxes, i, b);
    BxSink<FILL> sink{entries, capacity};
    if (FILL && i < n) sink.base = offsets[i];
    Counters cnt; cnt.nodes = cnt.tris = cnt.drops = cnt.maxstack = 0;
    for (uint32_t base = 0; base < A.num_tris; base += kBxBruteTile) {
        const uint32_t tile = min(kBxBruteTile, A.num_tris - base);
        __syncthreads();
        if (threadIdx.x < tile) {
            const float4* tp = A.tris + (size_t)(base + threadIdx.x) * 4;
            rec[threadIdx.x][0] = tp[0]; rec[threadIdx.x][1] = tp[1]; rec[threadIdx.x][2] = tp[2];
        }
        __syncthreads();
        if (walked) {
            for (uint32_t k = 0; k < tile; ++k) {
                uint32_t in;
                if (tri_overlaps(b, rec[k][0], rec[k][1], rec[k][2], in)) sink.accept(base + k, in);
            }
            if (STATS) cnt.tris += tile;
        }
    }
    if (!FILL && i < n) counts[i] = sink.count;
    if (STATS) add_stats(A, 0, i < n ? 1u : 0u, cnt);
}

hipError_t launch_box(const RenderArgs& A, const void* boxes, uint32_t n, void* counts, const unsigned long long* offsets, void* entries,
                      unsigned long long capacity, bool simple, bool stats, bool brute,
                      unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    const float4* p = (const float4*)boxes; uint32_t* c = (uint32_t*)counts; uint4* e = (uint4*)entries;
    const bool fill = offsets != nullptr;
    const dim3 g256((n + 255u) / 256u);
    if (brute) {
        if (fill) box_brute_kernel<true, false><<<g256, 256, 0, stream>>>(A, p, c, offsets, e, capacity, n);
        else if (stats) box_brute_kernel<false, true><<<g256, 256, 0, stream>>>(A, p, c, offsets, e, capacity, n);
        else box_brute_kernel<false, false><<<g256, 256, 0, stream>>>(A, p, c, offsets, e, capacity, n);
        return hipGetLastError();
    }
    if (simple || stats) {
        if (fill) box_simple_kernel<true, false><<<g256, 256, 0, stream>>>(A, p, c, offsets, e, capacity, n);
        else if (stats) box_simple_kernel<false, true><<<g256, 256, 0, stream>>>(A, p, c, offsets, e, capacity, n);
        else box_simple_kernel<false, false><<<g256, 256, 0, stream>>>(A, p, c, offsets, e, capacity, n);
        return hipGetLastError();
    }
    hipError_t err = walk_begin(queue, n, grid, stream);
    if (err != hipSuccess) return err;
    if (fill) box_kernel<true><<<grid, 64, 0, stream>>>(A, p, c, offsets, e, capacity, n, queue, spill, PT_BX_FILL);
    else box_kernel<false><<<grid, 64, 0, stream>>>(A, p, c, offsets, e, capacity, n, queue, spill, PT_BX_FILL);
    return hipGetLastError();
}

} // namespace ptk
