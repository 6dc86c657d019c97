// pt_region.h -- the count/fill frame of the region queries, once: every triangle that meets a region, counted and listed.  A region is
// a sphere around a point (pt_radius.hip: SphereRegion) or an axis-aligned box (pt_overlap.hip: BoxRegion); shared are the bodies of
// the two diagnostic kernels of each query and the dispatch:
//   * region_simple<R, FILL, STATS>      one region per thread with a private 64-entry stack (pt_points.h::key_traverse)
//   * region_brute<R, FILL, STATS>       every triangle in index order, the records streamed through LDS (pt_walk.h::brute_records)
//   * launch_region                      which of a query's eight kernels a call launches
// The persistent kernels' Qs (RadiusWalk, BoxWalk) stay in their files: shared, radius_kernel and box_kernel compiled to other streams,
// and rows of both timed outside the parent's run-to-run spread (profiles/point_share_ab.json).
// FILL = false counts the accepted leaves of a region; FILL = true walks the same walk again and stores entry k of region i at
// offsets[i] + k (pt_walk.h::ListSink).  The list of a region is its accepted leaves in visit order, which depends on the region and the
// tree alone -- nothing moves the bound -- so the two walks of a region take the same steps whichever lane, wavefront or kernel runs
// them, and an entry lands without an atomic.  The __global__ kernels stay in their files, as wrappers of the two bodies.
//
// A region policy R holds the thread's region and supplies:
//   void  load(in, i)                    read input record i
//   bool  walked()                       whether the region is walked at all (no NaN, a positive extent)
//   bool  child(w0, w1, w2, key)         whether the child with this packed f16 box is visited, and its key (below bound() if visited)
//   float bound()                        what a stacked key is re-validated against
//   void  leaf(tri, a, b, c, sink)       the test of triangle record (a, b, c); sink.accept(entry) if it passes
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_kernels.h"
#include "pt_device.h"
#include "pt_points.h"
#include "pt_walk.h"

namespace ptk {

template <class R, bool FILL, bool STATS>
__device__ __forceinline__ void region_simple(const RenderArgs& A, const float4* __restrict__ in, uint32_t* __restrict__ counts,
                                              const unsigned long long* __restrict__ offsets, uint4* __restrict__ entries,
                                              unsigned long long capacity, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    Counters cnt; cnt.nodes = cnt.tris = cnt.drops = cnt.maxstack = 0;
    if (i < n) {
        R r;
        r.load(in, i);
        ListSink<FILL> sink{entries, capacity};
        if (FILL) sink.base = offsets[i];
        if (r.walked()) {
            uint2 stk[kStackMax];
            const float bound = r.bound();
            key_traverse<STATS>(A, [&](uint32_t w0, uint32_t w1, uint32_t w2, float& key) __attribute__((always_inline)) { return r.child(w0, w1, w2, key); }, bound, stk, cnt,
                                [&](uint32_t cur, const float4 a, const float4 b, const float4 c) __attribute__((always_inline)) {
                r.leaf((cur & 0x7fffffffu) >> 2, a, b, c, sink);
            });
        }
        if (!FILL) counts[i] = sink.count;
    }
    if (STATS) add_stats(A, 0, i < n ? 1u : 0u, cnt);
}

template <class R, bool FILL, bool STATS>
__device__ __forceinline__ void region_brute(const RenderArgs& A, const float4* __restrict__ in, uint32_t* __restrict__ counts,
                                             const unsigned long long* __restrict__ offsets, uint4* __restrict__ entries,
                                             unsigned long long capacity, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    R r;
    if (i < n) r.load(in, i);
    const bool walked = (i < n) && r.walked();
    ListSink<FILL> sink{entries, capacity};
    if (FILL && i < n) sink.base = offsets[i];
    brute_records(A, walked, [&](uint32_t tri, const uint4 n0, const uint4 n1, const uint4 n2) __attribute__((always_inline)) {
        r.leaf(tri, as_float4(n0), as_float4(n1), as_float4(n2), sink);
    });
    if (!FILL && i < n) counts[i] = sink.count;
    if (STATS) {
        Counters cnt; cnt.nodes = cnt.drops = cnt.maxstack = 0;
        cnt.tris = walked ? A.num_tris : 0u;                              // a walked region tests every record
        add_stats(A, 0, i < n ? 1u : 0u, cnt);
    }
}

// The eight kernels of a region query -- fill, count + stats and count of the brute-force and the simple kernel, fill and count of the
// persistent one -- and the refill knob of the last.  offsets != nullptr asks for the fill walk; the counters are the count walk's.
using RegionKernel = void (*)(const RenderArgs, const float4*, uint32_t*, const unsigned long long*, uint4*, unsigned long long, uint32_t);
using RegionWalkKernel = void (*)(const RenderArgs, const float4*, uint32_t*, const unsigned long long*, uint4*, unsigned long long, uint32_t,
                                  unsigned long long*, unsigned long long*, uint32_t);
struct RegionKernels { RegionKernel brute[3], simple[3]; RegionWalkKernel walk[2]; uint32_t fill; };

inline hipError_t launch_region(const RegionKernels& K, const RenderArgs& A, const void* in, uint32_t n, void* counts, const unsigned long long* offsets,
                                void* entries, unsigned long long capacity, bool simple, bool stats, bool brute,
                                unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    const float4* p = (const float4*)in; uint32_t* c = (uint32_t*)counts; uint4* e = (uint4*)entries;
    const bool fill = offsets != nullptr;
    if (brute || simple || stats) {
        const RegionKernel k = (brute ? K.brute : K.simple)[fill ? 0 : stats ? 1 : 2];
        k<<<dim3((n + 255u) / 256u), 256, 0, stream>>>(A, p, c, offsets, e, capacity, n);
        return hipGetLastError();
    }
    hipError_t err = walk_begin(queue, n, grid, stream);
    if (err != hipSuccess) return err;
    K.walk[fill ? 0 : 1]<<<grid, 64, 0, stream>>>(A, p, c, offsets, e, capacity, n, queue, spill, K.fill);
    return hipGetLastError();
}

} // namespace ptk
