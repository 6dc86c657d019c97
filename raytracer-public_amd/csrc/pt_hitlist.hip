// pt_hitlist.hip -- every crossing along a ray, listed: t, triangle and u, v per crossing (include/mi355pt.h: pt_list_hits; DESIGN.md
// section 20).  The count walk is pt_crossings.hip's (launch_count_hits), the scan is pt_radius.hip's (launch_radius_scan); this file holds
// the second walk, which takes the steps of the count walk again and stores, and the sort:
//   * hit_fill_kernel                 the default: persistent wavefronts, one ray per lane; count_hits_kernel's walk with a leaf() that
//                                     stores entry k of ray i at offsets[i] + k
//   * hit_fill_simple_kernel          one ray per thread with a private 64-entry stack: PT_HITS_SIMPLE_KERNEL, PT_HITS_STATS
//   * hit_fill_brute_kernel           every triangle in index order, the records streamed through LDS: PT_HITS_BRUTE_FORCE
//   * hit_sort_kernel                 PT_HITS_SORTED: every fully stored list in place into ascending (t bits << 32 | prim)
//
// The list of a ray is the records pt_count_hits counts, in visit order: `best` = min(t_max, kInfT) never moves and no hit ends the ray, so
// the walk is a property of the ray and the tree and the two walks of a ray take the same steps whichever lane, wavefront or kernel runs
// them.  Entry k lands at offsets[i] + k without an atomic; each store is one plain 16-byte vector store at a 64-bit index.
// An entry is pt_rays.h::hit_entry of the accepted tri_hit, the function pt_rayquery.hip::hit_record writes its record with; the ray
// record, the lane state and the one-ray walk are pt_rays.h's too, shared with pt_crossings.hip's count walk; the LDS streaming loop and
// the sink's storage are pt_walk.h's, shared with the point side.
// Records: PtRay = two float4 (org.xyz, t_max | dir.xyz, reserved), an entry = PtHit = one uint4 (t bits, prim, u bits, v bits).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_kernels.h"
#include "pt_device.h"
#include "pt_rays.h"
#include "pt_walk.h"

namespace ptk {

// What the three kernels do with a crossing: pt_walk.h::ListSink's accept -- the entry stored when its global index is below the
// capacity -- behind the triangle test.
struct HlSink : ListSink<true> {
    __device__ __forceinline__ void leaf(F3 o, F3 d, float best, uint32_t tri, const uint4 n0, const uint4 n1, const uint4 n2) {
        float t;
        if (tri_hit(o, d, n0, n1, n2, t) & (t < best)) accept([&]() __attribute__((always_inline)) { return hit_entry(o, d, t, tri, n0, n1, n2); });
    }
};

// ------------------------------------------------------------------------------------
// one ray per thread: pt_rays.h::cross_traverse, the walk of count_hits_simple_kernel, with a store in place of the count
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hit_fill_simple_kernel(const RenderArgs A, const float4* __restrict__ rays, const unsigned long long* __restrict__ offsets,
                                                              uint4* __restrict__ entries, unsigned long long capacity, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    F3 o, d; float tmax;
    load_ray(rays, i, o, d, tmax);
    if (!ray_traced(o, d, tmax)) return;
    HlSink sink{{entries, capacity}};
    sink.base = offsets[i];
    Ray r; r.o = o; r.d = d; r.inv = safe_inv(d);
    uint2 stk[kStackMax];
    Counters cnt;                                                         // never counted: PT_HITS_STATS counts in the count walk
    const float best = wmin(tmax, kInfT);
    cross_traverse<false>(A, r, stk, cnt, best, [&](uint32_t tri, const uint4 n0, const uint4 n1, const uint4 n2) __attribute__((always_inline)) {
        sink.leaf(o, d, best, tri, n0, n1, n2);
    });
}

// ------------------------------------------------------------------------------------
// persistent kernel: one wavefront per workgroup, one ray per lane, lanes refilled from the wavefront's chunk
// ------------------------------------------------------------------------------------
// persistent_walk's Q (pt_walk.h) of a listed ray: pt_crossings.hip::CountWalk with a leaf() that stores.  `best` never moves: every
// stacked entry is walked.
struct HitWalk : RayState {
    static constexpr bool kWaveHooks = false;
    const float4* __restrict__ rays; const unsigned long long* __restrict__ offsets;
    HlSink sink;

    __device__ __forceinline__ bool start(const RenderArgs& A, uint32_t item, bool scene_ok) {
        float tmax;
        load_ray(rays, item, o, d, tmax);
        best = wmin(tmax, kInfT); sink.count = 0u;
        if (!enter_root(A, scene_ok, ray_traced(o, d, tmax))) return false;
        sink.base = offsets[item];
        return true;
    }
    __device__ __forceinline__ bool leaf(uint32_t cur, const uint4 n0, const uint4 n1, const uint4 n2) {
        sink.leaf(o, d, best, (cur & 0x7fffffffu) >> 2, n0, n1, n2);
        return false;                                                     // no hit ends the ray
    }
};
__global__ __launch_bounds__(64) void hit_fill_kernel(const RenderArgs A, const float4* __restrict__ rays, const unsigned long long* __restrict__ offsets,
                                                      uint4* __restrict__ entries, unsigned long long capacity, uint32_t n,
                                                      unsigned long long* __restrict__ queue, unsigned long long* __restrict__ spill, uint32_t fill) {
    HitWalk q; q.rays = rays; q.offsets = offsets; q.sink.entries = entries; q.sink.capacity = capacity;
    persistent_walk<PT_HL_SHORT_STACK>(A, n, queue, spill, fill, q);
}

// ------------------------------------------------------------------------------------
// brute force: one ray per thread, every triangle in index order (pt_walk.h::brute_records)
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hit_fill_brute_kernel(const RenderArgs A, const float4* __restrict__ rays, const unsigned long long* __restrict__ offsets,
                                                             uint4* __restrict__ entries, unsigned long long capacity, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    F3 o = f3(0, 0, 0), d = o; float tmax = 0.0f;
    if (i < n) load_ray(rays, i, o, d, tmax);
    const bool walked = (i < n) && ray_traced(o, d, tmax);
    const float best = wmin(tmax, kInfT);
    HlSink sink{{entries, capacity}};
    if (walked) sink.base = offsets[i];
    brute_records(A, walked, [&](uint32_t tri, const uint4 n0, const uint4 n1, const uint4 n2) __attribute__((always_inline)) {
        sink.leaf(o, d, best, tri, n0, n1, n2);
    });
}

// ------------------------------------------------------------------------------------
// the sort: one wavefront per 64 consecutive lists, in place, no memory that grows with the total
// ------------------------------------------------------------------------------------
// The batches this is laid out for hold millions of lists of 0 .. 10 entries and a few of hundreds or thousands.  The lists of 64
// consecutive rays lie next to each other in `entries`, so a wavefront takes them together:
//   * a list of at most PT_HL_LANE_MAX entries is sorted by its own lane, by insertion, on global memory: visit order is near -> far at
//     every node, so such a list is nearly sorted and the insertion mostly reads (one compare per entry when it is sorted already);
//   * a longer list is sorted by the whole wavefront, one list after the other, with a bitonic network in its flip form (the first stage of
//     a merge compares i with its mirror image in the block, the others i with i + j): every compare-exchange moves the smaller key down,
//     so the entries behind the end of a list whose length is no power of two behave as +inf without being stored and an index check is
//     all they need.  A list of at most PT_HL_LDS_MAX entries is sorted in LDS between one coalesced read and one coalesced write; a
//     longer one on global memory, stage by stage.
// Only a list with offsets[i + 1] <= capacity is sorted: the one list that straddles the capacity stays in visit order.
// The key is (t bits << 32) | prim: every stored t is positive and finite, so bit order is value order.  Equal keys belong to one
// triangle held by two leaves, whose entries are identical, so the sort need not be stable.
__device__ __forceinline__ unsigned long long hl_key(const uint4 e) { return ((unsigned long long)e.x << 32) | e.y; }

template <class P>
__device__ __forceinline__ void hl_compare_exchange(P x, uint32_t i, uint32_t p) {
    const uint4 a = x[i], b = x[p];
    if (hl_key(b) < hl_key(a)) { x[i] = b; x[p] = a; }
}
// `len` entries at x, sorted by the 64 lanes of a one-wavefront workgroup; the barrier orders a stage's stores before the next stage's loads
// (LDS, or global memory within the workgroup).  Every entry belongs to exactly one pair of a stage.
template <class P>
__device__ __forceinline__ void hl_bitonic_flip(P x, uint32_t len, uint32_t lane) {
    for (uint32_t lk = 1; (1u << (lk - 1u)) < len; ++lk) {
        // flip: pair t of block b = t >> (lk - 1) is (b * k + r, b * k + k - 1 - r); i grows with t
        const uint32_t k = 1u << lk, half = k >> 1;
        for (uint32_t t = lane; ; t += 64u) {
            const uint32_t r = t & (half - 1u), b0 = (t >> (lk - 1u)) << lk, i = b0 + r, p = b0 + (k - 1u - r);
            if (i >= len) break;
            if (p < len) hl_compare_exchange(x, i, p);
        }
        __syncthreads();
        for (uint32_t lj = lk - 1u; lj-- > 0u; ) {
            // disperse: pair t is (i, i + j) with bit j of i clear
            const uint32_t j = 1u << lj;
            for (uint32_t t = lane; ; t += 64u) {
                const uint32_t i = ((t >> lj) << (lj + 1u)) + (t & (j - 1u)), p = i + j;
                if (i >= len) break;
                if (p < len) hl_compare_exchange(x, i, p);
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(64) void hit_sort_kernel(const unsigned long long* __restrict__ offsets, uint4* entries, unsigned long long capacity, uint32_t n) {
    __shared__ uint4 buf[PT_HL_LDS_MAX];
    const uint32_t lane = threadIdx.x;
    const unsigned long long i = (unsigned long long)blockIdx.x * 64u + lane;
    unsigned long long base = 0; uint32_t len = 0;
    if (i < n) {
        base = offsets[i];
        const unsigned long long end = offsets[i + 1];
        if (end <= capacity) len = (uint32_t)(end - base);            // a list holds at most 2^32 - 1 entries: a count
    }
    if (len >= 2u && len <= PT_HL_LANE_MAX) {
        uint4* x = entries + base;
        for (uint32_t j = 1; j < len; ++j) {
            const uint4 e = x[j];
            const unsigned long long ke = hl_key(e);
            uint32_t k = j;
            while (k > 0u) {
                const uint4 f = x[k - 1u];
                if (!(ke < hl_key(f))) break;
                x[k] = f; --k;
            }
            if (k != j) x[k] = e;
        }
    }
    unsigned long long m = __ballot(len > PT_HL_LANE_MAX);
    while (m != 0ull) {
        const int src = __builtin_ctzll(m);
        m &= m - 1ull;
        uint4* x = entries + __shfl(base, src, 64);
        const uint32_t l = (uint32_t)__shfl((int)len, src, 64);
        if (l <= PT_HL_LDS_MAX) {
            for (uint32_t k = lane; k < l; k += 64u) buf[k] = x[k];
            __syncthreads();
            hl_bitonic_flip(buf, l, lane);
            for (uint32_t k = lane; k < l; k += 64u) x[k] = buf[k];
            __syncthreads();                                          // buf is free for the next list
        } else {
            hl_bitonic_flip(x, l, lane);
        }
    }
}

hipError_t launch_hit_fill(const RenderArgs& A, const void* rays, uint32_t n, const unsigned long long* offsets, void* entries, unsigned long long capacity,
                           bool simple, bool brute, unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    const float4* r = (const float4*)rays; uint4* e = (uint4*)entries;
    const dim3 g256((n + 255u) / 256u);
    if (brute) {
        hit_fill_brute_kernel<<<g256, 256, 0, stream>>>(A, r, offsets, e, capacity, n);
        return hipGetLastError();
    }
    if (simple) {
        hit_fill_simple_kernel<<<g256, 256, 0, stream>>>(A, r, offsets, e, capacity, n);
        return hipGetLastError();
    }
    hipError_t err = walk_begin(queue, n, grid, stream);
    if (err != hipSuccess) return err;
    hit_fill_kernel<<<grid, 64, 0, stream>>>(A, r, offsets, e, capacity, n, queue, spill, PT_HL_FILL);
    return hipGetLastError();
}

hipError_t launch_hit_sort(const unsigned long long* offsets, void* entries, unsigned long long capacity, uint32_t n, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    hit_sort_kernel<<<dim3((uint32_t)(((unsigned long long)n + 63u) / 64u)), 64, 0, stream>>>(offsets, (uint4*)entries, capacity, n);
    return hipGetLastError();
}

} // namespace ptk
