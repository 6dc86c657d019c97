// pt_walk.h -- the one persistent walk of the batched queries.  A kernel fills a Q -- the per-lane state of one
// item and what differs between the queries -- and calls persistent_walk, which owns the chunk queue, the refill, the 64 B step, the
// child ordering, the stack with its cap and the end of the wavefront.  The Qs:
//   rays (they derive from pt_rays.h::RayState)   RayWalk<ANYHIT> (pt_rayquery.hip: trace_rays_kernel), OcclusionWalk (pt_occlusion.hip:
//                                                 occlusion_kernel), CountWalk and ContainsWalk (pt_crossings.hip: count_hits_kernel,
//                                                 contains_kernel), HitWalk (pt_hitlist.hip: hit_fill_kernel)
//   points (helpers in pt_points.h)               PointWalk (pt_pointquery.hip: closest_points_kernel), RadiusWalk<FILL> (pt_radius.hip:
//                                                 radius_kernel), NearestWalk (pt_knn.hip: nearest_k_kernel<KCAP>)
//   boxes                                         BoxWalk<FILL> (pt_overlap.hip: box_kernel)
// Also here, because the ray side and the point side both use them: brute_records, the LDS streaming loop of every brute-force kernel,
// and ListSink<FILL>, what a list query does with an accepted leaf.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_kernels.h"
#include "pt_device.h"

namespace ptk {

constexpr uint32_t kWalkChunk = 64;             // items per queue claim: one per lane of the claiming wavefront
constexpr uint32_t kWalkXcds = 8;               // chunk ranges with a queue counter each (MI355X: 8 XCDs)
constexpr uint32_t kWalkQueueStride = 32;       // counters 256 bytes apart
static_assert(kRqQueueWords == kWalkXcds * kWalkQueueStride, "pt_kernels.h: the queue block holds one counter line per range");

// One wavefront per workgroup, one item (a ray, a point, a sample ray) per lane, lanes refilled from the wavefront's chunk.
// A step is the unified 64 B arena fetch (pt_device.h::arena_record: four child pieces of a wide node, or a triangle record) followed by
// Q's test of the four children (pass and key: tmin of the sign-selected slab test, or bound2 of a point; empty and degenerate slots hold
// the inverted box and fail by themselves) or Q's leaf test.  The stack is (key bits << 32 | reference): entries 0 .. SHORT-1 in LDS, one
// column per lane (bank-conflict free), deeper entries in the spill area at [entry - SHORT][grid lane].  The tree is walked exactly as
// render_rays_kernel walks it (pt_device.h::traverse): visit order and first-minimum ties of order_children, pushes far -> near, the
// silent drop at kStackMax entries, re-validation at pop against Q's bound().
// When at least `fill` lanes are idle (or every lane is), the idle lanes take the next items of the wavefront's chunk, in lane order;
// a chunk of 64 items is claimed with one atomic, one chunk ahead, from the range of the wavefront's XCD.  The wavefront ends when every
// range is used up and no lane traverses.
//
// Q supplies:
//   bool  start(A, item, scene_ok)    load item, set the lane's state; true: the item enters the root, false: it has ended (its result written)
//   bool  child(w0, w1, w2, key)      the test of one child piece: whether it is visited, and the key it is ordered and stacked by
//   bool  leaf(cur, n0, n1, n2)       the test of the triangle record of leaf reference `cur`; true: the item has ended
//   float bound()                     what a stacked key is re-validated against
//   void  finish(A)                   the item has ended after entering the root: write its result
//   kKeyInit                          order_children's tn0 (pt_device.h): a constant that is never compared
//   kWaveHooks, after_refill(lane), after_step(done, lane)
//                                     kWaveHooks: every lane of the wavefront (idle ones too) calls after_refill behind each hand-out of
//                                     items and after_step(the lane's item ended in this step) behind each step; without it the hooks are
//                                     never called and a wavefront's idle lanes skip the step.
template <int SHORT, class Q>
__device__ __forceinline__ void persistent_walk(const RenderArgs& A, uint32_t n, unsigned long long* __restrict__ queue,
                                                unsigned long long* __restrict__ spill, uint32_t fill, Q& q) {
    __shared__ unsigned long long lds_stack[SHORT][64];
    const uint32_t lane = threadIdx.x;
    unsigned long long* const stk = &lds_stack[0][lane];
    const size_t grid_lanes = (size_t)gridDim.x * 64u, my_lane = (size_t)blockIdx.x * 64u + lane;
    const bool scene_ok = !(A.root_ref == kInvalidRef || A.num_tris == 0u || A.root_degenerate != 0u);

    // wave-uniform: the unhanded items [next, end) of the current chunk.  The chunks are split into kWalkXcds contiguous ranges with a
    // counter each (on its own 256-byte line): a wavefront claims from the range of the XCD it runs on (HW_REG_XCC_ID) and moves on to the
    // next range when that one is used up -- one counter for the whole grid serialises the claims (device-scope atomics on one address,
    // about 20 ns each, measured as a ceiling of ~3.2 G rays/s whatever the rays did).  The next chunk is claimed when a chunk is taken, so
    // that the atomic's round trip overlaps the chunk's work.
    const uint32_t chunks = (uint32_t)(((unsigned long long)n + kWalkChunk - 1u) / kWalkChunk), per_xcd = (chunks + kWalkXcds - 1u) / kWalkXcds;
    uint32_t xcd = (uint32_t)__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & (kWalkXcds - 1u), hops = 0;
    unsigned long long ahead = 0;                         // lane 0: the claimed next chunk of range `xcd` (read where it is used)
    if (lane == 0u) ahead = atomicAdd(&queue[xcd * kWalkQueueStride], 1ull);
    uint32_t next = 0, end = 0; bool dry = false;
    bool trav = false;                                    // this lane walks an item
    uint32_t cur = 0; int sp = 0;

    for (;;) {
        unsigned long long idle = __ballot(!trav);
        if (idle == ~0ull || (uint32_t)__popcll(idle) >= fill) {
            while (idle != 0ull && !dry) {
                if (next == end) {
                    unsigned long long c = __shfl(ahead, 0, 64);
                    auto used_up = [&](uint32_t x, unsigned long long k) __attribute__((always_inline)) {
                        return (unsigned long long)x * per_xcd + k >= min((x + 1u) * per_xcd, chunks);
                    };
                    while (used_up(xcd, c)) {
                        if (++hops >= kWalkXcds) { dry = true; break; }
                        xcd = (xcd + 1u) & (kWalkXcds - 1u);
                        // a plain read first: a range that is used up costs no claim (every wavefront looks at every range once at the end)
                        unsigned long long seen = 0;
                        if (lane == 0u) seen = __hip_atomic_load(&queue[xcd * kWalkQueueStride], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        c = __shfl(seen, 0, 64);
                        if (used_up(xcd, c)) continue;
                        if (lane == 0u) ahead = atomicAdd(&queue[xcd * kWalkQueueStride], 1ull);
                        c = __shfl(ahead, 0, 64);
                    }
                    if (dry) break;
                    if (lane == 0u) ahead = atomicAdd(&queue[xcd * kWalkQueueStride], 1ull);
                    const uint32_t chunk = xcd * per_xcd + (uint32_t)c;
                    next = chunk * kWalkChunk; end = (uint32_t)min((unsigned long long)next + kWalkChunk, (unsigned long long)n);
                }
                const uint32_t take = min((uint32_t)__popcll(idle), end - next);
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
                if (!trav && rank < take) {
                    sp = 0;
                    if (q.start(A, next + rank, scene_ok)) { cur = A.root_ref; trav = true; }
                }
                if (Q::kWaveHooks) q.after_refill(lane);
                next += take;
                idle = __ballot(!trav);
            }
            if (idle == ~0ull) break;                     // the queue is dry and nothing traverses
        }
        if (!Q::kWaveHooks && !trav) continue;
        bool done = false;
        if (trav) {
            const uint4* np = arena_record(A, cur);
            const uint4 n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3];
            bool need_pop = true;
            if (cur & kLeaf) {
                done = q.leaf(cur, n0, n1, n2);
            } else {
                // child-major record (pt_host.h::WideNode): piece k = child k's box words + its reference
                float t0, t1, t2, t3;
                const bool h0 = q.child(n0.x, n0.y, n0.z, t0), h1 = q.child(n1.x, n1.y, n1.z, t1);
                const bool h2 = q.child(n2.x, n2.y, n2.z, t2), h3 = q.child(n3.x, n3.y, n3.z, t3);
                uint32_t enter;
                const bool go = order_children(h0, h1, h2, h3, t0, t1, t2, t3, n0.w, n1.w, n2.w, n3.w, Q::kKeyInit, sp, enter, [&](int at, uint32_t ref, float key) __attribute__((always_inline)) {
                    const unsigned long long e = ((unsigned long long)__float_as_uint(key) << 32) | ref;
                    if (__builtin_expect(at < SHORT, 1)) stk[at * 64] = e;
                    else spill[(size_t)(at - SHORT) * grid_lanes + my_lane] = e;
                });
                if (go) { cur = enter; need_pop = false; }
            }
            if (need_pop && !done) {
                // entries that the item no longer reaches (key >= bound) are skipped
                bool found = false;
                while (sp > 0) {
                    --sp;
                    const unsigned long long e = sp < SHORT ? stk[sp * 64] : spill[(size_t)(sp - SHORT) * grid_lanes + my_lane];
                    if (__uint_as_float((uint32_t)(e >> 32)) < q.bound()) { cur = (uint32_t)e; found = true; break; }
                }
                done = !found;
            }
            if (done) { q.finish(A); trav = false; }
        }
        if (Q::kWaveHooks) q.after_step(done, lane);
    }
}

// Brute force, rays and points alike: a 256-thread workgroup streams every triangle record through LDS, kBruteTile at a time, and each
// thread with `walked` set calls body(triangle, n0, n1, n2) on all of them in index order.  Every thread of the workgroup calls this (the
// barriers).  A walked thread tests every record: its cnt.tris is num_tris.
constexpr uint32_t kBruteTile = 256;
template <class Body>
__device__ __forceinline__ void brute_records(const RenderArgs& A, bool walked, Body body) {
    __shared__ uint4 rec[kBruteTile][3];
    const uint4* recs = (const uint4*)A.tris;
    for (uint32_t base = 0; base < A.num_tris; base += kBruteTile) {
        const uint32_t tile = min(kBruteTile, A.num_tris - base);
        __syncthreads();
        if (threadIdx.x < tile) {
            const uint4* tp = recs + (size_t)(base + threadIdx.x) * 4;
            rec[threadIdx.x][0] = tp[0]; rec[threadIdx.x][1] = tp[1]; rec[threadIdx.x][2] = tp[2];
        }
        __syncthreads();
        if (walked)
            for (uint32_t k = 0; k < tile; ++k) body(base + k, rec[k][0], rec[k][1], rec[k][2]);
    }
}

// What the kernels of a list query (radius search, box search, hit lists) do with an accepted leaf: count it, and with FILL store
// entry() -- one plain 16-byte vector store -- when its global index is below the capacity.  base + count is 64-bit: the total of a batch
// may pass 2^32.
template <bool FILL>
struct ListSink {
    uint4* __restrict__ entries; unsigned long long capacity;
    unsigned long long base = 0; uint32_t count = 0;
    template <class Entry>
    __device__ __forceinline__ void accept(Entry entry) {
        if (FILL) {
            const unsigned long long g = base + count;
            if (g < capacity) entries[g] = entry();
        }
        ++count;
    }
};

// the launch side: the queue block zeroed on `stream`, and `grid` clamped to the number of chunks -- more wavefronts would only find
// the queue dry
inline hipError_t walk_begin(unsigned long long* queue, uint32_t n, uint32_t& grid, hipStream_t stream) {
    grid = (uint32_t)min((unsigned long long)grid, ((unsigned long long)n + kWalkChunk - 1u) / kWalkChunk);
    return hipMemsetAsync(queue, 0, kRqQueueWords * sizeof(unsigned long long), stream);
}

} // namespace ptk
