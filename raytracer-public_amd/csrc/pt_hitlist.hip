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
// An entry is (t of the accepted tri_hit, triangle, u, v by the arithmetic of pt_rayquery.hip::hit_record on the same record).
// Records: PtRay = two float4 (org.xyz, t_max | dir.xyz, reserved), an entry = PtHit = one uint4 (t bits, prim, u bits, v bits).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_kernels.h"
#include "pt_device.h"
#include "pt_walk.h"

namespace ptk {

// pt_crossings.hip::cr_load_ray and cr_ray_walked, restated: the same instructions on the same operands
__device__ __forceinline__ void hl_load_ray(const float4* __restrict__ rays, uint32_t i, F3& o, F3& d, float& tmax) {
    const float4 a = rays[(size_t)i * 2], b = rays[(size_t)i * 2 + 1];
    o = f3(a.x, a.y, a.z); tmax = a.w; d = f3(b.x, b.y, b.z);
}
__device__ __forceinline__ bool hl_ray_walked(F3 o, F3 d, float tmax) {
    const bool nan = __builtin_isnan(o.x) | __builtin_isnan(o.y) | __builtin_isnan(o.z) | __builtin_isnan(d.x) | __builtin_isnan(d.y) | __builtin_isnan(d.z);
    return !nan & (tmax > 0.0f);
}
// pt_rayquery.hip::hit_record on a fetched triangle record (three axis-major pieces: v0[a], e1[a], e2[a]): the operations of the accepted
// test, so the bits pt_trace_rays gives if this triangle is the only one
__device__ __forceinline__ uint4 hl_entry(F3 o, F3 d, float t, uint32_t tri, const uint4 n0, const uint4 n1, const uint4 n2) {
    const F3 v0 = f3(__uint_as_float(n0.x), __uint_as_float(n1.x), __uint_as_float(n2.x));
    const F3 e1 = f3(__uint_as_float(n0.y), __uint_as_float(n1.y), __uint_as_float(n2.y));
    const F3 e2 = f3(__uint_as_float(n0.z), __uint_as_float(n1.z), __uint_as_float(n2.z));
    const F3 p = cross3(d, e2);
    const float det = dot3(e1, p);
    const float inv_det = 1.0f / det;
    const F3 s = o - v0;
    const float u = inv_det * dot3(s, p);
    const F3 q = cross3(s, e1);
    const float v = inv_det * dot3(d, q);
    return make_uint4(__float_as_uint(t), tri, __float_as_uint(u), __float_as_uint(v));
}

// What the three kernels do with a crossing: store its entry when its global index is below the capacity.  base + count is 64-bit: the
// total of a batch may pass 2^32.
struct HlSink {
    uint4* __restrict__ entries; unsigned long long capacity;
    unsigned long long base = 0; uint32_t count = 0;
    __device__ __forceinline__ void leaf(F3 o, F3 d, float best, uint32_t tri, const uint4 n0, const uint4 n1, const uint4 n2) {
        float t;
        if (tri_hit(o, d, n0, n1, n2, t) & (t < best)) {
            const unsigned long long g = base + count;
            if (g < capacity) entries[g] = hl_entry(o, d, t, tri, n0, n1, n2);
            ++count;
        }
    }
};

// ------------------------------------------------------------------------------------
// one ray per thread: pt_crossings.hip::count_traverse with a store in place of the count (the same visit order and cap)
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void hl_fill_traverse(const RenderArgs& A, const Ray& r, uint2* __restrict__ stk, float best, HlSink& sink) {
    if (A.root_ref == kInvalidRef || A.num_tris == 0u) return;
    if (A.root_degenerate) return;
    float troot;
    if (!slab(r, A.root_box[0], A.root_box[1], A.root_box[2], best, troot)) return;
    uint32_t cur = A.root_ref;
    int sp = 0;
    for (;;) {
        bool need_pop = false;
        if (cur & kLeaf) {
            const uint32_t ti4 = cur & 0x7fffffffu;
            if (ti4 < 4u * A.num_tris) {                          // an out-of-range leaf is skipped
                const uint4* tp = arena_record(A, cur);
                sink.leaf(r.o, r.d, best, ti4 >> 2, tp[0], tp[1], tp[2]);
            }
            need_pop = true;
        } else {
            const uint4* np = arena_record(A, cur);
            const uint4 n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3];
            float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f, t3 = 0.0f;
            const uint32_t r0 = n0.w, r1 = n1.w, r2 = n2.w, r3 = n3.w;
            const bool h0 = (r0 < kDegenerateRef) && slab(r, n0.x, n0.y, n0.z, best, t0);
            const bool h1 = (r1 < kDegenerateRef) && slab(r, n1.x, n1.y, n1.z, best, t1);
            const bool h2 = (r2 < kDegenerateRef) && slab(r, n2.x, n2.y, n2.z, best, t2);
            const bool h3 = (r3 < kDegenerateRef) && slab(r, n3.x, n3.y, n3.z, best, t3);
            uint32_t enter;
            const bool go = order_children(h0, h1, h2, h3, t0, t1, t2, t3, r0, r1, r2, r3, kInfT, sp, enter, [&](int at, uint32_t ref, float key) __attribute__((always_inline)) {
                stk[at] = make_uint2(ref, __float_as_uint(key));
            });
            if (go) cur = enter; else need_pop = true;
        }
        if (need_pop) {
            bool found = false;
            while (sp > 0) {
                --sp;
                const uint2 e = stk[sp];
                if (__uint_as_float(e.y) < best) { cur = e.x; found = true; break; }      // always passes: `best` never moves
            }
            if (!found) break;
        }
    }
}

__global__ __launch_bounds__(256) void hit_fill_simple_kernel(const RenderArgs A, const float4* __restrict__ rays, const unsigned long long* __restrict__ offsets,
                                                              uint4* __restrict__ entries, unsigned long long capacity, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    F3 o, d; float tmax;
    hl_load_ray(rays, i, o, d, tmax);
    if (!hl_ray_walked(o, d, tmax)) return;
    HlSink sink{entries, capacity};
    sink.base = offsets[i];
    Ray r; r.o = o; r.d = d; r.inv = safe_inv(d);
    uint2 stk[kStackMax];
    hl_fill_traverse(A, r, stk, wmin(tmax, kInfT), sink);
}

// ------------------------------------------------------------------------------------
// persistent kernel: one wavefront per workgroup, one ray per lane, lanes refilled from the wavefront's chunk
// ------------------------------------------------------------------------------------
// persistent_walk's Q (pt_walk.h) of a listed ray: pt_crossings.hip::CountWalk with a leaf() that stores.  A leaf whose triangle index is
// out of range points at the all-zero record behind the last triangle, which tri_hit rejects.
struct HitWalk {
    static constexpr bool kWaveHooks = false;
    static constexpr float kKeyInit = kInfT;      // pt_device.h::order_children
    const float4* __restrict__ rays; const unsigned long long* __restrict__ offsets;
    HlSink sink;
    float best = 0.0f;
    F3 o = f3(0, 0, 0), d = o, inv = o; RaySel sel = ray_selectors(inv);

    __device__ __forceinline__ bool start(const RenderArgs& A, uint32_t item, bool scene_ok) {
        float tmax;
        hl_load_ray(rays, item, o, d, tmax);
        best = wmin(tmax, kInfT); sink.count = 0u;
        inv = safe_inv(d); sel = ray_selectors(inv);
        Ray r; r.o = o; r.d = d; r.inv = inv;
        float troot;
        if (!(scene_ok && hl_ray_walked(o, d, tmax) && slab(r, A.root_box[0], A.root_box[1], A.root_box[2], best, troot))) return false;
        sink.base = offsets[item];
        return true;
    }
    __device__ __forceinline__ bool child(uint32_t w0, uint32_t w1, uint32_t w2, float& tmin) const { return lane_of(slab_sel(o, inv, sel, w0, w1, w2, best, tmin)); }
    __device__ __forceinline__ bool leaf(uint32_t cur, const uint4 n0, const uint4 n1, const uint4 n2) {
        sink.leaf(o, d, best, (cur & 0x7fffffffu) >> 2, n0, n1, n2);
        return false;                                                     // no hit ends the ray
    }
    __device__ __forceinline__ float bound() const { return best; }      // `best` never moves: every stacked entry is walked
    __device__ __forceinline__ void finish(const RenderArgs&) {}
    __device__ __forceinline__ void after_refill(uint32_t) {}
    __device__ __forceinline__ void after_step(bool, uint32_t) {}
};
__global__ __launch_bounds__(64) void hit_fill_kernel(const RenderArgs A, const float4* __restrict__ rays, const unsigned long long* __restrict__ offsets,
                                                      uint4* __restrict__ entries, unsigned long long capacity, uint32_t n,
                                                      unsigned long long* __restrict__ queue, unsigned long long* __restrict__ spill, uint32_t fill) {
    HitWalk q{rays, offsets, HlSink{entries, capacity}};
    persistent_walk<PT_HL_SHORT_STACK>(A, n, queue, spill, fill, q);
}

// ------------------------------------------------------------------------------------
// brute force: one ray per thread, every triangle in index order; a workgroup streams the records through LDS, kHlBruteTile at a time
// ------------------------------------------------------------------------------------
constexpr uint32_t kHlBruteTile = 256;
__global__ __launch_bounds__(256) void hit_fill_brute_kernel(const RenderArgs A, const float4* __restrict__ rays, const unsigned long long* __restrict__ offsets,
                                                             uint4* __restrict__ entries, unsigned long long capacity, uint32_t n) {
    __shared__ uint4 rec[kHlBruteTile][3];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    F3 o = f3(0, 0, 0), d = o; float tmax = 0.0f;
    if (i < n) hl_load_ray(rays, i, o, d, tmax);
    const bool walked = (i < n) && hl_ray_walked(o, d, tmax);
    const float best = wmin(tmax, kInfT);
    HlSink sink{entries, capacity};
    if (walked) sink.base = offsets[i];
    const uint4* recs = (const uint4*)A.tris;
    for (uint32_t base = 0; base < A.num_tris; base += kHlBruteTile) {
        const uint32_t tile = min(kHlBruteTile, A.num_tris - base);
        __syncthreads();
        if (threadIdx.x < tile) {
            const uint4* tp = recs + (size_t)(base + threadIdx.x) * 4;
            rec[threadIdx.x][0] = tp[0]; rec[threadIdx.x][1] = tp[1]; rec[threadIdx.x][2] = tp[2];
        }
        __syncthreads();
        if (walked)
            for (uint32_t k = 0; k < tile; ++k) sink.leaf(o, d, best, base + k, rec[k][0], rec[k][1], rec[k][2]);
    }
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
