// pt_rayquery.hip -- batched ray queries over the context's scene (include/mi355pt.h: pt_trace_rays, pt_camera_rays):
//   * trace_rays_kernel<ANYHIT>              the default: persistent wavefronts, one ray per lane, a lane whose ray has ended takes the
//                                            next ray of its wavefront's chunk (64 rays per queue claim)
//   * trace_rays_simple_kernel<ANYHIT,STATS> one ray per thread over the renderer's traverse() (pt_device.h): PT_TRACE_SIMPLE_KERNEL, PT_TRACE_STATS
//   * camera_rays_kernel                     the primary rays of PT_MODE_REFERENCE, written out as PtRay records
//
// Both trace kernels walk the tree exactly as render_rays_kernel does (visit order, first-minimum ties, pushes far -> near, the silent drop at
// 64 entries, re-validation at pop) with `best` starting at min(t_max, kInfT), so with t_max = +inf a result is the oracle's orc_trace_ray, bit for bit.
// Records: PtRay = two float4 (org.xyz, t_max | dir.xyz, reserved), PtHit = one uint4 (t bits, prim, u bits, v bits).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_kernels.h"
#include "pt_device.h"

namespace ptk {

constexpr int kRqShort = PT_RQ_SHORT_STACK;     // LDS stack entries per lane; entries from this depth on live in the spill area
constexpr uint32_t kRqChunk = 64;               // rays per queue claim: one per lane of the claiming wavefront
constexpr uint32_t kRqXcds = 8;                 // chunk ranges with a queue counter each (MI355X: 8 XCDs)
constexpr uint32_t kRqQueueStride = 32;         // counters 256 bytes apart

__device__ __forceinline__ void load_ray(const float4* __restrict__ rays, uint32_t i, F3& o, F3& d, float& tmax) {
    const float4 a = rays[(size_t)i * 2], b = rays[(size_t)i * 2 + 1];
    o = f3(a.x, a.y, a.z); tmax = a.w; d = f3(b.x, b.y, b.z);
}
// a ray with a NaN anywhere, or with t_max <= 0, is a miss and is not traversed (a NaN t_max fails the comparison as well)
__device__ __forceinline__ bool ray_traced(F3 o, F3 d, float tmax) {
    const bool nan = __builtin_isnan(o.x) | __builtin_isnan(o.y) | __builtin_isnan(o.z) | __builtin_isnan(d.x) | __builtin_isnan(d.y) | __builtin_isnan(d.z);
    return !nan & (tmax > 0.0f);
}
// The 16-byte result.  u, v are recomputed from the winning triangle's record with the arithmetic of the accepted test
// (renderer.wgsl:185-205, pt_device.h::traverse): the same operations on the same operands, so the same bits, and the traversal
// step keeps no registers for them.
__device__ __forceinline__ uint4 hit_record(const RenderArgs& A, F3 o, F3 d, float t, uint32_t tri) {
    if (tri == kInvalidRef) return make_uint4(0x7F800000u, kInvalidRef, 0u, 0u);      // +inf, no triangle, u = v = 0
    const float4* tp = A.tris + (size_t)tri * 4;
    const float4 a = tp[0], b = tp[1], c = tp[2];
    const F3 v0 = f3(a.x, b.x, c.x), e1 = f3(a.y, b.y, c.y), e2 = f3(a.z, b.z, c.z);   // axis-major record (pt_host.h::TriRecord)
    const F3 p = cross3(d, e2);
    const float det = dot3(e1, p);
    const float inv_det = 1.0f / det;
    const F3 s = o - v0;
    const float u = inv_det * dot3(s, p);
    const F3 q = cross3(s, e1);
    const float v = inv_det * dot3(d, q);
    return make_uint4(__float_as_uint(t), tri, __float_as_uint(u), __float_as_uint(v));
}

// ------------------------------------------------------------------------------------
// simple kernel: one ray per thread, the renderer's traversal with its 64-entry private stack
// ------------------------------------------------------------------------------------
template <bool ANYHIT, bool STATS>
__global__ __launch_bounds__(256) void trace_rays_simple_kernel(const RenderArgs A, const float4* __restrict__ rays, uint4* __restrict__ hits, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    Counters cnt; cnt.nodes = cnt.tris = cnt.drops = cnt.maxstack = 0;
    uint32_t n_rays = 0;
    if (i < n) {
        F3 o, d; float tmax;
        load_ray(rays, i, o, d, tmax);
        float t = __uint_as_float(0x7F800000u); uint32_t tri = kInvalidRef;
        n_rays = 1;
        if (ray_traced(o, d, tmax)) {
            Ray r; r.o = o; r.d = d; r.inv = safe_inv(d);
            uint2 stk[kStackMax];
            float bt; uint32_t bi;
            if (traverse<ANYHIT, STATS>(A, r, bt, bi, stk, cnt, wmin(tmax, kInfT))) { t = bt; tri = bi; }
        }
        hits[i] = hit_record(A, o, d, t, tri);
    }
    if (STATS) {      // the oracle's counters (PtStats order), summed over the wavefront first: one atomic per counter and wavefront
        uint32_t nodes = cnt.nodes, tris = cnt.tris, drops = cnt.drops, maxstack = cnt.maxstack;
        for (int off = 32; off > 0; off >>= 1) {
            n_rays += __shfl_xor(n_rays, off, 64); nodes += __shfl_xor(nodes, off, 64); tris += __shfl_xor(tris, off, 64);
            drops += __shfl_xor(drops, off, 64); maxstack = max(maxstack, (uint32_t)__shfl_xor(maxstack, off, 64));
        }
        if ((threadIdx.x & 63u) == 0u) {
            atomicAdd(&A.stats[ANYHIT ? 1 : 0], (unsigned long long)n_rays);
            atomicAdd(&A.stats[2], (unsigned long long)nodes);
            atomicAdd(&A.stats[3], (unsigned long long)tris);
            atomicAdd(&A.stats[4], (unsigned long long)drops);
            atomicMax(&A.stats[5], (unsigned long long)maxstack);
        }
    }
}

// ------------------------------------------------------------------------------------
// persistent kernel: one wavefront per workgroup, one ray per lane, lanes refilled from the wavefront's chunk
// ------------------------------------------------------------------------------------
// A step is the unified 64 B arena fetch (pt_device.h::arena_record: four child pieces of a wide node, or a triangle record) followed by
// the box tests of the four children (sign-selected slab, pt_device.h::slab_sel; empty and degenerate slots hold the inverted box and fail
// by themselves) or a branch-free Moller-Trumbore.  The stack is (tmin bits << 32 | reference): entries 0 .. kRqShort-1 in LDS, one
// column per lane (bank-conflict free), deeper entries in the spill area at [entry - kRqShort][grid lane].
// When at least `fill` lanes are idle (or every lane is), the idle lanes take the next rays of the wavefront's chunk, in lane order;
// a chunk of 64 rays is claimed with one atomic, one chunk ahead, from the range of the wavefront's XCD.  The wavefront ends when every
// range is used up and no lane traverses.
template <bool ANYHIT>
__global__ __launch_bounds__(64) void trace_rays_kernel(const RenderArgs A, const float4* __restrict__ rays, uint4* __restrict__ hits, uint32_t n,
                                                        unsigned long long* __restrict__ queue, unsigned long long* __restrict__ spill, uint32_t fill) {
    __shared__ unsigned long long lds_stack[kRqShort][64];
    const uint32_t lane = threadIdx.x;
    unsigned long long* const stk = &lds_stack[0][lane];
    const size_t grid_lanes = (size_t)gridDim.x * 64u, my_lane = (size_t)blockIdx.x * 64u + lane;
    const bool scene_ok = !(A.root_ref == kInvalidRef || A.num_tris == 0u || A.root_degenerate != 0u);

    // wave-uniform: the unhanded rays [next, end) of the current chunk.  The chunks are split into kRqXcds contiguous ranges with a counter
    // each (on its own 256-byte line): a wavefront claims from the range of the XCD it runs on (HW_REG_XCC_ID) and moves on to the next
    // range when that one is used up -- one counter for the whole grid serialises the claims (device-scope atomics on one address, about
    // 20 ns each, measured as a ceiling of ~3.2 G rays/s whatever the rays did).  The next chunk is claimed when a chunk is taken, so that
    // the atomic's round trip overlaps the chunk's work.
    const uint32_t chunks = (uint32_t)(((unsigned long long)n + kRqChunk - 1u) / kRqChunk), per_xcd = (chunks + kRqXcds - 1u) / kRqXcds;
    uint32_t xcd = (uint32_t)__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & (kRqXcds - 1u), hops = 0;
    unsigned long long ahead = 0;                         // lane 0: the claimed next chunk of range `xcd` (read where it is used)
    if (lane == 0u) ahead = atomicAdd(&queue[xcd * kRqQueueStride], 1ull);
    uint32_t next = 0, end = 0; bool dry = false;
    bool trav = false;                                    // this lane traverses a ray
    uint32_t rid = 0, cur = 0, btri = kInvalidRef; int sp = 0; float best = 0.0f;
    F3 o = f3(0, 0, 0), d = o, inv = o; RaySel sel = ray_selectors(inv);

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
                        if (++hops >= kRqXcds) { dry = true; break; }
                        xcd = (xcd + 1u) & (kRqXcds - 1u);
                        // a plain read first: a range that is used up costs no claim (every wavefront looks at every range once at the end)
                        unsigned long long seen = 0;
                        if (lane == 0u) seen = __hip_atomic_load(&queue[xcd * kRqQueueStride], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        c = __shfl(seen, 0, 64);
                        if (used_up(xcd, c)) continue;
                        if (lane == 0u) ahead = atomicAdd(&queue[xcd * kRqQueueStride], 1ull);
                        c = __shfl(ahead, 0, 64);
                    }
                    if (dry) break;
                    if (lane == 0u) ahead = atomicAdd(&queue[xcd * kRqQueueStride], 1ull);
                    const uint32_t chunk = xcd * per_xcd + (uint32_t)c;
                    next = chunk * kRqChunk; end = (uint32_t)min((unsigned long long)next + kRqChunk, (unsigned long long)n);
                }
                const uint32_t take = min((uint32_t)__popcll(idle), end - next);
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
                if (!trav && rank < take) {
                    rid = next + rank;
                    float tmax;
                    load_ray(rays, rid, o, d, tmax);
                    best = wmin(tmax, kInfT); btri = kInvalidRef; sp = 0;
                    inv = safe_inv(d); sel = ray_selectors(inv);
                    Ray r; r.o = o; r.d = d; r.inv = inv;
                    float troot;
                    if (scene_ok && ray_traced(o, d, tmax) && slab(r, A.root_box[0], A.root_box[1], A.root_box[2], best, troot)) { cur = A.root_ref; trav = true; }
                    else hits[rid] = hit_record(A, o, d, 0.0f, kInvalidRef);
                }
                next += take;
                idle = __ballot(!trav);
            }
            if (idle == ~0ull) break;                     // the queue is dry and nothing traverses
        }
        if (!trav) continue;
        const uint4* np = arena_record(A, cur);
        const uint4 n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3];
        bool need_pop = true, done = false;
        if (cur & kLeaf) {
            // branch-free Moller-Trumbore (renderer.wgsl:185-205): the operations and comparisons of traverse(), rejections combined at
            // the end.  A leaf whose triangle index is out of range points at the all-zero record behind the last triangle: |det| < eps.
            const F3 v0 = f3(__uint_as_float(n0.x), __uint_as_float(n1.x), __uint_as_float(n2.x));
            const F3 e1 = f3(__uint_as_float(n0.y), __uint_as_float(n1.y), __uint_as_float(n2.y));
            const F3 e2 = f3(__uint_as_float(n0.z), __uint_as_float(n1.z), __uint_as_float(n2.z));
            const F3 pv = cross3(d, e2);
            const float det = dot3(e1, pv);
            const bool ok_det = !(fabsf(det) < kTriEps);
            const float inv_det = 1.0f / det;
            const F3 sv = o - v0;
            const float u = inv_det * dot3(sv, pv);
            const bool ok_u = !((u < 0.0f) | (u > 1.0f));
            const F3 q = cross3(sv, e1);
            const float v = inv_det * dot3(d, q);
            const bool ok_v = !((v < 0.0f) | ((u + v) > 1.0f));
            const float t = inv_det * dot3(e2, q);
            if (ok_det & ok_u & ok_v & (t > kTriEps) & (t < best)) {
                best = t; btri = cur;
                if (ANYHIT) done = true;
            }
        } else {
            // child-major record (pt_host.h::WideNode): piece k = child k's box words + its reference
            const uint32_t r0 = n0.w, r1 = n1.w, r2 = n2.w, r3 = n3.w;
            float t0, t1, t2, t3;
            const bool h0 = lane_of(slab_sel(o, inv, sel, n0.x, n0.y, n0.z, best, t0));
            const bool h1 = lane_of(slab_sel(o, inv, sel, n1.x, n1.y, n1.z, best, t1));
            const bool h2 = lane_of(slab_sel(o, inv, sel, n2.x, n2.y, n2.z, best, t2));
            const bool h3 = lane_of(slab_sel(o, inv, sel, n3.x, n3.y, n3.z, best, t3));
            // nearest = first minimum in slot order (renderer.wgsl:315-318); first = first hit -- as traverse()
            int nslot = -1, fslot = -1; float tn = kInfT, tf = 0.0f; uint32_t rn = kInvalidRef, rf = kInvalidRef;
            if (h0) { nslot = 0; tn = t0; rn = r0; fslot = 0; tf = t0; rf = r0; }
            if (h1) { if (nslot < 0 || t1 < tn) { nslot = 1; tn = t1; rn = r1; } if (fslot < 0) { fslot = 1; tf = t1; rf = r1; } }
            if (h2) { if (nslot < 0 || t2 < tn) { nslot = 2; tn = t2; rn = r2; } if (fslot < 0) { fslot = 2; tf = t2; rf = r2; } }
            if (h3) { if (nslot < 0 || t3 < tn) { nslot = 3; tn = t3; rn = r3; } if (fslot < 0) { fslot = 3; tf = t3; rf = r3; } }
            if (nslot >= 0) {
                // pushes far -> near (renderer.wgsl:336-342); the slot the nearest child left holds the first hit; a push at 64 entries is dropped
                auto push = [&](uint32_t ref, float tmin) __attribute__((always_inline)) {
                    if (sp < kStackMax) {
                        const unsigned long long e = ((unsigned long long)__float_as_uint(tmin) << 32) | ref;
                        if (__builtin_expect(sp < kRqShort, 1)) stk[sp * 64] = e;
                        else spill[(size_t)(sp - kRqShort) * grid_lanes + my_lane] = e;
                        ++sp;
                    }
                };
                if (h3) { if (nslot == 3) { if (fslot != 3) push(rf, tf); } else if (fslot != 3) push(r3, t3); }
                if (h2) { if (nslot == 2) { if (fslot != 2) push(rf, tf); } else if (fslot != 2) push(r2, t2); }
                if (h1) { if (nslot == 1) { if (fslot != 1) push(rf, tf); } else if (fslot != 1) push(r1, t1); }
                if (sp < kStackMax) { cur = rn; need_pop = false; }       // the push of the nearest child would have fitted
            }
        }
        if (need_pop && !done) {
            // entries whose box the ray no longer reaches (tmin >= best) are skipped
            bool found = false;
            while (sp > 0) {
                --sp;
                const unsigned long long e = sp < kRqShort ? stk[sp * 64] : spill[(size_t)(sp - kRqShort) * grid_lanes + my_lane];
                if (__uint_as_float((uint32_t)(e >> 32)) < best) { cur = (uint32_t)e; found = true; break; }
            }
            done = !found;
        }
        if (done) {
            hits[rid] = hit_record(A, o, d, best, btri == kInvalidRef ? kInvalidRef : (btri & 0x7fffffffu) >> 2);
            trav = false;
        }
    }
}

// the camera rays of PT_MODE_REFERENCE: one through each pixel centre (renderer.wgsl:387-395), row-major, t_max = +inf
__global__ __launch_bounds__(256) void camera_rays_kernel(const RenderArgs A, float4* __restrict__ rays) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.width * A.height) return;
    const uint32_t px = i % A.width, py = i / A.width;
    const Ray r = primary_ray(A, (float)px + 0.5f, (float)py + 0.5f);
    rays[(size_t)i * 2] = make_float4(r.o.x, r.o.y, r.o.z, __uint_as_float(0x7F800000u));
    rays[(size_t)i * 2 + 1] = make_float4(r.d.x, r.d.y, r.d.z, 0.0f);
}

static_assert(kRqQueueWords == kRqXcds * kRqQueueStride, "pt_kernels.h: the queue block holds one counter line per range");
uint32_t rayquery_grid(int num_cus) { return (uint32_t)num_cus * 4u * PT_RQ_WAVES_PER_SIMD; }
size_t rayquery_spill_entries(uint32_t grid) { return (size_t)(kStackMax - kRqShort) * grid * 64u; }

hipError_t launch_trace_rays(const RenderArgs& A, const void* rays, void* hits, uint32_t n, bool anyhit, bool simple, bool stats,
                             unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    const float4* r = (const float4*)rays; uint4* h = (uint4*)hits;
    if (simple || stats) {
        const dim3 g((n + 255u) / 256u);
        if (stats) {
            if (anyhit) trace_rays_simple_kernel<true, true><<<g, 256, 0, stream>>>(A, r, h, n);
            else trace_rays_simple_kernel<false, true><<<g, 256, 0, stream>>>(A, r, h, n);
        } else {
            if (anyhit) trace_rays_simple_kernel<true, false><<<g, 256, 0, stream>>>(A, r, h, n);
            else trace_rays_simple_kernel<false, false><<<g, 256, 0, stream>>>(A, r, h, n);
        }
        return hipGetLastError();
    }
    hipError_t e = hipMemsetAsync(queue, 0, kRqQueueWords * sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    // no more wavefronts than there are chunks: the rest would only find the queue dry
    const uint32_t g = (uint32_t)min((unsigned long long)grid, ((unsigned long long)n + kRqChunk - 1u) / kRqChunk);
    if (anyhit) trace_rays_kernel<true><<<g, 64, 0, stream>>>(A, r, h, n, queue, spill, PT_RQ_FILL);
    else trace_rays_kernel<false><<<g, 64, 0, stream>>>(A, r, h, n, queue, spill, PT_RQ_FILL);
    return hipGetLastError();
}

hipError_t launch_camera_rays(const RenderArgs& A, void* rays, hipStream_t stream) {
    const uint32_t n = A.width * A.height;
    camera_rays_kernel<<<dim3((n + 255u) / 256u), 256, 0, stream>>>(A, (float4*)rays);
    return hipGetLastError();
}

} // namespace ptk
