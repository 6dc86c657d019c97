// pt_crossings.hip -- crossing counts, containment and the sign of the distance over the context's scene (include/mi355pt.h:
// pt_count_hits, pt_contains, pt_signed_distance):
//   * count_hits_kernel               the default: persistent wavefronts, one ray per lane; the walk never shrinks `best`, never ends at a
//                                     hit and counts every triangle record it reaches that the ray crosses
//   * contains_kernel                 the same walk over sample rays built in registers from the 16-byte point record; the odd counts of a
//                                     point are added to word 1 of its output record
//   * count_hits_simple_kernel<STATS>, contains_simple_kernel<STATS>
//                                     one ray per thread with a private 64-entry stack: PT_COUNT_SIMPLE_KERNEL / PT_COUNT_STATS,
//                                     PT_CONTAIN_SIMPLE_KERNEL / PT_CONTAIN_STATS
//   * count_hits_brute_kernel<STATS>  every triangle in index order, the records streamed through LDS: PT_COUNT_BRUTE_FORCE
//   * contains_finish_kernel          one thread per point: inside, samples and reserved around the counted `odd`
//   * apply_sign_kernel               one thread per point: the sign bit of PtClosest::dist from PtContainment::inside
//
// The walk is pt_walk.h::persistent_walk with the tests of pt_device.h, as in pt_rayquery.hip::trace_rays_kernel<true>: `best` is
// min(t_max, kInfT) in both and moves in neither, so the any-hit walk is a prefix of the counting walk and count >= 1 exactly when
// pt_trace_rays(PT_TRACE_ANY_HIT) reports a hit.  Sample ray s of point i is record i * samples + s of pt_occlusion_rays for the surfel
// {p, r_max = +inf, n = (0, 0, 1)} with bias 0: the functions of pt_occlusion.hip::sample_ray on the same operands, so the same bits.
// Records: PtRay = two float4 (org.xyz, t_max | dir.xyz, reserved), a count = one uint32_t, PtPoint = one float4 (p.xyz, r_max: ignored),
// PtContainment = one uint4 (inside, odd, samples, 0).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>

#include "pt_kernels.h"
#include "pt_device.h"
#include "pt_walk.h"

namespace ptk {

__device__ __forceinline__ void cr_load_ray(const float4* __restrict__ rays, uint32_t i, F3& o, F3& d, float& tmax) {
    const float4 a = rays[(size_t)i * 2], b = rays[(size_t)i * 2 + 1];
    o = f3(a.x, a.y, a.z); tmax = a.w; d = f3(b.x, b.y, b.z);
}
// pt_rayquery.hip::ray_traced: a ray with a NaN anywhere, or with t_max <= 0, is not walked (a NaN t_max fails the comparison as well)
__device__ __forceinline__ bool cr_ray_walked(F3 o, F3 d, float tmax) {
    const bool nan = __builtin_isnan(o.x) | __builtin_isnan(o.y) | __builtin_isnan(o.z) | __builtin_isnan(d.x) | __builtin_isnan(d.y) | __builtin_isnan(d.z);
    return !nan & (tmax > 0.0f);
}
// a point with a NaN in p is not traced (r_max is ignored)
__device__ __forceinline__ bool cr_point_traced(F3 p) { return !(__builtin_isnan(p.x) | __builtin_isnan(p.y) | __builtin_isnan(p.z)); }
// sample ray s of the point with sample index `pixel` = index_base + i (mod 2^32): pt_occlusion.hip::sample_ray for the normal (0, 0, 1)
// and bias 0, operation by operation (org = p + n * 0 turns a -0 into +0, as it does there)
__device__ __forceinline__ void cr_sample_ray(F3 p, uint32_t seed, uint32_t pixel, uint32_t s, F3& o, F3& d) {
    const F3 n = f3(0.0f, 0.0f, 1.0f);
    const uint32_t key = sample_key(seed, pixel, s);
    const float u1 = rnd(key, 0u, 2u), u2 = rnd(key, 0u, 3u);
    d = cosine_dir(n, u1, u2);
    o = p + n * 0.0f;
}
// The lanes of `odd` that hold the same point add their number to its counter with ONE atomic (the first of them issues it), the way
// pt_occlusion.hip::count_misses combines misses: the lanes of a chunk share a point.  Integer sums: any order gives the same bits.
__device__ __forceinline__ void count_odd(uint4* __restrict__ out, bool odd, uint32_t pid, uint32_t lane) {
    unsigned long long m = __ballot(odd);
    while (m != 0ull) {
        const int leader = __builtin_ctzll(m);
        const uint32_t p0 = (uint32_t)__shfl((int)pid, leader, 64);
        const unsigned long long same = __ballot(odd && pid == p0);
        if (lane == (uint32_t)leader) atomicAdd(&((uint32_t*)(out + p0))[1], (uint32_t)__popcll(same));
        m &= ~same;
    }
}

// ------------------------------------------------------------------------------------
// one ray per thread: pt_device.h::traverse with a count in place of the closest hit (the same visit order, cap and counters)
// ------------------------------------------------------------------------------------
template <bool STATS>
__device__ __forceinline__ uint32_t count_traverse(const RenderArgs& A, const Ray& r, uint2* __restrict__ stk, Counters& cnt, float best) {
    uint32_t count = 0;
    if (A.root_ref == kInvalidRef || A.num_tris == 0u) return 0u;
    if (STATS) { cnt.nodes += 1; if (cnt.maxstack < 1u) cnt.maxstack = 1u; }
    if (A.root_degenerate) return 0u;
    float troot;
    if (!slab(r, A.root_box[0], A.root_box[1], A.root_box[2], best, troot)) return 0u;
    uint32_t cur = A.root_ref;
    int sp = 0;
    for (;;) {
        bool need_pop = false;
        if (cur & kLeaf) {
            if ((cur & 0x7fffffffu) < 4u * A.num_tris) {          // an out-of-range leaf is skipped
                const uint4* tp = arena_record(A, cur);
                const uint4 n0 = tp[0], n1 = tp[1], n2 = tp[2];
                if (STATS) cnt.tris += 1;
                float t;
                if (tri_hit(r.o, r.d, n0, n1, n2, t) & (t < best)) ++count;
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
            if (STATS) cnt.nodes += (r0 != kInvalidRef) + (r1 != kInvalidRef) + (r2 != kInvalidRef) + (r3 != kInvalidRef);
            uint32_t enter;
            const int before = sp;
            const bool any = h0 | h1 | h2 | h3;
            const uint32_t wanted = (uint32_t)h0 + (uint32_t)h1 + (uint32_t)h2 + (uint32_t)h3;      // one entered, the others pushed
            const bool go = order_children(h0, h1, h2, h3, t0, t1, t2, t3, r0, r1, r2, r3, kInfT, sp, enter, [&](int at, uint32_t ref, float key) __attribute__((always_inline)) {
                stk[at] = make_uint2(ref, __float_as_uint(key));
            });
            if (STATS && any) {
                // pushes that did not fit, and the nearest child's own when the stack is full (pt_device.h::traverse)
                cnt.drops += (wanted - 1u) - (uint32_t)(sp - before) + (go ? 0u : 1u);
                const uint32_t depth = (uint32_t)sp + (go ? 1u : 0u);
                if (depth > cnt.maxstack) cnt.maxstack = depth;
            }
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
    return count;
}

template <bool STATS>
__global__ __launch_bounds__(256) void count_hits_simple_kernel(const RenderArgs A, const float4* __restrict__ rays, uint32_t* __restrict__ counts, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    Counters cnt; cnt.nodes = cnt.tris = cnt.drops = cnt.maxstack = 0;
    if (i < n) {
        F3 o, d; float tmax;
        cr_load_ray(rays, i, o, d, tmax);
        uint32_t count = 0;
        if (cr_ray_walked(o, d, tmax)) {
            Ray r; r.o = o; r.d = d; r.inv = safe_inv(d);
            uint2 stk[kStackMax];
            count = count_traverse<STATS>(A, r, stk, cnt, wmin(tmax, kInfT));
        }
        counts[i] = count;
    }
    if (STATS) add_stats(A, 0, i < n ? 1u : 0u, cnt);
}

template <bool STATS>
__global__ __launch_bounds__(256) void contains_simple_kernel(const RenderArgs A, const float4* __restrict__ points, uint4* __restrict__ out, uint32_t items,
                                                              uint32_t samples, uint32_t samples_magic, uint32_t seed, uint32_t index_base) {
    const unsigned long long gi = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    Counters cnt; cnt.nodes = cnt.tris = cnt.drops = cnt.maxstack = 0;
    uint32_t n_rays = 0, pid = 0;
    bool odd = false;
    if (gi < items) {
        uint32_t s; divmod_magic((uint32_t)gi, samples, samples_magic, pid, s);
        const float4 pt = points[pid];
        const F3 p = f3(pt.x, pt.y, pt.z);
        if (cr_point_traced(p)) {
            F3 o, d; cr_sample_ray(p, seed, index_base + pid, s, o, d);
            n_rays = 1;
            if (cr_ray_walked(o, d, kInfT)) {
                Ray r; r.o = o; r.d = d; r.inv = safe_inv(d);
                uint2 stk[kStackMax];
                odd = (count_traverse<STATS>(A, r, stk, cnt, kInfT) & 1u) != 0u;
            }
        }
    }
    count_odd(out, odd, pid, threadIdx.x & 63u);
    if (STATS) add_stats(A, 0, n_rays, cnt);
}

// ------------------------------------------------------------------------------------
// persistent kernels: one wavefront per workgroup, one ray per lane, lanes refilled from the wavefront's chunk
// ------------------------------------------------------------------------------------
// What persistent_walk's Q (pt_walk.h) of a counted ray holds whichever record the ray comes from: RayWalk<true> of pt_rayquery.hip with
// a counter in place of the hit, and a leaf test that never ends the ray.  A leaf whose triangle index is out of range points at the
// all-zero record behind the last triangle, which tri_hit rejects.
struct CrossState {
    static constexpr float kKeyInit = kInfT;      // pt_device.h::order_children
    uint32_t count = 0; float best = 0.0f;
    F3 o = f3(0, 0, 0), d = o, inv = o; RaySel sel = ray_selectors(inv);

    // the ray is set: whether it enters the root
    __device__ __forceinline__ bool enter_root(const RenderArgs& A, bool scene_ok, bool walked) {
        count = 0u;
        inv = safe_inv(d); sel = ray_selectors(inv);
        Ray r; r.o = o; r.d = d; r.inv = inv;
        float troot;
        return scene_ok && walked && slab(r, A.root_box[0], A.root_box[1], A.root_box[2], best, troot);
    }
    __device__ __forceinline__ bool child(uint32_t w0, uint32_t w1, uint32_t w2, float& tmin) const { return lane_of(slab_sel(o, inv, sel, w0, w1, w2, best, tmin)); }
    __device__ __forceinline__ bool leaf(uint32_t, const uint4 n0, const uint4 n1, const uint4 n2) {
        float t;
        if (tri_hit(o, d, n0, n1, n2, t) & (t < best)) ++count;
        return false;                                                     // no hit ends the ray
    }
    __device__ __forceinline__ float bound() const { return best; }      // `best` never moves: every stacked entry is walked
};

struct CountWalk : CrossState {
    static constexpr bool kWaveHooks = false;
    const float4* __restrict__ rays; uint32_t* __restrict__ counts;
    uint32_t rid = 0;

    __device__ __forceinline__ bool start(const RenderArgs& A, uint32_t item, bool scene_ok) {
        rid = item;
        float tmax;
        cr_load_ray(rays, rid, o, d, tmax);
        best = wmin(tmax, kInfT);
        if (enter_root(A, scene_ok, cr_ray_walked(o, d, tmax))) return true;
        counts[rid] = 0u;
        return false;
    }
    __device__ __forceinline__ void finish(const RenderArgs&) { counts[rid] = count; }
    __device__ __forceinline__ void after_refill(uint32_t) {}
    __device__ __forceinline__ void after_step(bool, uint32_t) {}
};
__global__ __launch_bounds__(64) void count_hits_kernel(const RenderArgs A, const float4* __restrict__ rays, uint32_t* __restrict__ counts, uint32_t n,
                                                        unsigned long long* __restrict__ queue, unsigned long long* __restrict__ spill, uint32_t fill) {
    CountWalk q; q.rays = rays; q.counts = counts;
    persistent_walk<PT_CR_SHORT_STACK>(A, n, queue, spill, fill, q);
}

// A sample ray of a point: 16 bytes of point instead of 32 bytes of ray, and a parity instead of a count.  A ray that ends where it starts
// has crossed nothing (even), so only the rays that end in a step count; that counting is wave-wide (count_odd) and sits in after_step.
struct ContainsWalk : CrossState {
    static constexpr bool kWaveHooks = true;
    const float4* __restrict__ points; uint4* __restrict__ out;
    uint32_t samples, samples_magic, seed, index_base;
    uint32_t pid = 0;

    __device__ __forceinline__ bool start(const RenderArgs& A, uint32_t item, bool scene_ok) {
        uint32_t s; divmod_magic(item, samples, samples_magic, pid, s);
        const float4 pt = points[pid];
        const F3 p = f3(pt.x, pt.y, pt.z);
        if (!cr_point_traced(p)) return false;
        cr_sample_ray(p, seed, index_base + pid, s, o, d);
        best = kInfT;
        return enter_root(A, scene_ok, cr_ray_walked(o, d, kInfT));
    }
    __device__ __forceinline__ void finish(const RenderArgs&) {}
    __device__ __forceinline__ void after_refill(uint32_t) {}
    // the lanes whose ray ended in this step with an odd count, combined per point
    __device__ __forceinline__ void after_step(bool done, uint32_t lane) {
        if (__ballot(done) != 0ull) count_odd(out, done && (count & 1u) != 0u, pid, lane);
    }
};
__global__ __launch_bounds__(64) void contains_kernel(const RenderArgs A, const float4* __restrict__ points, uint4* __restrict__ out, uint32_t items,
                                                      uint32_t samples, uint32_t samples_magic, uint32_t seed, uint32_t index_base,
                                                      unsigned long long* __restrict__ queue, unsigned long long* __restrict__ spill, uint32_t fill) {
    ContainsWalk q; q.points = points; q.out = out; q.samples = samples; q.samples_magic = samples_magic; q.seed = seed; q.index_base = index_base;
    persistent_walk<PT_CR_SHORT_STACK>(A, items, queue, spill, fill, q);
}

// one thread per point: the record around the count
__global__ __launch_bounds__(256) void contains_finish_kernel(const float4* __restrict__ points, uint4* __restrict__ out, uint32_t n, uint32_t samples) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 pt = points[i];
    if (!cr_point_traced(f3(pt.x, pt.y, pt.z))) { out[i] = make_uint4(0u, 0u, 0u, 0u); return; }
    const uint32_t odd = out[i].y;
    out[i] = make_uint4(2u * odd > samples ? 1u : 0u, odd, samples, 0u);
}

// one thread per point: PtClosest::dist gets the sign bit where PtContainment::inside is set (+inf becomes -inf: inside, nothing within r_max)
__global__ __launch_bounds__(256) void apply_sign_kernel(const uint4* __restrict__ contain, uint4* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (contain[i].x != 0u) ((uint32_t*)(out + i))[0] |= 0x80000000u;
}

// ------------------------------------------------------------------------------------
// brute force: one ray per thread, every triangle in index order; a workgroup streams the records through LDS, kCrBruteTile at a time
// ------------------------------------------------------------------------------------
constexpr uint32_t kCrBruteTile = 256;
template <bool STATS>
__global__ __launch_bounds__(256) void count_hits_brute_kernel(const RenderArgs A, const float4* __restrict__ rays, uint32_t* __restrict__ counts, uint32_t n) {
    __shared__ uint4 rec[kCrBruteTile][3];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    F3 o = f3(0, 0, 0), d = o; float tmax = 0.0f;
    if (i < n) cr_load_ray(rays, i, o, d, tmax);
    const bool walked = (i < n) && cr_ray_walked(o, d, tmax);
    const float best = wmin(tmax, kInfT);
    uint32_t count = 0;
    Counters cnt; cnt.nodes = cnt.tris = cnt.drops = cnt.maxstack = 0;
    const uint4* recs = (const uint4*)A.tris;
    for (uint32_t base = 0; base < A.num_tris; base += kCrBruteTile) {
        const uint32_t tile = min(kCrBruteTile, A.num_tris - base);
        __syncthreads();
        if (threadIdx.x < tile) {
            const uint4* tp = recs + (size_t)(base + threadIdx.x) * 4;
            rec[threadIdx.x][0] = tp[0]; rec[threadIdx.x][1] = tp[1]; rec[threadIdx.x][2] = tp[2];
        }
        __syncthreads();
        if (walked) {
            for (uint32_t k = 0; k < tile; ++k) {
                float t;
                if (tri_hit(o, d, rec[k][0], rec[k][1], rec[k][2], t) & (t < best)) ++count;
            }
            if (STATS) cnt.tris += tile;
        }
    }
    if (i < n) counts[i] = count;
    if (STATS) add_stats(A, 0, i < n ? 1u : 0u, cnt);
}

// floor(2^32 / d), saturated for d = 1 (divmod_magic's one correction covers the difference)
static uint32_t cr_magic_of(uint32_t d) { return (uint32_t)std::min<unsigned long long>((1ull << 32) / d, 0xFFFFFFFFull); }

hipError_t launch_count_hits(const RenderArgs& A, const void* rays, void* counts, uint32_t n, bool simple, bool stats, bool brute,
                             unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    const float4* r = (const float4*)rays; uint32_t* c = (uint32_t*)counts;
    const dim3 g256((n + 255u) / 256u);
    if (brute) {
        if (stats) count_hits_brute_kernel<true><<<g256, 256, 0, stream>>>(A, r, c, n);
        else count_hits_brute_kernel<false><<<g256, 256, 0, stream>>>(A, r, c, n);
        return hipGetLastError();
    }
    if (simple || stats) {
        if (stats) count_hits_simple_kernel<true><<<g256, 256, 0, stream>>>(A, r, c, n);
        else count_hits_simple_kernel<false><<<g256, 256, 0, stream>>>(A, r, c, n);
        return hipGetLastError();
    }
    hipError_t e = walk_begin(queue, n, grid, stream);
    if (e != hipSuccess) return e;
    count_hits_kernel<<<grid, 64, 0, stream>>>(A, r, c, n, queue, spill, PT_CR_FILL);
    return hipGetLastError();
}

hipError_t launch_contains(const RenderArgs& A, const void* points, void* out, uint32_t n, uint32_t samples, uint32_t seed, uint32_t index_base,
                           bool simple, bool stats, unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    const float4* p = (const float4*)points; uint4* o = (uint4*)out;
    const uint32_t items = n * samples, magic = cr_magic_of(samples);
    hipError_t e = hipMemsetAsync(out, 0, (size_t)n * sizeof(uint4), stream);
    if (e != hipSuccess) return e;
    if (simple || stats) {
        const dim3 g((uint32_t)(((unsigned long long)items + 255u) / 256u));
        if (stats) contains_simple_kernel<true><<<g, 256, 0, stream>>>(A, p, o, items, samples, magic, seed, index_base);
        else contains_simple_kernel<false><<<g, 256, 0, stream>>>(A, p, o, items, samples, magic, seed, index_base);
    } else {
        e = walk_begin(queue, items, grid, stream);
        if (e != hipSuccess) return e;
        contains_kernel<<<grid, 64, 0, stream>>>(A, p, o, items, samples, magic, seed, index_base, queue, spill, PT_CR_FILL);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    contains_finish_kernel<<<dim3((n + 255u) / 256u), 256, 0, stream>>>(p, o, n, samples);
    return hipGetLastError();
}

hipError_t launch_apply_sign(const void* contain, void* out, uint32_t n, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    apply_sign_kernel<<<dim3((n + 255u) / 256u), 256, 0, stream>>>((const uint4*)contain, (uint4*)out, n);
    return hipGetLastError();
}

} // namespace ptk
