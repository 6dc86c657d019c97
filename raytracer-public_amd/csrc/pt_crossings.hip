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
// The walk is pt_walk.h::persistent_walk with the tests of pt_device.h and the lane state of pt_rays.h::RayState, as in
// pt_rayquery.hip::trace_rays_kernel<true>: `best` is min(t_max, kInfT) in both and moves in neither, so the any-hit walk is a prefix of
// the counting walk and count >= 1 exactly when pt_trace_rays(PT_TRACE_ANY_HIT) reports a hit.  Sample ray s of point i is record
// i * samples + s of pt_occlusion_rays for the surfel {p, r_max = +inf, n = (0, 0, 1)} with bias 0: both call pt_rays.h::sample_ray.
// Records: PtRay = two float4 (org.xyz, t_max | dir.xyz, reserved), a count = one uint32_t, PtPoint = one float4 (p.xyz, r_max: ignored),
// PtContainment = one uint4 (inside, odd, samples, 0).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_kernels.h"
#include "pt_device.h"
#include "pt_rays.h"
#include "pt_walk.h"

namespace ptk {

// a point with a NaN in p is not traced (r_max is ignored)
__device__ __forceinline__ bool point_traced(F3 p) { return !(__builtin_isnan(p.x) | __builtin_isnan(p.y) | __builtin_isnan(p.z)); }
// sample ray s of the point with sample index `pixel` = index_base + i (mod 2^32): pt_rays.h::sample_ray of the surfel {p, n = (0, 0, 1)}
// with bias 0 (org = p + n * 0 turns a -0 into +0, as it does for pt_occlusion_rays)
__device__ __forceinline__ void point_sample_ray(F3 p, uint32_t seed, uint32_t pixel, uint32_t s, F3& o, F3& d) {
    Surfel sf; sf.p = p; sf.n = f3(0.0f, 0.0f, 1.0f); sf.r_max = kInfT;
    sample_ray(sf, seed, pixel, s, 0.0f, o, d);
}
// what every counting kernel does with a triangle record its ray reaches
__device__ __forceinline__ void count_crossing(F3 o, F3 d, float best, const uint4 n0, const uint4 n1, const uint4 n2, uint32_t& count) {
    float t;
    if (tri_hit(o, d, n0, n1, n2, t) & (t < best)) ++count;
}

// ------------------------------------------------------------------------------------
// one ray per thread: pt_rays.h::cross_traverse, pt_device.h::traverse with a count in place of the closest hit
// ------------------------------------------------------------------------------------
template <bool STATS>
__device__ __forceinline__ uint32_t count_traverse(const RenderArgs& A, const Ray& r, uint2* __restrict__ stk, Counters& cnt, float best) {
    uint32_t count = 0;
    cross_traverse<STATS>(A, r, stk, cnt, best, [&](uint32_t, const uint4 n0, const uint4 n1, const uint4 n2) __attribute__((always_inline)) {
        count_crossing(r.o, r.d, best, n0, n1, n2, count);
    });
    return count;
}

template <bool STATS>
__global__ __launch_bounds__(256) void count_hits_simple_kernel(const RenderArgs A, const float4* __restrict__ rays, uint32_t* __restrict__ counts, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    Counters cnt; cnt.nodes = cnt.tris = cnt.drops = cnt.maxstack = 0;
    if (i < n) {
        F3 o, d; float tmax;
        load_ray(rays, i, o, d, tmax);
        uint32_t count = 0;
        if (ray_traced(o, d, tmax)) {
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
        if (point_traced(p)) {
            F3 o, d; point_sample_ray(p, seed, index_base + pid, s, o, d);
            n_rays = 1;
            if (ray_traced(o, d, kInfT)) {
                Ray r; r.o = o; r.d = d; r.inv = safe_inv(d);
                uint2 stk[kStackMax];
                odd = (count_traverse<STATS>(A, r, stk, cnt, kInfT) & 1u) != 0u;
            }
        }
    }
    count_same(out, odd, pid, threadIdx.x & 63u);
    if (STATS) add_stats(A, 0, n_rays, cnt);
}

// ------------------------------------------------------------------------------------
// persistent kernels: one wavefront per workgroup, one ray per lane, lanes refilled from the wavefront's chunk
// ------------------------------------------------------------------------------------
// What persistent_walk's Q (pt_walk.h) of a counted ray holds whichever record the ray comes from: RayState (pt_rays.h) with a counter in
// place of the hit, and a leaf test that never ends the ray, so `best` never moves and every stacked entry is walked.
struct CrossState : RayState {
    uint32_t count = 0;
    __device__ __forceinline__ bool leaf(uint32_t, const uint4 n0, const uint4 n1, const uint4 n2) {
        count_crossing(o, d, best, n0, n1, n2, count);
        return false;                                                     // no hit ends the ray
    }
};

struct CountWalk : CrossState {
    static constexpr bool kWaveHooks = false;
    const float4* __restrict__ rays; uint32_t* __restrict__ counts;
    uint32_t rid = 0;

    __device__ __forceinline__ bool start(const RenderArgs& A, uint32_t item, bool scene_ok) {
        rid = item;
        float tmax;
        load_ray(rays, rid, o, d, tmax);
        best = wmin(tmax, kInfT); count = 0u;
        if (enter_root(A, scene_ok, ray_traced(o, d, tmax))) return true;
        counts[rid] = 0u;
        return false;
    }
    __device__ __forceinline__ void finish(const RenderArgs&) { counts[rid] = count; }
};
__global__ __launch_bounds__(64) void count_hits_kernel(const RenderArgs A, const float4* __restrict__ rays, uint32_t* __restrict__ counts, uint32_t n,
                                                        unsigned long long* __restrict__ queue, unsigned long long* __restrict__ spill, uint32_t fill) {
    CountWalk q; q.rays = rays; q.counts = counts;
    persistent_walk<PT_CR_SHORT_STACK>(A, n, queue, spill, fill, q);
}

// A sample ray of a point: 16 bytes of point instead of 32 bytes of ray, and a parity instead of a count.  A ray that ends where it starts
// has crossed nothing (even), so only the rays that end in a step count; that counting is wave-wide (count_same) and sits in after_step.
struct ContainsWalk : CrossState {
    static constexpr bool kWaveHooks = true;
    const float4* __restrict__ points; uint4* __restrict__ out;
    uint32_t samples, samples_magic, seed, index_base;
    uint32_t pid = 0;

    __device__ __forceinline__ bool start(const RenderArgs& A, uint32_t item, bool scene_ok) {
        uint32_t s; divmod_magic(item, samples, samples_magic, pid, s);
        const float4 pt = points[pid];
        const F3 p = f3(pt.x, pt.y, pt.z);
        if (!point_traced(p)) return false;
        point_sample_ray(p, seed, index_base + pid, s, o, d);
        best = kInfT; count = 0u;
        return enter_root(A, scene_ok, ray_traced(o, d, kInfT));
    }
    // the lanes whose ray ended in this step with an odd count, combined per point
    __device__ __forceinline__ void after_step(bool done, uint32_t lane) {
        if (__ballot(done) != 0ull) count_same(out, done && (count & 1u) != 0u, pid, lane);
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
    if (!point_traced(f3(pt.x, pt.y, pt.z))) { out[i] = make_uint4(0u, 0u, 0u, 0u); return; }
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
// brute force: one ray per thread, every triangle in index order (pt_walk.h::brute_records)
// ------------------------------------------------------------------------------------
template <bool STATS>
__global__ __launch_bounds__(256) void count_hits_brute_kernel(const RenderArgs A, const float4* __restrict__ rays, uint32_t* __restrict__ counts, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    F3 o = f3(0, 0, 0), d = o; float tmax = 0.0f;
    if (i < n) load_ray(rays, i, o, d, tmax);
    const bool walked = (i < n) && ray_traced(o, d, tmax);
    const float best = wmin(tmax, kInfT);
    uint32_t count = 0;
    brute_records(A, walked, [&](uint32_t, const uint4 n0, const uint4 n1, const uint4 n2) __attribute__((always_inline)) {
        count_crossing(o, d, best, n0, n1, n2, count);
    });
    if (i < n) counts[i] = count;
    if (STATS) {
        Counters cnt; cnt.nodes = cnt.drops = cnt.maxstack = 0;
        cnt.tris = walked ? A.num_tris : 0u;                              // a walked ray tests every record
        add_stats(A, 0, i < n ? 1u : 0u, cnt);
    }
}

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
    const uint32_t items = n * samples, magic = magic_of(samples);
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
