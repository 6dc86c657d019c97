// pt_occlusion.hip -- batched ambient-occlusion queries over the context's scene (include/mi355pt.h: pt_occlusion, pt_occlusion_rays,
// pt_hit_surfels):
//   * occlusion_kernel                the default: persistent wavefronts, one sample ray per lane, built in registers from the surfel record
//                                     and walked any-hit; a lane whose ray has ended takes the next item of its wavefront's chunk
//   * occlusion_simple_kernel<STATS>  one sample ray per thread over the renderer's traverse() (pt_device.h): PT_OCCLUSION_SIMPLE_KERNEL,
//                                     PT_OCCLUSION_STATS
//   * occlusion_finish_kernel         one thread per surfel: visibility, samples and reserved around the counted `unoccluded`
//   * occlusion_rays_kernel           the sample rays written out as PtRay records (what pt_trace_rays would be given)
//   * hit_surfels_kernel              PtRay + PtHit -> PtSurfel
//
// Item i * samples + s is sample ray s of surfel i.  Its ray is a pure function of the surfel record and (seed, index_base + i, s)
// (pt_rays.h::sample_ray), so the persistent kernel, the simple kernel and occlusion_rays_kernel produce the same bits, and a sample is occluded
// exactly when pt_trace_rays(PT_TRACE_ANY_HIT) reports a hit for the record occlusion_rays_kernel writes: occlusion_kernel and
// pt_rayquery.hip::trace_rays_kernel<true> are the same walk (pt_walk.h::persistent_walk) and the same tests (pt_device.h).
// The surfel record, the sample ray, the lane state of the walk and the per-id counting are pt_rays.h's, shared with pt_crossings.hip.
// Records: PtSurfel = two float4 (p.xyz, r_max | n.xyz, reserved), PtOcclusion = one uint4 (visibility bits, unoccluded, samples, 0).
// The counter of surfel i is word 1 of its output record: zeroed by the launch, incremented by vector atomics, completed by the finish kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_kernels.h"
#include "pt_device.h"
#include "pt_rays.h"
#include "pt_walk.h"

namespace ptk {

// ------------------------------------------------------------------------------------
// simple kernel: one sample ray per thread, the renderer's traversal with its 64-entry private stack
// ------------------------------------------------------------------------------------
template <bool STATS>
__global__ __launch_bounds__(256) void occlusion_simple_kernel(const RenderArgs A, const float4* __restrict__ surfels, uint4* __restrict__ out, uint32_t items,
                                                               uint32_t samples, uint32_t samples_magic, uint32_t seed, uint32_t index_base, float bias) {
    const unsigned long long gi = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    Counters cnt; cnt.nodes = cnt.tris = cnt.drops = cnt.maxstack = 0;
    uint32_t n_rays = 0, sid = 0;
    bool miss = false;
    if (gi < items) {
        uint32_t s; divmod_magic((uint32_t)gi, samples, samples_magic, sid, s);
        const Surfel sf = load_surfel(surfels, sid);
        if (surfel_traced(sf)) {
            F3 o, d; sample_ray(sf, seed, index_base + sid, s, bias, o, d);
            n_rays = 1; miss = true;
            if (ray_traced(o, d, sf.r_max)) {
                Ray r; r.o = o; r.d = d; r.inv = safe_inv(d);
                uint2 stk[kStackMax];
                float bt; uint32_t bi;
                if (traverse<true, STATS>(A, r, bt, bi, stk, cnt, wmin(sf.r_max, kInfT))) miss = false;
            }
        }
    }
    count_same(out, miss, sid, threadIdx.x & 63u);
    if (STATS) add_stats(A, 1, n_rays, cnt);
}

// ------------------------------------------------------------------------------------
// persistent kernel: one wavefront per workgroup, one sample ray per lane, lanes refilled from the wavefront's chunk
// ------------------------------------------------------------------------------------
// persistent_walk's Q (pt_walk.h) of a sample ray: RayState (pt_rays.h) as RayWalk<true> of pt_rayquery.hip has it, except where a ray
// comes from (32 bytes of surfel instead of 32 bytes of ray: no ray record is ever written) and where it goes (a count instead of a
// 16-byte hit record).  A lane keeps neither the hit triangle nor the ray's number: only the surfel id it counts for.  `best` never
// moves (the first hit ends the ray).  The counting is wave-wide (count_same), so it sits in the two hooks: behind a hand-out for the
// rays that end where they start, behind a step for those that ended in it without a hit.
struct OcclusionWalk : RayState {
    static constexpr bool kWaveHooks = true;
    const float4* __restrict__ surfels; uint4* __restrict__ out;
    uint32_t samples, samples_magic, seed, index_base; float bias;
    uint32_t sid = 0;
    bool miss = false;          // this lane's new ray ends where it starts: it is not walked, or it misses the root box
    bool occluded = false;      // this lane's ray ended in this step at a hit

    __device__ __forceinline__ bool start(const RenderArgs& A, uint32_t item, bool scene_ok) {
        uint32_t s; divmod_magic(item, samples, samples_magic, sid, s);
        const Surfel sf = load_surfel(surfels, sid);
        if (!surfel_traced(sf)) return false;
        sample_ray(sf, seed, index_base + sid, s, bias, o, d);
        best = wmin(sf.r_max, kInfT);
        if (enter_root(A, scene_ok, ray_traced(o, d, sf.r_max))) return true;
        miss = true;
        return false;
    }
    __device__ __forceinline__ bool leaf(uint32_t, const uint4 n0, const uint4 n1, const uint4 n2) {
        float t;
        if (tri_hit(o, d, n0, n1, n2, t) & (t < best)) occluded = true;      // any hit ends the ray
        return occluded;
    }
    __device__ __forceinline__ void after_refill(uint32_t lane) { count_same(out, miss, sid, lane); miss = false; }
    // the lanes whose ray ended in this step without a hit, combined per surfel
    __device__ __forceinline__ void after_step(bool done, uint32_t lane) {
        if (__ballot(done) != 0ull) count_same(out, done && !occluded, sid, lane);
        occluded = false;
    }
};
__global__ __launch_bounds__(64) void occlusion_kernel(const RenderArgs A, const float4* __restrict__ surfels, uint4* __restrict__ out, uint32_t items,
                                                       uint32_t samples, uint32_t samples_magic, uint32_t seed, uint32_t index_base, float bias,
                                                       unsigned long long* __restrict__ queue, unsigned long long* __restrict__ spill, uint32_t fill) {
    OcclusionWalk q; q.surfels = surfels; q.out = out; q.samples = samples; q.samples_magic = samples_magic; q.seed = seed; q.index_base = index_base; q.bias = bias;
    persistent_walk<PT_OC_SHORT_STACK>(A, items, queue, spill, fill, q);
}

// one thread per surfel: the record around the count
__global__ __launch_bounds__(256) void occlusion_finish_kernel(const float4* __restrict__ surfels, uint4* __restrict__ out, uint32_t n, uint32_t samples) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Surfel sf = load_surfel(surfels, i);
    if (!surfel_traced(sf)) { out[i] = make_uint4(0u, 0u, 0u, 0u); return; }
    const uint32_t unocc = out[i].y;
    const float vis = (float)unocc / (float)samples;
    out[i] = make_uint4(__float_as_uint(vis), unocc, samples, 0u);
}

// one thread per sample ray: the PtRay record of item i * samples + s
__global__ __launch_bounds__(256) void occlusion_rays_kernel(const float4* __restrict__ surfels, float4* __restrict__ rays, uint32_t items,
                                                             uint32_t samples, uint32_t samples_magic, uint32_t seed, uint32_t index_base, float bias) {
    const unsigned long long gi = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= items) return;
    uint32_t sid, s; divmod_magic((uint32_t)gi, samples, samples_magic, sid, s);
    const Surfel sf = load_surfel(surfels, sid);
    F3 o = sf.p, d = sf.n; float tmax = 0.0f;
    if (surfel_traced(sf)) { sample_ray(sf, seed, index_base + sid, s, bias, o, d); tmax = sf.r_max; }
    rays[(size_t)gi * 2] = make_float4(o.x, o.y, o.z, tmax);
    rays[(size_t)gi * 2 + 1] = make_float4(d.x, d.y, d.z, 0.0f);
}

// one thread per ray: the surfel at its hit, normal turned against the ray; a miss gives an untraced surfel
__global__ __launch_bounds__(256) void hit_surfels_kernel(const RenderArgs A, const float4* __restrict__ rays, const uint4* __restrict__ hits, uint32_t n,
                                                          float r_max, float4* __restrict__ surfels) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 a = rays[(size_t)i * 2], b = rays[(size_t)i * 2 + 1];
    const uint4 h = hits[i];
    F3 p = f3(a.x, a.y, a.z), nf = f3(b.x, b.y, b.z); float r = 0.0f;
    if (h.y < A.num_tris) {
        const F3 d = nf;
        const F3 nrm = tri_normal(A, h.y);
        p = p + d * __uint_as_float(h.x);
        nf = (dot3(nrm, d) < 0.0f) ? nrm : f3(-nrm.x, -nrm.y, -nrm.z);
        r = r_max;
    }
    surfels[(size_t)i * 2] = make_float4(p.x, p.y, p.z, r);
    surfels[(size_t)i * 2 + 1] = make_float4(nf.x, nf.y, nf.z, 0.0f);
}

hipError_t launch_occlusion(const RenderArgs& A, const void* surfels, void* out, uint32_t n, uint32_t samples, uint32_t seed, uint32_t index_base, float bias,
                            bool simple, bool stats, unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    const float4* sf = (const float4*)surfels; uint4* o = (uint4*)out;
    const uint32_t items = n * samples, magic = magic_of(samples);
    hipError_t e = hipMemsetAsync(out, 0, (size_t)n * sizeof(uint4), stream);
    if (e != hipSuccess) return e;
    if (simple || stats) {
        const dim3 g((uint32_t)(((unsigned long long)items + 255u) / 256u));
        if (stats) occlusion_simple_kernel<true><<<g, 256, 0, stream>>>(A, sf, o, items, samples, magic, seed, index_base, bias);
        else occlusion_simple_kernel<false><<<g, 256, 0, stream>>>(A, sf, o, items, samples, magic, seed, index_base, bias);
    } else {
        e = walk_begin(queue, items, grid, stream);
        if (e != hipSuccess) return e;
        occlusion_kernel<<<grid, 64, 0, stream>>>(A, sf, o, items, samples, magic, seed, index_base, bias, queue, spill, PT_OC_FILL);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    occlusion_finish_kernel<<<dim3((n + 255u) / 256u), 256, 0, stream>>>(sf, o, n, samples);
    return hipGetLastError();
}

hipError_t launch_occlusion_rays(const void* surfels, void* rays, uint32_t n, uint32_t samples, uint32_t seed, uint32_t index_base, float bias, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    const uint32_t items = n * samples;
    const dim3 g((uint32_t)(((unsigned long long)items + 255u) / 256u));
    occlusion_rays_kernel<<<g, 256, 0, stream>>>((const float4*)surfels, (float4*)rays, items, samples, magic_of(samples), seed, index_base, bias);
    return hipGetLastError();
}

hipError_t launch_hit_surfels(const RenderArgs& A, const void* rays, const void* hits, uint32_t n, float r_max, void* surfels, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    hit_surfels_kernel<<<dim3((n + 255u) / 256u), 256, 0, stream>>>(A, (const float4*)rays, (const uint4*)hits, n, r_max, (float4*)surfels);
    return hipGetLastError();
}

} // namespace ptk
