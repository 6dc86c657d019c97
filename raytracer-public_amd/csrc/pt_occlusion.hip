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
// (sample_ray below), so the persistent kernel, the simple kernel and occlusion_rays_kernel produce the same bits, and a sample is occluded
// exactly when pt_trace_rays(PT_TRACE_ANY_HIT) reports a hit for the record occlusion_rays_kernel writes: the walk below is the walk of
// pt_rayquery.hip::trace_rays_kernel<true>, kept as a private copy so that the resource line of that kernel does not depend on this file.
// Records: PtSurfel = two float4 (p.xyz, r_max | n.xyz, reserved), PtOcclusion = one uint4 (visibility bits, unoccluded, samples, 0).
// The counter of surfel i is word 1 of its output record: zeroed by the launch, incremented by vector atomics, completed by the finish kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>

#include "pt_kernels.h"
#include "pt_device.h"

namespace ptk {

constexpr int kOcShort = PT_OC_SHORT_STACK;     // LDS stack entries per lane; entries from this depth on live in the spill area
constexpr uint32_t kOcChunk = 64;               // items per queue claim: one per lane of the claiming wavefront
constexpr uint32_t kOcXcds = 8;                 // chunk ranges with a queue counter each (MI355X: 8 XCDs)
constexpr uint32_t kOcQueueStride = 32;         // counters 256 bytes apart

struct Surfel { F3 p, n; float r_max; };
__device__ __forceinline__ Surfel load_surfel(const float4* __restrict__ surfels, uint32_t i) {
    const float4 a = surfels[(size_t)i * 2], b = surfels[(size_t)i * 2 + 1];
    Surfel s; s.p = f3(a.x, a.y, a.z); s.r_max = a.w; s.n = f3(b.x, b.y, b.z);
    return s;
}
// a surfel with a NaN in p, n or r_max, or with r_max <= 0, is not traced (a NaN r_max fails the comparison as well)
__device__ __forceinline__ bool surfel_traced(const Surfel& s) {
    const bool nan = __builtin_isnan(s.p.x) | __builtin_isnan(s.p.y) | __builtin_isnan(s.p.z) | __builtin_isnan(s.n.x) | __builtin_isnan(s.n.y) | __builtin_isnan(s.n.z);
    return !nan & (s.r_max > 0.0f);
}
// sample ray s of the surfel with sample index `pixel` = index_base + i (mod 2^32): DESIGN.md section 4's cosine sampling around n as given
__device__ __forceinline__ void sample_ray(const Surfel& sf, uint32_t seed, uint32_t pixel, uint32_t s, float bias, F3& o, F3& d) {
    const uint32_t key = sample_key(seed, pixel, s);
    const float u1 = rnd(key, 0u, 2u), u2 = rnd(key, 0u, 3u);
    d = cosine_dir(sf.n, u1, u2);
    o = sf.p + sf.n * bias;
}
// pt_rayquery.hip::ray_traced: a ray with a NaN in org or dir is a miss and is not traversed (t_max = r_max > 0 holds for a traced surfel)
__device__ __forceinline__ bool ray_walks(F3 o, F3 d) {
    return !(__builtin_isnan(o.x) | __builtin_isnan(o.y) | __builtin_isnan(o.z) | __builtin_isnan(d.x) | __builtin_isnan(d.y) | __builtin_isnan(d.z));
}
// The lanes of `miss` that hold the same surfel add their number to its counter with ONE atomic (the first of them issues it): with 64
// samples per surfel the lanes of a chunk share a surfel, and one same-address atomic per ray would serialise in the L2.  Wave-uniform loop
// over the distinct surfels among the finishing lanes (one or two in practice).  Integer sums: any order gives the same bits.
__device__ __forceinline__ void count_misses(uint4* __restrict__ out, bool miss, uint32_t sid, uint32_t lane) {
    unsigned long long m = __ballot(miss);
    while (m != 0ull) {
        const int leader = __builtin_ctzll(m);
        const uint32_t s0 = (uint32_t)__shfl((int)sid, leader, 64);
        const unsigned long long same = __ballot(miss && sid == s0);
        if (lane == (uint32_t)leader) atomicAdd(&((uint32_t*)(out + s0))[1], (uint32_t)__popcll(same));
        m &= ~same;
    }
}

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
            if (ray_walks(o, d)) {
                Ray r; r.o = o; r.d = d; r.inv = safe_inv(d);
                uint2 stk[kStackMax];
                float bt; uint32_t bi;
                if (traverse<true, STATS>(A, r, bt, bi, stk, cnt, wmin(sf.r_max, kInfT))) miss = false;
            }
        }
    }
    count_misses(out, miss, sid, threadIdx.x & 63u);
    if (STATS) {      // the oracle's counters (PtStats order), summed over the wavefront first: one atomic per counter and wavefront
        uint32_t nodes = cnt.nodes, tris = cnt.tris, drops = cnt.drops, maxstack = cnt.maxstack;
        for (int off = 32; off > 0; off >>= 1) {
            n_rays += __shfl_xor(n_rays, off, 64); nodes += __shfl_xor(nodes, off, 64); tris += __shfl_xor(tris, off, 64);
            drops += __shfl_xor(drops, off, 64); maxstack = max(maxstack, (uint32_t)__shfl_xor(maxstack, off, 64));
        }
        if ((threadIdx.x & 63u) == 0u) {
            atomicAdd(&A.stats[1], (unsigned long long)n_rays);
            atomicAdd(&A.stats[2], (unsigned long long)nodes);
            atomicAdd(&A.stats[3], (unsigned long long)tris);
            atomicAdd(&A.stats[4], (unsigned long long)drops);
            atomicMax(&A.stats[5], (unsigned long long)maxstack);
        }
    }
}

// ------------------------------------------------------------------------------------
// persistent kernel: one wavefront per workgroup, one sample ray per lane, lanes refilled from the wavefront's chunk
// ------------------------------------------------------------------------------------
// Queue, chunks, refill, the 64 B step, the stack (entries 0 .. kOcShort-1 in LDS, one column per lane; deeper entries in the spill area at
// [entry - kOcShort][grid lane]) and the end of the wavefront are those of trace_rays_kernel<true> (pt_rayquery.hip); what differs is where
// a ray comes from (32 bytes of surfel instead of 32 bytes of ray: no ray record is ever written) and where it goes (a count instead of a
// 16-byte hit record).  A lane keeps neither the hit triangle nor the ray's number: only the surfel id it counts for.
__global__ __launch_bounds__(64) void occlusion_kernel(const RenderArgs A, const float4* __restrict__ surfels, uint4* __restrict__ out, uint32_t items,
                                                       uint32_t samples, uint32_t samples_magic, uint32_t seed, uint32_t index_base, float bias,
                                                       unsigned long long* __restrict__ queue, unsigned long long* __restrict__ spill, uint32_t fill) {
    __shared__ unsigned long long lds_stack[kOcShort][64];
    const uint32_t lane = threadIdx.x;
    unsigned long long* const stk = &lds_stack[0][lane];
    const size_t grid_lanes = (size_t)gridDim.x * 64u, my_lane = (size_t)blockIdx.x * 64u + lane;
    const bool scene_ok = !(A.root_ref == kInvalidRef || A.num_tris == 0u || A.root_degenerate != 0u);

    const uint32_t chunks = (uint32_t)(((unsigned long long)items + kOcChunk - 1u) / kOcChunk), per_xcd = (chunks + kOcXcds - 1u) / kOcXcds;
    uint32_t xcd = (uint32_t)__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & (kOcXcds - 1u), hops = 0;      // HW_REG_XCC_ID
    unsigned long long ahead = 0;                         // lane 0: the claimed next chunk of range `xcd` (read where it is used)
    if (lane == 0u) ahead = atomicAdd(&queue[xcd * kOcQueueStride], 1ull);
    uint32_t next = 0, end = 0; bool dry = false;
    bool trav = false;                                    // this lane traverses a ray
    uint32_t sid = 0, cur = 0; int sp = 0; float best = 0.0f;
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
                        if (++hops >= kOcXcds) { dry = true; break; }
                        xcd = (xcd + 1u) & (kOcXcds - 1u);
                        // a plain read first: a range that is used up costs no claim (every wavefront looks at every range once at the end)
                        unsigned long long seen = 0;
                        if (lane == 0u) seen = __hip_atomic_load(&queue[xcd * kOcQueueStride], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        c = __shfl(seen, 0, 64);
                        if (used_up(xcd, c)) continue;
                        if (lane == 0u) ahead = atomicAdd(&queue[xcd * kOcQueueStride], 1ull);
                        c = __shfl(ahead, 0, 64);
                    }
                    if (dry) break;
                    if (lane == 0u) ahead = atomicAdd(&queue[xcd * kOcQueueStride], 1ull);
                    const uint32_t chunk = xcd * per_xcd + (uint32_t)c;
                    next = chunk * kOcChunk; end = (uint32_t)min((unsigned long long)next + kOcChunk, (unsigned long long)items);
                }
                const uint32_t take = min((uint32_t)__popcll(idle), end - next);
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
                bool miss = false;                        // this lane's new ray ends here: it is not walked, or it misses the root box
                if (!trav && rank < take) {
                    uint32_t s; divmod_magic(next + rank, samples, samples_magic, sid, s);
                    const Surfel sf = load_surfel(surfels, sid);
                    if (surfel_traced(sf)) {
                        sample_ray(sf, seed, index_base + sid, s, bias, o, d);
                        best = wmin(sf.r_max, kInfT); sp = 0;
                        inv = safe_inv(d); sel = ray_selectors(inv);
                        Ray r; r.o = o; r.d = d; r.inv = inv;
                        float troot;
                        if (scene_ok && ray_walks(o, d) && slab(r, A.root_box[0], A.root_box[1], A.root_box[2], best, troot)) { cur = A.root_ref; trav = true; }
                        else miss = true;
                    }
                }
                count_misses(out, miss, sid, lane);
                next += take;
                idle = __ballot(!trav);
            }
            if (idle == ~0ull) break;                     // the queue is dry and nothing traverses
        }
        bool need_pop = true, done = false, occluded = false;
        if (trav) {
            const uint4* np = arena_record(A, cur);
            const uint4 n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3];
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
                if (ok_det & ok_u & ok_v & (t > kTriEps) & (t < best)) { done = true; occluded = true; }    // any hit ends the ray
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
                            if (__builtin_expect(sp < kOcShort, 1)) stk[sp * 64] = e;
                            else spill[(size_t)(sp - kOcShort) * grid_lanes + my_lane] = e;
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
                // entries whose box the ray no longer reaches (tmin >= best) are skipped; `best` never moves here (the first hit ends the ray)
                bool found = false;
                while (sp > 0) {
                    --sp;
                    const unsigned long long e = sp < kOcShort ? stk[sp * 64] : spill[(size_t)(sp - kOcShort) * grid_lanes + my_lane];
                    if (__uint_as_float((uint32_t)(e >> 32)) < best) { cur = (uint32_t)e; found = true; break; }
                }
                done = !found;
            }
            if (done) trav = false;
        }
        // the lanes whose ray ended in this step without a hit, combined per surfel
        if (__ballot(done) != 0ull) count_misses(out, done && !occluded, sid, lane);
    }
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

static_assert(kRqQueueWords == kOcXcds * kOcQueueStride, "pt_kernels.h: the queue block holds one counter line per range");
uint32_t occlusion_grid(int num_cus) { return (uint32_t)num_cus * 4u * PT_OC_WAVES_PER_SIMD; }
size_t occlusion_spill_entries(uint32_t grid) { return (size_t)(kStackMax - kOcShort) * grid * 64u; }

// floor(2^32 / d), saturated for d = 1 (divmod_magic's one correction covers the difference)
static uint32_t magic_of(uint32_t d) { return (uint32_t)std::min<unsigned long long>((1ull << 32) / d, 0xFFFFFFFFull); }

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
        e = hipMemsetAsync(queue, 0, kRqQueueWords * sizeof(unsigned long long), stream);
        if (e != hipSuccess) return e;
        // no more wavefronts than there are chunks: the rest would only find the queue dry
        const uint32_t g = (uint32_t)min((unsigned long long)grid, ((unsigned long long)items + kOcChunk - 1u) / kOcChunk);
        occlusion_kernel<<<g, 64, 0, stream>>>(A, sf, o, items, samples, magic, seed, index_base, bias, queue, spill, PT_OC_FILL);
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
