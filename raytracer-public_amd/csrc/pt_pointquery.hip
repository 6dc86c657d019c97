// pt_pointquery.hip -- batched closest-point queries over the context's tree (include/mi355pt.h: pt_closest_points):
//   * closest_points_kernel               the default: persistent wavefronts, one point per lane, a lane whose point is answered takes the
//                                         next point of its wavefront's chunk (64 points per queue claim)
//   * closest_points_simple_kernel<STATS> one point per thread with a private 64-entry stack: PT_CLOSEST_SIMPLE_KERNEL, PT_CLOSEST_STATS
//   * closest_points_brute_kernel         every triangle in index order, the records streamed through LDS: PT_CLOSEST_BRUTE_FORCE
//
// The walk is the ray queries' (pt_rayquery.hip, pt_device.h::traverse) with bound2, a squared lower bound of the distance from the point to
// a child's box, in place of tmin: children with bound2 < best2 keep slot order, the first minimum trades places with the first of them and is
// entered next, the others are pushed far -> near, a push at 64 entries is dropped, a stacked child is re-validated at pop.  The
// point-triangle arithmetic is pt_closest.h, shared with the host twin (pt_host.cpp::closest_points), which gives the same bits.
// Records: PtPoint = one float4 (p.xyz, r_max), PtClosest = one uint4 (dist bits, prim, u bits, v bits).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_kernels.h"
#include "pt_device.h"
#include "pt_closest.h"

namespace ptk {

constexpr int kPqShort = PT_PQ_SHORT_STACK;     // LDS stack entries per lane; entries from this depth on live in the spill area
constexpr uint32_t kPqChunk = 64;               // points per queue claim: one per lane of the claiming wavefront
constexpr uint32_t kPqXcds = 8;                 // chunk ranges with a queue counter each (MI355X: 8 XCDs)
constexpr uint32_t kPqQueueStride = 32;         // counters 256 bytes apart
constexpr uint32_t kInfBits = 0x7F800000u;

// p +- s, once per point: the box test subtracts them from the packed halves
struct PointSlack { F3 hi, lo; };
__device__ __forceinline__ PointSlack point_slack(F3 p) {
    PointSlack s;
    s.hi = f3(p.x + ptcp::kSlack, p.y + ptcp::kSlack, p.z + ptcp::kSlack);
    s.lo = f3(p.x - ptcp::kSlack, p.y - ptcp::kSlack, p.z - ptcp::kSlack);
    return s;
}
// o - float(low / high half of w) in one instruction: fma(h, -1.0, o), the f32 subtraction (one rounding of the exact difference)
__device__ __forceinline__ float minus_half_lo(float o, uint32_t w) { float r; asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(w), "v"(o)); return r; }
__device__ __forceinline__ float minus_half_hi(float o, uint32_t w) { float r; asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(w), "v"(o)); return r; }
// bound2 of one packed f16 box (w0 = mn.x | mn.y << 16, w1 = mn.z | mx.x << 16, w2 = mx.y | mx.z << 16): per axis
// g = max(mn - (p + s), (p - s) - mx, 0), three instructions straight from the packed halves (v_fma_mix_f32 twice, v_max3_f32).
// The inverted box of an empty or degenerate slot (mn = +inf) gives +inf, which is below no best2.  v_max ignores a NaN operand.
__device__ __forceinline__ float box_bound2(const PointSlack& s, uint32_t w0, uint32_t w1, uint32_t w2) {
    const float gx = wmax(wmax(half_lo_minus(w0, s.hi.x), minus_half_hi(s.lo.x, w1)), 0.0f);
    const float gy = wmax(wmax(half_hi_minus(w0, s.hi.y), minus_half_lo(s.lo.y, w2)), 0.0f);
    const float gz = wmax(wmax(half_lo_minus(w1, s.hi.z), minus_half_hi(s.lo.z, w2)), 0.0f);
    return (gx * gx + gy * gy) + gz * gz;
}

__device__ __forceinline__ void load_point(const float4* __restrict__ pts, uint32_t i, F3& p, float& rmax) {
    const float4 a = pts[i];
    p = f3(a.x, a.y, a.z); rmax = a.w;
}
// d2 of one triangle record (three axis-major pieces: v0[a], e1[a], e2[a])
__device__ __forceinline__ float tri_d2(F3 p, const float4 a, const float4 b, const float4 c) {
    const float ax = p.x - a.x, ay = p.y - b.x, az = p.z - c.x;
    float u, v;
    ptcp::closest_uv(ax, ay, az, a.y, b.y, c.y, a.z, b.z, c.z, u, v);
    return ptcp::closest_d2(ax, ay, az, a.y, b.y, c.y, a.z, b.z, c.z, u, v);
}
// The 16-byte result: dist = sqrtf(best2), u and v recomputed from the winning triangle's record with the operations of the accepted test
__device__ __forceinline__ uint4 closest_record(const float4* __restrict__ tris, F3 p, float best2, uint32_t tri) {
    if (tri == kInvalidRef) return make_uint4(kInfBits, kInvalidRef, 0u, 0u);
    const float4* tp = tris + (size_t)tri * 4;
    const float4 a = tp[0], b = tp[1], c = tp[2];
    float u, v;
    ptcp::closest_uv(p.x - a.x, p.y - b.x, p.z - c.x, a.y, b.y, c.y, a.z, b.z, c.z, u, v);
    return make_uint4(__float_as_uint(sqrtf(best2)), tri, __float_as_uint(u), __float_as_uint(v));
}
__device__ __forceinline__ uint4 as_uint4(const float4 f) { return make_uint4(__float_as_uint(f.x), __float_as_uint(f.y), __float_as_uint(f.z), __float_as_uint(f.w)); }
__device__ __forceinline__ float4 as_float4(const uint4 u) { return make_float4(__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w)); }

// ------------------------------------------------------------------------------------
// simple kernel: one point per thread, a private 64-entry stack; the counters of PT_CLOSEST_STATS by the rules of traverse<..., STATS>
// ------------------------------------------------------------------------------------
template <bool STATS>
__device__ __forceinline__ void walk_point(const RenderArgs& A, F3 p, float& best2, uint32_t& best_tri, uint2* __restrict__ stk, Counters& cnt) {
    best_tri = kInvalidRef;
    if (A.root_ref == kInvalidRef || A.num_tris == 0u) return;
    if (STATS) { cnt.nodes += 1; if (cnt.maxstack < 1u) cnt.maxstack = 1u; }      // the root record is fetched before its degenerate check
    if (A.root_degenerate) return;
    const PointSlack s = point_slack(p);
    if (!(box_bound2(s, A.root_box[0], A.root_box[1], A.root_box[2]) < best2)) return;
    uint32_t cur = A.root_ref;
    int sp = 0;
    for (;;) {
        bool need_pop = false;
        if (cur & kLeaf) {
            const uint32_t ti4 = cur & 0x7fffffffu;
            if (ti4 < 4u * A.num_tris) {                          // an out-of-range leaf points at the record behind the last triangle: skipped
                const float4* tp = (const float4*)arena_record(A, cur);
                if (STATS) cnt.tris += 1;
                const float d2 = tri_d2(p, tp[0], tp[1], tp[2]);
                if (d2 < best2) { best2 = d2; best_tri = ti4 >> 2; }
            }
            need_pop = true;
        } else {
            const uint4* np = arena_record(A, cur);
            const uint4 n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3];
            const uint32_t r0 = n0.w, r1 = n1.w, r2 = n2.w, r3 = n3.w;
            const float t0 = box_bound2(s, n0.x, n0.y, n0.z), t1 = box_bound2(s, n1.x, n1.y, n1.z);
            const float t2 = box_bound2(s, n2.x, n2.y, n2.z), t3 = box_bound2(s, n3.x, n3.y, n3.z);
            const bool h0 = t0 < best2, h1 = t1 < best2, h2 = t2 < best2, h3 = t3 < best2;
            if (STATS) cnt.nodes += (r0 != kInvalidRef) + (r1 != kInvalidRef) + (r2 != kInvalidRef) + (r3 != kInvalidRef);
            int nslot = -1, fslot = -1; float tn = 0.0f, tf = 0.0f; uint32_t rn = kInvalidRef, rf = kInvalidRef;
            if (h0) { nslot = 0; tn = t0; rn = r0; fslot = 0; tf = t0; rf = r0; }
            if (h1) { if (nslot < 0 || t1 < tn) { nslot = 1; tn = t1; rn = r1; } if (fslot < 0) { fslot = 1; tf = t1; rf = r1; } }
            if (h2) { if (nslot < 0 || t2 < tn) { nslot = 2; tn = t2; rn = r2; } if (fslot < 0) { fslot = 2; tf = t2; rf = r2; } }
            if (h3) { if (nslot < 0 || t3 < tn) { nslot = 3; tn = t3; rn = r3; } if (fslot < 0) { fslot = 3; tf = t3; rf = r3; } }
            if (nslot < 0) {
                need_pop = true;
            } else {
#define PT_PUSH(REF, B2) do { if (sp < kStackMax) { stk[sp] = make_uint2((REF), __float_as_uint(B2)); ++sp; } else if (STATS) { cnt.drops += 1; } } while (0)
                if (h3) { if (nslot == 3) { if (fslot != 3) PT_PUSH(rf, tf); } else if (fslot != 3) PT_PUSH(r3, t3); }
                if (h2) { if (nslot == 2) { if (fslot != 2) PT_PUSH(rf, tf); } else if (fslot != 2) PT_PUSH(r2, t2); }
                if (h1) { if (nslot == 1) { if (fslot != 1) PT_PUSH(rf, tf); } else if (fslot != 1) PT_PUSH(r1, t1); }
#undef PT_PUSH
                if (STATS) { const uint32_t depth = (uint32_t)sp + (sp < kStackMax ? 1u : 0u); if (depth > cnt.maxstack) cnt.maxstack = depth; }
                if (sp < kStackMax) cur = rn;          // the push of the nearest child would have fitted
                else { need_pop = true; if (STATS) cnt.drops += 1; }
            }
        }
        if (need_pop) {
            bool found = false;
            while (sp > 0) {
                --sp;
                const uint2 e = stk[sp];
                if (__uint_as_float(e.y) < best2) { cur = e.x; found = true; break; }
            }
            if (!found) break;
        }
    }
}

__device__ __forceinline__ void add_stats(const RenderArgs& A, uint32_t n_pts, const Counters& cnt) {
    uint32_t n = n_pts, nodes = cnt.nodes, tris = cnt.tris, drops = cnt.drops, maxstack = cnt.maxstack;
    for (int off = 32; off > 0; off >>= 1) {
        n += __shfl_xor(n, off, 64); nodes += __shfl_xor(nodes, off, 64); tris += __shfl_xor(tris, off, 64);
        drops += __shfl_xor(drops, off, 64); maxstack = max(maxstack, (uint32_t)__shfl_xor(maxstack, off, 64));
    }
    if ((threadIdx.x & 63u) == 0u) {
        atomicAdd(&A.stats[0], (unsigned long long)n);
        atomicAdd(&A.stats[2], (unsigned long long)nodes);
        atomicAdd(&A.stats[3], (unsigned long long)tris);
        atomicAdd(&A.stats[4], (unsigned long long)drops);
        atomicMax(&A.stats[5], (unsigned long long)maxstack);
    }
}

template <bool STATS>
__global__ __launch_bounds__(256) void closest_points_simple_kernel(const RenderArgs A, const float4* __restrict__ pts, uint4* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    Counters cnt; cnt.nodes = cnt.tris = cnt.drops = cnt.maxstack = 0;
    uint32_t n_pts = 0;
    if (i < n) {
        F3 p; float rmax;
        load_point(pts, i, p, rmax);
        float best2 = rmax * rmax; uint32_t tri = kInvalidRef;
        n_pts = 1;
        if (ptcp::point_walked(p.x, p.y, p.z, rmax)) {
            uint2 stk[kStackMax];
            walk_point<STATS>(A, p, best2, tri, stk, cnt);
        }
        out[i] = closest_record(A.tris, p, best2, tri);
    }
    if (STATS) add_stats(A, n_pts, cnt);
}

// ------------------------------------------------------------------------------------
// persistent kernel: one wavefront per workgroup, one point per lane, lanes refilled from the wavefront's chunk
// ------------------------------------------------------------------------------------
// A step is the unified 64 B arena fetch (four child pieces of a wide node, or a triangle record) followed by bound2 of the four children or
// the point-triangle test.  The stack is (bound2 bits << 32 | reference): entries 0 .. kPqShort-1 in LDS, one column per lane, deeper
// entries in the spill area at [entry - kPqShort][grid lane].  Queue, chunks and refill are trace_rays_kernel's (pt_rayquery.hip): the
// chunks are split into kPqXcds ranges with a counter each, a wavefront claims from the range of its XCD, one chunk ahead, and moves on to
// the next range when that one is used up; idle lanes take the next points of the chunk in lane order when `fill` of them are idle.
__global__ __launch_bounds__(64) void closest_points_kernel(const RenderArgs A, const float4* __restrict__ pts, uint4* __restrict__ out, uint32_t n,
                                                            unsigned long long* __restrict__ queue, unsigned long long* __restrict__ spill, uint32_t fill) {
    __shared__ unsigned long long lds_stack[kPqShort][64];
    const uint32_t lane = threadIdx.x;
    unsigned long long* const stk = &lds_stack[0][lane];
    const size_t grid_lanes = (size_t)gridDim.x * 64u, my_lane = (size_t)blockIdx.x * 64u + lane;
    const bool scene_ok = !(A.root_ref == kInvalidRef || A.num_tris == 0u || A.root_degenerate != 0u);
    const uint32_t leaf_end = 4u * A.num_tris;

    const uint32_t chunks = (uint32_t)(((unsigned long long)n + kPqChunk - 1u) / kPqChunk), per_xcd = (chunks + kPqXcds - 1u) / kPqXcds;
    uint32_t xcd = (uint32_t)__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & (kPqXcds - 1u), hops = 0;
    unsigned long long ahead = 0;                         // lane 0: the claimed next chunk of range `xcd`
    if (lane == 0u) ahead = atomicAdd(&queue[xcd * kPqQueueStride], 1ull);
    uint32_t next = 0, end = 0; bool dry = false;
    bool trav = false;                                    // this lane walks a point
    uint32_t rid = 0, cur = 0, btri = kInvalidRef; int sp = 0; float best2 = 0.0f;
    F3 p = f3(0, 0, 0); PointSlack s = point_slack(p);

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
                        if (++hops >= kPqXcds) { dry = true; break; }
                        xcd = (xcd + 1u) & (kPqXcds - 1u);
                        unsigned long long seen = 0;      // a plain read first: a range that is used up costs no claim
                        if (lane == 0u) seen = __hip_atomic_load(&queue[xcd * kPqQueueStride], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        c = __shfl(seen, 0, 64);
                        if (used_up(xcd, c)) continue;
                        if (lane == 0u) ahead = atomicAdd(&queue[xcd * kPqQueueStride], 1ull);
                        c = __shfl(ahead, 0, 64);
                    }
                    if (dry) break;
                    if (lane == 0u) ahead = atomicAdd(&queue[xcd * kPqQueueStride], 1ull);
                    const uint32_t chunk = xcd * per_xcd + (uint32_t)c;
                    next = chunk * kPqChunk; end = (uint32_t)min((unsigned long long)next + kPqChunk, (unsigned long long)n);
                }
                const uint32_t take = min((uint32_t)__popcll(idle), end - next);
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
                if (!trav && rank < take) {
                    rid = next + rank;
                    float rmax;
                    load_point(pts, rid, p, rmax);
                    best2 = rmax * rmax; btri = kInvalidRef; sp = 0;
                    s = point_slack(p);
                    if (scene_ok && ptcp::point_walked(p.x, p.y, p.z, rmax) && box_bound2(s, A.root_box[0], A.root_box[1], A.root_box[2]) < best2) { cur = A.root_ref; trav = true; }
                    else out[rid] = make_uint4(kInfBits, kInvalidRef, 0u, 0u);
                }
                next += take;
                idle = __ballot(!trav);
            }
            if (idle == ~0ull) break;                     // the queue is dry and nothing is walked
        }
        if (!trav) continue;
        const uint4* np = arena_record(A, cur);
        const uint4 n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3];
        bool need_pop = true;
        if (cur & kLeaf) {
            const float d2 = tri_d2(p, as_float4(n0), as_float4(n1), as_float4(n2));
            if (((cur & 0x7fffffffu) < leaf_end) & (d2 < best2)) { best2 = d2; btri = cur; }
        } else {
            const uint32_t r0 = n0.w, r1 = n1.w, r2 = n2.w, r3 = n3.w;
            const float t0 = box_bound2(s, n0.x, n0.y, n0.z), t1 = box_bound2(s, n1.x, n1.y, n1.z);
            const float t2 = box_bound2(s, n2.x, n2.y, n2.z), t3 = box_bound2(s, n3.x, n3.y, n3.z);
            const bool h0 = t0 < best2, h1 = t1 < best2, h2 = t2 < best2, h3 = t3 < best2;
            int nslot = -1, fslot = -1; float tn = 0.0f, tf = 0.0f; uint32_t rn = kInvalidRef, rf = kInvalidRef;
            if (h0) { nslot = 0; tn = t0; rn = r0; fslot = 0; tf = t0; rf = r0; }
            if (h1) { if (nslot < 0 || t1 < tn) { nslot = 1; tn = t1; rn = r1; } if (fslot < 0) { fslot = 1; tf = t1; rf = r1; } }
            if (h2) { if (nslot < 0 || t2 < tn) { nslot = 2; tn = t2; rn = r2; } if (fslot < 0) { fslot = 2; tf = t2; rf = r2; } }
            if (h3) { if (nslot < 0 || t3 < tn) { nslot = 3; tn = t3; rn = r3; } if (fslot < 0) { fslot = 3; tf = t3; rf = r3; } }
            if (nslot >= 0) {
                auto push = [&](uint32_t ref, float b2) __attribute__((always_inline)) {
                    if (sp < kStackMax) {
                        const unsigned long long e = ((unsigned long long)__float_as_uint(b2) << 32) | ref;
                        if (__builtin_expect(sp < kPqShort, 1)) stk[sp * 64] = e;
                        else spill[(size_t)(sp - kPqShort) * grid_lanes + my_lane] = e;
                        ++sp;
                    }
                };
                if (h3) { if (nslot == 3) { if (fslot != 3) push(rf, tf); } else if (fslot != 3) push(r3, t3); }
                if (h2) { if (nslot == 2) { if (fslot != 2) push(rf, tf); } else if (fslot != 2) push(r2, t2); }
                if (h1) { if (nslot == 1) { if (fslot != 1) push(rf, tf); } else if (fslot != 1) push(r1, t1); }
                if (sp < kStackMax) { cur = rn; need_pop = false; }       // the push of the nearest child would have fitted
            }
        }
        if (need_pop) {
            bool found = false;
            while (sp > 0) {
                --sp;
                const unsigned long long e = sp < kPqShort ? stk[sp * 64] : spill[(size_t)(sp - kPqShort) * grid_lanes + my_lane];
                if (__uint_as_float((uint32_t)(e >> 32)) < best2) { cur = (uint32_t)e; found = true; break; }
            }
            if (!found) {
                out[rid] = closest_record(A.tris, p, best2, btri == kInvalidRef ? kInvalidRef : (btri & 0x7fffffffu) >> 2);
                trav = false;
            }
        }
    }
}

// ------------------------------------------------------------------------------------
// brute force: one point per thread, every triangle in index order; a workgroup streams the records through LDS, kBruteTile at a time
// ------------------------------------------------------------------------------------
constexpr uint32_t kBruteTile = 256;
template <bool STATS>
__global__ __launch_bounds__(256) void closest_points_brute_kernel(const RenderArgs A, const float4* __restrict__ pts, uint4* __restrict__ out, uint32_t n) {
    __shared__ float4 rec[kBruteTile][3];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    F3 p = f3(0, 0, 0); float rmax = 0.0f;
    if (i < n) load_point(pts, i, p, rmax);
    const bool walked = (i < n) && ptcp::point_walked(p.x, p.y, p.z, rmax);
    float best2 = rmax * rmax; uint32_t tri = kInvalidRef;
    Counters cnt; cnt.nodes = cnt.tris = cnt.drops = cnt.maxstack = 0;
    for (uint32_t base = 0; base < A.num_tris; base += kBruteTile) {
        const uint32_t count = min(kBruteTile, A.num_tris - base);
        __syncthreads();
        if (threadIdx.x < count) {
            const float4* tp = A.tris + (size_t)(base + threadIdx.x) * 4;
            rec[threadIdx.x][0] = tp[0]; rec[threadIdx.x][1] = tp[1]; rec[threadIdx.x][2] = tp[2];
        }
        __syncthreads();
        if (walked) {
            for (uint32_t k = 0; k < count; ++k) {
                const float d2 = tri_d2(p, rec[k][0], rec[k][1], rec[k][2]);
                if (d2 < best2) { best2 = d2; tri = base + k; }
            }
            if (STATS) cnt.tris += count;
        }
    }
    if (i < n) out[i] = closest_record(A.tris, p, best2, tri);
    if (STATS) add_stats(A, i < n ? 1u : 0u, cnt);
}

static_assert(kRqQueueWords == kPqXcds * kPqQueueStride, "pt_kernels.h: the queue block holds one counter line per range");
uint32_t pointquery_grid(int num_cus) { return (uint32_t)num_cus * 4u * PT_PQ_WAVES_PER_SIMD; }
size_t pointquery_spill_entries(uint32_t grid) { return (size_t)(kStackMax - kPqShort) * grid * 64u; }

hipError_t launch_closest_points(const RenderArgs& A, const void* points, void* out, uint32_t n, bool simple, bool stats, bool brute,
                                 unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    const float4* p = (const float4*)points; uint4* o = (uint4*)out;
    const dim3 g256((n + 255u) / 256u);
    if (brute) {
        if (stats) closest_points_brute_kernel<true><<<g256, 256, 0, stream>>>(A, p, o, n);
        else closest_points_brute_kernel<false><<<g256, 256, 0, stream>>>(A, p, o, n);
        return hipGetLastError();
    }
    if (simple || stats) {
        if (stats) closest_points_simple_kernel<true><<<g256, 256, 0, stream>>>(A, p, o, n);
        else closest_points_simple_kernel<false><<<g256, 256, 0, stream>>>(A, p, o, n);
        return hipGetLastError();
    }
    hipError_t e = hipMemsetAsync(queue, 0, kRqQueueWords * sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    // no more wavefronts than there are chunks: the rest would only find the queue dry
    const uint32_t g = (uint32_t)min((unsigned long long)grid, ((unsigned long long)n + kPqChunk - 1u) / kPqChunk);
    closest_points_kernel<<<g, 64, 0, stream>>>(A, p, o, n, queue, spill, PT_PQ_FILL);
    return hipGetLastError();
}

} // namespace ptk
