// pt_expose.hip -- which triangles see the light unobstructed: one bit per triangle, computed once per tree
// version in front of a large PT_MODE_PATH launch.  The megakernel's shade pass adds the light term of a hit on such a triangle at
// once instead of tracing the shadow ray.  The arithmetic is pt_expose.h's, float64, shared with the host twin.
//
//   expose_prep_kernel   one thread per triangle: the triangles whose error factor as an occluder is above kKappaCap (slivers, and
//                        triangles nearly edge-on to the light whose |det| can still pass the test) go to a short list
//   expose_query_kernel  one thread per triangle T: every listed triangle, then a depth-first walk over the wide arena that enters a
//                        child whose LIVE f16 box, grown, reaches T's grown prism; at a leaf the exact clip test.  A query that runs
//                        out of its budget (nodes, leaves, stack) leaves T unflagged.  The walk answers for two tiers, which differ in
//                        the gate |n . d| a hit has to pass (ptex::kGate, kGate2) and so in one margin: the second flags a superset.
#include "pt_kernels.h"
#include "pt_bounds.h"
#include "pt_device.h"
#include "pt_expose.h"

namespace ptk {

namespace {

constexpr uint32_t kExBlock = 64;
constexpr int kExStack = 48;

__device__ __forceinline__ ptex::Tri ex_load_tri(const uint4* __restrict__ scene, uint32_t tri) {
    const uint4 a = scene[(size_t)tri * 4u], b = scene[(size_t)tri * 4u + 1u], c = scene[(size_t)tri * 4u + 2u];
    ptex::Tri t;
    t.v0[0] = __uint_as_float(a.x); t.e1[0] = __uint_as_float(a.y); t.e2[0] = __uint_as_float(a.z);
    t.v0[1] = __uint_as_float(b.x); t.e1[1] = __uint_as_float(b.y); t.e2[1] = __uint_as_float(b.z);
    t.v0[2] = __uint_as_float(c.x); t.e1[2] = __uint_as_float(c.y); t.e2[2] = __uint_as_float(c.z);
    return t;
}

__device__ __forceinline__ ptex::Light ex_light() { const F3 L = light_dir(); return ptex::make_light(L.x, L.y, L.z); }

__global__ __launch_bounds__(256) void expose_prep_kernel(const uint4* __restrict__ scene, uint32_t num_tris, uint32_t* __restrict__ info, uint32_t* __restrict__ bad) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= num_tris) return;
    const ptex::Light g = ex_light();
    const double k = ptex::kappa_of(ex_load_tri(scene, t), g);
    if (k < 0.0 || k <= ptex::kKappaCap) return;          // (a NaN is listed)
    const uint32_t at = atomicAdd(&info[kExposeBad], 1u);
    if (at < kExposeBadMax) bad[at] = t;
}

__global__ __launch_bounds__(kExBlock) void expose_query_kernel(const uint4* __restrict__ scene, uint32_t node_base16, uint32_t num_wide, uint32_t root_ref, uint32_t num_tris,
                                                                ptex::Bounds bounds, uint32_t node_budget, uint32_t leaf_budget,
                                                                uint32_t* __restrict__ info, const uint32_t* __restrict__ bad, uint32_t* __restrict__ mask, uint32_t first_only) {
    const uint32_t tri = blockIdx.x * kExBlock + threadIdx.x;
    bool exposed = false, exposed2 = false;
    if (tri < num_tris) {
        const ptex::Light g = ex_light();
        const uint4 nrm = scene[(size_t)tri * 4u + 3u];
        const float n32[3] = {__uint_as_float(nrm.x), __uint_as_float(nrm.y), __uint_as_float(nrm.z)};
        const ptex::Query q = ptex::make_query(ex_load_tri(scene, tri), n32, g, bounds, ptex::kGate);
        const double rho2 = ptex::rho_xy_at(q, bounds, ptex::kGate2);      // the second tier differs from the first in this one number
        const uint32_t n_bad = info[kExposeBad];
        // blocked: the first tier's answer; blocked2: the second's.  A candidate is tested for the second tier only when it blocks the first (or
        // the first is blocked already): the second tier's margins are the smaller ones, so blocked2 implies blocked by construction.
        bool blocked = !q.ok || n_bad > kExposeBadMax, blocked2 = blocked, gave_up = false;
        auto test = [&](const ptex::Tri& n) {
            if (!blocked) { blocked = ptex::blocks(q, q.rho_xy, n, g); if (!blocked) return; }
            blocked2 = ptex::blocks(q, rho2, n, g);
        };
        for (uint32_t i = 0; i < n_bad && !blocked2; ++i) test(ex_load_tri(scene, bad[i]));
        uint32_t stack[kExStack]; int sp = 0;
        uint32_t nodes = 0, leaves = 0;
        uint32_t cur = root_ref;
        bool have = !blocked2 && root_ref != kInvalidRef;
        // one walk for both tiers, its boxes culled with the first tier's (larger) margins: it goes on after the first tier is blocked until the
        // second is.  gave_up with the first tier blocked already is the second tier's alone.
        while (have && !blocked2) {
            if (cur & kLeaf) {
                const uint32_t n = (cur & 0x7fffffffu) >> 2;
                if (n < num_tris) {                      // (the record behind the last triangle is never hit)
                    if (++leaves > leaf_budget) { gave_up = true; break; }
                    test(ex_load_tri(scene, n));
                }
            } else {
                const uint32_t idx = (cur - node_base16) >> 2;
                if (cur < node_base16 || ((cur - node_base16) & 3u) || idx >= num_wide) { gave_up = true; break; }       // not a node of the arena
                if (++nodes > node_budget) { gave_up = true; break; }
                for (uint32_t s = 0; s < 4u; ++s) {
                    const uint4 piece = scene[(size_t)cur + s];
                    if (piece.w >= kDegenerateRef) continue;                  // empty, or entered by no ray
                    double mn[3], mx[3]; ptbd::unpack_box(piece.x, piece.y, piece.z, mn, mx);
                    if (!ptex::box_may_block(q, mn, mx, g)) continue;
                    if (sp >= kExStack) { gave_up = true; break; }
                    stack[sp++] = piece.w;
                }
                if (gave_up) break;
            }
            if (sp == 0) have = false; else cur = stack[--sp];
        }
        exposed = q.ok && !blocked && !gave_up;
        exposed2 = q.ok && !blocked2 && !gave_up;
        if (gave_up) atomicAdd(&info[blocked ? kExposeBudget2 : kExposeBudget], 1u);
        if (exposed) atomicAdd(&info[kExposeFlagged], 1u);
        if (exposed2) atomicAdd(&info[kExposeFlagged2], 1u);
    }
    // one wavefront = two words of each tier's mask, interleaved word by word (first tier, second tier: the shade pass fetches a triangle's two
    // words with one 8-byte load) and written whole, once as they are and once -- `first_only` bytes further on -- with the first tier's words in
    // both places: what a launch under "first tier only" (knob EXPOSE 5 / 6) is pointed at instead
    const unsigned long long m = __ballot(exposed), m2 = __ballot(exposed2);
    if (threadIdx.x == 0u) {
        const uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);
        uint4* both = (uint4*)mask + blockIdx.x;
        uint4* first = (uint4*)((char*)mask + first_only) + blockIdx.x;
        *both = make_uint4(lo, (uint32_t)m2, hi, (uint32_t)(m2 >> 32));
        *first = make_uint4(lo, lo, hi, hi);
    }
}

} // namespace

uint32_t expose_mask_words(uint32_t num_tris) { return ((num_tris + kExBlock - 1u) / kExBlock) * 2u; }
uint64_t expose_first_only_offset(uint32_t num_tris) { return ((uint64_t(expose_mask_words(num_tris)) * 8u + 65535u) / 65536u) * 65536u; }
uint64_t expose_mask_bytes(uint32_t num_tris) { return expose_first_only_offset(num_tris) + ((uint64_t(expose_mask_words(num_tris)) * 8u + 63u) / 64u) * 64u; }

hipError_t launch_expose(const uint4* scene, uint32_t node_base16, uint32_t num_wide, uint32_t root_ref, uint32_t num_tris, double s_max, double d_max,
                         uint32_t node_budget, uint32_t leaf_budget, uint32_t* info, uint32_t* bad, uint32_t* mask, hipStream_t stream) {
    if (num_tris == 0u) return hipSuccess;
    hipError_t e = hipMemsetAsync(info, 0, kExposeInfoWords * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(expose_prep_kernel, dim3((num_tris + 255u) / 256u), dim3(256), 0, stream, scene, num_tris, info, bad);
    ptex::Bounds b; b.s_max = s_max; b.d_max = d_max;
    hipLaunchKernelGGL(expose_query_kernel, dim3((num_tris + kExBlock - 1u) / kExBlock), dim3(kExBlock), 0, stream, scene, node_base16, num_wide, root_ref, num_tris, b,
                       node_budget, leaf_budget, info, bad, mask, (uint32_t)expose_first_only_offset(num_tris));
    return hipGetLastError();
}

} // namespace ptk
