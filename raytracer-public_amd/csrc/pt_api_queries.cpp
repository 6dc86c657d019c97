// pt_api_queries.cpp -- the batched queries over the context's tree (include/mi355pt.h): closest hit / any hit, closest point,
// occlusion, crossing counts, containment, signed distance, radius count / search, box count / search, triangle count / search, hit lists, k-nearest and sphere casts, with the host twins
// (*_bvh4) next to them.
#include "pt_context.h"

#include <algorithm>
#include <initializer_list>

using namespace pti;

// ---- what every query shares ------------------------------------------------------------------------------------------------------
namespace {

// The pieces of the argument checks.  Each check_* below is a list of them in the order that decides which error a caller sees:
// arguments (PT_ERR_INVALID_ARG) before the scene (PT_ERR_NO_SCENE).
bool aligned4(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 3u) == 0u; }
bool aligned8(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 7u) == 0u; }
bool aligned16(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 15u) == 0u; }
int bad_arg(PtContext* ctx, const char* fn, const std::string& what) { return fail(ctx, PT_ERR_INVALID_ARG, std::string(fn) + ": " + what); }
int check_flags(PtContext* ctx, const char* fn, uint32_t flags, uint32_t known) { return (flags & ~known) ? bad_arg(ctx, fn, "unknown flags") : PT_OK; }
int check_n(PtContext* ctx, const char* fn, uint64_t n, const char* noun) {
    return n > 0xFFFFFFFFull ? bad_arg(ctx, fn, std::string("more than 2^32 - 1 ") + noun) : PT_OK;
}
// `what` names the record arrays `ptrs`: each non-null and 16-byte aligned
int check_records(PtContext* ctx, const char* fn, const char* what, std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs) if (!aligned16(p)) return bad_arg(ctx, fn, std::string(what) + " must be non-null and 16-byte aligned");
    return PT_OK;
}
int check_counts(PtContext* ctx, const char* fn, const void* counts) {
    return aligned4(counts) ? PT_OK : bad_arg(ctx, fn, "counts must be non-null and 4-byte aligned");
}
// the outputs of a list query: n + 1 offsets, and `capacity` entries called `noun`
int check_list(PtContext* ctx, const char* fn, const void* offsets, const void* entries, uint64_t capacity, const char* noun) {
    if (!aligned8(offsets)) return bad_arg(ctx, fn, "offsets must be non-null and 8-byte aligned");
    if (capacity ? !aligned16(entries) : (entries && !aligned16(entries))) return bad_arg(ctx, fn, std::string(noun) + " must be 16-byte aligned, and non-null unless capacity is 0");
    return PT_OK;
}
int check_scene(PtContext* ctx, const char* fn) {
    if (!ctx->have_tris || !ctx->have_bvh) return fail(ctx, PT_ERR_NO_SCENE, std::string(fn) + ": scene not set (triangles + BVH)");
    return PT_OK;
}

// One walk of the tree on the context's stream, behind whatever pt_set_batch still holds.  begin_walk leaves `launch` false when there is
// nothing to launch (n = 0; a pending batch is flushed all the same).  Else it fills the arguments from the scene and the grid from
// `waves_per_simd`; with `stats` it arms the counters, and else, with `persistent` (no simple kernel, no brute force), it sees to the queue
// block and the spill area of the persistent kernels (pt_walk.h).  Every query shares those two: the launches are ordered by the stream, and
// DevBuf::ensure only ever grows a buffer, so the area fits whichever kernel asked for most.
struct Walk { ptk::RenderArgs A; uint32_t grid = 0; bool launch = false, stats = false; };

int begin_walk(PtContext* ctx, uint32_t n, uint32_t waves_per_simd, int short_stack, bool stats, bool persistent, Walk& W) {
    if (int rc = flush_pending(ctx)) return rc;
    if (n == 0u) return PT_OK;
    if (int rc = sync_refit_meta(ctx)) return rc;
    ptk::RenderArgs& A = W.A; std::memset(&A, 0, sizeof(A));
    A.nodes = ctx->wide(); A.tris = ctx->trirec(); A.scene = ctx->d_scene.ptr; A.node_off = uint32_t(ctx->node_off);
    A.num_tris = ctx->num_tris; A.tri_gate = 0xFFFFFFFFu;
    A.root_ref = ctx->wide_meta.root_ref; std::memcpy(A.root_box, ctx->wide_meta.root_box, 12);
    A.root_degenerate = ctx->wide_meta.root_degenerate ? 1u : 0u;
    W.grid = ptk::walk_grid(ctx->num_cus, waves_per_simd);
    if (stats) {
        ctx->stats_culled = 0;
        PT_HIP(ctx, hipMemsetAsync(ctx->d_stats.ptr, 0, 24 * sizeof(unsigned long long), ctx->stream));
        A.stats = ctx->d_stats.ptr;
    } else if (persistent) {
        PT_HIP(ctx, ctx->d_rq_queue.ensure(ptk::kRqQueueWords));
        PT_HIP(ctx, ctx->d_rq_spill.ensure(ptk::walk_spill_entries(W.grid, short_stack)));
    }
    W.launch = true; W.stats = stats;
    return PT_OK;
}
int end_walk(PtContext* ctx, const Walk& W) {
    if (W.stats) ctx->last_stats = true;
    return PT_OK;
}

// The staged round trip of a *_host form: n records of `in_bytes` each into the context's staging buffer, `run(staged in, staged out)` --
// the query's *_on_stream -- on them, n records of `out_bytes` each from `d_out` back to `out`, and the one host wait.
template <typename T, typename Run>
int staged(PtContext* ctx, uint64_t n, const void* in, size_t in_bytes, DevBuf<T>& d_out, void* out, size_t out_bytes, Run run) {
    if (int rc = flush_pending(ctx)) return rc;
    if (n == 0) return PT_OK;
    PT_HIP(ctx, ctx->d_rq_rays.ensure(size_t(n) * in_bytes / sizeof(uint4))); PT_HIP(ctx, d_out.ensure((size_t(n) * out_bytes + sizeof(T) - 1) / sizeof(T)));
    PT_HIP(ctx, hipMemcpyAsync(ctx->d_rq_rays.ptr, in, size_t(n) * in_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = run(ctx->d_rq_rays.ptr, d_out.ptr)) return rc;
    PT_HIP(ctx, hipMemcpyAsync(out, d_out.ptr, size_t(n) * out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PT_OK;
}

void stats_from(PtStats* stats, const uint64_t counters[5]) {
    std::memset(stats, 0, sizeof(*stats));
    stats->rays_closest = counters[0]; stats->nodes_examined = counters[1]; stats->tris_tested = counters[2];
    stats->stack_drops = counters[3]; stats->max_stack = counters[4];
}

} // namespace

extern "C" {

// ---- batched ray queries (include/mi355pt.h; pt_rayquery.hip) ----------------------------------------------------------------

static_assert(sizeof(PtRay) == 32 && sizeof(PtHit) == 16, "PtRay / PtHit are read and written as 2 x 16 B and 16 B records");

namespace {
constexpr uint32_t kTraceFlags = PT_TRACE_ANY_HIT | PT_TRACE_STATS | PT_TRACE_SIMPLE_KERNEL;

// arguments, then the scene
int check_trace(PtContext* ctx, const char* fn, const void* rays, uint64_t n, uint32_t flags, const void* hits) {
    if (int rc = check_flags(ctx, fn, flags, kTraceFlags)) return rc;
    if (int rc = check_n(ctx, fn, n, "rays")) return rc;
    if (int rc = check_records(ctx, fn, "rays and hits", {rays, hits})) return rc;
    return check_scene(ctx, fn);
}

// the launch itself: rays / hits in device memory
int trace_on_stream(PtContext* ctx, const void* rays, uint32_t n, uint32_t flags, void* hits) {
    const bool anyhit = (flags & PT_TRACE_ANY_HIT) != 0, stats = (flags & PT_TRACE_STATS) != 0, simple = (flags & PT_TRACE_SIMPLE_KERNEL) != 0;
    Walk W;
    if (int rc = begin_walk(ctx, n, PT_RQ_WAVES_PER_SIMD, PT_RQ_SHORT_STACK, stats, !simple, W)) return rc;
    if (W.launch) PT_HIP(ctx, ptk::launch_trace_rays(W.A, rays, hits, n, anyhit, simple, stats, ctx->d_rq_queue.ptr, ctx->d_rq_spill.ptr, W.grid, ctx->stream));
    return end_walk(ctx, W);
}
} // namespace

int pt_trace_rays(PtContext* ctx, const void* rays_device, uint64_t n, uint32_t flags, void* hits_device) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_trace(ctx, "pt_trace_rays", rays_device, n, flags, hits_device)) return rc;
    return trace_on_stream(ctx, rays_device, uint32_t(n), flags, hits_device);
}

int pt_trace_rays_host(PtContext* ctx, const PtRay* rays, uint64_t n, uint32_t flags, PtHit* hits) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_trace(ctx, "pt_trace_rays_host", rays, n, flags, hits)) return rc;
    return staged(ctx, n, rays, sizeof(PtRay), ctx->d_rq_hits, hits, sizeof(PtHit),
                  [&](const void* d_in, void* d_out) { return trace_on_stream(ctx, d_in, uint32_t(n), flags, d_out); });
}

int pt_camera_rays(PtContext* ctx, const PtRenderParams* p, void* rays_device) {
    if (int rc = bind(ctx)) return rc;
    if (!p) return bad_arg(ctx, "pt_camera_rays", "null params");
    if (int rc = check_records(ctx, "pt_camera_rays", "rays", {rays_device})) return rc;
    if (p->width == 0 || p->height == 0 || p->width > 32768 || p->height > 32768) return bad_arg(ctx, "pt_camera_rays", "bad resolution");
    if (int rc = flush_pending(ctx)) return rc;
    ptk::RenderArgs A; std::memset(&A, 0, sizeof(A));
    A.width = p->width; A.height = p->height; A.focal = p->focal; A.aspect = p->aspect;
    std::memcpy(A.cam, p->cam_pos, 12); std::memcpy(A.quat, p->cam_quat, 16);
    PT_HIP(ctx, ptk::launch_camera_rays(A, rays_device, ctx->stream));
    return PT_OK;
}

// ---- batched closest-point queries (include/mi355pt.h; pt_pointquery.hip) -----------------------------------------------------

static_assert(sizeof(PtPoint) == 16 && sizeof(PtClosest) == 16, "PtPoint / PtClosest are read and written as 16 B records");

namespace {
constexpr uint32_t kClosestFlags = PT_CLOSEST_STATS | PT_CLOSEST_SIMPLE_KERNEL | PT_CLOSEST_BRUTE_FORCE;

int check_closest(PtContext* ctx, const char* fn, const void* points, uint64_t n, uint32_t flags, const void* out) {
    if (int rc = check_flags(ctx, fn, flags, kClosestFlags)) return rc;
    if (int rc = check_n(ctx, fn, n, "points")) return rc;
    if (int rc = check_records(ctx, fn, "points and results", {points, out})) return rc;
    return check_scene(ctx, fn);
}

// the launch itself: points / results in device memory
int closest_on_stream(PtContext* ctx, const void* points, uint32_t n, uint32_t flags, void* out) {
    const bool stats = (flags & PT_CLOSEST_STATS) != 0, simple = (flags & PT_CLOSEST_SIMPLE_KERNEL) != 0, brute = (flags & PT_CLOSEST_BRUTE_FORCE) != 0;
    Walk W;
    if (int rc = begin_walk(ctx, n, PT_PQ_WAVES_PER_SIMD, PT_PQ_SHORT_STACK, stats, !simple && !brute, W)) return rc;
    if (W.launch) PT_HIP(ctx, ptk::launch_closest_points(W.A, points, out, n, simple, stats, brute, ctx->d_rq_queue.ptr, ctx->d_rq_spill.ptr, W.grid, ctx->stream));
    return end_walk(ctx, W);
}
} // namespace

int pt_closest_points(PtContext* ctx, const void* points_device, uint64_t n, uint32_t flags, void* out_device) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_closest(ctx, "pt_closest_points", points_device, n, flags, out_device)) return rc;
    return closest_on_stream(ctx, points_device, uint32_t(n), flags, out_device);
}

int pt_closest_points_host(PtContext* ctx, const PtPoint* points, uint64_t n, uint32_t flags, PtClosest* out) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_closest(ctx, "pt_closest_points_host", points, n, flags, out)) return rc;
    return staged(ctx, n, points, sizeof(PtPoint), ctx->d_rq_hits, out, sizeof(PtClosest),
                  [&](const void* d_in, void* d_out) { return closest_on_stream(ctx, d_in, uint32_t(n), flags, d_out); });
}

int pt_closest_points_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words,
                           const PtPoint* points, uint64_t n, uint32_t flags, PtClosest* out, PtStats* stats) {
    if (flags & ~kClosestFlags) return fail(nullptr, PT_ERR_INVALID_ARG, "pt_closest_points_bvh4: unknown flags");
    const bool brute = (flags & PT_CLOSEST_BRUTE_FORCE) != 0;
    if ((!tris && num_tris) || (n && (!points || !out)) || (!bvh4 && !brute)) return fail(nullptr, PT_ERR_INVALID_ARG, "pt_closest_points_bvh4: null pointer");
    if (n > 0xFFFFFFFFull) return fail(nullptr, PT_ERR_INVALID_ARG, "pt_closest_points_bvh4: more than 2^32 - 1 points");
    std::string err;
    uint64_t counters[5] = {0, 0, 0, 0, 0};
    if (!pt::closest_points(tris, num_tris, brute ? nullptr : bvh4, words, reinterpret_cast<const float*>(points), n,
                            reinterpret_cast<uint32_t*>(out), (flags & PT_CLOSEST_STATS) && stats ? counters : nullptr, err))
        return fail(nullptr, PT_ERR_BAD_BVH, err);
    if (stats) stats_from(stats, counters);
    return PT_OK;
}

// ---- sphere-cast queries (include/mi355pt.h; pt_sweep.hip) ---------------------------------------------------------------------

static_assert(sizeof(PtSweep) == 32, "PtSweep is read as 2 x 16 B");

namespace {
constexpr uint32_t kSweepFlags = PT_SWEEP_STATS | PT_SWEEP_SIMPLE_KERNEL | PT_SWEEP_BRUTE_FORCE;

int check_sweep(PtContext* ctx, const char* fn, const void* sweeps, uint64_t n, uint32_t flags, const void* hits) {
    if (int rc = check_flags(ctx, fn, flags, kSweepFlags)) return rc;
    if (int rc = check_n(ctx, fn, n, "sweeps")) return rc;
    if (int rc = check_records(ctx, fn, "sweeps and hits", {sweeps, hits})) return rc;
    return check_scene(ctx, fn);
}

// the launch itself: sweeps / hits in device memory
int sweep_on_stream(PtContext* ctx, const void* sweeps, uint32_t n, uint32_t flags, void* hits) {
    const bool stats = (flags & PT_SWEEP_STATS) != 0, simple = (flags & PT_SWEEP_SIMPLE_KERNEL) != 0, brute = (flags & PT_SWEEP_BRUTE_FORCE) != 0;
    Walk W;
    if (int rc = begin_walk(ctx, n, PT_SW_WAVES_PER_SIMD, PT_SW_SHORT_STACK, stats, !simple && !brute, W)) return rc;
    if (W.launch) PT_HIP(ctx, ptk::launch_sweep(W.A, sweeps, hits, n, simple, stats, brute, ctx->d_rq_queue.ptr, ctx->d_rq_spill.ptr, W.grid, ctx->stream));
    return end_walk(ctx, W);
}
} // namespace

int pt_sweep_spheres(PtContext* ctx, const void* sweeps_device, uint64_t n, uint32_t flags, void* hits_device) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_sweep(ctx, "pt_sweep_spheres", sweeps_device, n, flags, hits_device)) return rc;
    return sweep_on_stream(ctx, sweeps_device, uint32_t(n), flags, hits_device);
}

int pt_sweep_spheres_host(PtContext* ctx, const PtSweep* sweeps, uint64_t n, uint32_t flags, PtHit* hits) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_sweep(ctx, "pt_sweep_spheres_host", sweeps, n, flags, hits)) return rc;
    return staged(ctx, n, sweeps, sizeof(PtSweep), ctx->d_rq_hits, hits, sizeof(PtHit),
                  [&](const void* d_in, void* d_out) { return sweep_on_stream(ctx, d_in, uint32_t(n), flags, d_out); });
}

int pt_sweep_spheres_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words,
                          const PtSweep* sweeps, uint64_t n, uint32_t flags, PtHit* out, PtStats* stats) {
    if (flags & ~kSweepFlags) return fail(nullptr, PT_ERR_INVALID_ARG, "pt_sweep_spheres_bvh4: unknown flags");
    const bool brute = (flags & PT_SWEEP_BRUTE_FORCE) != 0;
    if ((!tris && num_tris) || (n && (!sweeps || !out)) || (!bvh4 && !brute)) return fail(nullptr, PT_ERR_INVALID_ARG, "pt_sweep_spheres_bvh4: null pointer");
    if (n > 0xFFFFFFFFull) return fail(nullptr, PT_ERR_INVALID_ARG, "pt_sweep_spheres_bvh4: more than 2^32 - 1 sweeps");
    std::string err;
    uint64_t counters[5] = {0, 0, 0, 0, 0};
    if (!pt::sweep_spheres(tris, num_tris, brute ? nullptr : bvh4, words, reinterpret_cast<const float*>(sweeps), n,
                           reinterpret_cast<uint32_t*>(out), (flags & PT_SWEEP_STATS) && stats ? counters : nullptr, err))
        return fail(nullptr, PT_ERR_BAD_BVH, err);
    if (stats) stats_from(stats, counters);
    return PT_OK;
}

// ---- batched ambient-occlusion queries (include/mi355pt.h; pt_occlusion.hip) --------------------------------------------------

static_assert(sizeof(PtSurfel) == 32 && sizeof(PtOcclusion) == 16, "PtSurfel / PtOcclusion are read and written as 2 x 16 B and 16 B records");

namespace {
constexpr uint32_t kOcclusionFlags = PT_OCCLUSION_STATS | PT_OCCLUSION_SIMPLE_KERNEL;

// the parameter block and the batch size; the pointers and the scene are checked by the callers (pointers before the scene)
int check_occlusion_params(PtContext* ctx, const char* fn, uint64_t n, const PtOcclusionParams* p) {
    if (!p) return bad_arg(ctx, fn, "null params");
    if (int rc = check_flags(ctx, fn, p->flags, kOcclusionFlags)) return rc;
    if (int rc = check_n(ctx, fn, n, "surfels")) return rc;
    if (p->samples < 1u || p->samples > 65536u) return bad_arg(ctx, fn, "samples must be 1..65536");
    if (int rc = check_n(ctx, fn, n * uint64_t(p->samples), "sample rays (n * samples)")) return rc;
    if (!(p->bias >= 0.0f)) return bad_arg(ctx, fn, "bias must be >= 0");
    return PT_OK;
}
int check_occlusion(PtContext* ctx, const char* fn, const void* surfels, uint64_t n, const PtOcclusionParams* p, const void* out, bool need_scene) {
    if (int rc = check_occlusion_params(ctx, fn, n, p)) return rc;
    if (int rc = check_records(ctx, fn, "surfels and results", {surfels, out})) return rc;
    return need_scene ? check_scene(ctx, fn) : PT_OK;
}

// the launch itself: surfels / results in device memory
int occlusion_on_stream(PtContext* ctx, const void* surfels, uint32_t n, const PtOcclusionParams& p, void* out) {
    const bool stats = (p.flags & PT_OCCLUSION_STATS) != 0, simple = (p.flags & PT_OCCLUSION_SIMPLE_KERNEL) != 0;
    Walk W;
    if (int rc = begin_walk(ctx, n, PT_OC_WAVES_PER_SIMD, PT_OC_SHORT_STACK, stats, !simple, W)) return rc;
    if (W.launch) PT_HIP(ctx, ptk::launch_occlusion(W.A, surfels, out, n, p.samples, p.seed, p.index_base, p.bias, simple, stats, ctx->d_rq_queue.ptr, ctx->d_rq_spill.ptr, W.grid, ctx->stream));
    return end_walk(ctx, W);
}
// rays and their hits in, surfels out: the batch size and the pointers, then the triangles (no tree is walked)
int check_surfels(PtContext* ctx, const char* fn, const void* rays, const void* hits, uint64_t n, const void* surfels) {
    if (int rc = check_n(ctx, fn, n, "rays")) return rc;
    if (int rc = check_records(ctx, fn, "rays, hits and surfels", {rays, hits, surfels})) return rc;
    if (!ctx->have_tris) return fail(ctx, PT_ERR_NO_SCENE, std::string(fn) + ": no triangles set");
    return PT_OK;
}
} // namespace

int pt_occlusion(PtContext* ctx, const void* surfels_device, uint64_t n, const PtOcclusionParams* params, void* out_device) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_occlusion(ctx, "pt_occlusion", surfels_device, n, params, out_device, true)) return rc;
    return occlusion_on_stream(ctx, surfels_device, uint32_t(n), *params, out_device);
}

int pt_occlusion_host(PtContext* ctx, const PtSurfel* surfels, uint64_t n, const PtOcclusionParams* params, PtOcclusion* out) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_occlusion(ctx, "pt_occlusion_host", surfels, n, params, out, true)) return rc;
    return staged(ctx, n, surfels, sizeof(PtSurfel), ctx->d_rq_hits, out, sizeof(PtOcclusion),
                  [&](const void* d_in, void* d_out) { return occlusion_on_stream(ctx, d_in, uint32_t(n), *params, d_out); });
}

int pt_occlusion_rays(PtContext* ctx, const void* surfels_device, uint64_t n, const PtOcclusionParams* params, void* rays_device) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_occlusion(ctx, "pt_occlusion_rays", surfels_device, n, params, rays_device, false)) return rc;
    if (int rc = flush_pending(ctx)) return rc;
    PT_HIP(ctx, ptk::launch_occlusion_rays(surfels_device, rays_device, uint32_t(n), params->samples, params->seed, params->index_base, params->bias, ctx->stream));
    return PT_OK;
}

int pt_occlusion_rays_host(const PtSurfel* surfels, uint64_t n, const PtOcclusionParams* params, PtRay* rays) {
    if (int rc = check_occlusion_params(nullptr, "pt_occlusion_rays_host", n, params)) return rc;
    if (n && (!surfels || !rays)) return fail(nullptr, PT_ERR_INVALID_ARG, "pt_occlusion_rays_host: null pointer");
    pt::occlusion_rays(reinterpret_cast<const float*>(surfels), n, params->samples, params->seed, params->index_base, params->bias, reinterpret_cast<float*>(rays));
    return PT_OK;
}

int pt_hit_surfels(PtContext* ctx, const void* rays_device, const void* hits_device, uint64_t n, float r_max, void* surfels_device) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_surfels(ctx, "pt_hit_surfels", rays_device, hits_device, n, surfels_device)) return rc;
    if (int rc = flush_pending(ctx)) return rc;
    if (n == 0) return PT_OK;
    ptk::RenderArgs A; std::memset(&A, 0, sizeof(A));
    A.tris = ctx->trirec(); A.num_tris = ctx->num_tris;
    PT_HIP(ctx, ptk::launch_hit_surfels(A, rays_device, hits_device, uint32_t(n), r_max, surfels_device, ctx->stream));
    return PT_OK;
}

int pt_hit_surfels_host(PtContext* ctx, const PtRay* rays, const PtHit* hits, uint64_t n, float r_max, PtSurfel* out) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_surfels(ctx, "pt_hit_surfels_host", rays, hits, n, out)) return rc;
    if (int rc = flush_pending(ctx)) return rc;
    if (n == 0) return PT_OK;
    PT_HIP(ctx, ctx->d_rq_rays.ensure(size_t(n) * 2)); PT_HIP(ctx, ctx->d_rq_hits.ensure(size_t(n))); PT_HIP(ctx, ctx->d_oc_surfels.ensure(size_t(n) * 2));
    PT_HIP(ctx, hipMemcpyAsync(ctx->d_rq_rays.ptr, rays, size_t(n) * sizeof(PtRay), hipMemcpyHostToDevice, ctx->stream));
    PT_HIP(ctx, hipMemcpyAsync(ctx->d_rq_hits.ptr, hits, size_t(n) * sizeof(PtHit), hipMemcpyHostToDevice, ctx->stream));
    ptk::RenderArgs A; std::memset(&A, 0, sizeof(A));
    A.tris = ctx->trirec(); A.num_tris = ctx->num_tris;
    PT_HIP(ctx, ptk::launch_hit_surfels(A, ctx->d_rq_rays.ptr, ctx->d_rq_hits.ptr, uint32_t(n), r_max, ctx->d_oc_surfels.ptr, ctx->stream));
    PT_HIP(ctx, hipMemcpyAsync(out, ctx->d_oc_surfels.ptr, size_t(n) * sizeof(PtSurfel), hipMemcpyDeviceToHost, ctx->stream));
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PT_OK;
}

// ---- crossing counts, containment, signed distance (include/mi355pt.h; pt_crossings.hip) ---------------------------------------

static_assert(sizeof(PtContainment) == 16 && sizeof(PtContainParams) == 16, "PtContainment is written as one 16 B record");

namespace {
constexpr uint32_t kCountFlags = PT_COUNT_STATS | PT_COUNT_SIMPLE_KERNEL | PT_COUNT_BRUTE_FORCE;
constexpr uint32_t kContainFlags = PT_CONTAIN_STATS | PT_CONTAIN_SIMPLE_KERNEL;

int check_count(PtContext* ctx, const char* fn, const void* rays, uint64_t n, uint32_t flags, const void* counts) {
    if (int rc = check_flags(ctx, fn, flags, kCountFlags)) return rc;
    if (int rc = check_n(ctx, fn, n, "rays")) return rc;
    if (!aligned16(rays) || !aligned4(counts)) return bad_arg(ctx, fn, "rays must be non-null and 16-byte aligned, counts non-null and 4-byte aligned");
    return check_scene(ctx, fn);
}
// the parameter block and the batch size; the pointers and the scene are checked by the callers (pointers before the scene)
int check_contain_params(PtContext* ctx, const char* fn, uint64_t n, const PtContainParams* p) {
    if (!p) return bad_arg(ctx, fn, "null params");
    if (int rc = check_flags(ctx, fn, p->flags, kContainFlags)) return rc;
    if (int rc = check_n(ctx, fn, n, "points")) return rc;
    if (p->samples < 1u || p->samples > 255u || (p->samples & 1u) == 0u) return bad_arg(ctx, fn, "samples must be odd and in 1..255");
    return check_n(ctx, fn, n * uint64_t(p->samples), "sample rays (n * samples)");
}
int check_contain(PtContext* ctx, const char* fn, const void* points, uint64_t n, const PtContainParams* p, const void* out) {
    if (int rc = check_contain_params(ctx, fn, n, p)) return rc;
    if (int rc = check_records(ctx, fn, "points and results", {points, out})) return rc;
    return check_scene(ctx, fn);
}

// the launches themselves: device memory
int count_on_stream(PtContext* ctx, const void* rays, uint32_t n, uint32_t flags, void* counts) {
    const bool stats = (flags & PT_COUNT_STATS) != 0, simple = (flags & PT_COUNT_SIMPLE_KERNEL) != 0, brute = (flags & PT_COUNT_BRUTE_FORCE) != 0;
    Walk W;
    if (int rc = begin_walk(ctx, n, PT_CR_WAVES_PER_SIMD, PT_CR_SHORT_STACK, stats, !simple && !brute, W)) return rc;
    if (W.launch) PT_HIP(ctx, ptk::launch_count_hits(W.A, rays, counts, n, simple, stats, brute, ctx->d_rq_queue.ptr, ctx->d_rq_spill.ptr, W.grid, ctx->stream));
    return end_walk(ctx, W);
}
int contains_on_stream(PtContext* ctx, const void* points, uint32_t n, const PtContainParams& p, void* out) {
    const bool stats = (p.flags & PT_CONTAIN_STATS) != 0, simple = (p.flags & PT_CONTAIN_SIMPLE_KERNEL) != 0;
    Walk W;
    if (int rc = begin_walk(ctx, n, PT_CR_WAVES_PER_SIMD, PT_CR_SHORT_STACK, stats, !simple, W)) return rc;
    if (W.launch) PT_HIP(ctx, ptk::launch_contains(W.A, points, out, n, p.samples, p.seed, p.index_base, simple, stats, ctx->d_rq_queue.ptr, ctx->d_rq_spill.ptr, W.grid, ctx->stream));
    return end_walk(ctx, W);
}
// three launches, no host wait: the closest points into `out`, the containment into the context's buffer, the sign
int signed_on_stream(PtContext* ctx, const void* points, uint32_t n, const PtContainParams& p, void* out) {
    if (int rc = flush_pending(ctx)) return rc;
    if (n == 0u) return PT_OK;
    PT_HIP(ctx, ctx->d_cr_contain.ensure(size_t(n)));
    if (int rc = closest_on_stream(ctx, points, n, 0u, out)) return rc;
    if (int rc = contains_on_stream(ctx, points, n, p, ctx->d_cr_contain.ptr)) return rc;
    PT_HIP(ctx, ptk::launch_apply_sign(ctx->d_cr_contain.ptr, out, n, ctx->stream));
    return PT_OK;
}
} // namespace

int pt_count_hits(PtContext* ctx, const void* rays_device, uint64_t n, uint32_t flags, void* counts_device) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_count(ctx, "pt_count_hits", rays_device, n, flags, counts_device)) return rc;
    return count_on_stream(ctx, rays_device, uint32_t(n), flags, counts_device);
}

int pt_count_hits_host(PtContext* ctx, const PtRay* rays, uint64_t n, uint32_t flags, uint32_t* counts) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_count(ctx, "pt_count_hits_host", rays, n, flags, counts)) return rc;
    return staged(ctx, n, rays, sizeof(PtRay), ctx->d_rq_hits, counts, sizeof(uint32_t),
                  [&](const void* d_in, void* d_out) { return count_on_stream(ctx, d_in, uint32_t(n), flags, d_out); });
}

int pt_count_hits_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words,
                       const PtRay* rays, uint64_t n, uint32_t flags, uint32_t* counts, PtStats* stats) {
    if (flags & ~kCountFlags) return fail(nullptr, PT_ERR_INVALID_ARG, "pt_count_hits_bvh4: unknown flags");
    const bool brute = (flags & PT_COUNT_BRUTE_FORCE) != 0;
    if ((!tris && num_tris) || (n && (!rays || !counts)) || (!bvh4 && !brute)) return fail(nullptr, PT_ERR_INVALID_ARG, "pt_count_hits_bvh4: null pointer");
    if (n > 0xFFFFFFFFull) return fail(nullptr, PT_ERR_INVALID_ARG, "pt_count_hits_bvh4: more than 2^32 - 1 rays");
    std::string err;
    uint64_t counters[5] = {0, 0, 0, 0, 0};
    if (!pt::count_hits(tris, num_tris, brute ? nullptr : bvh4, words, reinterpret_cast<const float*>(rays), n, counts,
                        (flags & PT_COUNT_STATS) && stats ? counters : nullptr, err))
        return fail(nullptr, PT_ERR_BAD_BVH, err);
    if (stats) stats_from(stats, counters);
    return PT_OK;
}

int pt_contains(PtContext* ctx, const void* points_device, uint64_t n, const PtContainParams* params, void* out_device) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_contain(ctx, "pt_contains", points_device, n, params, out_device)) return rc;
    return contains_on_stream(ctx, points_device, uint32_t(n), *params, out_device);
}

int pt_contains_host(PtContext* ctx, const PtPoint* points, uint64_t n, const PtContainParams* params, PtContainment* out) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_contain(ctx, "pt_contains_host", points, n, params, out)) return rc;
    return staged(ctx, n, points, sizeof(PtPoint), ctx->d_rq_hits, out, sizeof(PtContainment),
                  [&](const void* d_in, void* d_out) { return contains_on_stream(ctx, d_in, uint32_t(n), *params, d_out); });
}

int pt_contains_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words,
                     const PtPoint* points, uint64_t n, const PtContainParams* params, PtContainment* out, PtStats* stats) {
    if (int rc = check_contain_params(nullptr, "pt_contains_bvh4", n, params)) return rc;
    if ((!tris && num_tris) || (n && (!points || !out)) || !bvh4) return fail(nullptr, PT_ERR_INVALID_ARG, "pt_contains_bvh4: null pointer");
    std::string err;
    uint64_t counters[5] = {0, 0, 0, 0, 0};
    if (!pt::contains(tris, num_tris, bvh4, words, reinterpret_cast<const float*>(points), n, params->samples, params->seed, params->index_base,
                      reinterpret_cast<uint32_t*>(out), (params->flags & PT_CONTAIN_STATS) && stats ? counters : nullptr, err))
        return fail(nullptr, PT_ERR_BAD_BVH, err);
    if (stats) stats_from(stats, counters);
    return PT_OK;
}

int pt_signed_distance(PtContext* ctx, const void* points_device, uint64_t n, const PtContainParams* params, void* out_device) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_contain(ctx, "pt_signed_distance", points_device, n, params, out_device)) return rc;
    return signed_on_stream(ctx, points_device, uint32_t(n), *params, out_device);
}

int pt_signed_distance_host(PtContext* ctx, const PtPoint* points, uint64_t n, const PtContainParams* params, PtClosest* out) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_contain(ctx, "pt_signed_distance_host", points, n, params, out)) return rc;
    return staged(ctx, n, points, sizeof(PtPoint), ctx->d_rq_hits, out, sizeof(PtClosest),
                  [&](const void* d_in, void* d_out) { return signed_on_stream(ctx, d_in, uint32_t(n), *params, d_out); });
}

// ---- radius queries (include/mi355pt.h; pt_radius.hip) -------------------------------------------------------------------------

namespace {
constexpr uint32_t kRadiusFlags = PT_RADIUS_STATS | PT_RADIUS_SIMPLE_KERNEL | PT_RADIUS_BRUTE_FORCE;

// The region queries (radius: points, box: boxes) share their flags' values, their check and their walk.
static_assert(PT_BOX_STATS == PT_RADIUS_STATS && PT_BOX_SIMPLE_KERNEL == PT_RADIUS_SIMPLE_KERNEL && PT_BOX_BRUTE_FORCE == PT_RADIUS_BRUTE_FORCE,
              "the PT_BOX_* flags take the values of the PT_RADIUS_* flags");
constexpr uint32_t kBoxFlags = kRadiusFlags;

// flags, batch size and the input records called `noun`; the other pointers are checked by the callers, and the scene behind them
int check_region(PtContext* ctx, const char* fn, const void* in, uint64_t n, uint32_t flags, const char* noun) {
    if (int rc = check_flags(ctx, fn, flags, kRadiusFlags)) return rc;
    if (int rc = check_n(ctx, fn, n, noun)) return rc;
    return check_records(ctx, fn, noun, {in});
}

// One walk through `launch` (ptk::launch_radius, ptk::launch_box) with the grid and the stack of its two knobs: the count walk into
// `counts` (offsets = nullptr), or the fill walk from `offsets` into `entries`.  The STATS flag counts over the count walk only; its fill
// walk is the one-item-per-thread kernel.
int region_walk_on_stream(PtContext* ctx, decltype(&ptk::launch_radius) launch, uint32_t waves_per_simd, int short_stack, const void* in, uint32_t n,
                          uint32_t flags, void* counts, const unsigned long long* offsets, void* entries, uint64_t capacity) {
    const bool fill = offsets != nullptr, brute = (flags & PT_RADIUS_BRUTE_FORCE) != 0;
    const bool stats = (flags & PT_RADIUS_STATS) != 0 && !fill, simple = (flags & (PT_RADIUS_SIMPLE_KERNEL | PT_RADIUS_STATS)) != 0;
    Walk W;
    if (int rc = begin_walk(ctx, n, waves_per_simd, short_stack, stats, !simple && !brute, W)) return rc;
    if (W.launch) PT_HIP(ctx, launch(W.A, in, n, counts, offsets, entries, capacity, simple, stats, brute, ctx->d_rq_queue.ptr, ctx->d_rq_spill.ptr, W.grid, ctx->stream));
    return end_walk(ctx, W);
}
int radius_count_on_stream(PtContext* ctx, const void* points, uint32_t n, uint32_t flags, void* counts) {
    return region_walk_on_stream(ctx, ptk::launch_radius, PT_RD_WAVES_PER_SIMD, PT_RD_SHORT_STACK, points, n, flags, counts, nullptr, nullptr, 0);
}
int radius_fill_on_stream(PtContext* ctx, const void* points, uint32_t n, uint32_t flags, const unsigned long long* offsets, void* entries, uint64_t capacity) {
    return region_walk_on_stream(ctx, ptk::launch_radius, PT_RD_WAVES_PER_SIMD, PT_RD_SHORT_STACK, points, n, flags, nullptr, offsets, entries, capacity);
}

// A list query is a count walk, the scan of its counts into offsets, and a fill walk: radius search over points, box search over boxes,
// triangle search over caller triangles, hit lists over rays.  The counts, the scan's scratch and the staging buffers (d_rd_*) are shared: the queries use them between launches of one call on the
// context's stream, which orders them, and the host forms wait for the stream before they return.
struct ListQuery {
    size_t in_bytes;             // one input record
    int (*count)(PtContext*, const void* in, uint32_t n, uint32_t flags, void* counts);
    int (*fill)(PtContext*, const void* in, uint32_t n, uint32_t flags, const unsigned long long* offsets, void* entries, uint64_t capacity);
};

// the count walk into the context's buffer and the scan into `offsets`: two launches, no host wait
int list_offsets_on_stream(PtContext* ctx, const ListQuery& q, const void* in, uint32_t n, uint32_t flags, unsigned long long* offsets) {
    const size_t temp_bytes = ptk::radius_scan_temp_bytes(n);
    PT_HIP(ctx, ctx->d_rd_counts.ensure(size_t(n))); PT_HIP(ctx, ctx->d_rd_temp.ensure(temp_bytes));
    if (int rc = q.count(ctx, in, n, flags, ctx->d_rd_counts.ptr)) return rc;
    PT_HIP(ctx, ptk::launch_radius_scan(ctx->d_rd_counts.ptr, n, offsets, ctx->d_rd_temp.ptr, temp_bytes, ctx->stream));
    return PT_OK;
}
// device memory, no host wait: the counts into the context's buffer, their scan into offsets, the entries
int list_device(PtContext* ctx, const ListQuery& q, const void* in, uint64_t n, uint32_t flags, void* offsets_device, void* entries, uint64_t capacity) {
    if (int rc = flush_pending(ctx)) return rc;
    unsigned long long* offsets = static_cast<unsigned long long*>(offsets_device);
    if (n == 0) { PT_HIP(ctx, hipMemsetAsync(offsets, 0, sizeof(unsigned long long), ctx->stream)); return PT_OK; }
    if (int rc = list_offsets_on_stream(ctx, q, in, uint32_t(n), flags, offsets)) return rc;
    if (capacity == 0) return PT_OK;
    return q.fill(ctx, in, uint32_t(n), flags, offsets, entries, capacity);
}
// staged: the host reads the total between the scan and the fill walk, so the staging buffer holds min(total, capacity) entries
int list_host(PtContext* ctx, const ListQuery& q, const void* in, uint64_t n, uint32_t flags, uint64_t* offsets, void* entries, uint64_t capacity) {
    if (int rc = flush_pending(ctx)) return rc;
    if (n == 0) { offsets[0] = 0; return PT_OK; }
    PT_HIP(ctx, ctx->d_rq_rays.ensure(size_t(n) * q.in_bytes / sizeof(uint4))); PT_HIP(ctx, ctx->d_rd_offsets.ensure(size_t(n) + 1));
    PT_HIP(ctx, hipMemcpyAsync(ctx->d_rq_rays.ptr, in, size_t(n) * q.in_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = list_offsets_on_stream(ctx, q, ctx->d_rq_rays.ptr, uint32_t(n), flags, ctx->d_rd_offsets.ptr)) return rc;
    PT_HIP(ctx, hipMemcpyAsync(offsets, ctx->d_rd_offsets.ptr, (size_t(n) + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t held = std::min<uint64_t>(offsets[n], capacity);
    if (held == 0) return PT_OK;
    PT_HIP(ctx, ctx->d_rd_entries.ensure(size_t(held)));
    if (int rc = q.fill(ctx, ctx->d_rq_rays.ptr, uint32_t(n), flags, ctx->d_rd_offsets.ptr, ctx->d_rd_entries.ptr, held)) return rc;
    PT_HIP(ctx, hipMemcpyAsync(entries, ctx->d_rd_entries.ptr, size_t(held) * sizeof(uint4), hipMemcpyDeviceToHost, ctx->stream));
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PT_OK;
}
constexpr ListQuery kRadiusList = {sizeof(PtPoint), radius_count_on_stream, radius_fill_on_stream};

// The argument check of a list query's host twin (pt_radius_search_bvh4, pt_box_search_bvh4, pt_list_hits_bvh4): `in` holds n records
// called `noun`, a NULL bvh4 goes with brute force only.
int check_list_bvh4(const char* fn, uint32_t flags, uint32_t known, bool brute, const float* tris, uint32_t num_tris, const uint32_t* bvh4,
                    const void* in, uint64_t n, const char* noun, const uint64_t* offsets, const void* entries, uint64_t capacity) {
    const std::string f = std::string(fn) + ": ";
    if (flags & ~known) return fail(nullptr, PT_ERR_INVALID_ARG, f + "unknown flags");
    if ((!tris && num_tris) || (n && !in) || !offsets || (capacity && !entries) || (!bvh4 && !brute)) return fail(nullptr, PT_ERR_INVALID_ARG, f + "null pointer");
    if (!aligned8(offsets)) return fail(nullptr, PT_ERR_INVALID_ARG, f + "offsets must be 8-byte aligned");
    if (n > 0xFFFFFFFFull) return fail(nullptr, PT_ERR_INVALID_ARG, f + "more than 2^32 - 1 " + noun);
    return PT_OK;
}
} // namespace

int pt_radius_count(PtContext* ctx, const void* points_device, uint64_t n, uint32_t flags, void* counts_device) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_region(ctx, "pt_radius_count", points_device, n, flags, "points")) return rc;
    if (int rc = check_counts(ctx, "pt_radius_count", counts_device)) return rc;
    if (int rc = check_scene(ctx, "pt_radius_count")) return rc;
    return radius_count_on_stream(ctx, points_device, uint32_t(n), flags, counts_device);
}

int pt_radius_count_host(PtContext* ctx, const PtPoint* points, uint64_t n, uint32_t flags, uint32_t* counts) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_region(ctx, "pt_radius_count_host", points, n, flags, "points")) return rc;
    if (int rc = check_counts(ctx, "pt_radius_count_host", counts)) return rc;
    if (int rc = check_scene(ctx, "pt_radius_count_host")) return rc;
    return staged(ctx, n, points, sizeof(PtPoint), ctx->d_rd_counts, counts, sizeof(uint32_t),
                  [&](const void* d_in, void* d_out) { return radius_count_on_stream(ctx, d_in, uint32_t(n), flags, d_out); });
}

// three launches, no host wait (list_device)
int pt_radius_search(PtContext* ctx, const void* points_device, uint64_t n, uint32_t flags, void* offsets_device, void* entries_device, uint64_t capacity) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_region(ctx, "pt_radius_search", points_device, n, flags, "points")) return rc;
    if (int rc = check_list(ctx, "pt_radius_search", offsets_device, entries_device, capacity, "entries")) return rc;
    if (int rc = check_scene(ctx, "pt_radius_search")) return rc;
    return list_device(ctx, kRadiusList, points_device, n, flags, offsets_device, entries_device, capacity);
}

int pt_radius_search_host(PtContext* ctx, const PtPoint* points, uint64_t n, uint32_t flags, uint64_t* offsets, PtClosest* entries, uint64_t capacity) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_region(ctx, "pt_radius_search_host", points, n, flags, "points")) return rc;
    if (int rc = check_list(ctx, "pt_radius_search_host", offsets, entries, capacity, "entries")) return rc;
    if (int rc = check_scene(ctx, "pt_radius_search_host")) return rc;
    return list_host(ctx, kRadiusList, points, n, flags, offsets, entries, capacity);
}

int pt_radius_search_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const PtPoint* points, uint64_t n,
                          uint32_t flags, uint64_t* offsets, PtClosest* entries, uint64_t capacity, PtStats* stats) {
    const bool brute = (flags & PT_RADIUS_BRUTE_FORCE) != 0;
    if (int rc = check_list_bvh4("pt_radius_search_bvh4", flags, kRadiusFlags, brute, tris, num_tris, bvh4, points, n, "points", offsets, entries, capacity)) return rc;
    std::string err;
    uint64_t counters[5] = {0, 0, 0, 0, 0};
    if (!pt::radius_search(tris, num_tris, brute ? nullptr : bvh4, words, reinterpret_cast<const float*>(points), n, offsets,
                           reinterpret_cast<uint32_t*>(entries), capacity, (flags & PT_RADIUS_STATS) && stats ? counters : nullptr, err))
        return fail(nullptr, PT_ERR_BAD_BVH, err);
    if (stats) stats_from(stats, counters);
    return PT_OK;
}

// ---- box-overlap queries (include/mi355pt.h; pt_overlap.hip) --------------------------------------------------------------------

static_assert(sizeof(PtBox) == 32 && sizeof(PtOverlap) == sizeof(uint4), "PtBox / PtOverlap are read and written as 2 x 16 B and 16 B records");

namespace {
// the count walk and the fill walk (region_walk_on_stream)
int box_count_on_stream(PtContext* ctx, const void* boxes, uint32_t n, uint32_t flags, void* counts) {
    return region_walk_on_stream(ctx, ptk::launch_box, PT_BX_WAVES_PER_SIMD, PT_BX_SHORT_STACK, boxes, n, flags, counts, nullptr, nullptr, 0);
}
int box_fill_on_stream(PtContext* ctx, const void* boxes, uint32_t n, uint32_t flags, const unsigned long long* offsets, void* entries, uint64_t capacity) {
    return region_walk_on_stream(ctx, ptk::launch_box, PT_BX_WAVES_PER_SIMD, PT_BX_SHORT_STACK, boxes, n, flags, nullptr, offsets, entries, capacity);
}
constexpr ListQuery kBoxList = {sizeof(PtBox), box_count_on_stream, box_fill_on_stream};
} // namespace

int pt_box_count(PtContext* ctx, const void* boxes_device, uint64_t n, uint32_t flags, void* counts_device) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_region(ctx, "pt_box_count", boxes_device, n, flags, "boxes")) return rc;
    if (int rc = check_counts(ctx, "pt_box_count", counts_device)) return rc;
    if (int rc = check_scene(ctx, "pt_box_count")) return rc;
    return box_count_on_stream(ctx, boxes_device, uint32_t(n), flags, counts_device);
}

int pt_box_count_host(PtContext* ctx, const PtBox* boxes, uint64_t n, uint32_t flags, uint32_t* counts) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_region(ctx, "pt_box_count_host", boxes, n, flags, "boxes")) return rc;
    if (int rc = check_counts(ctx, "pt_box_count_host", counts)) return rc;
    if (int rc = check_scene(ctx, "pt_box_count_host")) return rc;
    return staged(ctx, n, boxes, sizeof(PtBox), ctx->d_rd_counts, counts, sizeof(uint32_t),
                  [&](const void* d_in, void* d_out) { return box_count_on_stream(ctx, d_in, uint32_t(n), flags, d_out); });
}

// three launches, no host wait (list_device)
int pt_box_search(PtContext* ctx, const void* boxes_device, uint64_t n, uint32_t flags, void* offsets_device, void* entries_device, uint64_t capacity) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_region(ctx, "pt_box_search", boxes_device, n, flags, "boxes")) return rc;
    if (int rc = check_list(ctx, "pt_box_search", offsets_device, entries_device, capacity, "entries")) return rc;
    if (int rc = check_scene(ctx, "pt_box_search")) return rc;
    return list_device(ctx, kBoxList, boxes_device, n, flags, offsets_device, entries_device, capacity);
}

int pt_box_search_host(PtContext* ctx, const PtBox* boxes, uint64_t n, uint32_t flags, uint64_t* offsets, PtOverlap* entries, uint64_t capacity) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_region(ctx, "pt_box_search_host", boxes, n, flags, "boxes")) return rc;
    if (int rc = check_list(ctx, "pt_box_search_host", offsets, entries, capacity, "entries")) return rc;
    if (int rc = check_scene(ctx, "pt_box_search_host")) return rc;
    return list_host(ctx, kBoxList, boxes, n, flags, offsets, entries, capacity);
}

int pt_box_search_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const PtBox* boxes, uint64_t n,
                       uint32_t flags, uint64_t* offsets, PtOverlap* entries, uint64_t capacity, PtStats* stats) {
    const bool brute = (flags & PT_BOX_BRUTE_FORCE) != 0;
    if (int rc = check_list_bvh4("pt_box_search_bvh4", flags, kBoxFlags, brute, tris, num_tris, bvh4, boxes, n, "boxes", offsets, entries, capacity)) return rc;
    std::string err;
    uint64_t counters[5] = {0, 0, 0, 0, 0};
    if (!pt::box_search(tris, num_tris, brute ? nullptr : bvh4, words, reinterpret_cast<const float*>(boxes), n, offsets,
                        reinterpret_cast<uint32_t*>(entries), capacity, (flags & PT_BOX_STATS) && stats ? counters : nullptr, err))
        return fail(nullptr, PT_ERR_BAD_BVH, err);
    if (stats) stats_from(stats, counters);
    return PT_OK;
}

// ---- triangle-overlap queries (include/mi355pt.h; pt_tritri.hip) -----------------------------------------------------------------

static_assert(sizeof(PtTri) == 48 && sizeof(PtCross) == sizeof(uint4), "PtTri / PtCross are read and written as 3 x 16 B and 16 B records");
static_assert(PT_TRI_STATS == PT_RADIUS_STATS && PT_TRI_SIMPLE_KERNEL == PT_RADIUS_SIMPLE_KERNEL && PT_TRI_BRUTE_FORCE == PT_RADIUS_BRUTE_FORCE,
              "the PT_TRI_* flags take the values of the PT_RADIUS_* flags");

namespace {
constexpr uint32_t kTriFlags = kRadiusFlags;
// the count walk and the fill walk (region_walk_on_stream)
int tri_count_on_stream(PtContext* ctx, const void* tris, uint32_t n, uint32_t flags, void* counts) {
    return region_walk_on_stream(ctx, ptk::launch_tri, PT_TT_WAVES_PER_SIMD, PT_TT_SHORT_STACK, tris, n, flags, counts, nullptr, nullptr, 0);
}
int tri_fill_on_stream(PtContext* ctx, const void* tris, uint32_t n, uint32_t flags, const unsigned long long* offsets, void* entries, uint64_t capacity) {
    return region_walk_on_stream(ctx, ptk::launch_tri, PT_TT_WAVES_PER_SIMD, PT_TT_SHORT_STACK, tris, n, flags, nullptr, offsets, entries, capacity);
}
constexpr ListQuery kTriList = {sizeof(PtTri), tri_count_on_stream, tri_fill_on_stream};
} // namespace

int pt_tri_count(PtContext* ctx, const void* tris_device, uint64_t n, uint32_t flags, void* counts_device) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_region(ctx, "pt_tri_count", tris_device, n, flags, "triangles")) return rc;
    if (int rc = check_counts(ctx, "pt_tri_count", counts_device)) return rc;
    if (int rc = check_scene(ctx, "pt_tri_count")) return rc;
    return tri_count_on_stream(ctx, tris_device, uint32_t(n), flags, counts_device);
}

int pt_tri_count_host(PtContext* ctx, const PtTri* tris, uint64_t n, uint32_t flags, uint32_t* counts) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_region(ctx, "pt_tri_count_host", tris, n, flags, "triangles")) return rc;
    if (int rc = check_counts(ctx, "pt_tri_count_host", counts)) return rc;
    if (int rc = check_scene(ctx, "pt_tri_count_host")) return rc;
    return staged(ctx, n, tris, sizeof(PtTri), ctx->d_rd_counts, counts, sizeof(uint32_t),
                  [&](const void* d_in, void* d_out) { return tri_count_on_stream(ctx, d_in, uint32_t(n), flags, d_out); });
}

// three launches, no host wait (list_device)
int pt_tri_search(PtContext* ctx, const void* tris_device, uint64_t n, uint32_t flags, void* offsets_device, void* entries_device, uint64_t capacity) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_region(ctx, "pt_tri_search", tris_device, n, flags, "triangles")) return rc;
    if (int rc = check_list(ctx, "pt_tri_search", offsets_device, entries_device, capacity, "entries")) return rc;
    if (int rc = check_scene(ctx, "pt_tri_search")) return rc;
    return list_device(ctx, kTriList, tris_device, n, flags, offsets_device, entries_device, capacity);
}

int pt_tri_search_host(PtContext* ctx, const PtTri* tris, uint64_t n, uint32_t flags, uint64_t* offsets, PtCross* entries, uint64_t capacity) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_region(ctx, "pt_tri_search_host", tris, n, flags, "triangles")) return rc;
    if (int rc = check_list(ctx, "pt_tri_search_host", offsets, entries, capacity, "entries")) return rc;
    if (int rc = check_scene(ctx, "pt_tri_search_host")) return rc;
    return list_host(ctx, kTriList, tris, n, flags, offsets, entries, capacity);
}

int pt_tri_search_bvh4(const float* mesh, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const PtTri* tris, uint64_t n,
                       uint32_t flags, uint64_t* offsets, PtCross* entries, uint64_t capacity, PtStats* stats) {
    const bool brute = (flags & PT_TRI_BRUTE_FORCE) != 0;
    if (int rc = check_list_bvh4("pt_tri_search_bvh4", flags, kTriFlags, brute, mesh, num_tris, bvh4, tris, n, "triangles", offsets, entries, capacity)) return rc;
    std::string err;
    uint64_t counters[5] = {0, 0, 0, 0, 0};
    if (!pt::tri_search(mesh, num_tris, brute ? nullptr : bvh4, words, reinterpret_cast<const float*>(tris), n, offsets,
                        reinterpret_cast<uint32_t*>(entries), capacity, (flags & PT_TRI_STATS) && stats ? counters : nullptr, err))
        return fail(nullptr, PT_ERR_BAD_BVH, err);
    if (stats) stats_from(stats, counters);
    return PT_OK;
}

// ---- hit lists (include/mi355pt.h; pt_hitlist.hip) ------------------------------------------------------------------------------

static_assert(sizeof(PtClosest) == sizeof(uint4) && sizeof(PtHit) == sizeof(uint4), "the entries of both list queries are staged as 16 B records");

namespace {
constexpr uint32_t kHitsFlags = PT_HITS_STATS | PT_HITS_SIMPLE_KERNEL | PT_HITS_BRUTE_FORCE | PT_HITS_SORTED;
static_assert(PT_HITS_STATS == PT_COUNT_STATS && PT_HITS_SIMPLE_KERNEL == PT_COUNT_SIMPLE_KERNEL && PT_HITS_BRUTE_FORCE == PT_COUNT_BRUTE_FORCE,
              "the count walk of pt_list_hits is pt_count_hits' with the same flags");

// flags, batch size and the pointers, then the scene
int check_hits(PtContext* ctx, const char* fn, const void* rays, uint64_t n, uint32_t flags, const void* offsets, const void* hits, uint64_t capacity) {
    if (int rc = check_flags(ctx, fn, flags, kHitsFlags)) return rc;
    if (int rc = check_n(ctx, fn, n, "rays")) return rc;
    if (int rc = check_records(ctx, fn, "rays", {rays})) return rc;
    if (int rc = check_list(ctx, fn, offsets, hits, capacity, "hits")) return rc;
    return check_scene(ctx, fn);
}
// the count walk: pt_count_hits' own launch, counters included
int hits_count_on_stream(PtContext* ctx, const void* rays, uint32_t n, uint32_t flags, void* counts) {
    return count_on_stream(ctx, rays, n, flags & kCountFlags, counts);
}
// the fill walk from `offsets` into `hits` and, with PT_HITS_SORTED, the sort: one or two launches, no host wait.  PT_HITS_STATS counted
// over the count walk; its fill walk is the one-ray-per-thread kernel.
int hits_fill_on_stream(PtContext* ctx, const void* rays, uint32_t n, uint32_t flags, const unsigned long long* offsets, void* hits, uint64_t capacity) {
    const bool brute = (flags & PT_HITS_BRUTE_FORCE) != 0, simple = (flags & (PT_HITS_SIMPLE_KERNEL | PT_HITS_STATS)) != 0;
    Walk W;
    if (int rc = begin_walk(ctx, n, PT_HL_WAVES_PER_SIMD, PT_HL_SHORT_STACK, false, !simple && !brute, W)) return rc;
    if (!W.launch) return PT_OK;
    PT_HIP(ctx, ptk::launch_hit_fill(W.A, rays, n, offsets, hits, capacity, simple, brute, ctx->d_rq_queue.ptr, ctx->d_rq_spill.ptr, W.grid, ctx->stream));
    if (flags & PT_HITS_SORTED) PT_HIP(ctx, ptk::launch_hit_sort(offsets, hits, capacity, n, ctx->stream));
    return end_walk(ctx, W);
}
constexpr ListQuery kHitsList = {sizeof(PtRay), hits_count_on_stream, hits_fill_on_stream};
} // namespace

// three or four launches, no host wait (list_device; the fourth is the sort)
int pt_list_hits(PtContext* ctx, const void* rays_device, uint64_t n, uint32_t flags, void* offsets_device, void* hits_device, uint64_t capacity) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_hits(ctx, "pt_list_hits", rays_device, n, flags, offsets_device, hits_device, capacity)) return rc;
    return list_device(ctx, kHitsList, rays_device, n, flags, offsets_device, hits_device, capacity);
}

int pt_list_hits_host(PtContext* ctx, const PtRay* rays, uint64_t n, uint32_t flags, uint64_t* offsets, PtHit* hits, uint64_t capacity) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_hits(ctx, "pt_list_hits_host", rays, n, flags, offsets, hits, capacity)) return rc;
    return list_host(ctx, kHitsList, rays, n, flags, offsets, hits, capacity);
}

int pt_list_hits_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const PtRay* rays, uint64_t n,
                      uint32_t flags, uint64_t* offsets, PtHit* hits, uint64_t capacity, PtStats* stats) {
    const bool brute = (flags & PT_HITS_BRUTE_FORCE) != 0;
    if (int rc = check_list_bvh4("pt_list_hits_bvh4", flags, kHitsFlags, brute, tris, num_tris, bvh4, rays, n, "rays", offsets, hits, capacity)) return rc;
    std::string err;
    uint64_t counters[5] = {0, 0, 0, 0, 0};
    if (!pt::list_hits(tris, num_tris, brute ? nullptr : bvh4, words, reinterpret_cast<const float*>(rays), n, offsets,
                       reinterpret_cast<uint32_t*>(hits), capacity, (flags & PT_HITS_SORTED) != 0, (flags & PT_HITS_STATS) && stats ? counters : nullptr, err))
        return fail(nullptr, PT_ERR_BAD_BVH, err);
    if (stats) stats_from(stats, counters);
    return PT_OK;
}

// ---- k-nearest queries (include/mi355pt.h; pt_knn.hip) --------------------------------------------------------------------------

static_assert(PT_NEAREST_MAX_K == ptk::kNearestMaxK && PT_NEAREST_MAX_K == pt::kNearestMaxK, "one PT_NEAREST_MAX_K for the header, the kernels and the twin");

namespace {
constexpr uint32_t kNearestFlags = PT_NEAREST_STATS | PT_NEAREST_SIMPLE_KERNEL | PT_NEAREST_BRUTE_FORCE;

int check_nearest(PtContext* ctx, const char* fn, const void* points, uint64_t n, uint32_t k, uint32_t flags, const void* out) {
    if (int rc = check_flags(ctx, fn, flags, kNearestFlags)) return rc;
    if (k == 0u || k > PT_NEAREST_MAX_K) return bad_arg(ctx, fn, "k must be 1 .. PT_NEAREST_MAX_K");
    if (int rc = check_n(ctx, fn, n, "points")) return rc;
    if (int rc = check_records(ctx, fn, "points and results", {points, out})) return rc;
    return check_scene(ctx, fn);
}

// the launch itself: points / rows in device memory; the grid depends on k
int nearest_on_stream(PtContext* ctx, const void* points, uint32_t n, uint32_t k, uint32_t flags, void* out) {
    const bool stats = (flags & PT_NEAREST_STATS) != 0, simple = (flags & PT_NEAREST_SIMPLE_KERNEL) != 0, brute = (flags & PT_NEAREST_BRUTE_FORCE) != 0;
    Walk W;
    if (int rc = begin_walk(ctx, n, ptk::nearest_k_waves_per_simd(k), PT_NK_SHORT_STACK, stats, !simple && !brute, W)) return rc;
    if (W.launch) PT_HIP(ctx, ptk::launch_nearest_k(W.A, points, out, n, k, simple, stats, brute, ctx->d_rq_queue.ptr, ctx->d_rq_spill.ptr, W.grid, ctx->stream));
    return end_walk(ctx, W);
}
} // namespace

int pt_nearest_k(PtContext* ctx, const void* points_device, uint64_t n, uint32_t k, uint32_t flags, void* out_device) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_nearest(ctx, "pt_nearest_k", points_device, n, k, flags, out_device)) return rc;
    return nearest_on_stream(ctx, points_device, uint32_t(n), k, flags, out_device);
}

// staged through the buffers of the ray and closest-point queries: n points in, n rows of k records out
int pt_nearest_k_host(PtContext* ctx, const PtPoint* points, uint64_t n, uint32_t k, uint32_t flags, PtClosest* out) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_nearest(ctx, "pt_nearest_k_host", points, n, k, flags, out)) return rc;
    return staged(ctx, n, points, sizeof(PtPoint), ctx->d_rq_hits, out, size_t(k) * sizeof(PtClosest),
                  [&](const void* d_in, void* d_out) { return nearest_on_stream(ctx, d_in, uint32_t(n), k, flags, d_out); });
}

int pt_nearest_k_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const PtPoint* points, uint64_t n,
                      uint32_t k, uint32_t flags, PtClosest* out, PtStats* stats) {
    if (flags & ~kNearestFlags) return fail(nullptr, PT_ERR_INVALID_ARG, "pt_nearest_k_bvh4: unknown flags");
    if (k == 0u || k > PT_NEAREST_MAX_K) return fail(nullptr, PT_ERR_INVALID_ARG, "pt_nearest_k_bvh4: k must be 1 .. PT_NEAREST_MAX_K");
    const bool brute = (flags & PT_NEAREST_BRUTE_FORCE) != 0;
    if ((!tris && num_tris) || (n && (!points || !out)) || (!bvh4 && !brute)) return fail(nullptr, PT_ERR_INVALID_ARG, "pt_nearest_k_bvh4: null pointer");
    if (n > 0xFFFFFFFFull) return fail(nullptr, PT_ERR_INVALID_ARG, "pt_nearest_k_bvh4: more than 2^32 - 1 points");
    std::string err;
    uint64_t counters[5] = {0, 0, 0, 0, 0};
    if (!pt::nearest_k(tris, num_tris, brute ? nullptr : bvh4, words, reinterpret_cast<const float*>(points), n, k,
                       reinterpret_cast<uint32_t*>(out), (flags & PT_NEAREST_STATS) && stats ? counters : nullptr, err))
        return fail(nullptr, PT_ERR_BAD_BVH, err);
    if (stats) stats_from(stats, counters);
    return PT_OK;
}

} // extern "C"
