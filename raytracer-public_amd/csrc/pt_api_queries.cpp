// pt_api_queries.cpp -- the batched queries over the context's tree (include/mi355pt.h): closest hit / any hit, closest point,
// occlusion, crossing counts, containment, signed distance, radius count / search, box count / search, triangle count / search, plane-cut count / search, hit lists,
// k-nearest and sphere casts, with the host twins (*_bvh4) next to them.
// Each query states its facts once -- the nouns of its error texts, its record sizes, its flags, its two launch knobs, its launcher and its
// pt::* twin -- as a descriptor: a WalkQuery (closest points, sphere casts, crossing counts), a ListQuery (radius, box, triangle, plane-cut search,
// hit lists), or a small struct that also carries the call's extra arguments (Trace, Nearest, Occlusion, Contains, SignedDistance).  The
// entry points are forwarding statements into the forms written once: item_device / item_host (n records in, n records out),
// list_search / list_search_host (offsets and entries), and for the twins walk_bvh4 / list_bvh4 over check_item_bvh4 / check_list_bvh4
// and run_twin.  Every entry point names itself in the call: that string is the prefix of its error texts.
#include "pt_context.h"

#include <algorithm>
#include <initializer_list>

using namespace pti;

// ---- what every query shares ------------------------------------------------------------------------------------------------------
namespace {

// The pieces of the argument checks.  Each check below is a list of them in the order that decides which error a caller sees:
// arguments (PT_ERR_INVALID_ARG) before the scene (PT_ERR_NO_SCENE).
bool aligned(const void* p, size_t bytes) { return p && (reinterpret_cast<uintptr_t>(p) & (bytes - 1u)) == 0u; }
int bad_arg(PtContext* ctx, const char* fn, const std::string& what) { return fail(ctx, PT_ERR_INVALID_ARG, std::string(fn) + ": " + what); }
int check_flags(PtContext* ctx, const char* fn, uint32_t flags, uint32_t known) { return (flags & ~known) ? bad_arg(ctx, fn, "unknown flags") : PT_OK; }
int check_n(PtContext* ctx, const char* fn, uint64_t n, const char* noun) {
    return n > 0xFFFFFFFFull ? bad_arg(ctx, fn, std::string("more than 2^32 - 1 ") + noun) : PT_OK;
}
// `what` names the record arrays `ptrs`: each non-null and 16-byte aligned
int check_records(PtContext* ctx, const char* fn, const char* what, std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs) if (!aligned(p, 16)) return bad_arg(ctx, fn, std::string(what) + " must be non-null and 16-byte aligned");
    return PT_OK;
}
// flags, batch size and the input records called `noun`
int check_input(PtContext* ctx, const char* fn, uint32_t flags, uint32_t known, uint64_t n, const char* noun, const void* in) {
    if (int rc = check_flags(ctx, fn, flags, known)) return rc;
    if (int rc = check_n(ctx, fn, n, noun)) return rc;
    return check_records(ctx, fn, noun, {in});
}
int check_counts(PtContext* ctx, const char* fn, const void* counts) {
    return aligned(counts, 4) ? PT_OK : bad_arg(ctx, fn, "counts must be non-null and 4-byte aligned");
}
// the outputs of a list query: n + 1 offsets, and `capacity` entries called `noun`
int check_list(PtContext* ctx, const char* fn, const void* offsets, const void* entries, uint64_t capacity, const char* noun) {
    if (!aligned(offsets, 8)) return bad_arg(ctx, fn, "offsets must be non-null and 8-byte aligned");
    if (capacity ? !aligned(entries, 16) : (entries && !aligned(entries, 16))) return bad_arg(ctx, fn, std::string(noun) + " must be 16-byte aligned, and non-null unless capacity is 0");
    return PT_OK;
}
int check_scene(PtContext* ctx, const char* fn) {
    if (!ctx->have_tris || !ctx->have_bvh) return fail(ctx, PT_ERR_NO_SCENE, std::string(fn) + ": scene not set (triangles + BVH)");
    return PT_OK;
}

// A query's flag word: every bit it knows, and the bits that ask for the counters, the one-item-per-thread kernel and brute force.
struct Flags { uint32_t known, stats, simple, brute; };

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
// the query's launch on the stream -- on them, n records of `out_bytes` each from `d_out` back to `out`, and the one host wait.
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

// The two context forms of an item-to-record query (n records in, n records out), called `fn`.  `q` is the query with the call's extra
// arguments in it: q.check(ctx, fn, in, n, out) is its argument check, scene included; q.run(ctx, in, n, out) its launch on the stream,
// device memory and no host wait; q.in_bytes and q.out_bytes its record sizes.  The host form stages through `d_out` of the context.
template <typename Q>
int item_device(PtContext* ctx, const char* fn, const Q& q, const void* in, uint64_t n, void* out) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = q.check(ctx, fn, in, n, out)) return rc;
    return q.run(ctx, in, uint32_t(n), out);
}
template <typename Q, typename T = uint4>
int item_host(PtContext* ctx, const char* fn, const Q& q, const void* in, uint64_t n, void* out, DevBuf<T> PtContext::* d_out = &PtContext::d_rq_hits) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = q.check(ctx, fn, in, n, out)) return rc;
    return staged(ctx, n, in, q.in_bytes, ctx->*d_out, out, q.out_bytes, [&](const void* d_in, void* d) { return q.run(ctx, d_in, uint32_t(n), d); });
}

// The host twins (*_bvh4) take no context.  The argument check of an item-to-record twin behind its flags (and nearest_k's k): `in` holds n
// records called `noun`, `out` takes n; a NULL bvh4 goes with brute force only.  The list twins have check_list_bvh4.
int check_item_bvh4(const char* fn, bool brute, const float* tris, uint32_t num_tris, const uint32_t* bvh4, const void* in, const void* out, uint64_t n, const char* noun) {
    if ((!tris && num_tris) || (n && (!in || !out)) || (!bvh4 && !brute)) return bad_arg(nullptr, fn, "null pointer");
    return check_n(nullptr, fn, n, noun);
}
int check_list_bvh4(const char* fn, uint32_t flags, uint32_t known, bool brute, const float* tris, uint32_t num_tris, const uint32_t* bvh4,
                    const void* in, uint64_t n, const char* noun, const uint64_t* offsets, const void* entries, uint64_t capacity) {
    if (int rc = check_flags(nullptr, fn, flags, known)) return rc;
    if ((!tris && num_tris) || (n && !in) || !offsets || (capacity && !entries) || (!bvh4 && !brute)) return bad_arg(nullptr, fn, "null pointer");
    if (!aligned(offsets, 8)) return bad_arg(nullptr, fn, "offsets must be 8-byte aligned");
    return check_n(nullptr, fn, n, noun);
}
// What every twin ends in: `twin(tree, counters, err)` is the call of the pt::* function, over every triangle with `brute`; the counters
// only when the flags ask (`want_stats`) and the caller takes them.
template <typename Twin>
int run_twin(const uint32_t* bvh4, bool brute, bool want_stats, PtStats* stats, Twin twin) {
    std::string err;
    uint64_t counters[5] = {0, 0, 0, 0, 0};
    if (!twin(brute ? nullptr : bvh4, want_stats && stats ? counters : nullptr, err)) return fail(nullptr, PT_ERR_BAD_BVH, err);
    if (!stats) return PT_OK;
    std::memset(stats, 0, sizeof(*stats));
    stats->rays_closest = counters[0]; stats->nodes_examined = counters[1]; stats->tris_tested = counters[2];
    stats->stack_drops = counters[3]; stats->max_stack = counters[4];
    return PT_OK;
}

// An item-to-record query whose flags are its only extra argument: closest points, sphere casts, crossing counts.
struct WalkQuery {
    const char* noun;              // the input records in "more than 2^32 - 1 <noun>"
    const char* pointers;          // what a bad input or output pointer is told; an output record is aligned to its size (16 or 4 bytes)
    size_t in_bytes, out_bytes;
    Flags flags;
    uint32_t waves_per_simd; int short_stack;      // the knobs of its launch
    decltype(&ptk::launch_closest_points) launch;
    decltype(&pt::closest_points) twin;
};
struct Walked {                    // one call of a WalkQuery
    const WalkQuery& q; uint32_t flags;
    size_t in_bytes = q.in_bytes, out_bytes = q.out_bytes;
    int check(PtContext* ctx, const char* fn, const void* in, uint64_t n, const void* out) const {
        if (int rc = check_flags(ctx, fn, flags, q.flags.known)) return rc;
        if (int rc = check_n(ctx, fn, n, q.noun)) return rc;
        if (!aligned(in, 16) || !aligned(out, q.out_bytes)) return bad_arg(ctx, fn, q.pointers);
        return check_scene(ctx, fn);
    }
    int run(PtContext* ctx, const void* in, uint32_t n, void* out) const {
        const bool stats = (flags & q.flags.stats) != 0, simple = (flags & q.flags.simple) != 0, brute = (flags & q.flags.brute) != 0;
        Walk W;
        if (int rc = begin_walk(ctx, n, q.waves_per_simd, q.short_stack, stats, !simple && !brute, W)) return rc;
        if (W.launch) PT_HIP(ctx, q.launch(W.A, in, out, n, simple, stats, brute, ctx->d_rq_queue.ptr, ctx->d_rq_spill.ptr, W.grid, ctx->stream));
        return end_walk(ctx, W);
    }
};
int walk_bvh4(const char* fn, const WalkQuery& q, const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words,
              const void* in, uint64_t n, uint32_t flags, void* out, PtStats* stats) {
    if (int rc = check_flags(nullptr, fn, flags, q.flags.known)) return rc;
    const bool brute = (flags & q.flags.brute) != 0;
    if (int rc = check_item_bvh4(fn, brute, tris, num_tris, bvh4, in, out, n, q.noun)) return rc;
    return run_twin(bvh4, brute, (flags & q.flags.stats) != 0, stats, [&](const uint32_t* tree, uint64_t* counters, std::string& err) {
        return q.twin(tris, num_tris, tree, words, static_cast<const float*>(in), n, static_cast<uint32_t*>(out), counters, err); });
}

// A list query is a count walk, the scan of its counts into offsets, and a fill walk: radius search over points, box search over boxes,
// triangle search over caller triangles, plane-cut search over planes, hit lists over rays.  The counts, the scan's scratch and the staging buffers (d_rd_*) are shared:
// the queries use them between launches of one call on the context's stream, which orders them, and the host forms wait for the stream
// before they return.
struct ListQuery {
    const char* noun;              // the input records in the error texts
    const char* entries;           // the output records there
    size_t in_bytes;
    Flags flags;
    uint32_t waves_per_simd; int short_stack;      // the knobs of its walk (hit lists: of the fill walk; the count walk is pt_count_hits')
    // the count walk into `counts` (offsets = nullptr), or the fill walk from `offsets` into `entries`: device memory, no host wait
    int (*walk)(PtContext*, const ListQuery&, const void* in, uint32_t n, uint32_t flags, void* counts, const unsigned long long* offsets, void* entries, uint64_t capacity);
    bool (*twin)(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const float* in, uint64_t n, uint64_t* offsets, uint32_t* entries,
                 uint64_t capacity, uint32_t flags, uint64_t* counters, std::string& err);
};

// the count walk into the context's buffer and the scan into `offsets`: two launches, no host wait
int list_offsets_on_stream(PtContext* ctx, const ListQuery& q, const void* in, uint32_t n, uint32_t flags, unsigned long long* offsets) {
    const size_t temp_bytes = ptk::radius_scan_temp_bytes(n);
    PT_HIP(ctx, ctx->d_rd_counts.ensure(size_t(n))); PT_HIP(ctx, ctx->d_rd_temp.ensure(temp_bytes));
    if (int rc = q.walk(ctx, q, in, n, flags, ctx->d_rd_counts.ptr, nullptr, nullptr, 0)) return rc;
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
    return q.walk(ctx, q, in, uint32_t(n), flags, nullptr, offsets, entries, capacity);
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
    if (int rc = q.walk(ctx, q, ctx->d_rq_rays.ptr, uint32_t(n), flags, nullptr, ctx->d_rd_offsets.ptr, ctx->d_rd_entries.ptr, held)) return rc;
    PT_HIP(ctx, hipMemcpyAsync(entries, ctx->d_rd_entries.ptr, size_t(held) * sizeof(uint4), hipMemcpyDeviceToHost, ctx->stream));
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PT_OK;
}

// The forms of a list query called `fn`: flags, batch size and the pointers, then the scene.  list_search: three launches, no host wait
// (hit lists with PT_HITS_SORTED: four).
int check_search(PtContext* ctx, const char* fn, const ListQuery& q, const void* in, uint64_t n, uint32_t flags, const void* offsets, const void* entries, uint64_t capacity) {
    if (int rc = check_input(ctx, fn, flags, q.flags.known, n, q.noun, in)) return rc;
    if (int rc = check_list(ctx, fn, offsets, entries, capacity, q.entries)) return rc;
    return check_scene(ctx, fn);
}
int list_search(PtContext* ctx, const char* fn, const ListQuery& q, const void* in, uint64_t n, uint32_t flags, void* offsets, void* entries, uint64_t capacity) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_search(ctx, fn, q, in, n, flags, offsets, entries, capacity)) return rc;
    return list_device(ctx, q, in, n, flags, offsets, entries, capacity);
}
int list_search_host(PtContext* ctx, const char* fn, const ListQuery& q, const void* in, uint64_t n, uint32_t flags, uint64_t* offsets, void* entries, uint64_t capacity) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_search(ctx, fn, q, in, n, flags, offsets, entries, capacity)) return rc;
    return list_host(ctx, q, in, n, flags, offsets, entries, capacity);
}
int list_bvh4(const char* fn, const ListQuery& q, const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const void* in, uint64_t n,
              uint32_t flags, uint64_t* offsets, void* entries, uint64_t capacity, PtStats* stats) {
    const bool brute = (flags & q.flags.brute) != 0;
    if (int rc = check_list_bvh4(fn, flags, q.flags.known, brute, tris, num_tris, bvh4, in, n, q.noun, offsets, entries, capacity)) return rc;
    return run_twin(bvh4, brute, (flags & q.flags.stats) != 0, stats, [&](const uint32_t* tree, uint64_t* counters, std::string& err) {
        return q.twin(tris, num_tris, tree, words, static_cast<const float*>(in), n, offsets, static_cast<uint32_t*>(entries), capacity, flags, counters, err); });
}

// The region queries (radius: points, box: boxes, tri: caller triangles, cut: planes) are list queries with one launcher for both walks, and a count of
// their own: the count walk alone, an item-to-record query.  The STATS flag counts over the count walk only; its fill walk is the
// one-item-per-thread kernel.
template <decltype(&ptk::launch_radius) launch>
int region_walk(PtContext* ctx, const ListQuery& q, const void* in, uint32_t n, uint32_t flags, void* counts, const unsigned long long* offsets, void* entries, uint64_t capacity) {
    const bool fill = offsets != nullptr, brute = (flags & q.flags.brute) != 0;
    const bool stats = (flags & q.flags.stats) != 0 && !fill, simple = (flags & (q.flags.simple | q.flags.stats)) != 0;
    Walk W;
    if (int rc = begin_walk(ctx, n, q.waves_per_simd, q.short_stack, stats, !simple && !brute, W)) return rc;
    if (W.launch) PT_HIP(ctx, launch(W.A, in, n, counts, offsets, entries, capacity, simple, stats, brute, ctx->d_rq_queue.ptr, ctx->d_rq_spill.ptr, W.grid, ctx->stream));
    return end_walk(ctx, W);
}
template <decltype(&pt::radius_search) twin>
bool region_twin(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const float* in, uint64_t n, uint64_t* offsets, uint32_t* entries,
                 uint64_t capacity, uint32_t, uint64_t* counters, std::string& err) {
    return twin(tris, num_tris, bvh4, words, in, n, offsets, entries, capacity, counters, err);
}
struct RegionCount {               // one call of a region query's count
    const ListQuery& q; uint32_t flags;
    size_t in_bytes = q.in_bytes, out_bytes = sizeof(uint32_t);
    int check(PtContext* ctx, const char* fn, const void* in, uint64_t n, const void* counts) const {
        if (int rc = check_input(ctx, fn, flags, q.flags.known, n, q.noun, in)) return rc;
        if (int rc = check_counts(ctx, fn, counts)) return rc;
        return check_scene(ctx, fn);
    }
    int run(PtContext* ctx, const void* in, uint32_t n, void* counts) const { return q.walk(ctx, q, in, n, flags, counts, nullptr, nullptr, 0); }
};

} // namespace

extern "C" {

// ---- batched ray queries (include/mi355pt.h; pt_rayquery.hip) ----------------------------------------------------------------

static_assert(sizeof(PtRay) == 32 && sizeof(PtHit) == 16, "PtRay / PtHit are read and written as 2 x 16 B and 16 B records");

namespace {
struct Trace {
    uint32_t flags;
    static constexpr uint32_t known = PT_TRACE_ANY_HIT | PT_TRACE_STATS | PT_TRACE_SIMPLE_KERNEL;
    static constexpr size_t in_bytes = sizeof(PtRay), out_bytes = sizeof(PtHit);
    int check(PtContext* ctx, const char* fn, const void* rays, uint64_t n, const void* hits) const {
        if (int rc = check_flags(ctx, fn, flags, known)) return rc;
        if (int rc = check_n(ctx, fn, n, "rays")) return rc;
        if (int rc = check_records(ctx, fn, "rays and hits", {rays, hits})) return rc;
        return check_scene(ctx, fn);
    }
    int run(PtContext* ctx, const void* rays, uint32_t n, void* hits) const {
        const bool anyhit = (flags & PT_TRACE_ANY_HIT) != 0, stats = (flags & PT_TRACE_STATS) != 0, simple = (flags & PT_TRACE_SIMPLE_KERNEL) != 0;
        Walk W;
        if (int rc = begin_walk(ctx, n, PT_RQ_WAVES_PER_SIMD, PT_RQ_SHORT_STACK, stats, !simple, W)) return rc;
        if (W.launch) PT_HIP(ctx, ptk::launch_trace_rays(W.A, rays, hits, n, anyhit, simple, stats, ctx->d_rq_queue.ptr, ctx->d_rq_spill.ptr, W.grid, ctx->stream));
        return end_walk(ctx, W);
    }
};
} // namespace

int pt_trace_rays(PtContext* ctx, const void* rays_device, uint64_t n, uint32_t flags, void* hits_device) {
    return item_device(ctx, "pt_trace_rays", Trace{flags}, rays_device, n, hits_device);
}

int pt_trace_rays_host(PtContext* ctx, const PtRay* rays, uint64_t n, uint32_t flags, PtHit* hits) {
    return item_host(ctx, "pt_trace_rays_host", Trace{flags}, rays, n, hits);
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
constexpr WalkQuery kClosest = {"points", "points and results must be non-null and 16-byte aligned", sizeof(PtPoint), sizeof(PtClosest),
                                {PT_CLOSEST_STATS | PT_CLOSEST_SIMPLE_KERNEL | PT_CLOSEST_BRUTE_FORCE, PT_CLOSEST_STATS, PT_CLOSEST_SIMPLE_KERNEL, PT_CLOSEST_BRUTE_FORCE},
                                PT_PQ_WAVES_PER_SIMD, PT_PQ_SHORT_STACK, ptk::launch_closest_points, pt::closest_points};
} // namespace

int pt_closest_points(PtContext* ctx, const void* points_device, uint64_t n, uint32_t flags, void* out_device) {
    return item_device(ctx, "pt_closest_points", Walked{kClosest, flags}, points_device, n, out_device);
}

int pt_closest_points_host(PtContext* ctx, const PtPoint* points, uint64_t n, uint32_t flags, PtClosest* out) {
    return item_host(ctx, "pt_closest_points_host", Walked{kClosest, flags}, points, n, out);
}

int pt_closest_points_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words,
                           const PtPoint* points, uint64_t n, uint32_t flags, PtClosest* out, PtStats* stats) {
    return walk_bvh4("pt_closest_points_bvh4", kClosest, tris, num_tris, bvh4, words, points, n, flags, out, stats);
}

// ---- sphere-cast queries (include/mi355pt.h; pt_sweep.hip) ---------------------------------------------------------------------

static_assert(sizeof(PtSweep) == 32, "PtSweep is read as 2 x 16 B");

namespace {
constexpr WalkQuery kSweep = {"sweeps", "sweeps and hits must be non-null and 16-byte aligned", sizeof(PtSweep), sizeof(PtHit),
                              {PT_SWEEP_STATS | PT_SWEEP_SIMPLE_KERNEL | PT_SWEEP_BRUTE_FORCE, PT_SWEEP_STATS, PT_SWEEP_SIMPLE_KERNEL, PT_SWEEP_BRUTE_FORCE},
                              PT_SW_WAVES_PER_SIMD, PT_SW_SHORT_STACK, ptk::launch_sweep, pt::sweep_spheres};
} // namespace

int pt_sweep_spheres(PtContext* ctx, const void* sweeps_device, uint64_t n, uint32_t flags, void* hits_device) {
    return item_device(ctx, "pt_sweep_spheres", Walked{kSweep, flags}, sweeps_device, n, hits_device);
}

int pt_sweep_spheres_host(PtContext* ctx, const PtSweep* sweeps, uint64_t n, uint32_t flags, PtHit* hits) {
    return item_host(ctx, "pt_sweep_spheres_host", Walked{kSweep, flags}, sweeps, n, hits);
}

int pt_sweep_spheres_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words,
                          const PtSweep* sweeps, uint64_t n, uint32_t flags, PtHit* out, PtStats* stats) {
    return walk_bvh4("pt_sweep_spheres_bvh4", kSweep, tris, num_tris, bvh4, words, sweeps, n, flags, out, stats);
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
struct Occlusion {
    const PtOcclusionParams* p;
    static constexpr size_t in_bytes = sizeof(PtSurfel), out_bytes = sizeof(PtOcclusion);
    int check(PtContext* ctx, const char* fn, const void* surfels, uint64_t n, const void* out) const { return check_occlusion(ctx, fn, surfels, n, p, out, true); }
    int run(PtContext* ctx, const void* surfels, uint32_t n, void* out) const {
        const bool stats = (p->flags & PT_OCCLUSION_STATS) != 0, simple = (p->flags & PT_OCCLUSION_SIMPLE_KERNEL) != 0;
        Walk W;
        if (int rc = begin_walk(ctx, n, PT_OC_WAVES_PER_SIMD, PT_OC_SHORT_STACK, stats, !simple, W)) return rc;
        if (W.launch) PT_HIP(ctx, ptk::launch_occlusion(W.A, surfels, out, n, p->samples, p->seed, p->index_base, p->bias, simple, stats, ctx->d_rq_queue.ptr, ctx->d_rq_spill.ptr, W.grid, ctx->stream));
        return end_walk(ctx, W);
    }
};
// rays and their hits in, surfels out: the batch size and the pointers, then the triangles (no tree is walked)
int check_surfels(PtContext* ctx, const char* fn, const void* rays, const void* hits, uint64_t n, const void* surfels) {
    if (int rc = check_n(ctx, fn, n, "rays")) return rc;
    if (int rc = check_records(ctx, fn, "rays, hits and surfels", {rays, hits, surfels})) return rc;
    if (!ctx->have_tris) return fail(ctx, PT_ERR_NO_SCENE, std::string(fn) + ": no triangles set");
    return PT_OK;
}
} // namespace

int pt_occlusion(PtContext* ctx, const void* surfels_device, uint64_t n, const PtOcclusionParams* params, void* out_device) {
    return item_device(ctx, "pt_occlusion", Occlusion{params}, surfels_device, n, out_device);
}

int pt_occlusion_host(PtContext* ctx, const PtSurfel* surfels, uint64_t n, const PtOcclusionParams* params, PtOcclusion* out) {
    return item_host(ctx, "pt_occlusion_host", Occlusion{params}, surfels, n, out);
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
constexpr WalkQuery kCount = {"rays", "rays must be non-null and 16-byte aligned, counts non-null and 4-byte aligned", sizeof(PtRay), sizeof(uint32_t),
                              {PT_COUNT_STATS | PT_COUNT_SIMPLE_KERNEL | PT_COUNT_BRUTE_FORCE, PT_COUNT_STATS, PT_COUNT_SIMPLE_KERNEL, PT_COUNT_BRUTE_FORCE},
                              PT_CR_WAVES_PER_SIMD, PT_CR_SHORT_STACK, ptk::launch_count_hits, pt::count_hits};
constexpr uint32_t kContainFlags = PT_CONTAIN_STATS | PT_CONTAIN_SIMPLE_KERNEL;

// the parameter block and the batch size; the pointers and the scene are checked by the callers (pointers before the scene)
int check_contain_params(PtContext* ctx, const char* fn, uint64_t n, const PtContainParams* p) {
    if (!p) return bad_arg(ctx, fn, "null params");
    if (int rc = check_flags(ctx, fn, p->flags, kContainFlags)) return rc;
    if (int rc = check_n(ctx, fn, n, "points")) return rc;
    if (p->samples < 1u || p->samples > 255u || (p->samples & 1u) == 0u) return bad_arg(ctx, fn, "samples must be odd and in 1..255");
    return check_n(ctx, fn, n * uint64_t(p->samples), "sample rays (n * samples)");
}
struct Contains {
    const PtContainParams* p;
    static constexpr size_t in_bytes = sizeof(PtPoint), out_bytes = sizeof(PtContainment);
    int check(PtContext* ctx, const char* fn, const void* points, uint64_t n, const void* out) const {
        if (int rc = check_contain_params(ctx, fn, n, p)) return rc;
        if (int rc = check_records(ctx, fn, "points and results", {points, out})) return rc;
        return check_scene(ctx, fn);
    }
    int run(PtContext* ctx, const void* points, uint32_t n, void* out) const {
        const bool stats = (p->flags & PT_CONTAIN_STATS) != 0, simple = (p->flags & PT_CONTAIN_SIMPLE_KERNEL) != 0;
        Walk W;
        if (int rc = begin_walk(ctx, n, PT_CR_WAVES_PER_SIMD, PT_CR_SHORT_STACK, stats, !simple, W)) return rc;
        if (W.launch) PT_HIP(ctx, ptk::launch_contains(W.A, points, out, n, p->samples, p->seed, p->index_base, simple, stats, ctx->d_rq_queue.ptr, ctx->d_rq_spill.ptr, W.grid, ctx->stream));
        return end_walk(ctx, W);
    }
};
// containment's check and records (PtClosest is as large as PtContainment); three launches, no host wait: the closest points into `out`,
// the containment into the context's buffer, the sign
struct SignedDistance : Contains {
    int run(PtContext* ctx, const void* points, uint32_t n, void* out) const {
        if (int rc = flush_pending(ctx)) return rc;
        if (n == 0u) return PT_OK;
        PT_HIP(ctx, ctx->d_cr_contain.ensure(size_t(n)));
        if (int rc = Walked{kClosest, 0u}.run(ctx, points, n, out)) return rc;
        if (int rc = Contains::run(ctx, points, n, ctx->d_cr_contain.ptr)) return rc;
        PT_HIP(ctx, ptk::launch_apply_sign(ctx->d_cr_contain.ptr, out, n, ctx->stream));
        return PT_OK;
    }
};
static_assert(sizeof(PtClosest) == sizeof(PtContainment), "pt_signed_distance_host stages its results as pt_contains_host does");
} // namespace

int pt_count_hits(PtContext* ctx, const void* rays_device, uint64_t n, uint32_t flags, void* counts_device) {
    return item_device(ctx, "pt_count_hits", Walked{kCount, flags}, rays_device, n, counts_device);
}

int pt_count_hits_host(PtContext* ctx, const PtRay* rays, uint64_t n, uint32_t flags, uint32_t* counts) {
    return item_host(ctx, "pt_count_hits_host", Walked{kCount, flags}, rays, n, counts);
}

int pt_count_hits_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words,
                       const PtRay* rays, uint64_t n, uint32_t flags, uint32_t* counts, PtStats* stats) {
    return walk_bvh4("pt_count_hits_bvh4", kCount, tris, num_tris, bvh4, words, rays, n, flags, counts, stats);
}

int pt_contains(PtContext* ctx, const void* points_device, uint64_t n, const PtContainParams* params, void* out_device) {
    return item_device(ctx, "pt_contains", Contains{params}, points_device, n, out_device);
}

int pt_contains_host(PtContext* ctx, const PtPoint* points, uint64_t n, const PtContainParams* params, PtContainment* out) {
    return item_host(ctx, "pt_contains_host", Contains{params}, points, n, out);
}

// no brute force: the tree is always needed
int pt_contains_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words,
                     const PtPoint* points, uint64_t n, const PtContainParams* params, PtContainment* out, PtStats* stats) {
    if (int rc = check_contain_params(nullptr, "pt_contains_bvh4", n, params)) return rc;
    if (int rc = check_item_bvh4("pt_contains_bvh4", false, tris, num_tris, bvh4, points, out, n, "points")) return rc;
    return run_twin(bvh4, false, (params->flags & PT_CONTAIN_STATS) != 0, stats, [&](const uint32_t* tree, uint64_t* counters, std::string& err) {
        return pt::contains(tris, num_tris, tree, words, reinterpret_cast<const float*>(points), n, params->samples, params->seed, params->index_base,
                            reinterpret_cast<uint32_t*>(out), counters, err); });
}

int pt_signed_distance(PtContext* ctx, const void* points_device, uint64_t n, const PtContainParams* params, void* out_device) {
    return item_device(ctx, "pt_signed_distance", SignedDistance{{params}}, points_device, n, out_device);
}

int pt_signed_distance_host(PtContext* ctx, const PtPoint* points, uint64_t n, const PtContainParams* params, PtClosest* out) {
    return item_host(ctx, "pt_signed_distance_host", SignedDistance{{params}}, points, n, out);
}

// ---- radius queries (include/mi355pt.h; pt_radius.hip) -------------------------------------------------------------------------

namespace {
// The region queries share their flags' values.
constexpr Flags kRegionFlags = {PT_RADIUS_STATS | PT_RADIUS_SIMPLE_KERNEL | PT_RADIUS_BRUTE_FORCE, PT_RADIUS_STATS, PT_RADIUS_SIMPLE_KERNEL, PT_RADIUS_BRUTE_FORCE};
static_assert(PT_BOX_STATS == PT_RADIUS_STATS && PT_BOX_SIMPLE_KERNEL == PT_RADIUS_SIMPLE_KERNEL && PT_BOX_BRUTE_FORCE == PT_RADIUS_BRUTE_FORCE,
              "the PT_BOX_* flags take the values of the PT_RADIUS_* flags");
static_assert(PT_TRI_STATS == PT_RADIUS_STATS && PT_TRI_SIMPLE_KERNEL == PT_RADIUS_SIMPLE_KERNEL && PT_TRI_BRUTE_FORCE == PT_RADIUS_BRUTE_FORCE,
              "the PT_TRI_* flags take the values of the PT_RADIUS_* flags");

constexpr ListQuery kRadius = {"points", "entries", sizeof(PtPoint), kRegionFlags, PT_RD_WAVES_PER_SIMD, PT_RD_SHORT_STACK,
                               region_walk<ptk::launch_radius>, region_twin<pt::radius_search>};
} // namespace

int pt_radius_count(PtContext* ctx, const void* points_device, uint64_t n, uint32_t flags, void* counts_device) {
    return item_device(ctx, "pt_radius_count", RegionCount{kRadius, flags}, points_device, n, counts_device);
}

int pt_radius_count_host(PtContext* ctx, const PtPoint* points, uint64_t n, uint32_t flags, uint32_t* counts) {
    return item_host(ctx, "pt_radius_count_host", RegionCount{kRadius, flags}, points, n, counts, &PtContext::d_rd_counts);
}

int pt_radius_search(PtContext* ctx, const void* points_device, uint64_t n, uint32_t flags, void* offsets_device, void* entries_device, uint64_t capacity) {
    return list_search(ctx, "pt_radius_search", kRadius, points_device, n, flags, offsets_device, entries_device, capacity);
}

int pt_radius_search_host(PtContext* ctx, const PtPoint* points, uint64_t n, uint32_t flags, uint64_t* offsets, PtClosest* entries, uint64_t capacity) {
    return list_search_host(ctx, "pt_radius_search_host", kRadius, points, n, flags, offsets, entries, capacity);
}

int pt_radius_search_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const PtPoint* points, uint64_t n,
                          uint32_t flags, uint64_t* offsets, PtClosest* entries, uint64_t capacity, PtStats* stats) {
    return list_bvh4("pt_radius_search_bvh4", kRadius, tris, num_tris, bvh4, words, points, n, flags, offsets, entries, capacity, stats);
}

// ---- box-overlap queries (include/mi355pt.h; pt_overlap.hip) --------------------------------------------------------------------

static_assert(sizeof(PtBox) == 32 && sizeof(PtOverlap) == sizeof(uint4), "PtBox / PtOverlap are read and written as 2 x 16 B and 16 B records");

namespace {
constexpr ListQuery kBox = {"boxes", "entries", sizeof(PtBox), kRegionFlags, PT_BX_WAVES_PER_SIMD, PT_BX_SHORT_STACK,
                            region_walk<ptk::launch_box>, region_twin<pt::box_search>};
} // namespace

int pt_box_count(PtContext* ctx, const void* boxes_device, uint64_t n, uint32_t flags, void* counts_device) {
    return item_device(ctx, "pt_box_count", RegionCount{kBox, flags}, boxes_device, n, counts_device);
}

int pt_box_count_host(PtContext* ctx, const PtBox* boxes, uint64_t n, uint32_t flags, uint32_t* counts) {
    return item_host(ctx, "pt_box_count_host", RegionCount{kBox, flags}, boxes, n, counts, &PtContext::d_rd_counts);
}

int pt_box_search(PtContext* ctx, const void* boxes_device, uint64_t n, uint32_t flags, void* offsets_device, void* entries_device, uint64_t capacity) {
    return list_search(ctx, "pt_box_search", kBox, boxes_device, n, flags, offsets_device, entries_device, capacity);
}

int pt_box_search_host(PtContext* ctx, const PtBox* boxes, uint64_t n, uint32_t flags, uint64_t* offsets, PtOverlap* entries, uint64_t capacity) {
    return list_search_host(ctx, "pt_box_search_host", kBox, boxes, n, flags, offsets, entries, capacity);
}

int pt_box_search_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const PtBox* boxes, uint64_t n,
                       uint32_t flags, uint64_t* offsets, PtOverlap* entries, uint64_t capacity, PtStats* stats) {
    return list_bvh4("pt_box_search_bvh4", kBox, tris, num_tris, bvh4, words, boxes, n, flags, offsets, entries, capacity, stats);
}

// ---- triangle-overlap queries (include/mi355pt.h; pt_tritri.hip) -----------------------------------------------------------------

static_assert(sizeof(PtTri) == 48 && sizeof(PtCross) == sizeof(uint4), "PtTri / PtCross are read and written as 3 x 16 B and 16 B records");

namespace {
constexpr ListQuery kTri = {"triangles", "entries", sizeof(PtTri), kRegionFlags, PT_TT_WAVES_PER_SIMD, PT_TT_SHORT_STACK,
                            region_walk<ptk::launch_tri>, region_twin<pt::tri_search>};
} // namespace

int pt_tri_count(PtContext* ctx, const void* tris_device, uint64_t n, uint32_t flags, void* counts_device) {
    return item_device(ctx, "pt_tri_count", RegionCount{kTri, flags}, tris_device, n, counts_device);
}

int pt_tri_count_host(PtContext* ctx, const PtTri* tris, uint64_t n, uint32_t flags, uint32_t* counts) {
    return item_host(ctx, "pt_tri_count_host", RegionCount{kTri, flags}, tris, n, counts, &PtContext::d_rd_counts);
}

int pt_tri_search(PtContext* ctx, const void* tris_device, uint64_t n, uint32_t flags, void* offsets_device, void* entries_device, uint64_t capacity) {
    return list_search(ctx, "pt_tri_search", kTri, tris_device, n, flags, offsets_device, entries_device, capacity);
}

int pt_tri_search_host(PtContext* ctx, const PtTri* tris, uint64_t n, uint32_t flags, uint64_t* offsets, PtCross* entries, uint64_t capacity) {
    return list_search_host(ctx, "pt_tri_search_host", kTri, tris, n, flags, offsets, entries, capacity);
}

int pt_tri_search_bvh4(const float* mesh, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const PtTri* tris, uint64_t n,
                       uint32_t flags, uint64_t* offsets, PtCross* entries, uint64_t capacity, PtStats* stats) {
    return list_bvh4("pt_tri_search_bvh4", kTri, mesh, num_tris, bvh4, words, tris, n, flags, offsets, entries, capacity, stats);
}

// ---- plane-cut queries (include/mi355pt.h; pt_cut.hip) ---------------------------------------------------------------------------

static_assert(sizeof(PtCutPlane) == 48 && sizeof(PtCut) == sizeof(uint4), "PtCutPlane / PtCut are read and written as 3 x 16 B and 16 B records");
static_assert(PT_CUT_STATS == PT_RADIUS_STATS && PT_CUT_SIMPLE_KERNEL == PT_RADIUS_SIMPLE_KERNEL && PT_CUT_BRUTE_FORCE == PT_RADIUS_BRUTE_FORCE,
              "the PT_CUT_* flags take the values of the PT_RADIUS_* flags");

namespace {
constexpr ListQuery kCut = {"planes", "entries", sizeof(PtCutPlane), kRegionFlags, PT_CT_WAVES_PER_SIMD, PT_CT_SHORT_STACK,
                            region_walk<ptk::launch_cut>, region_twin<pt::cut_search>};
} // namespace

int pt_cut_count(PtContext* ctx, const void* planes_device, uint64_t n, uint32_t flags, void* counts_device) {
    return item_device(ctx, "pt_cut_count", RegionCount{kCut, flags}, planes_device, n, counts_device);
}

int pt_cut_count_host(PtContext* ctx, const PtCutPlane* planes, uint64_t n, uint32_t flags, uint32_t* counts) {
    return item_host(ctx, "pt_cut_count_host", RegionCount{kCut, flags}, planes, n, counts, &PtContext::d_rd_counts);
}

int pt_cut_search(PtContext* ctx, const void* planes_device, uint64_t n, uint32_t flags, void* offsets_device, void* entries_device, uint64_t capacity) {
    return list_search(ctx, "pt_cut_search", kCut, planes_device, n, flags, offsets_device, entries_device, capacity);
}

int pt_cut_search_host(PtContext* ctx, const PtCutPlane* planes, uint64_t n, uint32_t flags, uint64_t* offsets, PtCut* entries, uint64_t capacity) {
    return list_search_host(ctx, "pt_cut_search_host", kCut, planes, n, flags, offsets, entries, capacity);
}

int pt_cut_search_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const PtCutPlane* planes, uint64_t n,
                       uint32_t flags, uint64_t* offsets, PtCut* entries, uint64_t capacity, PtStats* stats) {
    return list_bvh4("pt_cut_search_bvh4", kCut, tris, num_tris, bvh4, words, planes, n, flags, offsets, entries, capacity, stats);
}

// ---- hit lists (include/mi355pt.h; pt_hitlist.hip) ------------------------------------------------------------------------------

static_assert(sizeof(PtClosest) == sizeof(uint4) && sizeof(PtHit) == sizeof(uint4), "the entries of both list queries are staged as 16 B records");

namespace {
static_assert(PT_HITS_STATS == PT_COUNT_STATS && PT_HITS_SIMPLE_KERNEL == PT_COUNT_SIMPLE_KERNEL && PT_HITS_BRUTE_FORCE == PT_COUNT_BRUTE_FORCE,
              "the count walk of pt_list_hits is pt_count_hits' with the same flags");

// The count walk: pt_count_hits' own launch, counters included.  The fill walk from `offsets` into `hits` and, with PT_HITS_SORTED, the
// sort: one or two launches.  PT_HITS_STATS counted over the count walk; its fill walk is the one-ray-per-thread kernel.
int hits_walk(PtContext* ctx, const ListQuery& q, const void* rays, uint32_t n, uint32_t flags, void* counts, const unsigned long long* offsets, void* hits, uint64_t capacity) {
    if (!offsets) return Walked{kCount, flags & kCount.flags.known}.run(ctx, rays, n, counts);
    const bool brute = (flags & PT_HITS_BRUTE_FORCE) != 0, simple = (flags & (PT_HITS_SIMPLE_KERNEL | PT_HITS_STATS)) != 0;
    Walk W;
    if (int rc = begin_walk(ctx, n, q.waves_per_simd, q.short_stack, false, !simple && !brute, W)) return rc;
    if (!W.launch) return PT_OK;
    PT_HIP(ctx, ptk::launch_hit_fill(W.A, rays, n, offsets, hits, capacity, simple, brute, ctx->d_rq_queue.ptr, ctx->d_rq_spill.ptr, W.grid, ctx->stream));
    if (flags & PT_HITS_SORTED) PT_HIP(ctx, ptk::launch_hit_sort(offsets, hits, capacity, n, ctx->stream));
    return end_walk(ctx, W);
}
bool hits_twin(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const float* rays, uint64_t n, uint64_t* offsets, uint32_t* hits,
               uint64_t capacity, uint32_t flags, uint64_t* counters, std::string& err) {
    return pt::list_hits(tris, num_tris, bvh4, words, rays, n, offsets, hits, capacity, (flags & PT_HITS_SORTED) != 0, counters, err);
}
constexpr ListQuery kHits = {"rays", "hits", sizeof(PtRay),
                             {PT_HITS_STATS | PT_HITS_SIMPLE_KERNEL | PT_HITS_BRUTE_FORCE | PT_HITS_SORTED, PT_HITS_STATS, PT_HITS_SIMPLE_KERNEL, PT_HITS_BRUTE_FORCE},
                             PT_HL_WAVES_PER_SIMD, PT_HL_SHORT_STACK, hits_walk, hits_twin};
} // namespace

int pt_list_hits(PtContext* ctx, const void* rays_device, uint64_t n, uint32_t flags, void* offsets_device, void* hits_device, uint64_t capacity) {
    return list_search(ctx, "pt_list_hits", kHits, rays_device, n, flags, offsets_device, hits_device, capacity);
}

int pt_list_hits_host(PtContext* ctx, const PtRay* rays, uint64_t n, uint32_t flags, uint64_t* offsets, PtHit* hits, uint64_t capacity) {
    return list_search_host(ctx, "pt_list_hits_host", kHits, rays, n, flags, offsets, hits, capacity);
}

int pt_list_hits_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const PtRay* rays, uint64_t n,
                      uint32_t flags, uint64_t* offsets, PtHit* hits, uint64_t capacity, PtStats* stats) {
    return list_bvh4("pt_list_hits_bvh4", kHits, tris, num_tris, bvh4, words, rays, n, flags, offsets, hits, capacity, stats);
}

// ---- k-nearest queries (include/mi355pt.h; pt_knn.hip) --------------------------------------------------------------------------

static_assert(PT_NEAREST_MAX_K == ptk::kNearestMaxK && PT_NEAREST_MAX_K == pt::kNearestMaxK, "one PT_NEAREST_MAX_K for the header, the kernels and the twin");

namespace {
// n points in, n rows of k records out; the grid depends on k
struct Nearest {
    uint32_t k, flags;
    static constexpr uint32_t known = PT_NEAREST_STATS | PT_NEAREST_SIMPLE_KERNEL | PT_NEAREST_BRUTE_FORCE;
    size_t in_bytes = sizeof(PtPoint), out_bytes = size_t(k) * sizeof(PtClosest);
    int check_k(PtContext* ctx, const char* fn) const {
        if (int rc = check_flags(ctx, fn, flags, known)) return rc;
        return k == 0u || k > PT_NEAREST_MAX_K ? bad_arg(ctx, fn, "k must be 1 .. PT_NEAREST_MAX_K") : PT_OK;
    }
    int check(PtContext* ctx, const char* fn, const void* points, uint64_t n, const void* out) const {
        if (int rc = check_k(ctx, fn)) return rc;
        if (int rc = check_n(ctx, fn, n, "points")) return rc;
        if (int rc = check_records(ctx, fn, "points and results", {points, out})) return rc;
        return check_scene(ctx, fn);
    }
    int run(PtContext* ctx, const void* points, uint32_t n, void* out) const {
        const bool stats = (flags & PT_NEAREST_STATS) != 0, simple = (flags & PT_NEAREST_SIMPLE_KERNEL) != 0, brute = (flags & PT_NEAREST_BRUTE_FORCE) != 0;
        Walk W;
        if (int rc = begin_walk(ctx, n, ptk::nearest_k_waves_per_simd(k), PT_NK_SHORT_STACK, stats, !simple && !brute, W)) return rc;
        if (W.launch) PT_HIP(ctx, ptk::launch_nearest_k(W.A, points, out, n, k, simple, stats, brute, ctx->d_rq_queue.ptr, ctx->d_rq_spill.ptr, W.grid, ctx->stream));
        return end_walk(ctx, W);
    }
};
} // namespace

int pt_nearest_k(PtContext* ctx, const void* points_device, uint64_t n, uint32_t k, uint32_t flags, void* out_device) {
    return item_device(ctx, "pt_nearest_k", Nearest{k, flags}, points_device, n, out_device);
}

int pt_nearest_k_host(PtContext* ctx, const PtPoint* points, uint64_t n, uint32_t k, uint32_t flags, PtClosest* out) {
    return item_host(ctx, "pt_nearest_k_host", Nearest{k, flags}, points, n, out);
}

int pt_nearest_k_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const PtPoint* points, uint64_t n,
                      uint32_t k, uint32_t flags, PtClosest* out, PtStats* stats) {
    if (int rc = Nearest{k, flags}.check_k(nullptr, "pt_nearest_k_bvh4")) return rc;
    const bool brute = (flags & PT_NEAREST_BRUTE_FORCE) != 0;
    if (int rc = check_item_bvh4("pt_nearest_k_bvh4", brute, tris, num_tris, bvh4, points, out, n, "points")) return rc;
    return run_twin(bvh4, brute, (flags & PT_NEAREST_STATS) != 0, stats, [&](const uint32_t* tree, uint64_t* counters, std::string& err) {
        return pt::nearest_k(tris, num_tris, tree, words, reinterpret_cast<const float*>(points), n, k, reinterpret_cast<uint32_t*>(out), counters, err); });
}

} // extern "C"
