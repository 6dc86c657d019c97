// pt_context.h -- private to libmi355pt: the context behind the opaque PtContext of include/mi355pt.h, and the few helpers that every
// translation unit of the C ABI starts an entry point with (pt_api.cpp defines them; pt_api_queries.cpp is their other user).
// Declarations and types only.
#pragma once
#include "mi355pt.h"
#include "pt_host.h"
#include "pt_kernels.h"

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

template <typename T>
struct DevBuf {
    T* ptr = nullptr; size_t cap = 0;   // capacity in elements
    hipError_t ensure(size_t n) {
        if (n <= cap && ptr) return hipSuccess;
        if (ptr) { (void)hipFree(ptr); ptr = nullptr; cap = 0; }
        if (n == 0) n = 1;
        hipError_t e = hipMalloc((void**)&ptr, n * sizeof(T));
        if (e == hipSuccess) cap = n;
        return e;
    }
    void release() { if (ptr) (void)hipFree(ptr); ptr = nullptr; cap = 0; }
};

// Development overrides of the megakernel's launch heuristics.  kAuto = use the measured default for the launch at hand.
// Read from PT_TUNE_* ONCE, when the context is created (a shipped library does not consult the environment per launch);
// tests and tools/ab/sweep.sh change them through pt_debug_set_tune.
struct PtTune {
    static constexpr uint32_t kAuto = 0xFFFFFFFFu;
    uint32_t grid_div = kAuto, rows = kAuto, chunk = kAuto, xcd = kAuto, shade = kAuto, fill = kAuto,
             slots = kAuto, cull = kAuto, stats_batch = kAuto, quad = kAuto, fork = kAuto, bounded = kAuto, timeline = kAuto, expose = kAuto, expose_budget = kAuto;
    uint32_t* find(const char* name) {
        static const struct { const char* n; uint32_t PtTune::* m; } tab[] = {
            {"GRIDDIV", &PtTune::grid_div}, {"ROWS", &PtTune::rows}, {"CHUNK", &PtTune::chunk}, {"XCD", &PtTune::xcd}, {"SHADE", &PtTune::shade},
            {"FILL", &PtTune::fill}, {"SLOTS", &PtTune::slots}, {"CULL", &PtTune::cull}, {"STATSBATCH", &PtTune::stats_batch}, {"QUAD", &PtTune::quad}, {"FORK", &PtTune::fork}, {"BOUNDED", &PtTune::bounded}, {"TIMELINE", &PtTune::timeline}, {"EXPOSE", &PtTune::expose}, {"EXBUDGET", &PtTune::expose_budget}};
        for (const auto& t : tab) if (std::strcmp(name, t.n) == 0) return &(this->*(t.m));
        return nullptr;
    }
    void from_environment() {
        static const char* names[] = {"GRIDDIV", "ROWS", "CHUNK", "XCD", "SHADE", "FILL", "SLOTS", "CULL", "STATSBATCH", "QUAD", "FORK", "BOUNDED", "TIMELINE", "EXPOSE", "EXBUDGET"};
        for (const char* n : names) {
            const std::string key = std::string("PT_TUNE_") + n;
            const char* v = std::getenv(key.c_str());
            if (v && *v) *find(n) = uint32_t(std::strtoul(v, nullptr, 10));
        }
    }
    static uint32_t pick(uint32_t knob, uint32_t dflt) { return knob == kAuto ? dflt : knob; }
};

struct PtContext {
    int device = 0;
    PtTune tune;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    bool timed = false;
    std::string err;

    // scene (host mirrors kept for rebuilds / readback of small metadata only)
    uint32_t num_tris = 0, num_nodes2 = 0, num_nodes4 = 0;
    bool edges_small = false;        // every |edge component| of the uploaded triangles is below 2^20 (pt_set_triangles; see arith_is_bounded)
    DevBuf<uint32_t> d_edge_max;
    bool have_tris = false, have_bvh = false, have_bvh2 = false;
    bool bvh2_refit_pending = false;  // pt_build_bvh leaves the internal BVH2 bounds to the first pt_read_bvh2 (nothing on the render path reads them)
    pt::WideBvh wide_meta;           // root info; nodes vector emptied after upload

    DevBuf<float> d_tris9;           // reference layout
    // One arena for the two record arrays the traversal gathers from: [triangle records, 64 B each, padded to a multiple of
    // 64 B | wide nodes, 64 B each]: one allocation, one base address, 32-bit byte offsets reach both kinds.
    DevBuf<uint4> d_scene; uint64_t node_off = 0, node_cap = 0; uint32_t scene_tris = 0;
    float4* trirec() const { return (float4*)d_scene.ptr; }
    uint4* wide() const { return d_scene.ptr + node_off / 16; }
    DevBuf<uint32_t> d_bvh2, d_bvh4; // reference layouts
    DevBuf<uint32_t> d_morton, d_triidx, d_parent, d_flags;
    // device-side scene build (pt_build.hip): scratch kept for rebuilds
    DevBuf<unsigned long long> d_bounds; DevBuf<uint32_t> d_counters, d_code_tmp, d_index_tmp, d_node2, d_subtree, d_ids, d_bnd;
    DevBuf<uint4> d_child_pos; DevBuf<unsigned char> d_build_temp; uint32_t* h_word = nullptr;
    DevBuf<uint32_t> d_ploc;         // PT_ACCEL_PLOC cluster buffers (ptk::ploc_words), allocated on first use
    DevBuf<float4> d_spheres; uint32_t num_spheres = 0;
    // refit in place (pt_update_triangles, pt_refit.hip).  The plan (ptk::RefitBuffers) is derived at the first update or pt_bvh_cost after
    // a tree was installed; every call that installs a tree drops it.  tree_built: the BVH4 is this library's own build (every node
    // reachable, d_ids still holds the wide indices of launch_internal_scan), so the plan is derived on the device.
    bool tree_built = false, refit_ready = false, refit2_ready = false;
    uint32_t num_wide = 0;            // wide nodes in the arena
    DevBuf<uint2> d_refit_up, d_refit_self; DevBuf<uint4> d_refit_ref; DevBuf<uint32_t> d_refit_arrive, d_refit_parent2, d_refit_arrive2;
    DevBuf<double> d_cost;
    bool bvh2_stale = false;          // the BVH2 still holds the boxes of earlier triangles: refitted by the next pt_read_bvh2
    // the host's copies after an update (root box, edge maximum) come back through a pinned block behind the refit; whoever reads them
    // next waits for that copy (sync_refit_meta)
    uint32_t* h_refit = nullptr; hipEvent_t ev_refit = nullptr; bool meta_pending = false, meta_has_root = false;
    // Tile cover (pt_cover.hip).  The cut of the wide tree is taken whenever a tree is installed (install_cut); tree_version counts
    // everything that changes a box (install, refit).  A cover -- the tiles the cut's live boxes reach from a set of cameras -- is
    // computed on a stream of its own that waits for nothing, read back through a pinned block, and kept until the cameras, the
    // resolution or the tree change: with an unchanged camera a launch adds no kernel, no copy and no host wait.  The last kCovers results
    // are kept (least recently used goes first), so a few alternating views -- stereo eyes, a diagnostics call between launches -- do
    // not evict each other.
    DevBuf<uint32_t> d_cut; uint32_t cut_count = 0, tree_version = 0;
    hipStream_t cover_stream = nullptr; DevBuf<uint32_t> d_cover; uint32_t* h_cover = nullptr; size_t h_cover_cap = 0;
    struct Cover {
        bool valid = false, computed = false, usable = false;      // valid: the view has been seen; computed: its mask is there; usable: every box could be projected (else the launch keeps the rectangle)
        uint32_t tree_version = 0, width = 0, height = 0, id = 0; uint64_t used = 0;
        std::vector<ptk::CoverCam> cams; std::vector<uint32_t> mask;
    };
    static constexpr int kCovers = 4;
    Cover covers[kCovers]; uint64_t cover_clock = 0;
    std::vector<ptk::CoverCam> cover_cams;                 // the distinct cameras of the launch being planned
    uint32_t cover_ids = 0;
    // Exposed triangles (pt_expose.hip): one bit per triangle that no shadow ray of the fixed light can be occluded on, computed in front of
    // the first large PT_MODE_PATH launch of a tree version (after pt_update_triangles: of the second, so geometry that moves every frame never
    // pays for it), on that launch's side stream, with no host wait.  expose_version: the tree version the mask holds for (0: none);
    // expose_cam / expose_s / expose_d: the camera distance and the operand bounds (ptex::Bounds) it was computed for.
    // The mask lives in the scene arena, behind the wide nodes (expose_off: its byte offset there), so that the megakernel reaches it from the
    // arena's base like every record.
    DevBuf<uint32_t> d_expose_info, d_expose_bad, d_expose_skipped; uint64_t expose_off = 0;      // (d_expose_skipped: the COUNTERS variant's one word, nobody else's)
    uint32_t* expose_mask() const { return (uint32_t*)((char*)d_scene.ptr + expose_off); }
    // expose_gen counts the masks computed, whatever the tree version: a recompute for a farther camera keeps the version, and every stream that
    // is to read the new mask has to wait for it (FrameSlot::expose_waited is compared with this, not with the version).
    uint32_t expose_version = 0, expose_gen = 0, expose_noted = 0, expose_tris = 0; bool tree_updated = false, expose_last_used = false;
    double expose_cam = 0.0, expose_s = 0.0, expose_d = 0.0;
    hipEvent_t ev_expose = nullptr, ev_expose_t0 = nullptr, ev_expose_t1 = nullptr;
    // batched ray queries (pt_trace_rays): queue word and deep-stack spill area of the persistent kernel, staging of pt_trace_rays_host
    DevBuf<unsigned long long> d_rq_queue, d_rq_spill; DevBuf<uint4> d_rq_rays, d_rq_hits;
    DevBuf<uint4> d_oc_surfels;         // staging of pt_hit_surfels_host's result (its rays and hits use the two above)
    DevBuf<uint4> d_cr_contain;         // pt_signed_distance: the PtContainment records between its containment launch and the sign kernel
    // radius queries (pt_radius_search): the counts between the count walk and the scan, the scan's scratch (grown like the staging buffers),
    // and the staging of pt_radius_search_host's offsets and entries
    DevBuf<uint32_t> d_rd_counts; DevBuf<unsigned char> d_rd_temp; DevBuf<unsigned long long> d_rd_offsets; DevBuf<uint4> d_rd_entries;

    // frame
    DevBuf<float4> d_out, d_accum, d_compact, d_compact_accum;
    DevBuf<uint32_t> d_tiles, d_u32tmp;
    // Frame slots: the trace phase of consecutive pt_render calls runs on alternating side streams
    // (own sample / control / scratch buffers each), so the sparse tail of one frame overlaps the
    // dense start of the next; the resolve passes stay in call order on the main stream.
    struct FrameSlot {
        hipStream_t side = nullptr; hipEvent_t resolved = nullptr, done = nullptr; bool used = false;
        uint32_t expose_waited = 0;                                     // the mask generation (PtContext::expose_gen) this slot's stream has waited for (PtContext::ev_expose)
        uint64_t resolved_seq = 0;                                      // launch sequence number of the latest record of `resolved` (pt_buffer_busy)
        DevBuf<uint32_t> queue; DevBuf<float4> samples; DevBuf<uint2> spill; DevBuf<uint4> rays;
        // owned-tile slots that the launch in this slot traces (the others are culled: every camera ray misses the root box, or every box
        // of the tree's cut), followed by the tile cover's bitmask (RenderArgs::trace_slots); key word 8 = the cover's id (0: rectangle only)
        DevBuf<uint32_t> trace_slots; uint32_t* h_trace = nullptr; size_t h_trace_cap = 0; hipEvent_t trace_copied = nullptr;
        uint32_t cull_key[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; uint32_t num_trace_tiles = 0; bool cull_valid = false;
        DevBuf<ptk::FrameParams> frame_params; DevBuf<float4*> frame_outs;      // per-frame parameters / targets of the launch in this slot
        const void* primed_ptr = nullptr; size_t primed_samples = 0;   // what the resident prefill covers
    };
    static constexpr int kMaxSlots = 16;
    FrameSlot slots[kMaxSlots]; int num_slots = 0; uint32_t next_slot = 0;
    // frames queued for one batched launch (pt_set_batch): launched when full or when anything needs their result
    uint32_t batch_size = 1; uint32_t pending = 0; ptk::RenderArgs pendingA; bool pending_ring = false; uint32_t pending_rank = 0, pending_count = 1;
    std::vector<ptk::FrameParams> pending_frames; std::vector<float4*> pending_outs;
    DevBuf<unsigned long long> d_wave_times; uint32_t wave_times_n = 0;
    int num_cus = 0;
    DevBuf<unsigned long long> d_stats;
    std::vector<uint32_t> tiles_host; uint32_t tiles_w = 0, tiles_h = 0, tiles_rank = 0, tiles_count = 0;
    uint32_t out_w = 0, out_h = 0;   // dimensions of the last full-frame result in d_out
    uint32_t accum_w = 0, accum_h = 0, accum_count = 0, accum_rank = 0;
    uint64_t compact_floats = 0;
    uint32_t share_w = 0, share_h = 0, share_count = 0, share_max_tiles = 0;      // cached: largest tile share of a (W, H, count) split (pt_deinterleave*)
    float4* ext_compact = nullptr; uint64_t ext_compact_floats = 0;
    float4* ext_out = nullptr; uint64_t ext_out_floats = 0;      // caller-owned whole-frame target (pt_set_output_buffer)
    const float4* last_full = nullptr;                          // where the last whole-frame result lives (d_out or a caller's buffer)
    bool last_stats = false;
    uint64_t stats_culled = 0;          // pixel-samples of the last instrumented launch that were culled (counted as one root-box miss each)
    std::vector<hipEvent_t> ring;    // start/stop pairs recorded by pt_render while timing is on
    uint32_t ring_used = 0;
    // pt_buffer_busy: the byte ranges that launches not yet known to be delivered write into.  Every launch appends its targets with its
    // sequence number.  The context's stream is in order and every launch's last write is followed there by an event that exists anyway
    // (the frame slot's `resolved`, re-recorded by the slot's next launch; `misc_fence` behind the kernels that do not use a slot), each
    // remembering the sequence number of its LATEST record: once such an event has completed, every launch up to that number has been
    // delivered -- whatever frame slot it ran in and however many launches were submitted after it.  (No event of its own per launch:
    // one more marker on the stream cost the reference's 0.16 ms frame 18 % with one render() per launch.)
    struct InFlight { const char* lo; const char* hi; uint64_t seq; };
    std::vector<InFlight> inflight;
    uint64_t launch_seq = 0, delivered_seq = 0;
    hipEvent_t misc_fence = nullptr; uint64_t misc_fence_seq = 0;
};

namespace pti {

// records the message (in the context, or for a null context per thread: pt_last_error(NULL)) and returns `code`
int fail(PtContext* ctx, int code, const std::string& msg);
int fail_hip(PtContext* ctx, hipError_t e, const char* what);
#define PT_HIP(ctx, call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return fail_hip((ctx), e__, #call); } while (0)

// every context entry point begins with it: a null context is refused, the context's device is made current
int bind(PtContext* ctx);
// waits for the host's copies of what pt_update_triangles changed (root box, edges_small), if a refit still owes them
int sync_refit_meta(PtContext* ctx);
// launches the frames that pt_set_batch still holds; returns at once when there are none
int flush_pending(PtContext* ctx);

} // namespace pti
