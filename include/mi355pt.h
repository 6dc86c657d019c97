/* mi355pt.h -- C ABI of libmi355pt.so, the MI355X-native drop-in for the per-pixel-sample
 * hot path of 31415Hacker/RayTracer-public (src/shaders/renderer.wgsl) and for the
 * scene-build steps that feed it.
 *
 * This is the boundary a reference-side binding attaches to (N-API addon:
 * raytracer-public_amd/napi/addon.c; ctypes: raytracer-public_amd/__init__.py; see
 * INTEGRATION.md).  Plain pointers and sizes only.  Every entry point names the reference
 * interface it replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - every function returns a PtStatus (0 = OK); pt_last_error(ctx) gives the message of
 *     the last failure on that context (pt_last_error(NULL): last context-less failure).
 *     The reference signals errors by JS exceptions / rejected Promises
 *     (src/libs/io.js:3, src/libs/Scene.js:27-30) -- the N-API layer turns a non-zero status
 *     into exactly that.
 *   - host arrays are copied during the call and never retained, like queue.writeBuffer
 *     (src/libs/PathTracer.js:679,692-699,740,789).
 *   - one context = one GPU = one caller thread at a time; work is issued in order on one HIP
 *     stream (the WebGPU queue of the reference is in-order as well).
 *   - buffer layouts are the reference's own:
 *       triangles  f32[9*N]            v0xyz v1xyz v2xyz               (renderer.wgsl:82-89)
 *       BVH2       u32[1 + 6*(2N-1)]   word0 = node count              (BVHBuilder.wgsl:5-7,83-132)
 *       BVH (BVH4) u32[1 + 8*M]        word0 = node count              (renderer.wgsl:91-111)
 *     radiance out: f32 RGBA, row py, column px, py = 0 <-> p.y = -1 (no flip; renderer.wgsl:387-411).
 */
#ifndef MI355PT_H
#define MI355PT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the entry points declared in this header are its whole dynamic symbol table
 * (tests/test_host_build.py checks both directions against `nm -D`). */
#if defined(__GNUC__)
#define PT_API __attribute__((visibility("default")))
#else
#define PT_API
#endif

typedef struct PtContext PtContext;

typedef enum PtStatus {
    PT_OK = 0,
    PT_ERR_INVALID_ARG = 1,
    PT_ERR_NO_DEVICE = 2,     /* no HIP device / HIP runtime failure at create */
    PT_ERR_HIP = 3,           /* a HIP call failed (message in pt_last_error) */
    PT_ERR_NO_SCENE = 4,      /* render / readback before triangles + BVH were set */
    PT_ERR_BAD_BVH = 5,       /* malformed BVH buffer (size, child index, cycle) */
    PT_ERR_IO = 6,
    PT_ERR_OOM = 7
} PtStatus;

/* renderer modes */
enum {
    PT_MODE_REFERENCE_PACKET = 0, /* literal renderer.wgsl:355-413: 2x2 ray packets with one shared stack + lane masks (a quad of lanes per packet) */
    PT_MODE_REFERENCE        = 1, /* same image, one ray per lane (identical except on exact-t ties) */
    PT_MODE_PATH             = 2  /* build-defined extension: spp, bounces, NEE, Russian roulette */
};

/* Mirrors RendererUBO (renderer.wgsl:14-19, packed at PathTracer.js:764-787) plus the
 * build-defined extension fields. */
typedef struct PtRenderParams {
    uint32_t width, height;      /* resolution.xy  */
    float    focal, aspect;      /* resolution.zw: 1/tan(35 deg), W/H (PathTracer.js:761-769) */
    float    cam_pos[3];         /* camPosNumTris.xyz */
    uint32_t num_tris;           /* u32(camPosNumTris.w) (renderer.wgsl:398); must be <= uploaded count */
    float    cam_quat[4];        /* camQuat xyzw */
    uint32_t frame;              /* frameCounter.x (unused by the reference shader; sample index base in PT_MODE_PATH) */
    uint32_t mode;               /* PT_MODE_* */
    uint32_t spp;                /* PT_MODE_PATH: samples per pixel this frame (>= 1) */
    uint32_t max_bounces;        /* PT_MODE_PATH: indirect bounces after the primary hit */
    uint32_t seed;               /* PT_MODE_PATH: RNG seed */
    uint32_t accumulate;         /* PT_MODE_PATH: 0 = replace, 1 = add this frame to the running per-pixel sum */
    uint32_t tile_rank;          /* pixel-tile sharding: this context renders 8x8 tiles with (tx+ty) % tile_count == tile_rank */
    uint32_t tile_count;         /* 0 or 1 = whole frame, row-major output */
    uint32_t flags;              /* PT_FLAG_* */
} PtRenderParams;

enum {
    PT_FLAG_STATS = 1u,          /* run the instrumented kernel variant and fill PtStats */
    PT_FLAG_SIMPLE_KERNEL = 2u,  /* PT_MODE_PATH, PT_MODE_REFERENCE: one-pixel-per-lane kernel instead of the persistent megakernel (A/B checks) */
    PT_FLAG_BRUTE_FORCE = 4u,    /* modes 1, 2: ignore the BVH, test every triangle and every sphere of pt_set_spheres (config C1) */
    PT_FLAG_COMPACT = 8u         /* tile-major compact output (pt_compact_radiance / pt_set_compact_buffer) also when tile_count <= 1: the layout
                                    a one-member group gathers, so that one code path serves every group size */
};

/* Traversal counters of the last PT_FLAG_STATS render (algorithmic-bytes bookkeeping,
 * bytes = 32*nodes_examined + 36*tris_tested + 16*samples). */
typedef struct PtStats {
    uint64_t rays_closest, rays_shadow;
    uint64_t nodes_examined;     /* node records box-tested, each once per examination */
    uint64_t tris_tested;
    uint64_t stack_drops;        /* pushes dropped at the 64-entry cap (renderer.wgsl:337) */
    uint64_t max_stack;
    uint64_t samples;
} PtStats;

/* ---- library / context ------------------------------------------------------------ */

/* PathTracer.initialize() (PathTracer.js:97-173): picks the device, creates the stream and
 * the fixed-size buffers.  device_ordinal < 0 selects the current HIP device. */
PT_API int  pt_create(int device_ordinal, PtContext** out);
PT_API void pt_destroy(PtContext* ctx);
PT_API const char* pt_last_error(const PtContext* ctx);
PT_API const char* pt_version(void);
/* Issue all work of this context on a caller-owned hipStream_t (e.g. torch's current
 * stream) instead of the context's own stream.  NULL restores the own stream. */
PT_API int  pt_set_stream(PtContext* ctx, void* hip_stream);
PT_API int  pt_synchronize(PtContext* ctx);
/* The hipStream_t the context currently issues on (its own non-blocking stream unless pt_set_stream
 * replaced it) -- e.g. to wrap it as torch.cuda.ExternalStream so collectives order after the render. */
PT_API int  pt_get_stream(PtContext* ctx, void** hip_stream);

/* ---- host-side scene build (no GPU touched; the reference runs these in JS) ------------ */

/* computeBVH2Sizing / computeBVH4Sizing (PathTracer.js:227-238) */
PT_API int pt_compute_bvh2_sizing(uint32_t num_tris, uint32_t* num_nodes2, uint64_t* bytes);
PT_API int pt_compute_bvh4_sizing(uint32_t num_nodes4, uint64_t* bytes);
/* buildMortonAndSort (PathTracer.js:427-481): outputs hold num_tris words each */
PT_API int pt_morton_sort(const float* tris, uint32_t num_tris, uint32_t* morton_sorted, uint32_t* tri_index_sorted);
/* collapseLBVH2ToBVH4 (PathTracer.js:506-667): out holds up to 1 + 8*(2N-1) words */
PT_API int pt_collapse_lbvh2_to_bvh4(const uint32_t* bvh2, uint32_t num_tris, uint32_t* out, uint64_t out_words, uint32_t* num_nodes4);
/* Opt-in tree quality.  The reference builds one tree, LBVH2 + first-internal collapse ("BVH-only, no
 * SAH"); levels 1 and 2 depart from it in the TREE only, every buffer stays in the reference layout (BVH2 u32[1 + 6(2N-1)], root 0,
 * internal nodes 0..N-2, leaf N-1+k = Morton-sorted triangle k with the LBVH's leaf words; BVH4 u32[1 + 8M] in DFS pre-order, one
 * triangle per leaf), so readBVH2 / data/BVH2.bin / pt_bvh2_to_bvh4_wide and the oracle's traversal work on them unchanged.
 *   PT_ACCEL_REFERENCE      the reference's tree, exactly (pt_build_bvh)
 *   PT_ACCEL_AREA_COLLAPSE  the same LBVH2; the collapse expands the internal entry of LARGEST SURFACE AREA instead of the first
 *                           one (PathTracer.js:608-621 departs here)
 *   PT_ACCEL_PLOC           a PLOC BVH2 (Meister & Bittner, TVCG 2018; radius 16) instead of the LBVH2 of BVHBuilder.wgsl:152-240,
 *                           same leaves, same refit (:242-306), then the area-guided collapse
 * A BVH2 installed with pt_set_bvh2 (e.g. a level-2 data/BVH2.bin reloaded) is collapsed the reference's way, first-internal. */
#define PT_ACCEL_REFERENCE     0
#define PT_ACCEL_AREA_COLLAPSE 1
#define PT_ACCEL_PLOC          2
/* collapseLBVH2ToBVH4 with the collapse rule of `accel` (0: identical to pt_collapse_lbvh2_to_bvh4; 1, 2: area-guided, which
 * reads the internal BVH2 bounds -- give it a complete BVH2, e.g. pt_read_bvh2's or pt_build_bvh2_ploc's) */
PT_API int pt_collapse_bvh2_to_bvh4_accel(const uint32_t* bvh2, uint32_t num_tris, uint32_t accel, uint32_t* out, uint64_t out_words, uint32_t* num_nodes4);
/* PLOC BVH2 of PT_ACCEL_PLOC on the host, refit bounds included (the device build equals it word for word); out holds
 * 1 + 6*(2N-1) words.  Replaces the reference's LBVH2 kernels (BVHBuilder.wgsl:152-240) by PLOC; leaves and refit as there. */
PT_API int pt_build_bvh2_ploc(const float* tris, uint32_t num_tris, uint32_t* out, uint64_t out_words);
/* BVH2 -> BVH4_wide promotion (tests/test.cpp:106-196): out holds 1 + 8*bvh2[0] words */
PT_API int pt_bvh2_to_bvh4_wide(const uint32_t* bvh2, uint64_t bvh2_words, uint32_t* out, uint64_t out_words);
/* data/BVH2.bin, data/BVH4_wide.bin: raw little-endian u32 dumps (src/server/api.js:27-31,
 * tests/test.cpp:16-33).  pt_file_read_u32 returns the word count through *words; call with
 * dst = NULL to query the size. */
PT_API int pt_file_write_u32(const char* path, const uint32_t* src, uint64_t words);
PT_API int pt_file_read_u32(const char* path, uint32_t* dst, uint64_t dst_words, uint64_t* words);

/* Deterministic procedural stand-in scenes (the reference's dragon.glb / Sponza are absent,
 * SURVEY.md 0.3).  kind 0 = "dragon-class" closed bumpy knot, kind 1 = "sponza-class"
 * interior.  Writes exactly num_tris triangles (9 f32 each), normalised to [-1,1]^3. */
PT_API int pt_scene_procedural(uint32_t kind, uint32_t seed, uint32_t num_tris, float* tris_out);

/* ---- device scene state ------------------------------------------------------------ */

/* device.queue.writeBuffer(triangles) (PathTracer.js:679); N <= 932,067 in the reference
 * (32 MiB buffer, :140-143) -- no such cap here. */
PT_API int pt_set_triangles(PtContext* ctx, const float* tris, uint32_t num_tris);
/* buildBVH (PathTracer.js:671-749): Morton codes + sort (:411-481), LBVH2 kernels (BVHBuilder.wgsl), greedy collapse to
 * BVH4 (:506-667) -- every step on the device, same BVH2 / BVH4 buffers bit for bit as the reference's CPU + WebGPU split
 * (the host entry points below mirror the JS steps one by one).  The bounds of the INTERNAL BVH2 nodes, which only a BVH2
 * read-back looks at, are filled in by the first pt_read_bvh2. */
PT_API int pt_build_bvh(PtContext* ctx);
/* pt_build_bvh with a tree-quality level (PT_ACCEL_*; departures from the reference listed there).  accel 0 is pt_build_bvh.
 * Every level builds on the device; levels 1 and 2 leave a complete BVH2 (internal bounds included) for pt_read_bvh2.  Any other
 * value returns PT_ERR_INVALID_ARG and leaves the context as it was. */
PT_API int pt_build_bvh_accel(PtContext* ctx, uint32_t accel);
/* LBVH2 kernels only, from caller-supplied sorted codes (the two dispatches at
 * PathTracer.js:709-728); result stays on the device for pt_read_bvh2. */
PT_API int pt_build_lbvh2(PtContext* ctx, const uint32_t* morton_sorted, const uint32_t* tri_index_sorted);
/* readBVH2 (PathTracer.js:485-502): copies min(bytes, buffer size) bytes */
PT_API int pt_read_bvh2(PtContext* ctx, uint32_t* dst, uint64_t bytes);
/* writeBuffer(BVH) (PathTracer.js:739-740): install a BVH4 buffer in the reference layout
 * (collapse output or BVH4_wide).  Validated: sizes, child indices, no node reachable twice. */
PT_API int pt_set_bvh4(PtContext* ctx, const uint32_t* bvh4, uint64_t words);
/* load a BVH2 buffer (data/BVH2.bin) and collapse it like buildBVH does after readback */
PT_API int pt_set_bvh2(PtContext* ctx, const uint32_t* bvh2, uint64_t words);
PT_API int pt_read_bvh4(PtContext* ctx, uint32_t* dst, uint64_t bytes);
/* Build-defined extension for BASELINE config C1 (Cornell box: triangles + analytic spheres, no BVH):
 * n spheres as (x, y, z, r) f32 quadruples, used only by PT_FLAG_BRUTE_FORCE renders. */
PT_API int pt_set_spheres(PtContext* ctx, const float* xyzr, uint32_t num_spheres);
PT_API int pt_scene_info(PtContext* ctx, uint32_t* num_tris, uint32_t* num_nodes2, uint32_t* num_nodes4);

/* ---- the hot path ----------------------------------------------------------------- */

/* PathTracer.render() compute pass (PathTracer.js:756-802 + renderer.wgsl:355-413).
 * Asynchronous on the context's stream; results are read with pt_read_radiance. */
PT_API int pt_render(PtContext* ctx, const PtRenderParams* params);
/* Batched submission (PT_MODE_PATH): queue `frames_per_launch` (1..256, default 1) consecutive pt_render calls of
 * the same shape and trace them with ONE persistent launch -- small frames (e.g. a 1/8 tile share of a
 * multi-GPU run) then fill the chip like a whole frame does.  A partial batch is launched by whatever
 * needs its result: pt_synchronize, any read-back, pt_compact_radiance / pt_deinterleave, scene changes.
 * Each frame still resolves into the output target that was current when it was submitted. */
PT_API int pt_set_batch(PtContext* ctx, uint32_t frames_per_launch);
/* Launch a partially filled batch now (asynchronous, no host synchronisation). */
PT_API int pt_flush(PtContext* ctx);
/* Device time of the last pt_render's kernel(s), by hipEvents on the stream it ran on.
 * Synchronises the stream. */
PT_API int pt_last_render_ms(PtContext* ctx, float* ms);
/* Per-launch kernel timing without host synchronisation inside a timed loop: after
 * pt_timing_begin(ctx, capacity) every pt_render records its own hipEvent pair (on the stream
 * the kernel is launched on) into a ring; pt_timing_collect synchronises once and returns the
 * elapsed milliseconds of the recorded launches (oldest first) and their count. */
PT_API int pt_timing_begin(PtContext* ctx, uint32_t capacity);
PT_API int pt_timing_collect(PtContext* ctx, float* ms, uint32_t capacity, uint32_t* count);
/* The same, plus when each recorded launch started relative to the first one (launches of consecutive batches overlap on the
 * context's side streams: the union of the [start, start + duration] intervals is the time the GPU was busy tracing). */
PT_API int pt_timing_collect_spans(PtContext* ctx, float* start_ms, float* dur_ms, uint32_t capacity, uint32_t* count);
PT_API int pt_get_stats(PtContext* ctx, PtStats* out);
/* Full-frame f32 RGBA W*H*4 (tile_count <= 1).  Synchronises. */
PT_API int pt_read_radiance(PtContext* ctx, float* dst, uint64_t dst_floats);
/* rgba8unorm equivalent of the reference's outputTex (PathTracer.js:163-172) */
PT_API int pt_read_rgba8(PtContext* ctx, uint8_t* dst, uint64_t dst_bytes);
/* tonemapper.wgsl:24-41 applied to the last frame: Reinhard, gamma 1/2.2, vertical flip;
 * from_rgba8 != 0 first quantises to rgba8unorm like the reference's texture. */
PT_API int pt_read_tonemapped(PtContext* ctx, int from_rgba8, uint8_t* dst, uint64_t dst_bytes);

/* ---- checkpoint / resume of a progressive accumulation (PtRenderParams.accumulate) ------------------------------------------
 * The reference has no accumulation; its only persistence is the raw BVH2 dump (src/server/api.js:27-31).  A
 * progressive render of BASELINE configuration C5 (64 spp as 16 accumulated frames) is long enough to want the same: the running
 * per-pixel state is ONE f32 RGBA buffer -- sums of the sample radiances in x, y, z, the sample count in w -- dumped and restored raw.
 * Whole frame: W*H*4 floats, row-major like the radiance; a tile share (tile_count > 1 or PT_FLAG_COMPACT): tiles*64*4 floats,
 * tile-major like the compact buffer (pt_tile_ids gives the order).  A restored context continues bit for bit: the next pt_render with
 * accumulate = 1 and the same shape adds to the restored sums, with frame indices continuing where the dumped run stopped. */
typedef struct PtAccumInfo {
    uint32_t width, height;
    uint32_t tile_rank, tile_count;   /* the share the sums cover (0 or 1 = every tile) */
    uint32_t compact;                 /* 1: tile-major share layout, 0: whole frame, row-major */
    uint32_t samples;                 /* samples per pixel accumulated so far (the w channel of every pixel) */
    uint64_t floats;                  /* size of the dump; 0 = no running accumulation */
} PtAccumInfo;
PT_API int pt_accum_info(PtContext* ctx, PtAccumInfo* out);
/* Launches what is queued and waits for it; dst holds at least info.floats floats. */
PT_API int pt_read_accum(PtContext* ctx, float* dst, uint64_t dst_floats);
/* Install running sums (the host array is copied during the call).  The scene must be set as for rendering; changing the scene
 * afterwards restarts the accumulation, like it does for one that was rendered. */
PT_API int pt_set_accum(PtContext* ctx, const PtAccumInfo* info, const float* src);

/* ---- batched ray queries: what does a ray hit? (an extension beyond the reference) ------------------
 * The reference asks this only in its debug tool (tests/test.py:149-230, traverse_bvh_debug: one ray over a whole tree).
 *
 * Closest hit (default): the renderer's single-ray traversal (render_rays_kernel, PT_MODE_REFERENCE) over the context's CURRENT tree,
 * whatever set it -- pt_build_bvh / pt_build_bvh_accel of any level, pt_set_bvh4, pt_set_bvh2: the same visit order, the same tie-breaking
 * (first minimum in slot order), the same silent drop of pushes at 64 stack entries, the same Moller-Trumbore acceptance
 * (t > 1e-7 and strictly t < best).  `best` starts at min(t_max, 1e30): with t_max = +inf a result is exactly the oracle's
 * (oracle/pt_oracle.cpp::orc_trace_ray).  A smaller t_max prunes boxes and triangles at t >= t_max from the start.
 *   hit:  t = the accepted test's t, bit for bit; prim = the triangle index; u, v = the barycentrics of that test (recomputed after the
 *         traversal from the triangle's record with the same arithmetic: the same bits).
 *   miss: t = +INFINITY, prim = 0xFFFFFFFF, u = v = 0.
 * PT_TRACE_ANY_HIT: the first accepted hit in traversal order ends the ray (the renderer's shadow-ray semantics; t and prim equal
 *   orc_trace_ray(..., anyhit = 1)).
 * Rays with no traversal: a NaN in org, dir or t_max, or t_max <= 0: a miss.
 * Scene contents: triangles only.  Spheres (pt_set_spheres) take no part in ray queries.
 * Ordering: frames queued by pt_set_batch are launched first (as pt_flush does), so stream order is call order; a scene change after a
 *   query does not change its results.  pt_trace_rays does not wait: the caller's buffers must stay allocated until a later
 *   pt_synchronize has returned (the rule of pt_set_output_buffer).
 * Errors: no triangles + tree: PT_ERR_NO_SCENE.  A NULL or non-16-byte-aligned pointer, unknown flags or n > UINT32_MAX:
 *   PT_ERR_INVALID_ARG (checked before the scene).  n = 0: PT_OK, nothing is launched.
 * PT_TRACE_STATS: the counting variant (one ray per thread) fills pt_get_stats like a PT_FLAG_STATS render: rays_closest or rays_shadow,
 *   nodes_examined, tris_tested, stack_drops and max_stack, counted as the oracle counts them (samples = 0).
 * PT_TRACE_SIMPLE_KERNEL: the one-ray-per-thread kernel instead of the persistent one (A/B checks); the results are the same. */
typedef struct PtRay { float org[3]; float t_max; float dir[3]; uint32_t reserved; } PtRay;   /* 32 B, 16-byte aligned arrays; reserved: ignored */
typedef struct PtHit { float t; uint32_t prim; float u, v; } PtHit;                           /* 16 B */
enum {
    PT_TRACE_ANY_HIT = 1u,
    PT_TRACE_STATS = 2u,
    PT_TRACE_SIMPLE_KERNEL = 4u
};
/* n rays from device memory, n hits into device memory (rays_device, hits_device: 16-byte aligned, on the context's device).
 * Asynchronous on the context's stream (pt_get_stream). */
PT_API int pt_trace_rays(PtContext* ctx, const void* rays_device, uint64_t n, uint32_t flags, void* hits_device);
/* The same from host arrays: staged through device buffers of the context; returns when the hits are written. */
PT_API int pt_trace_rays_host(PtContext* ctx, const PtRay* rays, uint64_t n, uint32_t flags, PtHit* hits);
/* The rays PT_MODE_REFERENCE traces, with identical bits: one through each pixel centre of params (width, height, focal, aspect,
 * cam_pos, cam_quat; renderer.wgsl:387-395), row-major (pixel (px, py) at py * width + px), t_max = +inf, reserved = 0.
 * width * height PtRay records into rays_device (16-byte aligned).  Needs no scene.  Asynchronous on the context's stream. */
PT_API int pt_camera_rays(PtContext* ctx, const PtRenderParams* params, void* rays_device);

/* ---- batched closest-point queries: which triangle is nearest to a point? (an extension beyond the reference)
 * For every point the nearest triangle of the scene within r_max, over the context's CURRENT tree, whatever set it (pt_build_bvh /
 * pt_build_bvh_accel of any level, pt_set_bvh4, pt_set_bvh2, refitted by pt_update_triangles or not).
 *   found:   prim = the triangle with the smallest squared distance d2, evaluated in f32 (below); dist = sqrtf(d2), correctly rounded;
 *            u, v = the closest point as v0 + u*e1 + v*e2 with e1 = v1 - v0, e2 = v2 - v0 as the triangle record stores them (each
 *            rounded to f32 once at upload).  u, v are recomputed after the walk from the winning record with the same operations (the
 *            same bits), as the ray queries do, so the walk keeps no registers for them.
 *   nothing: dist = +INFINITY, prim = 0xFFFFFFFF, u = v = 0.
 * Point-triangle arithmetic (f32, every operation rounded once, no contraction; dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z), on
 *   (ap = p - v0, e1, e2), operation by operation in DESIGN.md section 15 and csrc/pt_closest.h: the unconstrained minimum by one
 *   Gram-Schmidt step (f = e2 - (b / a) e1; vq = (f . ap) / (f . f), uq = (d1 - vq * b) / a), Eberly's seven regions from the signs of
 *   uq, vq and 1 - (uq + vq), folded onto the face or the edge that holds the minimum, and on an edge a quotient clamped to exactly 0
 *   and 1.  Three reciprocals: 1 / a, 1 / (f . f), and 1 / den of the edges v0 v2 and v1 v2.  u, v >= 0 and u + v <= 1 + 2^-22.
 *   d2 = dot(diff, diff) with diff = ap - (e1*u + e2*v).  NaN operands fail every comparison, reach the edge v1 v2 and leave a NaN d2,
 *   as does a triangle collapsed to a point (0 / 0); a NaN d2 is never accepted.  A triangle collapsed to a segment still gets a point
 *   of that segment.
 * r_max: the best squared distance starts at r_max * r_max (+inf stays +inf); a triangle is accepted only when d2 < best2, strictly, and
 *   the first minimum in visit order wins.  A point with a NaN in p or r_max, or with r_max <= 0, finds nothing and is not walked.
 * The walk: the ray queries' walk with a squared lower bound of the distance to a child's box, bound2, in place of tmin.  A child is
 *   entered only if bound2 < best2; passing children keep slot order, the first minimum trades places with the first passing child and
 *   is entered next, the others are pushed far -> near; a stacked child is re-validated at pop by bound2 < best2.  Empty and degenerate
 *   slots hold the inverted box (bound2 = +inf) and reject themselves; a leaf with t >= num_tris is skipped; a degenerate root box
 *   means that every point finds nothing, as every ray misses.  The stack holds 64 entries; a push at the cap is dropped (and counted).
 * bound2: per axis g = max(mn - (p + s), (p - s) - mx, 0) with s = 2^-12 and mn, mx the box's f16 bounds; bound2 = (gx*gx + gy*gy) + gz*gz.
 *   The slack s covers the f16 subnormal flush of the internal boxes (a triangle may stick out of an ancestor's box by less than 2^-14)
 *   and every rounding of bound2 and of d2: for vertex coordinates within [-4, 4] and point coordinates within [-32, 32] no triangle with
 *   a smaller d2 is ever pruned (proof: DESIGN.md section 15).
 * Exactness: wherever the walk drops nothing at the cap (stack_drops = 0) and every triangle is reachable from the root, dist has the
 *   bits of the brute-force minimum over all triangles, and prim is a triangle with exactly that d2.
 * PT_CLOSEST_BRUTE_FORCE: every triangle in index order, no tree (the precedent of PT_FLAG_BRUTE_FORCE): the tree-independent check.
 * PT_CLOSEST_STATS: the counting variant (one point per thread) fills pt_get_stats: rays_closest = the number of points, nodes_examined,
 *   tris_tested, stack_drops and max_stack by the rules of the ray queries' counters (rays_shadow = samples = 0).  With
 *   PT_CLOSEST_BRUTE_FORCE only rays_closest and tris_tested are counted.
 * PT_CLOSEST_SIMPLE_KERNEL: the one-point-per-thread kernel instead of the persistent one (A/B checks); the results are the same.
 * Scene contents: triangles only.  Spheres (pt_set_spheres) take no part.
 * Ordering, errors and alignment: as pt_trace_rays.  Frames queued by pt_set_batch are launched first; pt_closest_points does not wait
 *   (the caller's buffers must stay allocated until a later pt_synchronize has returned); a scene change after a query does not change
 *   its results.  A NULL or non-16-byte-aligned pointer, unknown flags or n > UINT32_MAX: PT_ERR_INVALID_ARG (checked before the
 *   scene).  No triangles + tree: PT_ERR_NO_SCENE.  n = 0: PT_OK, nothing is launched. */
typedef struct PtPoint   { float p[3]; float r_max; } PtPoint;                  /* 16 B, 16-byte aligned arrays */
typedef struct PtClosest { float dist; uint32_t prim; float u, v; } PtClosest;  /* 16 B */
enum {
    PT_CLOSEST_STATS = 1u,
    PT_CLOSEST_SIMPLE_KERNEL = 2u,
    PT_CLOSEST_BRUTE_FORCE = 4u
};
/* n points from device memory, n results into device memory (both 16-byte aligned, on the context's device).  Asynchronous on the
 * context's stream (pt_get_stream). */
PT_API int pt_closest_points(PtContext* ctx, const void* points_device, uint64_t n, uint32_t flags, void* out_device);
/* The same from host arrays: staged through device buffers of the context; returns when the results are written. */
PT_API int pt_closest_points_host(PtContext* ctx, const PtPoint* points, uint64_t n, uint32_t flags, PtClosest* out);
/* Host twin (no context, no GPU): the same PtClosest bits and, with PT_CLOSEST_STATS and stats != NULL, the same counters as the device
 * gives for the tree pt_set_bvh4(bvh4) installs over pt_set_triangles(tris).  bvh4 = NULL (words = 0) only with PT_CLOSEST_BRUTE_FORCE;
 * stats may be NULL; PT_CLOSEST_SIMPLE_KERNEL is accepted and changes nothing.  tris: f32[9 * num_tris]; bvh4: u32[1 + 8 * numNodes]
 * (a malformed one: PT_ERR_BAD_BVH); a NULL points or out pointer with n > 0, or unknown flags: PT_ERR_INVALID_ARG. */
PT_API int pt_closest_points_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words,
                                  const PtPoint* points, uint64_t n, uint32_t flags, PtClosest* out, PtStats* stats);

/* ---- sphere-cast queries: when does a moving sphere first touch the mesh, and where? (an extension beyond the reference; DESIGN.md
 * section 22) -------------------------------------------------------------------------------------------------------------------
 * For every sweep -- a sphere of radius `radius` whose centre moves from org along dir -- the first contact with a triangle of the scene
 * at 0 <= t < t_max, over the context's CURRENT tree, whatever set it (built, installed or refitted).  dir need not be unit length: t is
 * in units of dir.  radius = 0 is a moving point.
 *   hit:  t = the time of first contact (0 for a sphere that overlaps a triangle at the start); prim = the triangle touched; u, v = the
 *         contact point on it as v0 + u*e1 + v*e2: pt_closest_points' (u, v) of the centre c = org + t*dir (the product rounded, then the
 *         sum) against the winning record, recomputed after the walk.
 *   miss: t = +INFINITY, prim = 0xFFFFFFFF, u = v = 0.
 * Sweeps with no walk, a miss: a NaN in org, dir, t_max or radius; t_max <= 0; radius < 0; dir = (0, 0, 0).
 * Arithmetic (f32, every operation rounded once, no contraction), operation by operation in DESIGN.md section 22 and csrc/pt_sweep.h.
 *   Per triangle record, in this order: (1) the slab test of pt_trace_rays on the bounds of the record's three vertices, the origin moved
 *   by the radius (near planes against org + radius or org - radius), which rejects the triangle or gives t_in = max(tmin, 0); (2) the
 *   squared distance d2 of pt_closest_points from org: d2 <= radius^2 gives t_c = 0; (3) otherwise t_c = the smallest valid candidate of
 *   the face (approached from the side org is on, the touched point's barycentrics inside the triangle), the three edges as cylinders
 *   (the smaller root, the foot parameter in [0, 1]) and the three vertices as spheres (the smaller root), roots >= 0 only, each root
 *   taken from the time t0 and the offset w of the closest approach (a vertex: t0 - sqrt((r^2 - |w|^2) / |dir|^2); an edge: the same in
 *   cross products with the edge; both written out in csrc/pt_sweep.h);
 *   (4) t_T = max(t_c, t_in), accepted iff t_T < best, strictly; best starts at t_max and the first minimum in visit order wins.  A
 *   contact at t_T = 0 ends the walk of its sweep: nothing can be accepted behind it.  A NaN fails every comparison and is never accepted.  A component of dir with |dir_k| <= 1e-8 is
 *   treated by the box tests as parallel to the slab (pt_trace_rays' safe inverse).
 * The walk: pt_trace_rays' walk, with a child entered iff the slab test passes on its packed f16 box grown by radius + 2^-12 and its
 *   key tmin < best; the key orders the children and is re-validated at pop.  The stack holds 64 entries; a push at the cap is dropped
 *   (and counted).
 * Exactness: for vertex coordinates within [-4, 4], |org_k| <= 32, radius <= 16 and finite dir, wherever the walk drops nothing at the
 *   cap (stack_drops = 0) and every triangle is reachable from the root, t has the bits of the brute-force minimum over all triangles,
 *   and prim is a triangle with exactly that t_T (proof: DESIGN.md section 22).
 * PT_SWEEP_BRUTE_FORCE, PT_SWEEP_STATS, PT_SWEEP_SIMPLE_KERNEL: as PT_CLOSEST_BRUTE_FORCE, PT_CLOSEST_STATS, PT_CLOSEST_SIMPLE_KERNEL
 *   (rays_closest = the number of sweeps).
 * Scene contents: triangles only.  Spheres (pt_set_spheres) take no part.
 * Ordering, errors and alignment: as pt_trace_rays.  Frames queued by pt_set_batch are launched first; pt_sweep_spheres does not wait
 *   (the caller's buffers must stay allocated until a later pt_synchronize has returned); a scene change after a query does not change
 *   its results.  A NULL or non-16-byte-aligned pointer, unknown flags or n > UINT32_MAX: PT_ERR_INVALID_ARG (checked before the
 *   scene).  No triangles + tree: PT_ERR_NO_SCENE.  n = 0: PT_OK, nothing is launched. */
typedef struct PtSweep { float org[3]; float t_max; float dir[3]; float radius; } PtSweep;   /* 32 B, 16-byte aligned arrays: PtRay with the radius in the reserved word */
enum {
    PT_SWEEP_STATS = 1u,
    PT_SWEEP_SIMPLE_KERNEL = 2u,
    PT_SWEEP_BRUTE_FORCE = 4u
};
/* n sweeps from device memory, n PtHit records into device memory (both 16-byte aligned, on the context's device).  Asynchronous on the
 * context's stream (pt_get_stream). */
PT_API int pt_sweep_spheres(PtContext* ctx, const void* sweeps_device, uint64_t n, uint32_t flags, void* hits_device);
/* The same from host arrays: staged through device buffers of the context; returns when the hits are written. */
PT_API int pt_sweep_spheres_host(PtContext* ctx, const PtSweep* sweeps, uint64_t n, uint32_t flags, PtHit* hits);
/* Host twin (no context, no GPU): the same PtHit bits and, with PT_SWEEP_STATS and stats != NULL, the same counters as the device gives
 * for the tree pt_set_bvh4(bvh4) installs over pt_set_triangles(tris).  bvh4 = NULL (words = 0) only with PT_SWEEP_BRUTE_FORCE; stats
 * may be NULL; PT_SWEEP_SIMPLE_KERNEL is accepted and changes nothing.  A malformed bvh4: PT_ERR_BAD_BVH; a NULL sweeps or out pointer
 * with n > 0, or unknown flags: PT_ERR_INVALID_ARG. */
PT_API int pt_sweep_spheres_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words,
                                 const PtSweep* sweeps, uint64_t n, uint32_t flags, PtHit* out, PtStats* stats);

/* ---- batched ambient-occlusion queries: how open is the hemisphere above a surface point? (an extension beyond the reference;
 * DESIGN.md section 16) ---------------------------------------------------------------------------------------------------------
 * For every surfel (a point p with a normal n) `samples` cosine-distributed rays around n are walked any-hit over the context's CURRENT
 * tree, whatever set it, and the rays that reach nothing within r_max are counted: visibility = unoccluded / samples.  The result is an
 * integer that equals, bit for bit, what pt_occlusion_rays -> pt_trace_rays(PT_TRACE_ANY_HIT) -> counting the misses gives; the ray
 * records and hit records of that composition (48 bytes per ray) never reach memory.
 * All arithmetic is f32, every operation rounded once, no contraction; dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.
 * Sample ray s (s < samples) of surfel i:
 *   key = sample_key(seed, index_base + i, s) with index_base + i taken mod 2^32; u1 = rnd(key, 0, 2), u2 = rnd(key, 0, 3);
 *   dir = cosine_dir(n, u1, u2) -- the counter RNG and the cosine sampling of DESIGN.md section 4, the functions behind the oracle's
 *   orc_rnd(seed, pixel, sidx, 0, dim) and orc_cosine_dir.  n is used as given: callers pass unit normals, the library does not normalise.
 *   org.a = p.a + n.a * bias per component; t_max = r_max; reserved = 0.
 * Which surfels are traced: a surfel is traced iff p, n and r_max hold no NaN and r_max > 0 (+inf is allowed).  An untraced surfel yields
 *   {visibility 0, unoccluded 0, samples 0}; pt_occlusion_rays writes `samples` records {org = p, t_max = 0, dir = n} for it (rays that
 *   pt_trace_rays does not traverse).
 * Occlusion: a sample is occluded iff pt_trace_rays(PT_TRACE_ANY_HIT) on that ray record reports a hit: the same walk, the same acceptance
 *   rule, best = min(t_max, 1e30), the same 64-entry cap, and no traversal for a ray with a NaN (a NaN dir, e.g. from a zero normal, is a
 *   miss and counts as unoccluded).  unoccluded = the number of misses; samples = params.samples;
 *   visibility = (float)unoccluded / (float)samples, one correctly rounded division; reserved = 0.
 * Arguments: samples in 1..65536 and n * samples <= 2^32 - 1, a bias that is not NaN and not negative, else PT_ERR_INVALID_ARG.  A NULL or
 *   non-16-byte-aligned pointer, unknown flags, NULL params or n > UINT32_MAX: PT_ERR_INVALID_ARG (checked before the scene).  No triangles
 *   + tree: PT_ERR_NO_SCENE (pt_occlusion_rays needs none; pt_hit_surfels needs the triangles).  n = 0: PT_OK, nothing is launched.
 * Ordering: as pt_trace_rays.  Frames queued by pt_set_batch are launched first; pt_occlusion does not wait and synchronises nothing on the
 *   host (the caller's buffers must stay allocated until a later pt_synchronize has returned); a scene change after the call does not
 *   change its result.
 * PT_OCCLUSION_STATS: the counting variant (one sample ray per thread) fills pt_get_stats: rays_shadow = samples * the number of traced
 *   surfels; nodes_examined, tris_tested, stack_drops and max_stack exactly what pt_trace_rays(ANY_HIT | STATS) reports for the rays of the
 *   traced surfels; rays_closest = samples = 0.
 * PT_OCCLUSION_SIMPLE_KERNEL: the one-ray-per-thread kernel instead of the persistent one (A/B checks); the results are the same.
 * pt_hit_surfels: hits -> surfels, so that camera rays -> pt_trace_rays -> surfels -> pt_occlusion stays on the device.  A hit with
 *   prim < the triangle count: P.a = org.a + dir.a * t; nf = the triangle record's stored normal if dot3(normal, dir) < 0, else its negation
 *   (the path tracer's rule); the surfel is {P, r_max, nf, 0}.  A miss, or prim out of range: {org, 0, dir, 0}, an
 *   untraced surfel. */
typedef struct PtSurfel    { float p[3]; float r_max; float n[3]; uint32_t reserved; } PtSurfel;        /* 32 B: the shape of PtRay (org, t_max, dir) */
typedef struct PtOcclusion { float visibility; uint32_t unoccluded; uint32_t samples; uint32_t reserved; } PtOcclusion;  /* 16 B */
typedef struct PtOcclusionParams { uint32_t samples; uint32_t seed; uint32_t index_base; float bias; uint32_t flags; } PtOcclusionParams;
enum {
    PT_OCCLUSION_STATS = 1u,
    PT_OCCLUSION_SIMPLE_KERNEL = 2u
};
/* n surfels from device memory, n results into device memory (both 16-byte aligned, on the context's device).  Asynchronous on the
 * context's stream (pt_get_stream). */
PT_API int pt_occlusion(PtContext* ctx, const void* surfels_device, uint64_t n, const PtOcclusionParams* params, void* out_device);
/* The same from host arrays: staged through device buffers of the context; returns when the results are written. */
PT_API int pt_occlusion_host(PtContext* ctx, const PtSurfel* surfels, uint64_t n, const PtOcclusionParams* params, PtOcclusion* out);
/* The sample rays themselves: n * samples PtRay records into rays_device, sample s of surfel i at i * samples + s.  Needs no scene. */
PT_API int pt_occlusion_rays(PtContext* ctx, const void* surfels_device, uint64_t n, const PtOcclusionParams* params, void* rays_device);
/* Host twin (no context, no GPU): the same bits.  params->flags: the known flags are accepted and change nothing. */
PT_API int pt_occlusion_rays_host(const PtSurfel* surfels, uint64_t n, const PtOcclusionParams* params, PtRay* rays);
/* n rays + their n hits -> n surfels, all in device memory (16-byte aligned).  Asynchronous on the context's stream. */
PT_API int pt_hit_surfels(PtContext* ctx, const void* rays_device, const void* hits_device, uint64_t n, float r_max, void* surfels_device);
/* The same from host arrays (16-byte aligned): staged; returns when the surfels are written. */
PT_API int pt_hit_surfels_host(PtContext* ctx, const PtRay* rays, const PtHit* hits, uint64_t n, float r_max, PtSurfel* out);

/* ---- crossing counts, containment and signed distance: how many surfaces does a ray cross, is a point inside? (an extension beyond
 * the reference) ---------------------------------------------------------------------------------------------
 * pt_count_hits: for every ray the number of triangle records that the walk reaches and for which the Moller-Trumbore test of the ray
 *   queries holds (two-sided, t > 1e-7, u and v edges inclusive as they stand) and t < best.  best = min(t_max, 1e30), constant for the
 *   whole walk: no hit shrinks it and no hit ends the ray.
 * The walk: the ray queries' walk over the context's CURRENT tree (built at any level, installed, refitted): children tested against
 *   `best`, visited in the order of the ray queries (first minimum entered, the others pushed far -> near), a stacked entry re-validated
 *   at pop against `best` (which always passes here), 64 stack entries with a push at the cap dropped (and counted), a leaf with
 *   t >= num_tris skipped, a degenerate root box: 0.  Spheres (pt_set_spheres) take no part.
 * Rays with no walk: a NaN in org, dir or t_max, or t_max <= 0: count 0.
 * Three consequences of the walk being the shared one (tested as equalities):
 *   1. count >= 1 exactly when pt_trace_rays(PT_TRACE_ANY_HIT) reports a hit for the same record -- always, with stack drops too: `best`
 *      moves in neither walk, so the any-hit walk is a prefix of the counting walk.
 *   2. the walk's count never exceeds the brute-force count on a tree whose leaves hold each triangle once.
 *   3. the two are equal wherever nothing is dropped at the cap and no crossing is lost to an f16 box.
 * PT_COUNT_BRUTE_FORCE: every triangle in index order, no tree.
 * PT_COUNT_STATS: the counting variant (one ray per thread) fills pt_get_stats: rays_closest = n, rays_shadow = samples = 0,
 *   nodes_examined, tris_tested, stack_drops and max_stack by the rules of the ray queries' counters.  With PT_COUNT_BRUTE_FORCE only
 *   rays_closest and tris_tested are counted.
 * PT_COUNT_SIMPLE_KERNEL: the one-ray-per-thread kernel instead of the persistent one (A/B checks); the results are the same.
 * Ordering, errors and alignment: as pt_trace_rays (rays 16-byte aligned, counts 4-byte aligned).  n = 0: PT_OK, nothing is launched.
 *
 * pt_contains: crossing parity by majority vote over `samples` rays per point.  Sample ray s of point i is, bit for bit, record
 *   i * samples + s of pt_occlusion_rays_host for the surfels {p, r_max = +inf, n = (0, 0, 1)} with bias = 0 and the same samples, seed and
 *   index_base (a cosine-distributed direction around +z; t_max = +inf).  odd = the number of those rays whose pt_count_hits count is odd;
 *   inside = (2 * odd > samples); samples = params.samples; reserved = 0.  The point's r_max field is ignored.  A point with a NaN in p is
 *   not traced and yields {0, 0, 0, 0}.
 *   Meaning: on a closed mesh this is the point-in-solid test.  On an open or self-intersecting mesh it is whatever the parity is;
 *   odd / samples tells the caller how much the rays disagreed.  No mesh is repaired and no orientation is consulted.
 *   Arguments: samples odd and in 1..255, n * samples <= 2^32 - 1, known flags, non-NULL params, else PT_ERR_INVALID_ARG; pointers
 *   16-byte aligned; the scene as for pt_trace_rays.
 *   PT_CONTAIN_STATS counts like pt_count_hits(PT_COUNT_STATS) over the rays of the traced points (rays_closest = samples * their number).
 *   PT_CONTAIN_SIMPLE_KERNEL: the one-ray-per-thread kernel instead of the persistent one; the results are the same.
 *
 * pt_signed_distance: the PtClosest record of pt_closest_points(flags = 0) with the sign bit of dist set where pt_contains says inside
 *   (-inf: inside, and nothing within r_max).  Three launches on the context's stream, no host wait: the closest points into out, the
 *   containment into a buffer of the context, one thread per point for the sign.  params as for pt_contains. */
typedef struct PtContainment { uint32_t inside; uint32_t odd; uint32_t samples; uint32_t reserved; } PtContainment;   /* 16 B */
typedef struct PtContainParams { uint32_t samples; uint32_t seed; uint32_t index_base; uint32_t flags; } PtContainParams;
enum { PT_COUNT_STATS = 1u, PT_COUNT_SIMPLE_KERNEL = 2u, PT_COUNT_BRUTE_FORCE = 4u };
enum { PT_CONTAIN_STATS = 1u, PT_CONTAIN_SIMPLE_KERNEL = 2u };
/* n rays from device memory (PtRay[n], 16-byte aligned), n counts into device memory (uint32_t[n], 4-byte aligned).  Asynchronous on
 * the context's stream (pt_get_stream). */
PT_API int pt_count_hits(PtContext* ctx, const void* rays_device, uint64_t n, uint32_t flags, void* counts_device);
/* The same from host arrays: staged through device buffers of the context; returns when the counts are written. */
PT_API int pt_count_hits_host(PtContext* ctx, const PtRay* rays, uint64_t n, uint32_t flags, uint32_t* counts);
/* Host twin (no context, no GPU): the same counts and, with PT_COUNT_STATS and stats != NULL, the same counters as the device gives for
 * the tree pt_set_bvh4(bvh4) installs over pt_set_triangles(tris).  bvh4 = NULL (words = 0) only with PT_COUNT_BRUTE_FORCE; a malformed
 * bvh4: PT_ERR_BAD_BVH; a NULL rays or counts pointer with n > 0, or unknown flags: PT_ERR_INVALID_ARG. */
PT_API int pt_count_hits_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words,
                              const PtRay* rays, uint64_t n, uint32_t flags, uint32_t* counts, PtStats* stats);
/* n points from device memory (PtPoint[n]), n PtContainment records into device memory (both 16-byte aligned).  Asynchronous. */
PT_API int pt_contains(PtContext* ctx, const void* points_device, uint64_t n, const PtContainParams* params, void* out_device);
PT_API int pt_contains_host(PtContext* ctx, const PtPoint* points, uint64_t n, const PtContainParams* params, PtContainment* out);
/* Host twin (no context, no GPU): pt_occlusion_rays_host -> pt_count_hits_bvh4 -> parity -> majority; the same records and counters. */
PT_API int pt_contains_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words,
                            const PtPoint* points, uint64_t n, const PtContainParams* params, PtContainment* out, PtStats* stats);
/* n points from device memory, n PtClosest records into device memory (both 16-byte aligned).  Asynchronous, no host wait. */
PT_API int pt_signed_distance(PtContext* ctx, const void* points_device, uint64_t n, const PtContainParams* params, void* out_device);
PT_API int pt_signed_distance_host(PtContext* ctx, const PtPoint* points, uint64_t n, const PtContainParams* params, PtClosest* out);

/* ---- radius queries: which triangles lie within r of a point -- all of them, each with its contact point? (an extension beyond the
 * reference) ----------------------------------------------------------------------------------------------
 * For every point the walk of pt_closest_points runs over the context's CURRENT tree with best2 held constant at r2, and every triangle it
 * reaches with d2 < r2 is counted (pt_radius_count) and listed (pt_radius_search).  Every result is an integer or a bit pattern.
 * Walked points: a point is walked iff p and r_max hold no NaN and r_max > 0 (ptcp::point_walked, as pt_closest_points); otherwise its
 *   count is 0 and its list is empty.
 * r2 = r_max * r_max in f32 (+inf stays +inf), constant for the whole walk.
 * Accepted leaves: a reached leaf with tri < num_tris is accepted iff d2 < r2, strictly; d2 by the point-triangle arithmetic of
 *   pt_closest_points (csrc/pt_closest.h: closest_uv, then closest_d2) on the triangle record as stored.  A NaN d2 is never accepted.
 * The walk: pt_closest_points' with best2 replaced by r2 -- bound2 with the same slack s = 2^-12; a child is entered iff bound2 < r2;
 *   passing children keep slot order, the first minimum trades places with the first passing child and is entered next, the others are
 *   pushed far -> near; a stacked child is re-validated at pop by bound2 < r2 (which always passes here: the walk is the shared one); the
 *   stack holds 64 entries and a push at the cap is dropped (and counted); a degenerate root box gives 0 for every point.  Spheres
 *   (pt_set_spheres) take no part.
 * The list: count[i] = the number of accepted leaves of point i; its list is those leaves IN VISIT ORDER, which is a property of the point
 *   and the tree, not of the scheduling: every kernel variant and the host twin give the same order.
 * Entries: one PtClosest per accepted leaf: dist = sqrtf(d2), prim = the triangle, u, v from the same operations -- the bits
 *   pt_closest_points(PT_CLOSEST_BRUTE_FORCE) gives for that point if that triangle is the only one.
 * pt_radius_search: offsets[0] = 0 and offsets[i + 1] - offsets[i] = count[i] in uint64_t (no wrap); offsets[n] = the total.  The entry
 *   with global index g = offsets[i] + k is written iff g < capacity; entries at and beyond min(total, capacity) are not touched.  The
 *   offsets are always complete: offsets[n] > capacity says that the list was truncated and how large the retry must be.
 *   entries_device = NULL is allowed with capacity = 0 (offsets only).  Three launches on the context's stream, no host wait: the count
 *   walk into a buffer of the context, an exclusive scan, a second walk of the same steps that stores entry k of point i at
 *   offsets[i] + k.  No atomic appends anything, so the order never depends on scheduling.
 * PT_RADIUS_BRUTE_FORCE: every triangle in index order, no tree; the list is then in index order.
 * PT_RADIUS_STATS: the counting variant (one point per thread) fills pt_get_stats: rays_closest = n, nodes_examined, tris_tested,
 *   stack_drops and max_stack by the rules of PT_CLOSEST_STATS, counted over the count walk only (rays_shadow = samples = 0).  With
 *   PT_RADIUS_BRUTE_FORCE only rays_closest and tris_tested are counted.
 * PT_RADIUS_SIMPLE_KERNEL: the one-point-per-thread kernels instead of the persistent one (A/B checks); the results are the same.
 * Completeness: for vertex coordinates within [-4, 4] and point coordinates within [-32, 32], wherever every triangle is reachable from
 *   the root and the walk drops nothing at the cap (stack_drops = 0), the set listed for a point equals the set PT_RADIUS_BRUTE_FORCE lists
 *   (bound2 < best2 never prunes a triangle with d2 < best2).
 *   STACK DROPS LOSE ENTRIES.  A radius that covers much of a deep tree pushes up to three siblings per level and nothing is ever pruned
 *   behind it, so the 64-entry cap is nearer here than in any sibling query.  A dropped subtree is missing from the list without a mark
 *   on the item; the only report is stack_drops of PT_RADIUS_STATS, as in the sibling queries.  A caller that needs every triangle for
 *   large radii checks that counter, or uses PT_RADIUS_BRUTE_FORCE.  With drops the walk's list is still a subset of the brute-force set.
 * Ordering, errors and alignment: as pt_closest_points.  Points and entries 16-byte aligned, offsets 8-byte, counts 4-byte; a NULL or
 *   misaligned pointer (entries: unless capacity = 0), unknown flags or n > UINT32_MAX: PT_ERR_INVALID_ARG (checked before the scene).
 *   No triangles + tree: PT_ERR_NO_SCENE.  n = 0: PT_OK, no kernel is launched (pt_radius_search still sets offsets[0] = 0).  A scene
 *   change after a call does not change its results. */
enum { PT_RADIUS_STATS = 1u, PT_RADIUS_SIMPLE_KERNEL = 2u, PT_RADIUS_BRUTE_FORCE = 4u };
/* n points from device memory (PtPoint[n], 16-byte aligned), n counts into device memory (uint32_t[n], 4-byte aligned).  Asynchronous on
 * the context's stream (pt_get_stream). */
PT_API int pt_radius_count(PtContext* ctx, const void* points_device, uint64_t n, uint32_t flags, void* counts_device);
/* The same from host arrays: staged through device buffers of the context; returns when the counts are written. */
PT_API int pt_radius_count_host(PtContext* ctx, const PtPoint* points, uint64_t n, uint32_t flags, uint32_t* counts);
/* n points from device memory -> offsets_device: uint64_t[n + 1] (8-byte aligned); entries_device: PtClosest[capacity] (16-byte aligned).
 * Asynchronous on the context's stream, no host wait. */
PT_API int pt_radius_search(PtContext* ctx, const void* points_device, uint64_t n, uint32_t flags,
                            void* offsets_device, void* entries_device, uint64_t capacity);
/* The same from host arrays: staged; the host reads the total between the scan and the second walk; returns when everything is written. */
PT_API int pt_radius_search_host(PtContext* ctx, const PtPoint* points, uint64_t n, uint32_t flags,
                                 uint64_t* offsets, PtClosest* entries, uint64_t capacity);
/* Host twin (no context, no GPU): the same offsets, entry bits and order (and the same truncation at `capacity`) and, with PT_RADIUS_STATS
 * and stats != NULL, the same counters as the device gives for the tree pt_set_bvh4(bvh4) installs over pt_set_triangles(tris).
 * bvh4 = NULL (words = 0) only with PT_RADIUS_BRUTE_FORCE; a malformed bvh4: PT_ERR_BAD_BVH; a NULL points pointer with n > 0, NULL
 * offsets, NULL entries with capacity > 0, offsets not 8-byte aligned, or unknown flags: PT_ERR_INVALID_ARG.  points and entries need
 * only the alignment of their types here. */
PT_API int pt_radius_search_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const PtPoint* points, uint64_t n,
                                 uint32_t flags, uint64_t* offsets, PtClosest* entries, uint64_t capacity, PtStats* stats);

/* ---- box-overlap queries: which triangles overlap an axis-aligned box -- all of them? (an extension beyond the reference; DESIGN.md
 * section 21) --------------------------------------------------------------------------------------------------------------------
 * Records: PtBox in (32 B, read as 2 x 16 B like PtRay; the pads are ignored), one PtOverlap per accepted triangle out (16 B, written as
 *   one record; both reserved words are written as 0); offsets is uint64_t[n + 1].  Every result is an integer.
 *   verts_inside: bit i is set when vertex i lies in the closed box; 7 means that the whole triangle is inside.
 * Walked boxes: a box is walked iff its six coordinates are finite and lo[k] <= hi[k] on every axis.  Zero-extent boxes (a point, a
 *   segment, a rectangle) are valid.  Any other box has count 0 and an empty list.
 * The triangle test (csrc/pt_overlap.h, one text for the kernels and the host twin; plain f32, each operation rounded once) on a triangle
 *   record as stored (v0, e1 = v1 - v0, e2 = v2 - v0):
 *   vertices: v1 = v0 + e1, v2 = v0 + e2, per component.
 *   (a) the box axes, compared directly with the corners as given, no centre involved: on each axis k, min(v0k, v1k, v2k) <= hi[k] and
 *       max(v0k, v1k, v2k) >= lo[k], and no v_ik is a NaN.  The same comparisons give verts_inside.
 *   (b) the plane, relative to the centre: c = (lo + hi) * 0.5f, h = (hi - lo) * 0.5f, a_i = v_i - c, n = e1 x e2 (each product rounded,
 *       then the difference): |(n.x a0.x + n.y a0.y) + n.z a0.z| <= (|n.x| h.x + |n.y| h.y) + |n.z| h.z.
 *   (c) nine edge axes: for f = e1, e2 - e1, e2 in that order, crossed with x, y, z in that order, the projections p_i of a_0..a_2 and the
 *       box radius r, every product rounded, then the difference or the sum:
 *         x: p_i = a_i.z f.y - a_i.y f.z, r = h.y |f.z| + h.z |f.y|;   y: p_i = a_i.x f.z - a_i.z f.x, r = h.x |f.z| + h.z |f.x|;
 *         z: p_i = a_i.y f.x - a_i.x f.y, r = h.x |f.y| + h.y |f.x|;   the axis passes iff min p <= r and max p >= -r.
 *   A triangle is ACCEPTED iff (a) passes and either verts_inside != 0 or (b) and all of (c) pass: a vertex in the closed box is an overlap
 *   with no rounding involved.  Every comparison is written so that a NaN operand fails it: a NaN triangle is never accepted.  Touching
 *   counts as overlap.  The result is a pure boolean, so early exits change nothing.
 * The node test, on a packed f16 child box (mn, mx): a child is entered iff mn[k] <= hi[k] + s and mx[k] >= lo[k] - s on every axis, with
 *   s = 2^-12 (the slack of pt_closest_points); hi + s and lo - s are computed once per box.  The inverted box of an empty slot fails.
 * The walk: the shared walk of the point queries with every key equal -- passing children are walked depth first in slot order; the stack
 *   holds 64 entries and a push at the cap is dropped (and counted); a degenerate root box gives 0 for every box; a leaf with
 *   tri >= num_tris is skipped.  Spheres (pt_set_spheres) take no part.
 * The list: count[i] = the number of accepted leaves of box i; its list is those leaves IN VISIT ORDER, which is a property of the box and
 *   the tree, not of the scheduling: every kernel variant and the host twin give the same order.
 * pt_box_search: offsets[0] = 0 and offsets[i + 1] - offsets[i] = count[i] in uint64_t (no wrap); offsets[n] = the total.  The entry with
 *   global index g = offsets[i] + k is written iff g < capacity; entries at and beyond min(total, capacity) are not touched.  The offsets
 *   are always complete: offsets[n] > capacity says that the list was truncated and how large the retry must be.  entries_device = NULL is
 *   allowed with capacity = 0 (offsets only).  Three launches on the context's stream, no host wait: the count walk into a buffer of the
 *   context, an exclusive scan, a second walk of the same steps that stores entry k of box i at offsets[i] + k.  No atomic appends anything.
 * PT_BOX_BRUTE_FORCE: every triangle in index order through the same triangle test, no tree; the list is then in index order.
 * PT_BOX_STATS: the counting variant (one box per thread) fills pt_get_stats: rays_closest = n, nodes_examined, tris_tested, stack_drops
 *   and max_stack by the rules of PT_RADIUS_STATS, counted over the count walk only.  With PT_BOX_BRUTE_FORCE only rays_closest and
 *   tris_tested are counted.
 * PT_BOX_SIMPLE_KERNEL: the one-box-per-thread kernels instead of the persistent one (A/B checks); the results are the same.
 * Completeness: for vertex coordinates within [-4, 4] and box coordinates within [-32, 32], wherever every triangle is reachable from the
 *   root and the walk drops nothing at the cap (stack_drops = 0), the walk lists exactly the set PT_BOX_BRUTE_FORCE lists (DESIGN.md
 *   section 21 has the proof).  STACK DROPS LOSE ENTRIES: nothing is ever pruned behind a large box, so it reaches the 64-entry cap as a
 *   large radius does; the only report is stack_drops of PT_BOX_STATS.  With drops the walk's list is a subset of the brute-force list.
 * Ordering, errors and alignment: as pt_radius_search.  Boxes and entries 16-byte aligned, offsets 8-byte, counts 4-byte; a NULL or
 *   misaligned pointer (entries: unless capacity = 0), unknown flags or n > UINT32_MAX: PT_ERR_INVALID_ARG (checked before the scene).
 *   No triangles + tree: PT_ERR_NO_SCENE.  n = 0: PT_OK, no kernel is launched (pt_box_search still sets offsets[0] = 0).  A scene change
 *   after a call does not change its results. */
typedef struct PtBox     { float lo[3]; float pad0; float hi[3]; float pad1; } PtBox;             /* 32 B, 16-byte aligned arrays */
typedef struct PtOverlap { uint32_t prim; uint32_t verts_inside; uint32_t reserved[2]; } PtOverlap; /* 16 B */
enum { PT_BOX_STATS = 1u, PT_BOX_SIMPLE_KERNEL = 2u, PT_BOX_BRUTE_FORCE = 4u };
/* n boxes from device memory (PtBox[n], 16-byte aligned), n counts into device memory (uint32_t[n], 4-byte aligned).  Asynchronous on
 * the context's stream (pt_get_stream). */
PT_API int pt_box_count(PtContext* ctx, const void* boxes_device, uint64_t n, uint32_t flags, void* counts_device);
/* The same from host arrays: staged through device buffers of the context; returns when the counts are written. */
PT_API int pt_box_count_host(PtContext* ctx, const PtBox* boxes, uint64_t n, uint32_t flags, uint32_t* counts);
/* n boxes from device memory -> offsets_device: uint64_t[n + 1] (8-byte aligned); entries_device: PtOverlap[capacity] (16-byte aligned).
 * Asynchronous on the context's stream, no host wait. */
PT_API int pt_box_search(PtContext* ctx, const void* boxes_device, uint64_t n, uint32_t flags,
                         void* offsets_device, void* entries_device, uint64_t capacity);
/* The same from host arrays: staged; the host reads the total between the scan and the second walk; returns when everything is written. */
PT_API int pt_box_search_host(PtContext* ctx, const PtBox* boxes, uint64_t n, uint32_t flags,
                              uint64_t* offsets, PtOverlap* entries, uint64_t capacity);
/* Host twin (no context, no GPU): the same offsets, entry words and order (and the same truncation at `capacity`) and, with PT_BOX_STATS
 * and stats != NULL, the same counters as the device gives for the tree pt_set_bvh4(bvh4) installs over pt_set_triangles(tris).
 * bvh4 = NULL (words = 0) only with PT_BOX_BRUTE_FORCE; a malformed bvh4: PT_ERR_BAD_BVH; a NULL boxes pointer with n > 0, NULL offsets,
 * NULL entries with capacity > 0, offsets not 8-byte aligned, or unknown flags: PT_ERR_INVALID_ARG.  boxes and entries need only the
 * alignment of their types here. */
PT_API int pt_box_search_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const PtBox* boxes, uint64_t n,
                              uint32_t flags, uint64_t* offsets, PtOverlap* entries, uint64_t capacity, PtStats* stats);

/* ---- triangle-overlap queries: which mesh triangles does a caller triangle cut -- all of them? (an extension beyond the reference;
 * DESIGN.md section 23) ----------------------------------------------------------------------------------------------------------
 * Records: PtTri in (48 B, read as 3 x 16 B; the pads are ignored), one PtCross per accepted mesh triangle out (16 B, written as one
 *   record; both reserved words are written as 0); offsets is uint64_t[n + 1].  Every result is an integer.
 *   edges: bits 0-2 say which of the caller triangle's edges q0->q1, q1->q2, q2->q0 cross the mesh triangle; bits 3-5 say which of the
 *   mesh triangle's edges (v0, e1), (v1, e2 - e1), (v0, e2) -- with v1 = v0 + e1 per component, as in the box query -- cross the caller's
 *   triangle.  In general position exactly two of the six bits are set: the two crossing edges give the end points of the intersection
 *   segment.
 * Walked triangles: a caller triangle is walked iff its nine coordinates are finite.  Any other triangle has count 0 and an empty list.  A
 *   degenerate triangle (zero area) is walked; it is then a segment or a point, and only the mesh side's tests can accept it.
 * The bounding box: lo[k] = min, hi[k] = max of the three vertices as given (exact).
 * The segment test (csrc/pt_tritri.h, one text for the kernels and the host twin; plain f32, each operation rounded once) of a segment
 *   (p, d) -- from p to p + d -- against a triangle (a, f1, f2), a division-free, scale-free Moeller-Trumbore with dot(a, b) =
 *   (a.x b.x + a.y b.y) + a.z b.z and cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x), every product rounded:
 *     pv = cross(d, f2), det = dot(f1, pv), sv = p - a, U = dot(sv, pv), qv = cross(sv, f1), V = dot(d, qv), T = dot(f2, qv);
 *     crosses iff det > 0 and U >= 0, V >= 0, U + V <= det, T >= 0, T <= det, or det < 0 and the same five comparisons mirrored.
 *   det == 0 or a NaN crosses nothing.  There is no epsilon: touching counts wherever the rounded values say so.
 * The triangle test on a record as stored (v0, e1 = v1 - v0, e2 = v2 - v0):
 *   (a) the box-axis stage of pt_box_search's triangle test, of the record's three vertices against lo, hi;
 *   (b) the six segment tests: the caller's edges (q0, q1 - q0), (q1, q2 - q1), (q2, q0 - q2) against (v0, e1, e2), and the mesh edges
 *       (v0, e1), (v1, e2 - e1), (v0, e2) against (q0, q1 - q0, q2 - q0); every difference per component, with one rounding.
 *   A triangle is ACCEPTED iff (a) passes and edges != 0.
 * COPLANAR PAIRS ARE NOT LISTED: every det is 0 for them.  A caller who needs them runs a 2-D test on the candidates of pt_box_search.
 * The node test and the walk: pt_box_search's, on the caller triangle's bounding box (the slack s = 2^-12, depth-first slot order, 64 stack
 *   entries with a push at the cap dropped and counted, a degenerate root box: 0 for every triangle, a leaf with tri >= num_tris skipped).
 * The list, the offsets, the capacity and its truncation, n = 0, the three launches without a host wait, PT_TRI_BRUTE_FORCE, PT_TRI_STATS
 *   and PT_TRI_SIMPLE_KERNEL: as pt_box_search and its PT_BOX_* flags, word for word.
 * Completeness: for vertex coordinates within [-4, 4] and caller coordinates within [-32, 32], wherever every triangle is reachable from
 *   the root and the walk drops nothing at the cap (stack_drops = 0), the walk lists exactly the set PT_TRI_BRUTE_FORCE lists: an accepted
 *   triangle passed (a), which is the premise of the box query's proof.  With drops the walk's list is a subset.
 * Ordering, errors and alignment: as pt_box_search.  Triangles and entries 16-byte aligned, offsets 8-byte, counts 4-byte. */
typedef struct PtTri   { float v0[3]; float pad0; float v1[3]; float pad1; float v2[3]; float pad2; } PtTri;   /* 48 B, 16-byte aligned arrays */
typedef struct PtCross { uint32_t prim; uint32_t edges; uint32_t reserved[2]; } PtCross;                      /* 16 B */
enum { PT_TRI_STATS = 1u, PT_TRI_SIMPLE_KERNEL = 2u, PT_TRI_BRUTE_FORCE = 4u };
/* n caller triangles from device memory (PtTri[n], 16-byte aligned), n counts into device memory (uint32_t[n], 4-byte aligned).
 * Asynchronous on the context's stream (pt_get_stream). */
PT_API int pt_tri_count(PtContext* ctx, const void* tris_device, uint64_t n, uint32_t flags, void* counts_device);
/* The same from host arrays: staged through device buffers of the context; returns when the counts are written. */
PT_API int pt_tri_count_host(PtContext* ctx, const PtTri* tris, uint64_t n, uint32_t flags, uint32_t* counts);
/* n caller triangles from device memory -> offsets_device: uint64_t[n + 1] (8-byte aligned); entries_device: PtCross[capacity] (16-byte
 * aligned).  Asynchronous on the context's stream, no host wait. */
PT_API int pt_tri_search(PtContext* ctx, const void* tris_device, uint64_t n, uint32_t flags,
                         void* offsets_device, void* entries_device, uint64_t capacity);
/* The same from host arrays: staged; the host reads the total between the scan and the second walk; returns when everything is written. */
PT_API int pt_tri_search_host(PtContext* ctx, const PtTri* tris, uint64_t n, uint32_t flags,
                              uint64_t* offsets, PtCross* entries, uint64_t capacity);
/* Host twin (no context, no GPU): the same offsets, entry words and order (and the same truncation at `capacity`) and, with PT_TRI_STATS
 * and stats != NULL, the same counters as the device gives for the tree pt_set_bvh4(bvh4) installs over pt_set_triangles(mesh).
 * bvh4 = NULL (words = 0) only with PT_TRI_BRUTE_FORCE; errors as pt_box_search_bvh4. */
PT_API int pt_tri_search_bvh4(const float* mesh, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const PtTri* tris, uint64_t n,
                              uint32_t flags, uint64_t* offsets, PtCross* entries, uint64_t capacity, PtStats* stats);

/* ---- plane-cut queries: which mesh triangles does a plane cut inside a window, and where? (an extension beyond the reference;
 * DESIGN.md section 24) ----------------------------------------------------------------------------------------------------------
 * Records: PtCutPlane in (48 B, read as 3 x 16 B; the pads are ignored), one PtCut per accepted mesh triangle out (16 B, written as one
 *   record); offsets is uint64_t[n + 1].  The plane is n.x = d; n need not be normalised.  [lo, hi] is a window, an axis-aligned box: it
 *   bounds a list and lets a caller tile one plane over many records.  THE WINDOW DOES NOT CLIP: it filters on the triangle's bounding
 *   box (stage (a) below), so a triangle whose box overlaps two windows is listed by both, with the same code, t0 and t1.
 * Walked records: a record is walked iff n and d are finite, n is not the zero vector, and the window's six coordinates are finite with
 *   lo <= hi on every axis (a zero-extent window is valid).  Any other record has count 0 and an empty list.
 * The plane function (csrc/pt_cut.h, one text for the kernels and the host twin; plain f32, each operation rounded once, no fused
 *   multiply-add): side(x, y, z) = ((n.x*x + n.y*y) + n.z*z) - d, in that order.
 * The triangle test on a record as stored (v0, e1 = v1 - v0, e2 = v2 - v0), with v1 = v0 + e1, v2 = v0 + e2 per component:
 *   (a) the box-axis stage of pt_box_search's triangle test, of the record's three vertices against lo, hi;
 *   (b) s_i = side(v_i): every s_i passes >= 0 or < 0 (a NaN fails), some s_i >= 0 and some s_i < 0.
 *   A triangle is ACCEPTED iff (a) and (b) pass.  This is the half-open rule of slicers: a triangle lying in the plane is not listed, nor
 *   one that touches the plane from the >= 0 side; one that touches it from below with one vertex is listed as a zero-length segment at
 *   that vertex.  Every accepted triangle has one lone vertex and exactly two crossing edges, so on a closed mesh the segments of a
 *   plane close into loops.
 * code: bits 0-2 say which edges cross, v0-v1, v1-v2, v0-v2 (the numbering of PtCross bits 3-5): exactly two are set.  Bits 3-5 are the
 *   classes s_0 >= 0, s_1 >= 0, s_2 >= 0.
 * t0, t1: t0 belongs to the lowest set edge bit, t1 to the highest.  Each is s_a / (s_a - s_b), a being that edge's vertex with s < 0
 *   and b the one with s >= 0: measured from a towards b, one subtraction and one division, within [0, 1].  The crossing point is
 *   v_a + t (v_b - v_a).
 * The node test: a child is entered iff pt_box_search's node test passes on the window AND, with the child's f16 box grown by the slack
 *   s = 2^-12 to fl(mn - s), fl(mx + s), side(p-corner) >= 0 and side(n-corner) < 0, the p-corner taking the grown upper value on the
 *   axes where n_k >= 0 and the lower one elsewhere, the n-corner the opposite.  The walk is pt_box_search's (depth-first slot order,
 *   64 stack entries with a push at the cap dropped and counted, a degenerate root box: 0 for every plane, a leaf with tri >= num_tris
 *   skipped).
 * The list, the offsets, the capacity and its truncation, n = 0, the three launches without a host wait, PT_CUT_BRUTE_FORCE, PT_CUT_STATS
 *   and PT_CUT_SIMPLE_KERNEL: as pt_box_search and its PT_BOX_* flags, word for word.
 * Completeness: for vertex coordinates within [-4, 4], window coordinates within [-32, 32] and |n_k|, |d| <= 2^100, wherever every
 *   triangle is reachable from the root and the walk drops nothing at the cap (stack_drops = 0), the walk lists exactly the set
 *   PT_CUT_BRUTE_FORCE lists: every f32 operation is monotone in each operand, so side of any point between the grown corners lies between
 *   side(n-corner) and side(p-corner) in the rounded values.  With drops the walk's list is a subset.
 * Ordering, errors and alignment: as pt_box_search.  Planes and entries 16-byte aligned, offsets 8-byte, counts 4-byte. */
typedef struct PtCutPlane { float n[3]; float d; float lo[3]; float pad0; float hi[3]; float pad1; } PtCutPlane;   /* 48 B, 16-byte aligned arrays */
typedef struct PtCut { uint32_t prim; uint32_t code; float t0; float t1; } PtCut;                                /* 16 B */
enum { PT_CUT_STATS = 1u, PT_CUT_SIMPLE_KERNEL = 2u, PT_CUT_BRUTE_FORCE = 4u };
/* n records from device memory (PtCutPlane[n], 16-byte aligned), n counts into device memory (uint32_t[n], 4-byte aligned).
 * Asynchronous on the context's stream (pt_get_stream). */
PT_API int pt_cut_count(PtContext* ctx, const void* planes_device, uint64_t n, uint32_t flags, void* counts_device);
/* The same from host arrays: staged through device buffers of the context; returns when the counts are written. */
PT_API int pt_cut_count_host(PtContext* ctx, const PtCutPlane* planes, uint64_t n, uint32_t flags, uint32_t* counts);
/* n records from device memory -> offsets_device: uint64_t[n + 1] (8-byte aligned); entries_device: PtCut[capacity] (16-byte aligned).
 * Asynchronous on the context's stream, no host wait. */
PT_API int pt_cut_search(PtContext* ctx, const void* planes_device, uint64_t n, uint32_t flags,
                         void* offsets_device, void* entries_device, uint64_t capacity);
/* The same from host arrays: staged; the host reads the total between the scan and the second walk; returns when everything is written. */
PT_API int pt_cut_search_host(PtContext* ctx, const PtCutPlane* planes, uint64_t n, uint32_t flags,
                              uint64_t* offsets, PtCut* entries, uint64_t capacity);
/* Host twin (no context, no GPU): the same offsets, entry words and order (and the same truncation at `capacity`) and, with PT_CUT_STATS
 * and stats != NULL, the same counters as the device gives for the tree pt_set_bvh4(bvh4) installs over pt_set_triangles(tris).
 * bvh4 = NULL (words = 0) only with PT_CUT_BRUTE_FORCE; errors as pt_box_search_bvh4. */
PT_API int pt_cut_search_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const PtCutPlane* planes, uint64_t n,
                              uint32_t flags, uint64_t* offsets, PtCut* entries, uint64_t capacity, PtStats* stats);

/* ---- hit lists: which triangles does a ray cross, and where -- all of them, each with t and u, v? (an extension beyond the reference;
 * DESIGN.md section 20) -----------------------------------------------------------------------------------------------------------
 * Records: PtRay in, one PtHit (t, prim, u, v) per crossing out; offsets is uint64_t[n + 1].  Every result is an integer or a bit pattern.
 * Which crossings: exactly the records pt_count_hits counts for the same ray and flags -- the same walk over the context's CURRENT tree in
 *   the same visit order, best = min(t_max, 1e30) constant, a record accepted iff the Moller-Trumbore test of the ray queries holds and
 *   t < best, 64 stack entries with a push at the cap dropped (and counted), a leaf with t >= num_tris skipped, a degenerate root box: no
 *   crossing.  Rays with no walk (a NaN in org or dir, or t_max <= 0 or NaN) have an empty list.  So offsets[i + 1] - offsets[i] equals
 *   pt_count_hits' count of ray i, always, with stack drops too, and a list is non-empty exactly when pt_trace_rays(PT_TRACE_ANY_HIT)
 *   reports a hit.  Misses are never stored.
 * Entries: t is the t of the accepted test; u, v come from the arithmetic of pt_trace_rays' result on the same triangle record -- the bits
 *   pt_trace_rays gives for that ray if that triangle is the only one.
 * Order: without PT_HITS_SORTED the list of a ray is in VISIT ORDER, which is a property of the ray and the tree, not of the scheduling:
 *   every kernel variant and the host twin give the same order.  With PT_HITS_BRUTE_FORCE it is triangle index order.  With
 *   PT_HITS_SORTED every fully stored list is in ascending order of the 64-bit key (bits(t) << 32) | prim; every stored t is positive and
 *   finite, so bit order is value order, and the sorted list depends on neither the tree, the kernel variant nor the scheduling (equal keys
 *   can only be one triangle held by two leaves, whose entries are identical).
 * pt_list_hits: offsets[0] = 0 and offsets[i + 1] - offsets[i] = count[i] in uint64_t (no wrap); offsets[n] = the total.  The entry
 *   with global index g = offsets[i] + k is written iff g < capacity; entries at and beyond min(total, capacity) are not touched.  The
 *   offsets are always complete: offsets[n] > capacity says that the list was truncated and how large the retry must be.
 *   hits_device = NULL is allowed with capacity = 0 (offsets only).  With PT_HITS_SORTED only the lists with offsets[i + 1] <= capacity are
 *   sorted: the one list that straddles the capacity stays in visit order.  Three launches on the context's stream (four with
 *   PT_HITS_SORTED), no host wait: pt_count_hits' walk into a buffer of the context, an exclusive scan, a second walk of the same steps
 *   that stores entry k of ray i at offsets[i] + k, the in-place sort.  No atomic appends anything.
 * PT_HITS_BRUTE_FORCE, PT_HITS_STATS, PT_HITS_SIMPLE_KERNEL: what PT_COUNT_BRUTE_FORCE, PT_COUNT_STATS and PT_COUNT_SIMPLE_KERNEL mean for
 *   pt_count_hits; the counters are counted over the count walk only.
 * Completeness: the list is a subset of the PT_HITS_BRUTE_FORCE list on a tree whose leaves hold each triangle once; the two are equal (as
 *   sets, and bit for bit when sorted) wherever nothing is dropped at the cap and no crossing is lost to an f16 box.
 *   STACK DROPS LOSE ENTRIES, as they lose counts in pt_count_hits: a dropped subtree is missing from the list without a mark on the item;
 *   the only report is stack_drops of PT_HITS_STATS.  A caller that needs every crossing checks that counter, or uses PT_HITS_BRUTE_FORCE.
 * Ordering, errors and alignment: as pt_radius_search.  Rays and hits 16-byte aligned, offsets 8-byte; a NULL or misaligned pointer (hits:
 *   unless capacity = 0), unknown flags or n > UINT32_MAX: PT_ERR_INVALID_ARG (checked before the scene).  No triangles + tree:
 *   PT_ERR_NO_SCENE.  n = 0: PT_OK, no kernel is launched, offsets[0] = 0.  A scene change after a call does not change its results. */
enum { PT_HITS_STATS = 1u, PT_HITS_SIMPLE_KERNEL = 2u, PT_HITS_BRUTE_FORCE = 4u, PT_HITS_SORTED = 8u };
/* n rays from device memory (PtRay[n], 16-byte aligned) -> offsets_device: uint64_t[n + 1] (8-byte aligned); hits_device: PtHit[capacity]
 * (16-byte aligned).  Asynchronous on the context's stream (pt_get_stream), no host wait. */
PT_API int pt_list_hits(PtContext* ctx, const void* rays_device, uint64_t n, uint32_t flags,
                        void* offsets_device, void* hits_device, uint64_t capacity);
/* The same from host arrays: staged; the host reads the total between the scan and the second walk; returns when everything is written. */
PT_API int pt_list_hits_host(PtContext* ctx, const PtRay* rays, uint64_t n, uint32_t flags,
                             uint64_t* offsets, PtHit* hits, uint64_t capacity);
/* Host twin (no context, no GPU): the same offsets, entry bits and order (and the same truncation at `capacity`; it sorts by the same key)
 * and, with PT_HITS_STATS and stats != NULL, the same counters as the device gives for the tree pt_set_bvh4(bvh4) installs over
 * pt_set_triangles(tris).  bvh4 = NULL (words = 0) only with PT_HITS_BRUTE_FORCE; a malformed bvh4: PT_ERR_BAD_BVH; a NULL rays pointer
 * with n > 0, NULL offsets, NULL hits with capacity > 0, offsets not 8-byte aligned, or unknown flags: PT_ERR_INVALID_ARG.  rays and hits
 * need only the alignment of their types here. */
PT_API int pt_list_hits_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const PtRay* rays, uint64_t n,
                             uint32_t flags, uint64_t* offsets, PtHit* hits, uint64_t capacity, PtStats* stats);

/* ---- k-nearest queries: which k triangles are closest to a point, each with its contact point? (an extension beyond the reference;
 * DESIGN.md section 19) -----------------------------------------------------------------------------------------------------------
 * Records: PtPoint in, PtClosest out.  out holds n * k PtClosest, row i at out[i*k .. i*k + k-1].  Every result is an integer or a bit
 * pattern.
 * Per point: a point is walked exactly when ptcp::point_walked holds (p and r_max hold no NaN, r_max > 0, as pt_closest_points).
 *   r2 = r_max * r_max in f32 (+inf stays +inf).  The lane keeps a list L of at most k pairs (d2, leaf reference), sorted ascending by d2.
 *   worst2 = r2 while |L| < k; otherwise it is the d2 of L's last pair.  A reached leaf with tri < num_tris is accepted when d2 < worst2,
 *   strictly; a NaN is never accepted; d2 comes from csrc/pt_closest.h (closest_uv, then closest_d2) on the record as stored.  An accepted
 *   pair is inserted behind every pair with d2' <= d2, so equal distances keep visit order.  If L held k pairs, the last one falls off.
 * The walk: pt_closest_points' with best2 replaced by worst2 -- a child is entered iff box_bound2 < worst2 (the same slack s = 2^-12);
 *   bound() returns worst2, and a stacked child is re-validated at pop against it; the order of order_children (passing children keep slot
 *   order, the first minimum trades places with the first passing child and is entered next, the others are pushed far -> near); 64 stack
 *   entries, a push at the cap dropped and counted; a degenerate root finds nothing.  Spheres (pt_set_spheres) take no part.
 * Output: row i, entry j < |L|: dist = sqrtf(d2), prim, and u, v recomputed from the record with the operations of the accepted test --
 *   the bits pt_closest_points gives for that triangle.  Entries j >= |L|, and every entry of a point that is not walked: dist = +inf,
 *   prim = 0xFFFFFFFF, u = v = 0.  Every one of the n * k records is written.  Nothing behind them is touched.
 * Arguments: k = 0 or k > PT_NEAREST_MAX_K: PT_ERR_INVALID_ARG.  Pointers, alignment (16 bytes), unknown flags, n > UINT32_MAX, n = 0
 *   (PT_OK, no kernel), ordering against queued frames, and scene changes after the call: as pt_closest_points.
 * PT_NEAREST_BRUTE_FORCE: every triangle in index order with the same list rule.  Ties are then in index order.
 * PT_NEAREST_STATS: rays_closest = n, nodes_examined, tris_tested, stack_drops, max_stack by the rules of PT_CLOSEST_STATS, served by the
 *   one-point-per-thread kernel.  PT_NEAREST_SIMPLE_KERNEL: that kernel without counters (A/B checks); the results are the same.
 * Consequences: k = 1 gives the bits of pt_closest_points on every point, prim included.  For vertex coordinates within [-4, 4] and point
 *   coordinates within [-32, 32], wherever every triangle is reachable from the root and stack_drops = 0, the multiset of d2 in a row equals
 *   brute force's k smallest d2 < r2 (a pruned subtree has d2 >= bound2 >= worst2 at that moment, and worst2 only falls); prim may differ
 *   from brute force only among triangles whose d2 bits are equal.  The persistent kernel, the simple kernel and the host twin visit in the
 *   same order, so they agree bit for bit, ties included.  With drops a row is still made of true (prim, dist, u, v) records within r_max,
 *   but nearer triangles may be missing; the only report is stack_drops of PT_NEAREST_STATS. */
#define PT_NEAREST_MAX_K 64
enum { PT_NEAREST_STATS = 1u, PT_NEAREST_SIMPLE_KERNEL = 2u, PT_NEAREST_BRUTE_FORCE = 4u };
/* n points from device memory (PtPoint[n]) -> n * k records into device memory (PtClosest[n * k]), both 16-byte aligned.  Asynchronous on
 * the context's stream (pt_get_stream), no host wait, one launch (plus the zeroing of the walk's queue block). */
PT_API int pt_nearest_k(PtContext* ctx, const void* points_device, uint64_t n, uint32_t k, uint32_t flags, void* out_device);
/* The same from host arrays: staged through device buffers of the context like pt_closest_points_host; returns when the rows are written. */
PT_API int pt_nearest_k_host(PtContext* ctx, const PtPoint* points, uint64_t n, uint32_t k, uint32_t flags, PtClosest* out);
/* Host twin (no context, no GPU): the same rows and, with PT_NEAREST_STATS and stats != NULL, the same counters as the device gives for the
 * tree pt_set_bvh4(bvh4) installs over pt_set_triangles(tris).  Argument rules of pt_closest_points_bvh4: bvh4 = NULL (words = 0) only with
 * PT_NEAREST_BRUTE_FORCE; a malformed bvh4: PT_ERR_BAD_BVH; a NULL points or out pointer with n > 0, unknown flags, or k out of range:
 * PT_ERR_INVALID_ARG.  points and out need only the alignment of their types here. */
PT_API int pt_nearest_k_bvh4(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const PtPoint* points, uint64_t n,
                             uint32_t k, uint32_t flags, PtClosest* out, PtStats* stats);

/* ---- animated geometry: new vertices, the same tree (an extension beyond the reference) --------------
 * The reference rebuilds its tree whenever a vertex moves (PathTracer.buildBVH).  An update keeps the TOPOLOGY of the context's
 * current tree -- whatever installed it: pt_build_bvh, pt_build_bvh_accel of any level, pt_set_bvh4, pt_set_bvh2 -- and recomputes
 * every box from the new triangles, in place, on the device.  Child indices, leaf words, node counts and ids are untouched; the
 * result is a BVH4 in the reference's layout (pt_read_bvh4), so every frame after an update can be checked against the oracle.
 * The result depends on the topology and the current triangles only, not on earlier updates.
 *
 * Rules (host twins below, word for word):
 *   BVH4 leaf (word 7 has the leaf bit, triangle t < num_tris): the component-wise min / max of the three vertices, each rounded to
 *     nearest-even f16 and then stepped one f16 outwards, always (BVHBuilder.wgsl:63-102).  A leaf with t >= num_tris keeps its words.
 *   BVH4 internal node: Math.min / Math.max over the exactly decoded boxes of its valid children (index != 0xFFFFFFFF and < numNodes)
 *     in slot order, starting from +-inf, packed by truncation with f16 subnormals flushed to signed zero (PathTracer.js:42-51,
 *     640-661).  A node whose four slots are all invalid keeps its words.  Only nodes reachable from the root are refitted; a tree in
 *     which a node is reachable twice is refused by pt_set_bvh4 already.
 *   Device layouts: the 64-byte triangle records are rewritten, and every internal node's 64-byte wide record is what the build writes
 *     from the refitted BVH4 -- including the inverted box of an empty slot and the "fetched, never entered" mark of a child whose box
 *     became degenerate.
 *   BVH2 (when the context holds one): leaves by the leaf rule, internal nodes by the reference's propagateUp (the union of the two
 *     children, stepped outwards once more; BVHBuilder.wgsl:242-275).  Deferred to the next pt_read_bvh2; nothing else reads it.
 * Without a tree the call only replaces the triangles.
 * Arguments: num_tris must equal the context's triangle count (pt_set_triangles changes it).  A NULL pointer, a device pointer that is
 *   not 16-byte aligned, or another count: PT_ERR_INVALID_ARG (pointers are checked first).  No triangles uploaded yet: PT_ERR_NO_SCENE.
 *   After either error the context is exactly as it was.  num_tris == 0 (an empty scene): PT_OK, nothing is launched.
 * Ordering: frames queued by pt_set_batch are launched first (as pt_flush does): frames submitted before the update show the old
 *   geometry, frames after it the new.  A running accumulation restarts, as on any scene change.
 * The host's copies of what the tile cull and the kernel choice read -- the root box, its degenerate flag, the largest edge component --
 *   come back in one 16-byte copy behind the refit.  pt_update_triangles waits for it; pt_update_triangles_device does not: the next
 *   call that plans a launch (pt_render, pt_trace_rays, pt_traced_tile_rect) or changes the scene waits for that copy first.
 * The first update (or pt_bvh_cost) after a tree was installed also derives the parent links the climb needs, once: on the device for
 *   a tree this library built, by one read-back and a host walk for an installed one. */
/* tris: f32[9 * num_tris] on the host, copied during the call; returns when the update is done. */
PT_API int pt_update_triangles(PtContext* ctx, const float* tris, uint32_t num_tris);
/* tris_device: f32[9 * num_tris] on the context's device, 16-byte aligned.  Asynchronous on the context's stream (pt_get_stream): the
 * array is read by a copy queued there and may be reused once a later pt_synchronize has returned. */
PT_API int pt_update_triangles_device(PtContext* ctx, const void* tris_device, uint32_t num_tris);
/* Quality of the current tree: the sum, over the internal BVH4 nodes reachable from the root, of halfArea(node box) / halfArea(root
 * box), with halfArea = dx*dy + dy*dz + dz*dx of the exactly decoded f16 bounds in f64.  A box that is degenerate (a min above its max)
 * or has a NaN bound counts 0; the result is 0 when the root is a leaf or its half-area is 0 or not finite.  A refitted tree's cost
 * grows with the deformation: rebuild when it exceeds the cost at build by a factor of the caller's choice (nothing rebuilds by itself).
 * Device and host twin agree to a relative numNodes * 2^-51 (the order of the summation differs).  PT_ERR_NO_SCENE without a tree. */
PT_API int pt_bvh_cost(PtContext* ctx, double* cost);
/* Host twins (no context, no GPU), in place: the words the device refit leaves in pt_read_bvh4 / pt_read_bvh2 for the same topology and
 * triangles.  bvh4: u32[1 + 8 * numNodes]; bvh2: u32[1 + 6 * numNodes] with both children of an internal node in range and different
 * (a node where they are not keeps its words, as do its ancestors).  A buffer shorter than its node count or a BVH4 node reachable
 * twice: PT_ERR_BAD_BVH; a NULL pointer: PT_ERR_INVALID_ARG. */
PT_API int pt_refit_bvh4(const float* tris, uint32_t num_tris, uint32_t* bvh4, uint64_t words);
PT_API int pt_refit_bvh2(const float* tris, uint32_t num_tris, uint32_t* bvh2, uint64_t words);
PT_API int pt_bvh4_cost(const uint32_t* bvh4, uint64_t words, double* cost);

/* ---- pixel-tile sharding across GPUs (one context per GPU / rank) ------------------ */

/* Number of 8x8 tiles / pixels-slots this rank owns for a W x H frame split tile_count ways. */
PT_API int pt_tile_layout(uint32_t width, uint32_t height, uint32_t tile_rank, uint32_t tile_count,
                   uint32_t* num_tiles, uint64_t* compact_floats);
/* The tile ids (ty * ceil(W/8) + tx) this rank owns, in the order of its compact buffer: slot s of the buffer holds tile ids[s]
 * (64 pixels, row-major inside the 8x8 tile).  ids may be NULL to ask for the count only; capacity in entries.  This is the list
 * pt_render uploads for the share -- callers that assemble or check compact buffers themselves take the order from here. */
PT_API int pt_tile_ids(uint32_t width, uint32_t height, uint32_t tile_rank, uint32_t tile_count,
                uint32_t* ids, uint32_t capacity, uint32_t* num_tiles);
/* Device pointer + size of this rank's compact radiance buffer (tile-major, 64 px per tile,
 * f32 RGBA) after a render with tile_count > 1: the send buffer of the RCCL gather. */
PT_API int pt_compact_radiance(PtContext* ctx, void** device_ptr, uint64_t* floats);
/* Render tile-sharded frames straight into a caller-owned device buffer (e.g. a torch tensor
 * that is then handed to the RCCL gather) instead of the context's own compact buffer.
 * `floats` is the buffer's capacity.  The buffer that is current when a frame is submitted is that frame's
 * target, also for frames still queued by pt_set_batch when the target changes.  Lifetime rule: a buffer
 * handed in here must stay allocated until a pt_synchronize (or any read-back) issued after the last frame
 * that was submitted while it was current has returned -- or until pt_buffer_busy says it is free.  device_ptr = NULL
 * restores the internal buffer, launches whatever is still queued for caller-owned targets AND waits for it: when the call
 * returns no frame targets a caller-owned buffer any more. */
PT_API int pt_set_compact_buffer(PtContext* ctx, void* device_ptr, uint64_t floats);
/* The same for whole frames (tile_count <= 1): render into a caller-owned row-major f32 RGBA device buffer of at least
 * width*height*4 floats instead of the context's own frame buffer, e.g. one buffer per frame of a batched launch so that
 * every frame stays available (frames of one launch that share a target leave only the last one's result, exactly as if they
 * had been rendered one after the other).  The read-backs read the target of the last frame.  Same lifetime rule as
 * pt_set_compact_buffer; NULL restores the internal buffer, launches what is still queued and waits for it. */
PT_API int pt_set_output_buffer(PtContext* ctx, void* device_ptr, uint64_t floats);
/* *busy = 1 while a frame that is queued (pt_set_batch) or in flight (launched, not yet delivered) still writes into bytes that
 * overlap [device_ptr, device_ptr + bytes) -- whichever kernel renders it, however many launches were submitted after it: the check
 * to make before freeing or re-using a buffer that was handed to pt_set_compact_buffer / pt_set_output_buffer.  Does not wait. */
PT_API int pt_buffer_busy(PtContext* ctx, const void* device_ptr, uint64_t bytes, int* busy);
/* Rank 0: scatter `tile_count` gathered compact buffers (device memory, concatenated in rank
 * order, each padded to `stride_floats`) into the context's full-frame radiance buffer. */
PT_API int pt_deinterleave(PtContext* ctx, const void* gathered_device, uint64_t stride_floats,
                    uint32_t width, uint32_t height, uint32_t tile_count);
/* The same for a gathered BATCH of frames in one launch: rank r's share of frame j sits at gathered + r * rank_stride_floats +
 * j * frame_stride_floats (what one gather of `num_frames` consecutive compact buffers per rank leaves on the root); frame j is
 * scattered to frames_out_device + j * out_stride_floats (row-major f32 RGBA, caller-owned).  frames_out_device = NULL: the
 * context's own frame buffer, which holds one frame -- only the last frame of the batch is scattered (the earlier ones would
 * be replaced by it).  The read-backs then read the last frame. */
PT_API int pt_deinterleave_batch(PtContext* ctx, const void* gathered_device, uint64_t rank_stride_floats, uint64_t frame_stride_floats,
                          uint32_t num_frames, uint32_t width, uint32_t height, uint32_t tile_count,
                          void* frames_out_device, uint64_t out_stride_floats);

/* Packed tile shares: what a sharded frame needs to ship.  Outside the rectangle of tiles in which a camera ray can reach the scene's
 * root box at all, every pixel is the camera-miss value (renderer.wgsl:410) whatever is traced there -- two thirds of the tiles of the
 * dragon-class frame -- and alpha is 1 everywhere.  So a rank packs only its tiles INSIDE the rectangle, 12 bytes per pixel (its tiles
 * in row-major order, 64 x 3 floats each), the packed buffers are gathered, and rank 0 rebuilds the row-major frames: a quarter of the
 * bytes of the compact buffers for that frame.  Non-accumulating frames only (a running sum outside the rectangle depends on history).
 *
 * pt_traced_tile_rect: rect = {tx0, ty0, tx1, ty1}, half-open, in 8x8 tiles -- the rectangle this context's launches trace for a frame
 * with these parameters (the whole image when nothing can be left out); for several frames use the union. */
PT_API int pt_traced_tile_rect(PtContext* ctx, const PtRenderParams* params, uint32_t rect[4]);
/* Largest packed share over the ranks: tiles, and floats per frame (tiles * 192) -- the per-frame count of the gather. */
PT_API int pt_packed_layout(uint32_t width, uint32_t height, uint32_t tile_count, const uint32_t rect[4], uint32_t* max_tiles, uint64_t* floats_per_frame);
/* The tile ids (ty * ceil(W/8) + tx) of a rank's packed share, in the order of the packed buffer: slot s holds tile ids[s] as 64 pixels x
 * (r, g, b).  ids may be NULL to ask for the count only.  (What pt_tile_ids is for the compact buffer.) */
PT_API int pt_packed_tile_ids(uint32_t width, uint32_t height, uint32_t tile_rank, uint32_t tile_count, const uint32_t rect[4],
                              uint32_t* ids, uint32_t capacity, uint32_t* num_tiles);
/* Pack `num_frames` compact buffers of this rank (frame j at compact_device + j * frame_stride_floats, tile-major f32 RGBA as pt_render
 * leaves them) into packed_device + j * packed_frame_stride_floats.  Asynchronous on the context's stream, behind the frames' resolve. */
PT_API int pt_pack_shares(PtContext* ctx, const void* compact_device, uint64_t frame_stride_floats, uint32_t num_frames, uint32_t width, uint32_t height,
                          uint32_t tile_rank, uint32_t tile_count, const uint32_t rect[4], void* packed_device, uint64_t packed_frame_stride_floats);
/* Rank 0: rank r's packed share of frame j sits at gathered_device + r * rank_stride_floats + j * frame_stride_floats; frame j is rebuilt
 * at frames_out_device + j * out_stride_floats (row-major f32 RGBA; NULL: the context's own frame buffer, last frame only, as
 * pt_deinterleave_batch).  `spp` = samples per pixel of the frames (1 in the reference modes): the value outside the rectangle is the
 * mean of spp camera-miss samples, formed exactly as the resolve pass forms it. */
PT_API int pt_unpack_batch(PtContext* ctx, const void* gathered_device, uint64_t rank_stride_floats, uint64_t frame_stride_floats, uint32_t num_frames,
                           uint32_t width, uint32_t height, uint32_t tile_count, const uint32_t rect[4], uint32_t spp,
                           void* frames_out_device, uint64_t out_stride_floats);

/* ---- one image from all GPUs of the node: a group of contexts inside ONE process ------------------------------
 *
 * PathTracer.render() yields one image per call (src/main.js:54-76); a group keeps that call shape over N GPUs.  Member r renders
 * the 8x8 tiles with (tx + ty) % N == r into a compact buffer (pt_render with tile_rank / tile_count), RCCL gathers the compact
 * buffers on rank 0 over xGMI (ncclCommInitAll + one ncclGather per batch of frames, every sender on its own link to the root), rank 0
 * de-interleaves them into the row-major frame (pt_deinterleave).  The scene is replicated (each member builds it on its own GPU);
 * images are bit-identical for every N.  Accumulating frames (PtRenderParams.accumulate) keep their running sums on the members and
 * are gathered only when an image is asked for.  pt_group_last_error(NULL): last failure without a group. */
typedef struct PtGroup PtGroup;
enum {
    PT_GROUP_TRANSPORT_RCCL = 0,   /* ncclGather over xGMI; one distinct GPU per member */
    PT_GROUP_TRANSPORT_COPY = 1    /* diagnostics: hipMemcpyPeerAsync instead of the collective; members may share a GPU (what RCCL refuses),
                                      so the N > 1 logic can be exercised on a one-GPU machine */
};
/* device_ordinals = NULL: devices 0 .. num_devices-1; num_devices = 0: every visible device */
PT_API int  pt_group_create(const int* device_ordinals, uint32_t num_devices, uint32_t transport, PtGroup** out);
PT_API void pt_group_destroy(PtGroup* group);
PT_API const char* pt_group_last_error(const PtGroup* group);
PT_API int  pt_group_size(const PtGroup* group, uint32_t* num_members);
/* The member context of a rank (borrowed: valid until pt_group_destroy), e.g. rank 0 for pt_read_bvh2 / pt_scene_info. */
PT_API int  pt_group_context(PtGroup* group, uint32_t rank, PtContext** ctx);
/* scene, replicated on every member: pt_set_triangles / pt_build_bvh / pt_set_bvh2 / pt_set_bvh4 */
PT_API int  pt_group_set_triangles(PtGroup* group, const float* tris, uint32_t num_tris);
/* pt_update_triangles on every member (the same host array): every member ends up with the same refitted tree */
PT_API int  pt_group_update_triangles(PtGroup* group, const float* tris, uint32_t num_tris);
PT_API int  pt_group_build_bvh(PtGroup* group);
/* pt_build_bvh_accel on every member: the build is deterministic, every member holds the same tree */
PT_API int  pt_group_build_bvh_accel(PtGroup* group, uint32_t accel);
PT_API int  pt_group_set_bvh2(PtGroup* group, const uint32_t* bvh2, uint64_t words);
PT_API int  pt_group_set_bvh4(PtGroup* group, const uint32_t* bvh4, uint64_t words);
/* pt_set_batch for every member; the gather then moves one batch per collective.  A group delivers ONE image per batch: the batch's LAST frame
 * (pt_group_read_* return it; the frames before it are traced -- an accumulating sequence sums them -- but not rebuilt on rank 0).  The frames of a
 * batch may differ in camera: what travels is cut to the union of their traced tile rectangles (none at all when no frame can see the scene). */
PT_API int  pt_group_set_batch(PtGroup* group, uint32_t frames_per_launch);
/* One frame over all members (tile_rank / tile_count of `params` are ignored).  Asynchronous. */
PT_API int  pt_group_render(PtGroup* group, const PtRenderParams* params);
/* Launch, gather and de-interleave what is queued (a partial batch, an accumulating sequence).  Asynchronous. */
PT_API int  pt_group_flush(PtGroup* group);
PT_API int  pt_group_synchronize(PtGroup* group);
/* pt_read_radiance / pt_read_rgba8 / pt_read_tonemapped of the last gathered frame (rank 0).  Synchronise. */
PT_API int  pt_group_read_radiance(PtGroup* group, float* dst, uint64_t dst_floats);
PT_API int  pt_group_read_rgba8(PtGroup* group, uint8_t* dst, uint64_t dst_bytes);
PT_API int  pt_group_read_tonemapped(PtGroup* group, int from_rgba8, uint8_t* dst, uint64_t dst_bytes);

/* ---- diagnostics: NOT part of the drop-in surface -------------------------------------------------------------------------
 * Exported for this repository's own tests and tools (tests/test_gpu_parity.py, tools/ab/sweep.sh, tools/wave_timeline.py); a binding
 * for the reference has no use for them and they may change between builds of the library. */
/* Override one launch heuristic of this context ("GRIDDIV", "ROWS", "CHUNK", "XCD", "SHADE", "FILL", "SLOTS", "CULL",
 * "STATSBATCH", "QUAD", "FORK", "BOUNDED", "TIMELINE", "EXPOSE", "EXBUDGET"); value 0xFFFFFFFF restores the measured default.  Launches the open batch first.  The same knobs are read
 * from PT_TUNE_<NAME> once, when a context is created.  "TIMELINE" = 1: ordinary (non-STATS) megakernel launches run the TIMELINE variant of the kernel --
 * the production kernel plus wave-uniform bookkeeping in scalar registers, same registers / occupancy, no scratch -- and leave the record pt_debug_wave_times reads. */
PT_API int pt_debug_set_tune(PtContext* ctx, const char* name, uint32_t value);
/* The launch heuristics as a pure function of the launch's shape (no GPU, no context; the measured defaults): out[12] = workgroups, rows / columns of
 * the queue's batch transposition, logical items, items per claim, items per XCD range (0: one queue), shade / fill thresholds, paths at which a
 * wavefront goes on with one ray per quad, shadow-ray forking, frame slots in rotation, frame slots set up.  (tests/test_launch_plan.py) */
PT_API int pt_debug_launch_plan(uint32_t num_cus, uint32_t frames, uint32_t tile_count, uint32_t launches_in_flight, uint32_t traced_batches, uint32_t batch_size, uint32_t out[12]);
/* The same pure function under overridden knobs: names[i] (pt_debug_set_tune's names) set to values[i], i < n, every other knob at its default -- the plan a
 * context with those overrides would be given.  No GPU, no context, and the environment is not read.  (tests/test_queue_model.py) */
PT_API int pt_debug_launch_plan_tuned(uint32_t num_cus, uint32_t frames, uint32_t tile_count, uint32_t launches_in_flight, uint32_t traced_batches, uint32_t batch_size,
                                      const char* const* names, const uint32_t* values, uint32_t n, uint32_t out[12]);
/* Raw counter block (24 words) of the last PT_FLAG_STATS launch: PtStats order in [0..6], then the instrumented megakernel's own
 * diagnostics (stack pushes by depth, longest path / ray in traversal steps, re-seated wavefronts, ...). */
PT_API int pt_debug_counters(PtContext* ctx, unsigned long long* dst24);
/* Per-wavefront timeline of the last PT_FLAG_STATS or TIMELINE megakernel launch, 24 words per wavefront: [0] begin, [1] queue found dry, [2] end (100 MHz ticks),
 * [3] traversal steps, [4] shade passes, [5] refill passes, [6] steps / [8] traversing lanes / [15] shade passes when the queue ran dry, [7] traversing lanes summed
 * over the steps, [9] of them at a leaf, [16..18] tick / steps / lanes when the wavefront re-seated its paths one per quad (0: never), [20] the variant that wrote it
 * (1 COUNTERS, 2 TIMELINE); COUNTERS only: [10..13] cycle shares (shade, refill, step, step before queue-dry), [14] longest path that ended after queue-dry, [19].
 * *n_waves = wavefronts written (<= max_waves).  Read it after pt_synchronize.  Both kinds of launch trace every tile of the root box's rectangle
 * (their lane counts are compared with each other and with the oracle's): not the production launch, which also leaves out the tiles the tile cover
 * drops (pt_debug_traced_tiles). */
PT_API int pt_debug_wave_times(PtContext* ctx, unsigned long long* dst, uint32_t max_waves, uint32_t* n_waves);
/* Which 8x8 tiles a megakernel launch of this one frame would trace, without launching anything: the tiles of the params' tile share inside the
 * root box's screen rectangle (pt_traced_tile_rect) that the tile cover keeps -- the union of the screen rectangles of the live boxes of a
 * breadth-first cut of the tree.  Follows knob "CULL" (0: every tile, 1: the rectangle, 2 = default: the cover) and
 * PT_FLAG_STATS / knob "TIMELINE" (instrumented launches keep the rectangle). bitmask_out (optional, `words` >= ceil(tiles / 32) words): bit ty * tiles_x + tx
 * set for a traced tile.  *rect_tiles = owned tiles inside the rectangle, *traced_tiles = those of them that are traced.  This is the plan of a view
 * that stays: a small launch (fewer than 2^24 pixel-samples x (bounces + 1)) keeps the rectangle the first time it sees a set of cameras (or a refitted tree) and pays for their cover -- one small kernel and a
 * host wait -- when the view repeats; this call computes the cover at once and leaves it for the launches that follow.  The frames pt_set_batch holds
 * are not touched. */
PT_API int pt_debug_traced_tiles(PtContext* ctx, const PtRenderParams* params, uint32_t* bitmask_out, uint32_t words, uint32_t* rect_tiles, uint32_t* traced_tiles);
/* Exposed triangles: PT_MODE_PATH's light is directional and fixed, so a triangle on which no shadow ray can be occluded
 * is known from the scene alone; a megakernel launch adds the light term of a hit on such a triangle without tracing the ray.  The mask (one bit
 * per triangle, 2 * ceil(num_tris / 64) words) is computed on the device in front of the first launch of at least 2^24 ray segments that sees a tree
 * version -- after pt_update_triangles the second such launch.  Knob "EXPOSE": 0 every shadow ray is traced, 1 = default, 2 instrumented launches
 * skip as well and count what they skip; knob "EXBUDGET": the leaves a query may test before it gives up and leaves its triangle unflagged.
 * pt_debug_exposure: params != NULL computes the mask now, for the current tree and that camera's distance, and waits for it; NULL reports the mask
 * there is.  info_out[7] = {1 when the mask holds for the current tree version, flagged triangles, queries that gave up, triangles too ill-conditioned
 * as occluders to be left to the walk, shadow rays the last "EXPOSE" = 2 PT_FLAG_STATS launch did not trace, words of the mask, 1 when the last megakernel launch -- of any variant -- read the mask}; *kernel_ms = duration
 * of the two kernels; bounds_out[3] = {s_max, d_max of pt_exposure_flags_host, the camera distance} the mask holds for; mask_out (optional,
 * `words` >= info_out[5]). */
PT_API int pt_debug_exposure(PtContext* ctx, const PtRenderParams* params, uint32_t info_out[7], double bounds_out[3], float* kernel_ms, uint32_t* mask_out, uint32_t words);
/* The same flags on the CPU from the triangles alone (every pair tested, the arithmetic of the device route; no GPU, no context) for ray
 * origins within s_max of every scene point and hit coordinates up to d_max; mask: 2 * ceil(num_tris / 64) words. */
PT_API int pt_exposure_flags_host(const float* tris, uint32_t num_tris, double s_max, double d_max, uint32_t* mask_out, uint32_t words, uint32_t* flagged);
/* Two tiers.  The mask above is the first tier's: it covers hits at |n . d| >= 0.1002.  The device computes a second mask in the same pass,
 * for hits at |n . d| >= 0.3008 only: steeper hits need a third of the margin inside the triangle's plane, so the second tier flags a superset
 * of the first.  A launch skips the shadow ray of a hit whose triangle the second tier flags when the hit passes the gate of the best tier
 * that flags the triangle.  Knob "EXPOSE" + 4 (5, 6): launches use the first tier only (A/Bs, tests).
 * pt_debug_exposure_tier2 reports the second tier of the mask there is: info_out[2] = {flagged triangles, walks that ran out of their budget
 * after the first tier was settled as blocked}; mask_out (optional) as above.  pt_exposure_flags_host_gate: the CPU twin for any gate (the f64
 * bound on |n . d| / |d|: 0.0999 for the first tier, what pt_exposure_flags_host uses, and 0.2999 for the second). */
PT_API int pt_debug_exposure_tier2(PtContext* ctx, uint32_t info_out[2], uint32_t* mask_out, uint32_t words);
PT_API int pt_exposure_flags_host_gate(const float* tris, uint32_t num_tris, double s_max, double d_max, double gate, uint32_t* mask_out, uint32_t words, uint32_t* flagged);

#ifdef __cplusplus
}
#endif
#endif /* MI355PT_H */
