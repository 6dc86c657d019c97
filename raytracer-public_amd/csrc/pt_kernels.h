// pt_kernels.h -- kernel argument block and launchers shared by pt_kernels.hip and pt_api.cpp
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PT_KMODE_PACKET    0
#define PT_KMODE_REFERENCE 1
#define PT_KMODE_PATH      2

// megakernel tuning knobs (overridable with -D at build time)
#ifndef PT_SHORT_STACK
#define PT_SHORT_STACK 12          // LDS stack entries per lane (8 B each); deeper entries spill to global scratch
#endif
#ifndef PT_MEGA_WAVES_PER_SIMD
#define PT_MEGA_WAVES_PER_SIMD 6   // resident 256-thread blocks per CU = waves per SIMD
#endif
#ifndef PT_FRAME_SLOTS
#define PT_FRAME_SLOTS 3            // whole frames whose trace phases may be in flight at once (side streams); tile-sharded frames use 8
#endif
#ifndef PT_MEGA_BLOCK
#define PT_MEGA_BLOCK 64           // threads per workgroup of the persistent kernel: single-wave groups free their CU slot as soon as the wave drains
#endif
#ifndef PT_SHADE_THRESHOLD
#define PT_SHADE_THRESHOLD 16       // lanes waiting for a shade pass before one runs (or nothing traverses); 16 measured best in long launches, 8..16 equal for single frames (tools/ab/sweep.sh SHADE)
#endif
#ifndef PT_QUAD
#define PT_QUAD 1                  // 1: a wavefront with nothing left to start and at most PT_QUAD_LIVE paths goes on with one ray per quad of lanes (pt_megakernel.hip); 0: never; 2: quads from the first ray on (A/B builds)
#endif
#ifndef PT_FORK_LANES
#define PT_FORK_LANES 1            // 1: shadow rays are also handed to idle LANES once a wavefront has nothing left to start (fork_shadow >= 2); 0: only to idle quads in quad mode
#endif
#ifndef PT_FORK_SHADOW
#define PT_FORK_SHADOW 2          // quad mode: a path hands its shadow ray to an idle quad of its wavefront and goes on with the next bounce at once (pt_megakernel.hip)
#endif
#ifndef PT_QUAD_LIVE
#define PT_QUAD_LIVE 16            // paths a wavefront may hold when it re-seats them (16 quads per wavefront)
#endif
// batched ray queries (pt_rayquery.hip)
#ifndef PT_RQ_SHORT_STACK
#define PT_RQ_SHORT_STACK 12        // LDS stack entries per lane of trace_rays_kernel; deeper entries spill to the context's spill area
#endif
#ifndef PT_RQ_WAVES_PER_SIMD
#define PT_RQ_WAVES_PER_SIMD 6      // wavefronts of trace_rays_kernel per SIMD in the launch grid (what its registers and LDS allow)
#endif
#ifndef PT_RQ_FILL
#define PT_RQ_FILL 8                // idle lanes of a wavefront at which they take the next rays of its chunk
#endif
// batched closest-point queries (pt_pointquery.hip)
#ifndef PT_PQ_SHORT_STACK
#define PT_PQ_SHORT_STACK 12        // LDS stack entries per lane of closest_points_kernel; deeper entries spill to the context's spill area
#endif
#ifndef PT_PQ_WAVES_PER_SIMD
#define PT_PQ_WAVES_PER_SIMD 6      // wavefronts of closest_points_kernel per SIMD in the launch grid (what its registers and LDS allow)
#endif
#ifndef PT_PQ_FILL
#define PT_PQ_FILL 8                // idle lanes of a wavefront at which they take the next points of its chunk
#endif
// batched ambient-occlusion queries (pt_occlusion.hip)
#ifndef PT_OC_SHORT_STACK
#define PT_OC_SHORT_STACK 12        // LDS stack entries per lane of occlusion_kernel; deeper entries spill to the context's spill area
#endif
#ifndef PT_OC_WAVES_PER_SIMD
#define PT_OC_WAVES_PER_SIMD 6      // wavefronts of occlusion_kernel per SIMD in the launch grid (what its registers and LDS allow)
#endif
#ifndef PT_OC_FILL
#define PT_OC_FILL 8                // idle lanes of a wavefront at which they take the next items of its chunk
#endif
// crossing counts and containment (pt_crossings.hip): the ray queries' values taken over, not measured for these kernels
#ifndef PT_CR_SHORT_STACK
#define PT_CR_SHORT_STACK 12        // LDS stack entries per lane of count_hits_kernel / contains_kernel; deeper entries spill to the context's spill area
#endif
#ifndef PT_CR_WAVES_PER_SIMD
#define PT_CR_WAVES_PER_SIMD 6      // wavefronts of count_hits_kernel / contains_kernel per SIMD in the launch grid (what their registers and LDS allow)
#endif
#ifndef PT_CR_FILL
#define PT_CR_FILL 8                // idle lanes of a wavefront at which they take the next items of its chunk
#endif
// radius queries (pt_radius.hip): the point queries' values taken over, unmeasured for these kernels until tools/radius_bench.py has run
#ifndef PT_RD_SHORT_STACK
#define PT_RD_SHORT_STACK 12        // LDS stack entries per lane of radius_kernel<FILL>; deeper entries spill to the context's spill area
#endif
#ifndef PT_RD_WAVES_PER_SIMD
#define PT_RD_WAVES_PER_SIMD 6      // wavefronts of radius_kernel<FILL> per SIMD in the launch grid (what its registers and LDS allow)
#endif
#ifndef PT_RD_FILL
#define PT_RD_FILL 8                // idle lanes of a wavefront at which they take the next points of its chunk
#endif
// box-overlap queries (pt_overlap.hip): the radius queries' values taken over.  tools/box_bench.py ran with them (profiles/box_ab.json); no
// other value has been tried, so as choices they are unmeasured.  box_kernel<FILL> compiles to 78 / 79 VGPRs: 80 is the most that holds 6 waves per SIMD
#ifndef PT_BX_SHORT_STACK
#define PT_BX_SHORT_STACK 12        // LDS stack entries per lane of box_kernel<FILL>; deeper entries spill to the context's spill area
#endif
#ifndef PT_BX_WAVES_PER_SIMD
#define PT_BX_WAVES_PER_SIMD 6      // wavefronts of box_kernel<FILL> per SIMD in the launch grid (what its registers and LDS allow)
#endif
#ifndef PT_BX_FILL
#define PT_BX_FILL 8                // idle lanes of a wavefront at which they take the next boxes of its chunk
#endif
// triangle-overlap queries (pt_tritri.hip): the box queries' values taken over, UNMEASURED for these kernels -- no GPU run has compared
// them with any other value, nor the form of tri_kernel<FILL> that holds the caller's nine coordinates for the whole walk (kept: 66 / 69
// VGPRs, 7 waves per SIMD by registers) with the one that reads the record again at a leaf (68 / 81 VGPRs, 5 waves; DESIGN.md section
// 23).  The LDS stack is what holds the grid at 6 waves per SIMD: 7 x 4 x PT_TT_SHORT_STACK x 512 B is above a CU's 160 KiB
#ifndef PT_TT_SHORT_STACK
#define PT_TT_SHORT_STACK 12        // LDS stack entries per lane of tri_kernel<FILL>; deeper entries spill to the context's spill area
#endif
#ifndef PT_TT_WAVES_PER_SIMD
#define PT_TT_WAVES_PER_SIMD 6      // wavefronts of tri_kernel<FILL> per SIMD in the launch grid (what its registers and LDS allow)
#endif
#ifndef PT_TT_FILL
#define PT_TT_FILL 8                // idle lanes of a wavefront at which they take the next triangles of its chunk
#endif
// plane-cut queries (pt_cut.hip): the box queries' values taken over, UNMEASURED for these kernels -- no GPU run has compared them with
// any other value, nor the form of cut_kernel<FILL> that derives the corner selectors from the sign of n_k at each node (kept: 61 / 62
// VGPRs, 7 waves per SIMD by registers) with the one that holds the three selectors per lane (62 / 63 VGPRs, 7 waves; DESIGN.md section
// 24).  The LDS stack is what holds the grid at 6 waves per SIMD: 7 x 4 x PT_CT_SHORT_STACK x 512 B is above a CU's 160 KiB
#ifndef PT_CT_SHORT_STACK
#define PT_CT_SHORT_STACK 12        // LDS stack entries per lane of cut_kernel<FILL>; deeper entries spill to the context's spill area
#endif
#ifndef PT_CT_WAVES_PER_SIMD
#define PT_CT_WAVES_PER_SIMD 6      // wavefronts of cut_kernel<FILL> per SIMD in the launch grid (what its registers and LDS allow)
#endif
#ifndef PT_CT_FILL
#define PT_CT_FILL 8                // idle lanes of a wavefront at which they take the next planes of its chunk
#endif
// sphere-cast queries (pt_sweep.hip): the ray queries' values taken over.  tools/sweep_bench.py ran with them (profiles/sweep_ab.json); no
// other value has been tried, so as choices they are unmeasured
#ifndef PT_SW_SHORT_STACK
#define PT_SW_SHORT_STACK 12        // LDS stack entries per lane of sweep_kernel; deeper entries spill to the context's spill area
#endif
#ifndef PT_SW_WAVES_PER_SIMD
#define PT_SW_WAVES_PER_SIMD 6      // wavefronts of sweep_kernel per SIMD in the launch grid (what its registers and LDS allow)
#endif
#ifndef PT_SW_FILL
#define PT_SW_FILL 8                // idle lanes of a wavefront at which they take the next sweeps of its chunk
#endif
// hit lists (pt_hitlist.hip): the crossing counts' values taken over for the fill walk, unmeasured for it until tools/hitlist_bench.py has run
#ifndef PT_HL_SHORT_STACK
#define PT_HL_SHORT_STACK 12        // LDS stack entries per lane of hit_fill_kernel; deeper entries spill to the context's spill area
#endif
#ifndef PT_HL_WAVES_PER_SIMD
#define PT_HL_WAVES_PER_SIMD 6      // wavefronts of hit_fill_kernel per SIMD in the launch grid (what its registers and LDS allow)
#endif
#ifndef PT_HL_FILL
#define PT_HL_FILL 8                // idle lanes of a wavefront at which they take the next rays of its chunk
#endif
#ifndef PT_HL_LANE_MAX
#define PT_HL_LANE_MAX 16           // hit_sort_kernel: a list of at most this many entries is sorted by one lane, a longer one by its wavefront
#endif
#ifndef PT_HL_LDS_MAX
#define PT_HL_LDS_MAX 512           // hit_sort_kernel: a list of at most this many entries is sorted in LDS (16 bytes each), a longer one on global memory
#endif
// k-nearest queries (pt_knn.hip).  The short stack and the fill are the point queries' values taken over: tools/knn_bench.py ran with them
// (profiles/knn_ab.json), no other value has been tried, so as choices they are unmeasured.  The waves per SIMD follow from the LDS of a one-wavefront workgroup, 8 * 64 * (PT_NK_SHORT_STACK + KCAP)
// bytes: floor(floor(163,840 / LDS) / 4), capped at the point queries' 6 -- 8,192 B, 14,336 B and 38,912 B for the tiers 4, 16 and 64.
#ifndef PT_NK_SHORT_STACK
#define PT_NK_SHORT_STACK 12        // LDS stack entries per lane of nearest_k_kernel<KCAP>; deeper entries spill to the context's spill area
#endif
#ifndef PT_NK_FILL
#define PT_NK_FILL 8                // idle lanes of a wavefront at which they take the next points of its chunk
#endif
#ifndef PT_NK_WAVES_PER_SIMD_4
#define PT_NK_WAVES_PER_SIMD_4 5    // wavefronts of nearest_k_kernel<4> per SIMD in the launch grid (what its LDS allows)
#endif
#ifndef PT_NK_WAVES_PER_SIMD_16
#define PT_NK_WAVES_PER_SIMD_16 2   // the same of nearest_k_kernel<16>
#endif
#ifndef PT_NK_WAVES_PER_SIMD_64
#define PT_NK_WAVES_PER_SIMD_64 1   // the same of nearest_k_kernel<64>
#endif
#ifndef PT_FILL_THRESHOLD
#define PT_FILL_THRESHOLD 4        // hand out ready camera rays when this many lanes of a wavefront are without a path (a fetch from the ray buffer is cheap: 4 beats 8 by 2 %)
#endif

namespace ptk {

constexpr int kStackMax = 64;            // stack entries of a traversal, in every kernel (renderer.wgsl:8): a push beyond them is dropped
constexpr uint32_t kWaveTimeWords = 24;  // STATS diagnostics: 64-bit words per wavefront in RenderArgs::wave_times
#define PT_MAX_BATCH 256    // frames per persistent launch (their per-frame parameters live in a small device array)
// Per-frame part of the UBO for a batched launch (several consecutive frames traced by one persistent launch).
struct FrameParams {
    float cam[3]; float focal;
    float quat[4];
    float aspect; uint32_t frame; uint32_t seed;
    uint32_t accum_mode;        // bits 0..7: 0 no accumulation buffer, 1 restart the running sum, 2 add to it;
                                // bit 8: a later frame of the same launch has the same output target (this frame's result is not kept)
};
constexpr int kFrameChunk = 32; // frames per upload kernel (their parameters travel as that kernel's argument)
struct FrameChunk { FrameParams f[kFrameChunk]; float4* o[kFrameChunk]; };

// Passed by value as the kernel argument (lives in SGPRs / the kernarg segment).
struct RenderArgs {
    // device scene, MI355X layouts
    const uint4*  nodes;        // WideNode[]: 64 B per internal BVH4 node, read as 4 x dwordx4
    const float4* tris;         // TriRecord[]: 64 B per triangle (three axis-major pieces + the normal)
    const uint4*  scene;        // the arena both arrays live in: triangle record t at byte 64 t, wide node i at byte node_off + 64 i;
                                // child references are positions in it in 16-byte units (packed references, pt_host.h)
    uint32_t      node_off;
    uint32_t      rcp_short;    // 1: the operands of every reciprocal and square root of this launch are bounded (pt_api.cpp::arith_is_bounded): launch_trace picks the BOUNDED kernel variant (short forms, pt_device.h)
    uint32_t      tri_gate;     // the leaf reference of triangle numTris (0x80000000 | 4 * numTris) when the UBO's numTris is smaller than the uploaded triangle count (leaves from it on are entered, not tested), else 0xFFFFFFFF
    // device scene, reference layouts (literal packet kernel, LBVH build, readback)
    const uint32_t* bvh4_ref;   // u32[1 + 8*M]   renderer.wgsl:91-111
    const float*    tris9;      // f32[9*N]       renderer.wgsl:82-89
    // outputs
    float4*   out;              // radiance: row-major W*H, or compact tile-major (64 px per owned tile)
    float4*   accum;            // running per-pixel sums (xyz) + sample count (w); nullptr in reference modes
    uint32_t* tri_ids;          // optional: closest-hit triangle of the primary ray (reference modes)
    const float4* spheres;      // config C1 brute-force scenes: (x, y, z, r) per sphere
    uint32_t num_spheres, brute;
    const uint32_t* tiles;      // owned tile ids, nullptr = every tile in row-major order
    unsigned long long* stats;  // 7 counters (PtStats order)
    uint32_t num_tiles, tiles_x;
    // RendererUBO (renderer.wgsl:14-19)
    uint32_t width, height; float focal, aspect;
    float cam[3]; uint32_t num_tris;
    float quat[4];
    uint32_t frame;
    // wide-BVH root
    uint32_t root_ref; uint32_t root_box[3]; uint32_t root_degenerate;
    // extension
    uint32_t spp, max_bounces, seed, accumulate, compact;
    // persistent megakernel
    float4*   samples;          // per-sample radiance, item = (slot*spp + s)*64 + lane_in_tile; primed per batch by the trace (camera-ray generation), read by resolve_kernel
    uint32_t* queue;            // global item cursor
    uint2*    spill;            // deep stack entries: [entry][grid lane]
    uint4*    raybuf;           // per wavefront of the grid: 64 camera-ray records of 3 x uint4 (o, d, inv, key, sample index), generated 64 at a time
    unsigned long long* wave_times;   // STATS diagnostics: kWaveTimeWords words per wave (begin, queue-empty, end ticks @100 MHz, loop counts, ...)
    // Queue enumeration vs sample storage.  The queue hands out (frame, traced tile, sample) batches of 64 pixel-samples;
    // `trace_slots` lists the owned-tile slots that are traced at all (nullptr = every owned tile): tiles whose every camera ray
    // provably misses the root box are left out (pt_api.cpp: screen rectangle of the root box) and keep the primed miss value.
    // Samples are stored by (frame, owned-tile slot, sample), whatever subset is traced.  Behind the num_trace_tiles slots the array holds
    // the launch's tile cover, one bit per tile of the frame (tile ty * tiles_x + tx; pt_cover.hip): a tile inside trace_rect whose bit
    // is clear is not traced either (resolve_kernel reads the bit; the trace only sees the list).
    const uint32_t* trace_slots; uint32_t num_trace_tiles;
    uint32_t  trace_rect[4];                  // tiles [tx0, tx1) x [ty0, ty1) that are traced when trace_slots is set: the rest keeps the primed value (resolve_kernel writes it without reading)
    uint32_t  trace_bpf, trace_bpf_magic;     // traced batches per frame (num_trace_tiles * spp) and floor(2^32 / that)
    uint32_t  spp_magic, tiles_x_magic;       // floor(2^32 / spp), floor(2^32 / tiles_x): division by multiply + one correction
    uint32_t  num_sample_batches;             // (frame, owned tile, sample) batches in the sample buffer = num_frames * batches_per_frame
    uint32_t  total_items, chunk_items;   // logical items (64*64*perm_cols) and items per queue claim
    uint32_t  xcd_span;                   // 0: one queue; else items per XCD range (8 cursors at queue[8..15])
    uint32_t  num_batches, perm_cols;     // real (frame, traced tile, sample) batches of the queue; columns of the batch transpose
    uint32_t  perm_rows, perm_rows_magic; // its rows and floor(2^32 / rows) for the division
    uint32_t  shade_threshold, fill_threshold;
    uint32_t  fork_shadow;      // quad mode: shadow rays of paths that go on are traced by idle quads, next to the path's next ray (0: by the path itself, in turn)
    uint32_t  quad_live;        // re-seat the paths one per quad once the wavefront has nothing left to start and holds at most this many (0: never)
    // batched launch: frames[i] / outs[i] for i < num_frames; items of frame i are batches [i*batches_per_frame, ...)
    const FrameParams* frames; float4* const* outs;     // device arrays of the frame slot, filled by launch_frame_params
    uint32_t  num_frames, batches_per_frame;
    uint32_t  prime;            // 1: launch_trace must zero the control block itself
    uint32_t  ref_mode;         // 1: PT_MODE_REFERENCE on the megakernel -- one primary ray through each pixel centre, shade() of renderer.wgsl:348-353 (spp = 1, no bounces)
    // The megakernel's bounce limit (bits 0..15: min(max_bounces, 65535), the bounce count of a path being a 16-bit field) and, in bits 16..31, the
    // byte offset in the arena, in units of 64 KiB, of the exposure mask (pt_expose.hip, DESIGN.md section 6.2: one bit per triangle and tier, the tiers' words interleaved), or 0 -- every
    // shadow ray is traced (no mask yet, a camera or the scene beyond the bounds it was computed for, an instrumented launch).  One word, because the
    // shade pass reads both at the same place: a second launch constant there costs spilled scalar registers.
    uint32_t bounces_expose;
    uint32_t* expose_skipped;   // COUNTERS variant under knob EXPOSE = 2: the shadow rays not traced are counted here
};

hipError_t launch_render(const RenderArgs& args, int kmode, bool stats, hipStream_t stream);
// k0/k1 (optional): events recorded immediately around the trace_paths_kernel launches
hipError_t launch_trace(const RenderArgs& args, bool stats, uint32_t grid_blocks, hipStream_t stream, hipEvent_t k0, hipEvent_t k1);
hipError_t launch_prime(uint32_t* queue, hipStream_t stream);   // first use of a frame slot: its control block zeroed
// per-frame parameters and output targets of a launch into the slot's device arrays (asynchronous: the data travels as kernel arguments)
hipError_t launch_frame_params(const FrameParams* frames, float4* const* outs, uint32_t n, FrameParams* d_frames, float4** d_outs, hipStream_t stream);
hipError_t launch_resolve(const RenderArgs& args, hipStream_t stream);
uint32_t megakernel_grid(int num_cus);
uint32_t megakernel_block();
// refit = false leaves the internal BVH2 nodes without bounds (the BVH4 collapse does not read them); launch_lbvh2_refit adds them
hipError_t launch_lbvh2(uint32_t* bvh2, const float* tris9, const uint32_t* morton, const uint32_t* tri_index,
                        uint32_t* parent, uint32_t* flags, uint32_t num_tris, bool refit, hipStream_t stream);
hipError_t launch_lbvh2_refit(uint32_t* bvh2, const uint32_t* parent, uint32_t* flags, uint32_t num_tris, hipStream_t stream);
// leaf records and the refit walk in one launch, over any topology given by parent[] (parent[root] = 0xFFFFFFFF, flags[0..N-2] zero)
hipError_t launch_lbvh2_leaves(uint32_t* bvh2, const float* tris9, const uint32_t* tri_index, const uint32_t* parent, uint32_t* flags, uint32_t num_tris, hipStream_t stream);
// ---- device-side scene build (pt_build.hip) -------------------------------------------------
constexpr int kBuildCounters = 256;      // one append counter per BVH4 level (an LBVH2 over 30-bit codes + index bits is < 64 deep)
struct BuildBuffers {
    unsigned long long* bounds;          // [6] centroid bounds as order-preserving u64 keys
    uint32_t* counters;                  // [kBuildCounters]
    uint32_t *code_tmp, *index_tmp;      // [n] Morton codes / triangle ids before the sort
    uint32_t *morton, *tri_index;        // [n] after the sort: the inputs of launch_lbvh2
    void* temp; size_t temp_bytes;       // rocPRIM scratch (build_temp_bytes)
    uint32_t* node2; uint4* child_pos; uint32_t *subtree, *ids, *bnd;   // [2n-1] per BVH4 node in breadth-first order (bnd: 3 words each)
    uint32_t* host_word;                 // pinned host word for the per-level counts
};
size_t build_temp_bytes(uint32_t num_tris);
// edge_max (optional, zeroed by the caller): receives the largest |edge component| of the triangles as f32 bits
hipError_t launch_tri_records(const float* tris9, uint32_t num_tris, float4* records, uint32_t* edge_max, hipStream_t stream);
hipError_t launch_morton_sort(const BuildBuffers& B, const float* tris9, uint32_t num_tris, hipStream_t stream);
// synchronises the stream once per BVH4 level (the level sizes size the next launch); *num_nodes4 = M on return
// by_area: the area-guided collapse of PT_ACCEL_AREA_COLLAPSE / PT_ACCEL_PLOC (needs the internal BVH2 bounds)
hipError_t collapse_on_device(const BuildBuffers& B, const uint32_t* bvh2, uint32_t num_tris, uint32_t* bvh4, uint32_t* num_nodes4, bool by_area, hipStream_t stream);
// PLOC BVH2 (PT_ACCEL_PLOC) from B.tri_index (launch_morton_sort first): topology, parent[], leaf records and refit bounds.  `ploc` holds
// ploc_words(n) words, B.temp at least ploc_temp_bytes(n) bytes; synchronises once per iteration (*iterations on return).
// hipErrorInvalidValue: an iteration merged nothing
size_t ploc_words(uint32_t num_tris);
size_t ploc_temp_bytes(uint32_t num_tris);
hipError_t build_ploc_on_device(const BuildBuffers& B, uint32_t* ploc, const float* tris9, uint32_t num_tris, uint32_t* bvh2, uint32_t* parent, uint32_t* flags,
                                uint32_t* iterations, hipStream_t stream);
// B.subtree[i] = 1 for internal node id i, B.ids = its exclusive prefix sum (the wide-node index)
hipError_t launch_internal_scan(const BuildBuffers& B, const uint32_t* bvh4, uint32_t num_nodes4, hipStream_t stream);
hipError_t launch_wide_nodes(const BuildBuffers& B, const uint32_t* bvh4, uint32_t num_nodes4, uint4* wide, uint32_t num_tris, uint32_t node_base16, hipStream_t stream);
// gathered: rank r's share of frame j at gathered + r * rank_stride_px + j * frame_stride_px; frame j goes to full + j * full_stride_px
hipError_t launch_deinterleave(const float4* gathered, uint64_t rank_stride_px, uint64_t frame_stride_px, uint32_t frames, float4* full, uint64_t full_stride_px,
                               uint32_t width, uint32_t height, uint32_t count, hipStream_t stream);
// packed tile shares (pt_kernels.hip): rank's tiles inside the tile rectangle rect = {tx0, ty0, tx1, ty1}, 64 x 3 floats each
hipError_t launch_pack_shares(const float4* compact, uint64_t frame_stride_px, uint32_t frames, float* packed, uint64_t packed_stride_floats, uint32_t width,
                              uint32_t rank, uint32_t count, const uint32_t rect[4], hipStream_t stream);
hipError_t launch_unpack_frames(const float* gathered, uint64_t rank_stride_floats, uint64_t frame_stride_floats, uint32_t frames, float4* full, uint64_t full_stride_px,
                                uint32_t width, uint32_t height, uint32_t count, const uint32_t rect[4], uint32_t spp, hipStream_t stream);
// ---- the persistent walk of the batched queries (pt_walk.h) ----------------------------------
// What the three queries below share on the launch side: a queue block of kRqQueueWords 64-bit words (zeroed by each launch) and a spill
// area of 8-byte entries, both the context's, for a grid of one-wavefront workgroups.  The knobs differ per kernel (PT_RQ_*, PT_PQ_*, PT_OC_*).
constexpr uint32_t kRqQueueWords = 256;
inline uint32_t walk_grid(int num_cus, uint32_t waves_per_simd) { return (uint32_t)num_cus * 4u * waves_per_simd; }
inline size_t walk_spill_entries(uint32_t grid, int short_stack) { return (size_t)(kStackMax - short_stack) * grid * 64u; }
// ---- batched ray queries (pt_rayquery.hip) -------------------------------------------------
// rays: PtRay[n] (2 x float4 each), hits: PtHit[n] (uint4 each), both 16-byte aligned device memory.  simple or stats: one ray per thread
// (stats: PtStats counters into A.stats, zeroed by the caller); else the persistent kernel with `grid` wavefronts at most
// (walk_grid(.., PT_RQ_WAVES_PER_SIMD)), the queue block and walk_spill_entries(grid, PT_RQ_SHORT_STACK) spill entries.
hipError_t launch_trace_rays(const RenderArgs& A, const void* rays, void* hits, uint32_t n, bool anyhit, bool simple, bool stats,
                             unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream);
// A.width * A.height PtRay records of the PT_MODE_REFERENCE camera (A.focal, A.aspect, A.cam, A.quat), row-major
hipError_t launch_camera_rays(const RenderArgs& A, void* rays, hipStream_t stream);
// ---- batched closest-point queries (pt_pointquery.hip) ----------------------------------------
// points: PtPoint[n] (float4 each), out: PtClosest[n] (uint4 each), both 16-byte aligned device memory.  brute: every triangle in index
// order; simple or stats: one point per thread (stats: PtStats counters into A.stats, zeroed by the caller); else the persistent kernel
// with `grid` wavefronts at most (walk_grid(.., PT_PQ_WAVES_PER_SIMD)), the queue block and walk_spill_entries(grid, PT_PQ_SHORT_STACK)
// spill entries.
hipError_t launch_closest_points(const RenderArgs& A, const void* points, void* out, uint32_t n, bool simple, bool stats, bool brute,
                                 unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream);
// ---- sphere-cast queries (pt_sweep.hip) ------------------------------------------------------
// sweeps: PtSweep[n] (2 x float4 each), hits: PtHit[n] (uint4 each), both 16-byte aligned device memory.  brute, simple, stats, grid,
// queue and spill as launch_closest_points, with PT_SW_WAVES_PER_SIMD and PT_SW_SHORT_STACK.
hipError_t launch_sweep(const RenderArgs& A, const void* sweeps, void* hits, uint32_t n, bool simple, bool stats, bool brute,
                        unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream);
// ---- batched ambient-occlusion queries (pt_occlusion.hip) -------------------------------------
// surfels: PtSurfel[n] (2 x float4 each), out: PtOcclusion[n] (uint4 each), 16-byte aligned device memory; n * samples <= 2^32 - 1.  The launch
// zeroes `out`, counts the unoccluded samples of every traced surfel into word 1 of its record and completes the records in a finishing
// kernel.  simple or stats: one sample ray per thread (stats: PtStats counters into A.stats, zeroed by the caller); else the persistent
// kernel with `grid` wavefronts at most (walk_grid(.., PT_OC_WAVES_PER_SIMD)), the queue block and
// walk_spill_entries(grid, PT_OC_SHORT_STACK) spill entries.
hipError_t launch_occlusion(const RenderArgs& A, const void* surfels, void* out, uint32_t n, uint32_t samples, uint32_t seed, uint32_t index_base, float bias,
                            bool simple, bool stats, unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream);
// the n * samples sample rays as PtRay records (item i * samples + s); needs no scene
hipError_t launch_occlusion_rays(const void* surfels, void* rays, uint32_t n, uint32_t samples, uint32_t seed, uint32_t index_base, float bias, hipStream_t stream);
// PtRay[n] + PtHit[n] -> PtSurfel[n] (A.tris, A.num_tris)
hipError_t launch_hit_surfels(const RenderArgs& A, const void* rays, const void* hits, uint32_t n, float r_max, void* surfels, hipStream_t stream);
// ---- crossing counts, containment, signed distance (pt_crossings.hip) ---------------------------
// rays: PtRay[n] (2 x float4 each, 16-byte aligned), counts: uint32_t[n].  brute: every triangle in index order; simple or stats: one ray
// per thread (stats: PtStats counters into A.stats, zeroed by the caller); else the persistent kernel with `grid` wavefronts at most
// (walk_grid(.., PT_CR_WAVES_PER_SIMD)), the queue block and walk_spill_entries(grid, PT_CR_SHORT_STACK) spill entries.
hipError_t launch_count_hits(const RenderArgs& A, const void* rays, void* counts, uint32_t n, bool simple, bool stats, bool brute,
                             unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream);
// points: PtPoint[n] (float4 each), out: PtContainment[n] (uint4 each), 16-byte aligned; samples odd, n * samples <= 2^32 - 1.  The launch
// zeroes `out`, counts the odd sample rays of every traced point into word 1 of its record and completes the records in a finishing kernel.
hipError_t launch_contains(const RenderArgs& A, const void* points, void* out, uint32_t n, uint32_t samples, uint32_t seed, uint32_t index_base,
                           bool simple, bool stats, unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream);
// PtClosest[n] in `out` gets the sign bit of dist where PtContainment[n] in `contain` says inside
hipError_t launch_apply_sign(const void* contain, void* out, uint32_t n, hipStream_t stream);
// ---- radius queries (pt_radius.hip): every triangle within r_max of a point ----------------------------------------------------
// points: PtPoint[n] (float4 each, 16-byte aligned).  One walk per launch, the closest-point walk with best2 held at r_max^2:
//   offsets = nullptr: the count walk, counts[i] = the number of accepted leaves of point i (uint32_t[n]);
//   offsets != nullptr: the fill walk, entry k of point i (a PtClosest record, in visit order) at entries[offsets[i] + k] where that index
//   is below `capacity`; counts is not touched.
// brute: every triangle in index order; simple or stats: one point per thread (stats: PtStats counters into A.stats, zeroed by the
// caller); else the persistent kernel with `grid` wavefronts at most (walk_grid(.., PT_RD_WAVES_PER_SIMD)), the queue block and
// walk_spill_entries(grid, PT_RD_SHORT_STACK) spill entries.
hipError_t launch_radius(const RenderArgs& A, const void* points, uint32_t n, void* counts, const unsigned long long* offsets, void* entries,
                         unsigned long long capacity, bool simple, bool stats, bool brute,
                         unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream);
// offsets[0 .. n] = the exclusive prefix sums of counts[0 .. n) in 64 bits, offsets[n] = the total (hipcub::DeviceScan over n + 1 items,
// item n read as 0); temp: at least radius_scan_temp_bytes(n) bytes
size_t radius_scan_temp_bytes(uint32_t n);
hipError_t launch_radius_scan(const void* counts, uint32_t n, unsigned long long* offsets, void* temp, size_t temp_bytes, hipStream_t stream);
// ---- box-overlap queries (pt_overlap.hip): every triangle that overlaps an axis-aligned box ------------------------------------
// boxes: PtBox[n] (two float4 each, 16-byte aligned).  One walk per launch, launch_radius' two forms: offsets = nullptr counts the accepted
// leaves of box i into counts[i]; offsets != nullptr stores entry k of box i (a PtOverlap record, in visit order) at
// entries[offsets[i] + k] where that index is below `capacity`.  brute, simple, stats, grid, queue and spill as launch_radius, with
// PT_BX_WAVES_PER_SIMD and PT_BX_SHORT_STACK.  The scan between the two is launch_radius_scan.
hipError_t launch_box(const RenderArgs& A, const void* boxes, uint32_t n, void* counts, const unsigned long long* offsets, void* entries,
                      unsigned long long capacity, bool simple, bool stats, bool brute,
                      unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream);
// ---- triangle-overlap queries (pt_tritri.hip): every mesh triangle that a caller triangle cuts --------------------------------------
// tris_in: PtTri[n] (three float4 each, 16-byte aligned).  One walk per launch, launch_radius' two forms: offsets = nullptr counts the
// accepted leaves of triangle i into counts[i]; offsets != nullptr stores entry k of triangle i (a PtCross record, in visit order) at
// entries[offsets[i] + k] where that index is below `capacity`.  brute, simple, stats, grid, queue and spill as launch_radius, with
// PT_TT_WAVES_PER_SIMD and PT_TT_SHORT_STACK.  The scan between the two is launch_radius_scan.
hipError_t launch_tri(const RenderArgs& A, const void* tris_in, uint32_t n, void* counts, const unsigned long long* offsets, void* entries,
                      unsigned long long capacity, bool simple, bool stats, bool brute,
                      unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream);
// ---- plane-cut queries (pt_cut.hip): every mesh triangle that a plane cuts inside a window, and where ---------------------------------
// planes: PtCutPlane[n] (three float4 each, 16-byte aligned).  One walk per launch, launch_radius' two forms: offsets = nullptr counts the
// accepted leaves of plane i into counts[i]; offsets != nullptr stores entry k of plane i (a PtCut record, in visit order) at
// entries[offsets[i] + k] where that index is below `capacity`.  brute, simple, stats, grid, queue and spill as launch_radius, with
// PT_CT_WAVES_PER_SIMD and PT_CT_SHORT_STACK.  The scan between the two is launch_radius_scan.
hipError_t launch_cut(const RenderArgs& A, const void* planes, uint32_t n, void* counts, const unsigned long long* offsets, void* entries,
                      unsigned long long capacity, bool simple, bool stats, bool brute,
                      unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream);
// ---- hit lists (pt_hitlist.hip): every crossing along a ray, with t, triangle and u, v -------------------------------------------
// The fill walk behind launch_count_hits and launch_radius_scan: rays: PtRay[n]; entry k of ray i (a PtHit record, in visit order) goes to
// entries[offsets[i] + k] where that index is below `capacity`.  brute: every triangle in index order; simple: one ray per thread; else the
// persistent kernel with `grid` wavefronts at most (walk_grid(.., PT_HL_WAVES_PER_SIMD)), the queue block and
// walk_spill_entries(grid, PT_HL_SHORT_STACK) spill entries.
hipError_t launch_hit_fill(const RenderArgs& A, const void* rays, uint32_t n, const unsigned long long* offsets, void* entries, unsigned long long capacity,
                           bool simple, bool brute, unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream);
// every list with offsets[i + 1] <= capacity in place into ascending (t bits << 32 | prim)
hipError_t launch_hit_sort(const unsigned long long* offsets, void* entries, unsigned long long capacity, uint32_t n, hipStream_t stream);
// ---- k-nearest queries (pt_knn.hip): the k closest triangles to each point ----------------------------------------------------------
// points: PtPoint[n] (float4 each, 16-byte aligned); out: PtClosest[n * k] (uint4 each), row i at out[i * k], sorted by distance and padded
// with (+inf, 0xFFFFFFFF, 0, 0); 1 <= k <= kNearestMaxK.  One launch, the closest-point walk with best2 replaced by the k-th best squared
// distance so far.  brute: every triangle in index order; simple or stats: one point per thread (stats: PtStats counters into A.stats,
// zeroed by the caller); else the persistent kernel of the smallest capacity tier (4, 16, 64) that holds k, with `grid` wavefronts at most
// (walk_grid(.., nearest_k_waves_per_simd(k))), the queue block and walk_spill_entries(grid, PT_NK_SHORT_STACK) spill entries.
constexpr uint32_t kNearestMaxK = 64;    // include/mi355pt.h: PT_NEAREST_MAX_K
uint32_t nearest_k_waves_per_simd(uint32_t k);
hipError_t launch_nearest_k(const RenderArgs& A, const void* points, void* out, uint32_t n, uint32_t k, bool simple, bool stats, bool brute,
                            unsigned long long* queue, unsigned long long* spill, uint32_t grid, hipStream_t stream);
// ---- refit in place (pt_refit.hip): pt_update_triangles, pt_bvh_cost ------------------------------------------------------
// What the climb needs beyond the reference's BVH4, derived once per installed tree (on the device for a tree this library built,
// launch_refit_prepare4; on the host for an installed one, pt::refit_plan4 -- the same contents):
constexpr uint32_t kRefitLeaf = 0x80000000u, kRefitDead = 0xFFFFFFFFu;
struct RefitBuffers {
    uint2* up;              // [M] per BVH4 node: (parent id, slot in the parent); parent 0xFFFFFFFF for the root and for nodes that are not reachable
    uint2* self;            // [M] (kind, wide index): kind = number of valid children (0..4) of an internal node, kRefitLeaf, or kRefitDead (not reachable)
    uint4* child_ref;       // [internal nodes, by wide index] the packed references of the four slots (0xFFFFFFFF = empty): the part of a wide record no update changes
    uint32_t* arrive;       // [M] arrival counts, zero between updates (the thread that completes a count zeroes it)
};
// wide_index: launch_internal_scan's B.ids
hipError_t launch_refit_prepare4(const uint32_t* bvh4, uint32_t num_nodes4, const uint32_t* wide_index, uint32_t num_tris, uint32_t node_base16, const RefitBuffers& R, hipStream_t stream);
// leaf boxes from tris9 and internal boxes bottom-up in one launch, then the wide records from the refitted BVH4 in a second
hipError_t launch_refit4(const float* tris9, uint32_t num_tris, uint32_t* bvh4, uint32_t num_nodes4, const RefitBuffers& R, uint4* wide, hipStream_t stream);
// parent2[nn2] from the child words of the BVH2; then leaves and the reference's propagateUp over it (arrive[nn2] zero, left zero)
hipError_t launch_refit_prepare2(const uint32_t* bvh2, uint32_t nn2, uint32_t* parent2, hipStream_t stream);
hipError_t launch_refit2(const float* tris9, uint32_t num_tris, uint32_t* bvh2, uint32_t nn2, const uint32_t* parent2, uint32_t* arrive, hipStream_t stream);
// *out = sum over reachable internal nodes of halfArea(node) / halfArea(root) (f64)
hipError_t launch_bvh_cost(const uint32_t* bvh4, uint32_t num_nodes4, const uint2* self, double* out, hipStream_t stream);
// ---- tile cover (pt_cover.hip): which tiles of a frame a camera ray can reach the scene in at all ------------------------------
// The cut: a breadth-first frontier of the wide tree, at most kCutMax entries, each (wide node index << 2) | child slot -- the place
// of a child piece in the arena, not a copy of its box.  cut[kCutMax] receives the number of entries.
constexpr uint32_t kCutMax = 4096;
hipError_t launch_tile_cut(const uint4* wide, uint32_t num_wide, uint32_t node_base16, uint32_t root_index, uint32_t* cut, hipStream_t stream);
// The cover of up to kCoverCams cameras: the bits (tile ty * tiles_x + tx) of every tile that the screen rectangle of a cut entry's
// live box touches (projection and margin of pt_api.cpp::root_box_rect) are OR-ed into mask[0 .. words); mask[words] becomes nonzero
// when a box cannot be projected (a corner beside or behind the eye, a value that is not finite): the caller traces the rectangle then.
constexpr uint32_t kCoverCams = 16;
struct CoverCam { float cam[3]; float focal; float quat[4]; float aspect; };
struct CoverCams { CoverCam c[kCoverCams]; };
hipError_t launch_tile_cover(const uint4* wide, const uint32_t* cut, uint32_t count, const CoverCams& cams, uint32_t num_cams, uint32_t width, uint32_t height,
                             uint32_t* mask, uint32_t words, hipStream_t stream);
// ---- exposed triangles (pt_expose.hip): which triangles no shadow ray of the fixed light can be occluded on ------------------------
// info: kExposeInfoWords words, zeroed by the launch (flagged triangles, queries that ran out of their budget, listed ill-conditioned
// triangles, [a word the host fills in], the second tier's flagged triangles, walks that ran out of their budget with the first tier
// already blocked; the rest is spare); bad: kExposeBadMax words.
// mask: expose_mask_bytes(num_tris) bytes at a multiple of 64 KiB.  Two tiers (the gates of pt_expose.h: the second flags a superset of the
// first) of expose_mask_words(num_tris) words each, interleaved word by word -- first tier, second tier -- and every word written; behind
// them, expose_first_only_offset(num_tris) bytes (a multiple of 64 KiB) further on, the same layout with the first tier's words in both
// places, so that a launch is told "first tier only" by where RenderArgs::bounces_expose points and by nothing else.
// s_max, d_max: the operand bounds of ptex::Bounds (pt_expose.h) the flags hold for.
constexpr uint32_t kExposeInfoWords = 8, kExposeFlagged = 0, kExposeBudget = 1, kExposeBad = 2, kExposeSkipped = 3, kExposeFlagged2 = 4, kExposeBudget2 = 5, kExposeBadMax = 2048;
constexpr uint32_t kExposeNodeBudget = 2048, kExposeLeafBudget = 256;
uint32_t expose_mask_words(uint32_t num_tris);
uint64_t expose_first_only_offset(uint32_t num_tris);
uint64_t expose_mask_bytes(uint32_t num_tris);
hipError_t launch_expose(const uint4* scene, uint32_t node_base16, uint32_t num_wide, uint32_t root_ref, uint32_t num_tris, double s_max, double d_max,
                         uint32_t node_budget, uint32_t leaf_budget, uint32_t* info, uint32_t* bad, uint32_t* mask, hipStream_t stream);
hipError_t launch_rgba8(const float4* src, uint32_t* dst, uint32_t n, hipStream_t stream);
hipError_t launch_tonemap(const float4* src, uint32_t* dst, uint32_t width, uint32_t height, int from_rgba8, hipStream_t stream);

} // namespace ptk
