// pt_host.h -- host-side scene-build helpers of libmi355pt (no HIP calls in here).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "pt_bounds.h"

namespace pt {

// the layout constants and the packed leaf reference are pt_bounds.h's, which the kernels compile as well
using ptbd::kNode2Stride; using ptbd::kNode4Stride; using ptbd::kLeafFlag; using ptbd::kInvalid; using ptbd::kDegenerate;
using ptbd::kEmptyBox0; using ptbd::kEmptyBox1; using ptbd::kEmptyBox2;
using ptbd::packed_leaf_ref;

// ---- scene build -----------------------------------------------------------------
void morton_codes_sorted(const float* tris, uint32_t n, uint32_t* morton, uint32_t* tri_index);
// returns false on a malformed BVH2 (message in err)
bool collapse_to_bvh4(const uint32_t* bvh2, uint32_t num_tris, std::vector<uint32_t>& out, std::string& err);
// by_area = true: the area-guided collapse of PT_ACCEL_AREA_COLLAPSE / PT_ACCEL_PLOC -- expand the internal entry of
// largest surface area instead of the first one; reads the internal BVH2 bounds, so bvh2 must be a complete (refitted) BVH2
bool collapse_to_bvh4(const uint32_t* bvh2, uint32_t num_tris, bool by_area, std::vector<uint32_t>& out, std::string& err);
// PLOC BVH2 (PT_ACCEL_PLOC) in the reference's BVH2 layout: u32[1 + 6(2N-1)], root 0, leaves = the LBVH's leaf words,
// internal bounds = the reference's bottom-up refit on this topology.  The device build (pt_build.hip) gives the same words.
using ptbd::kPlocRadius;
bool build_bvh2_ploc(const float* tris, uint32_t n, std::vector<uint32_t>& out, std::string& err);
bool promote_to_bvh4_wide(const uint32_t* bvh2, uint64_t words, std::vector<uint32_t>& out, std::string& err);

// ---- device layouts ----------------------------------------------
// One 64-byte record per INTERNAL BVH4 node, child-major: four 16-byte pieces, piece k = child k's packed f16 box
// (3 words, reference packing, renderer.wgsl:94-99) + its reference.  A lane that fetches the whole record issues four
// dwordx4 loads (one ray per lane); the four lanes of a quad that share one ray fetch one piece each -- one 16-byte
// request per lane, the quad covers the 64-byte line (the drain's quad mode, pt_megakernel.hip).
struct WideNode {
    struct Child {
        uint32_t box[3];
        uint32_t ref;  // kInvalid = empty slot; kDegenerate = examined, never entered; else a packed reference (pt_bounds.h)
    } child[4];
};
static_assert(sizeof(WideNode) == 64, "WideNode must be 64 bytes");

// (child references are the packed references of pt_bounds.h)
struct WideBvh {
    std::vector<WideNode> nodes;
    uint32_t root_ref = kInvalid;      // same encoding as WideNode::ref; kInvalid = empty BVH
    uint32_t root_box[3] = {0, 0, 0};  // the root's own packed bounds
    bool     root_degenerate = false;  // any(mn > mx) on the root (renderer.wgsl:244)
    uint32_t num_nodes4 = 0;
};
// Validates the reference-layout BVH4 and builds the wide layout.  Rejects: short buffer,
// child reachable twice / cycles.  Children that the reference skips for every ray without
// fetching them (INVALID, index >= numNodes: renderer.wgsl:288) become empty slots; a child with a
// degenerate box (fetched, then rejected: renderer.wgsl:289-291) becomes a kDegenerate slot, which
// no ray enters but which counts as an examined record, exactly as in the reference.
bool build_wide_bvh(const uint32_t* bvh4, uint64_t words, uint32_t num_tris, uint32_t node_base16, WideBvh& out, std::string& err);

// ---- refit in place (pt_update_triangles; host twins of pt_refit.hip, the arithmetic of pt_bounds.h) ---------------------------
// New boxes for an unchanged topology.  BVH4: the nodes reachable from the root (the walk of build_wide_bvh; a node reachable
// twice is an error); a leaf whose triangle index is >= n, an internal node without a valid child and every unreachable node keep
// their words.  BVH2: every leaf, and every internal node both of whose children (two different nodes in range) are refitted.
bool refit_bvh4(const float* tris, uint32_t n, uint32_t* bvh4, uint64_t words, std::string& err);
bool refit_bvh2(const float* tris, uint32_t n, uint32_t* bvh2, uint64_t words, std::string& err);
// sum over the reachable internal nodes of halfArea(node box) / halfArea(root box), boxes decoded exactly, f64, in node order
bool bvh4_cost(const uint32_t* bvh4, uint64_t words, double& cost, std::string& err);
// What the device climb needs for an installed tree (pt_kernels.h::RefitBuffers): up[2M] = (parent, slot), self[2M] = (kind, wide
// index), child_ref[4 * internal] = the packed references of each wide record, by the wide indices build_wide_bvh assigns.
bool refit_plan4(const uint32_t* bvh4, uint64_t words, uint32_t num_tris, uint32_t node_base16,
                 std::vector<uint32_t>& up, std::vector<uint32_t>& self, std::vector<uint32_t>& child_ref, std::string& err);

// 64-byte triangle record (one cache line, like a wide node): v0, e1 = v1-v0, e2 = v2-v0, n = normalize(cross(e1,e2)) -- the same
// f32 operations renderer.wgsl:179-180,269 performs per visit, done once at upload.  Pieces 0..2 are axis-major: piece a (16 bytes)
// holds component a of the three vectors of the intersection test, (v0[a], e1[a], e2[a], 0) -- three lanes of a quad that fetch one
// piece each hold the triangle in structure-of-arrays form for the quad's Moller-Trumbore (pt_megakernel.hip); piece 3 is the
// normal (n, 0), which the shade pass fetches with ONE 16-byte request (as three components of three pieces it cost three, and the
// vector L1's request rate is what the dense traversal is closest to: +2..3 % frame time, profiles/r04_q2_ab.txt).
struct TriRecord { float axis[3][4]; float n[4]; };
static_assert(sizeof(TriRecord) == 64, "TriRecord must be 64 bytes");
void build_tri_records(const float* tris, uint32_t n, TriRecord* out);

// ---- exposed triangles (host twin of pt_expose.hip, the arithmetic of pt_expose.h) ---------------------------
// mask: 2 * ceil(num_tris / 64) words, bit t set when no shadow ray started on triangle t can be occluded, for ray origins within
// s_max of every scene point and hit coordinates up to d_max.  Every pair of triangles is tested: no tree, no budget -- the device's
// mask is this one without the queries that gave up.  gate: the smallest |n . d| / |d| of the hits covered (ptex::kGate for the first tier,
// ptex::kGate2 for the second).  Returns the number of flagged triangles.
uint32_t exposure_flags(const float* tris, uint32_t num_tris, double s_max, double d_max, double gate, uint32_t* mask);

// ---- closest-point queries (pt_closest_points; host twin of pt_pointquery.hip, bit for bit) --------------------------------------
// points: n x (x, y, z, r_max); out: n x (dist bits, prim, u bits, v bits).  bvh4 = nullptr: every triangle in index order; else the walk
// of the kernels over build_wide_bvh(bvh4) and build_tri_records(tris), with the arithmetic of pt_closest.h.  counters (optional):
// points, nodes examined, triangles tested, stack drops, max stack -- as the device's PT_CLOSEST_STATS counts them.
bool closest_points(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const float* points, uint64_t n,
                    uint32_t* out, uint64_t* counters, std::string& err);

// ---- radius queries (pt_radius_count, pt_radius_search; host twin of pt_radius.hip, bit for bit) -------------------------------------
// points: n x (x, y, z, r_max); offsets: n + 1 words, the exclusive prefix sums of the counts (offsets[n] = the total); entries: (dist bits,
// prim, u bits, v bits) per accepted leaf, the list of point i in visit order from offsets[i] on, written only below `capacity` (entries =
// nullptr with capacity 0: offsets only).  bvh4 = nullptr: every triangle in index order; else closest_points' walk with best2 held at
// r_max^2.  counters (optional): points, nodes examined, triangles tested, stack drops, max stack of the count walk -- as the device's
// PT_RADIUS_STATS counts them.
bool radius_search(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const float* points, uint64_t n,
                   uint64_t* offsets, uint32_t* entries, uint64_t capacity, uint64_t* counters, std::string& err);

// ---- box-overlap queries (pt_box_count, pt_box_search; host twin of pt_overlap.hip, word for word) -----------------------------------
// boxes: n x (lo.xyz, pad, hi.xyz, pad); offsets: n + 1 words, the exclusive prefix sums of the counts (offsets[n] = the total); entries:
// (prim, verts_inside, 0, 0) per accepted leaf, the list of box i in visit order from offsets[i] on, written only below `capacity` (entries =
// nullptr with capacity 0: offsets only).  bvh4 = nullptr: every triangle in index order; else closest_points' walk with every key equal
// (a child is entered iff pt_overlap.h::node_overlaps) and the triangle test of pt_overlap.h.  counters (optional): boxes, nodes examined,
// triangles tested, stack drops, max stack of the count walk -- as the device's PT_BOX_STATS counts them.
bool box_search(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const float* boxes, uint64_t n,
                uint64_t* offsets, uint32_t* entries, uint64_t capacity, uint64_t* counters, std::string& err);

// ---- triangle-overlap queries (pt_tri_count, pt_tri_search; host twin of pt_tritri.hip, word for word) -------------------------------
// in: n x (q0.xyz, pad, q1.xyz, pad, q2.xyz, pad); offsets and entries as box_search, an entry being (prim, edges, 0, 0).  bvh4 = nullptr:
// every triangle in index order; else box_search's walk on the caller triangle's exact bounding box, and the leaf test of pt_tritri.h.
// counters (optional): caller triangles, nodes examined, triangles tested, stack drops, max stack of the count walk -- as the device's
// PT_TRI_STATS counts them.
bool tri_search(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const float* in, uint64_t n,
                uint64_t* offsets, uint32_t* entries, uint64_t capacity, uint64_t* counters, std::string& err);

// ---- plane-cut queries (pt_cut_count, pt_cut_search; host twin of pt_cut.hip, word for word) -------------------------------------------
// in: n x (n.xyz, d, lo.xyz, pad, hi.xyz, pad); offsets and entries as box_search, an entry being (prim, code, t0 bits, t1 bits).
// bvh4 = nullptr: every triangle in index order; else box_search's walk on the window with the plane test of pt_cut.h::node_cut added to
// the node test, and the leaf test of pt_cut.h.  counters (optional): planes, nodes examined, triangles tested, stack drops, max stack of
// the count walk -- as the device's PT_CUT_STATS counts them.
bool cut_search(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const float* in, uint64_t n,
                uint64_t* offsets, uint32_t* entries, uint64_t capacity, uint64_t* counters, std::string& err);

// ---- sphere-cast queries (pt_sweep_spheres; host twin of pt_sweep.hip, bit for bit) ----------------------------------------------------
// sweeps: n x (org.xyz, t_max, dir.xyz, radius); out: n x (t bits, prim, u bits, v bits).  bvh4 = nullptr: every triangle in index order;
// else closest_points' walk with the key of a child = tmin of the slab test on its box grown by r + s (pt_sweep.h::node_pass) and `best`
// shrinking to each accepted t_T, with the arithmetic of pt_sweep.h.  counters (optional): sweeps, nodes examined, triangles tested,
// stack drops, max stack -- as the device's PT_SWEEP_STATS counts them.
bool sweep_spheres(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const float* sweeps, uint64_t n,
                   uint32_t* out, uint64_t* counters, std::string& err);

// ---- k-nearest queries (pt_nearest_k; host twin of pt_knn.hip, bit for bit) -----------------------------------------------------------
// points: n x (x, y, z, r_max); out: n * k records of four words (dist bits, prim, u bits, v bits), row i at out + i * k * 4: the at most k
// triangles nearest to point i within r_max in ascending order of distance, equal distances in visit order (index order without a tree),
// padded with (+inf bits, 0xFFFFFFFF, 0, 0).  1 <= k <= kNearestMaxK, else false.  bvh4 = nullptr: every triangle in index order; else
// closest_points' walk with best2 replaced by the k-th best d2 so far.  counters (optional): as closest_points.
constexpr uint32_t kNearestMaxK = 64;    // include/mi355pt.h: PT_NEAREST_MAX_K
bool nearest_k(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const float* points, uint64_t n, uint32_t k,
               uint32_t* out, uint64_t* counters, std::string& err);

// ---- crossing counts and containment (pt_count_hits, pt_contains; host twin of pt_crossings.hip, bit for bit) --------------------------
// rays: n x (org, t_max, dir, reserved); counts: n words.  bvh4 = nullptr: every triangle in index order; else the walk of the kernels over
// build_wide_bvh(bvh4) and build_tri_records(tris): a record is counted when tri_hit holds and t < best = min(t_max, 1e30), which never
// moves.  The ray arithmetic (ray_walked, safe_inv, tri_hit, hit_uv) is pt_raymath.h, the text the kernels compile.  counters (optional): rays, nodes examined, triangles tested, stack drops, max stack -- as the device's PT_COUNT_STATS counts them.
bool count_hits(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const float* rays, uint64_t n,
                uint32_t* counts, uint64_t* counters, std::string& err);
// points: n x (x, y, z, ignored); out: n x (inside, odd, samples, 0): occlusion_rays of {p, +inf, (0, 0, 1)} with bias 0 -> count_hits ->
// parity -> majority.  counters[0] = samples * the number of traced points.
bool contains(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const float* points, uint64_t n,
              uint32_t samples, uint32_t seed, uint32_t index_base, uint32_t* out, uint64_t* counters, std::string& err);

// ---- hit lists (pt_list_hits; host twin of pt_hitlist.hip, bit for bit) -----------------------------------------------------------------
// rays: as count_hits; offsets: n + 1 words, the exclusive prefix sums of count_hits' counts (offsets[n] = the total); entries: (t bits,
// prim, u bits, v bits) per crossing, the list of ray i in visit order (index order without a tree) from offsets[i] on, written only below
// `capacity` (entries = nullptr with capacity 0: offsets only).  sorted: every list with offsets[i + 1] <= capacity in ascending order of
// (t bits << 32 | prim).  counters (optional): as count_hits, over the count walk.
bool list_hits(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const float* rays, uint64_t n,
               uint64_t* offsets, uint32_t* entries, uint64_t capacity, bool sorted, uint64_t* counters, std::string& err);

// ---- procedural stand-in scenes ---------------------------------------------------
bool procedural_scene(uint32_t kind, uint32_t seed, uint32_t num_tris, float* out, std::string& err);

// ---- tiles ------------------------------------------------------------------------
constexpr uint32_t kTile = 8;   // 8x8-pixel tiles, one wavefront each
void tile_list(uint32_t width, uint32_t height, uint32_t rank, uint32_t count, std::vector<uint32_t>& tiles);
// tile_list(...).size() without building the list: per tile row, the rank's tiles are tx = first, first + count, ... with first = (rank - ty) mod count
uint32_t tile_count_of(uint32_t width, uint32_t height, uint32_t rank, uint32_t count);
// the rank's tiles inside the tile rectangle rect = {tx0, ty0, tx1, ty1} (half-open): what a packed share holds
uint32_t rect_tile_count_of(uint32_t rank, uint32_t count, const uint32_t rect[4]);

// ---- ambient-occlusion sample rays (host twin of pt_occlusion.hip::occlusion_rays_kernel; pt_occlusion_rays_host) ----
// surfels: 8 floats each (p, r_max, n, reserved); rays: n * samples records of 8 floats (org, t_max, dir, 0), item i * samples + s.
// The sampling functions are pt_raymath.h's, the text the kernels compile.
void occlusion_rays(const float* surfels, uint64_t n, uint32_t samples, uint32_t seed, uint32_t index_base, float bias, float* rays);

} // namespace pt
