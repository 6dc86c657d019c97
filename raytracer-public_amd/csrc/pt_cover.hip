// pt_cover.hip -- the tile cover of a launch: which 8x8 tiles of the frame a camera ray can reach the scene in at all.
//
// pt_api.cpp::root_box_rect leaves out the tiles outside the screen rectangle of the ROOT box.  For a closed mesh in front of the
// camera that rectangle is still about half empty: the corners of the rectangle, the space between limbs.
// The same projection applied to every box of a breadth-first CUT of the tree (a few thousand boxes) gives a much tighter,
// still conservative set: a ray that hits a triangle passes the box of every ancestor of that triangle, so it passes the box of
// the one cut entry above it, and its pixel lies inside that box's screen rectangle (widened by the same two pixels).
//
//   tile_cut_kernel    once per installed tree: the cut as (wide node, child slot) pairs -- places in the arena, not boxes
//   tile_cover_kernel  once per new (camera, resolution, tree version): reads the LIVE f16 child boxes at those places (so a refit
//                      in place needs no new cut), projects them, ORs the tiles they touch into a bitmask
#include "pt_kernels.h"
#include "pt_bounds.h"

namespace ptk {

namespace {

constexpr uint32_t kCutBlock = 1024;
constexpr uint32_t kCoverBlock = 64;
constexpr uint32_t kCutLeafBit = 0x80000000u;    // leaf references, empty slots (0xFFFFFFFF) and degenerate slots (0xFFFFFFFE) all carry it
constexpr uint32_t kCutEmpty = 0xFFFFFFFFu;

// the wide node behind an internal reference, or kCutEmpty when the reference does not point into the arena's nodes
__device__ __forceinline__ uint32_t cut_node_of(uint32_t ref, uint32_t node_base16, uint32_t num_wide) {
    if ((ref & kCutLeafBit) || ref < node_base16 || ((ref - node_base16) & 3u)) return kCutEmpty;
    const uint32_t idx = (ref - node_base16) >> 2;
    return idx < num_wide ? idx : kCutEmpty;
}

// One workgroup.  The frontier starts as the root's child slots and is expanded level by level: an entry whose child is a wide node
// is replaced by that node's non-empty slots; a leaf stays; a degenerate slot stays as well (no ray enters it, its inverted box
// covers no tile, but a refit may bring it back with the reference it had -- its triangles must stay below an entry).  Empty slots
// are never entries: no update fills them.  The walk stops at the last level that has at most kCutMax entries, so every triangle
// that the traversal can reach lies below exactly one entry.
__global__ __launch_bounds__(kCutBlock) void tile_cut_kernel(const uint4* __restrict__ wide, uint32_t num_wide, uint32_t node_base16, uint32_t root_index,
                                                             uint32_t* __restrict__ cut) {
    __shared__ uint32_t frontier[2][kCutMax];
    __shared__ uint32_t n_cur, n_next, expands;
    const uint32_t tid = threadIdx.x;
    if (tid == 0u) {
        uint32_t n = 0;
        if (root_index < num_wide)
            for (uint32_t s = 0; s < 4u; ++s) if (wide[(size_t)root_index * 4u + s].w != kCutEmpty) frontier[0][n++] = (root_index << 2) | s;
        n_cur = n; n_next = 0u; expands = 0u;
    }
    __syncthreads();
    uint32_t cur = 0u;
    for (uint32_t level = 0; level < 64u; ++level) {
        const uint32_t n = n_cur;
        uint32_t grows = 0u, internal = 0u;          // pass 1: the size of the next level
        for (uint32_t i = tid; i < n; i += kCutBlock) {
            const uint32_t e = frontier[cur][i];
            const uint32_t node = cut_node_of(wide[(size_t)(e >> 2) * 4u + (e & 3u)].w, node_base16, num_wide);
            if (node == kCutEmpty) { grows += 1u; continue; }
            internal = 1u;
            for (uint32_t s = 0; s < 4u; ++s) grows += wide[(size_t)node * 4u + s].w != kCutEmpty ? 1u : 0u;
        }
        if (grows) atomicAdd(&n_next, grows);
        if (internal) atomicOr(&expands, 1u);
        __syncthreads();
        const uint32_t total = n_next, any = expands;
        __syncthreads();
        if (total > kCutMax || any == 0u) break;     // uniform: the level at hand is the cut
        if (tid == 0u) { n_next = 0u; expands = 0u; }
        __syncthreads();
        for (uint32_t i = tid; i < n; i += kCutBlock) {      // pass 2: the next level (its order does not matter: the cover is a union)
            const uint32_t e = frontier[cur][i];
            const uint32_t node = cut_node_of(wide[(size_t)(e >> 2) * 4u + (e & 3u)].w, node_base16, num_wide);
            if (node == kCutEmpty) { frontier[cur ^ 1u][atomicAdd(&n_next, 1u)] = e; continue; }
            for (uint32_t s = 0; s < 4u; ++s)
                if (wide[(size_t)node * 4u + s].w != kCutEmpty) frontier[cur ^ 1u][atomicAdd(&n_next, 1u)] = (node << 2) | s;
        }
        __syncthreads();
        if (tid == 0u) { n_cur = n_next; n_next = 0u; expands = 0u; }     // n_next == total <= kCutMax: every store above was in range
        cur ^= 1u;
        __syncthreads();
    }
    const uint32_t n = n_cur;
    for (uint32_t i = tid; i < n; i += kCutBlock) cut[i] = frontier[cur][i];
    if (tid == 0u) cut[kCutMax] = n;
}

// One thread per (cut entry, camera = blockIdx.y).  The arithmetic is root_box_rect's (pt_api.cpp), in f64, on the entry's live box.
// Single-wavefront groups, like the resolve pass: the kernel runs next to persistent trace launches, and a group of one wavefront fits into
// any wave slot they leave (256-thread groups wait for four at once, profiles/r04_v3_resolve_block_ab.txt).
__global__ __launch_bounds__(kCoverBlock) void tile_cover_kernel(const uint4* __restrict__ wide, const uint32_t* __restrict__ cut, uint32_t count, const CoverCams cams,
                                                         uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t tiles_y, uint32_t* mask, uint32_t words) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t e = cut[i];
    const uint4 piece = wide[(size_t)(e >> 2) * 4u + (e & 3u)];
    if (piece.w == kCutEmpty || ptbd::box_degenerate(piece.x, piece.y, piece.z)) return;       // no ray enters it (the traversal's own rule)
    const CoverCam& c = cams.c[blockIdx.y];
    double mn[3], mx[3]; ptbd::unpack_box(piece.x, piece.y, piece.z, mn, mx);
    const double qx = c.quat[0], qy = c.quat[1], qz = c.quat[2], qw = c.quat[3];
    double x0 = 1e300, x1 = -1e300, y0 = 1e300, y1 = -1e300;
    bool ok = true;
    for (int k = 0; k < 8; ++k) {
        const double p[3] = {((k & 1) ? mx[0] : mn[0]) - c.cam[0], ((k & 2) ? mx[1] : mn[1]) - c.cam[1], ((k & 4) ? mx[2] : mn[2]) - c.cam[2]};
        const double ux = -qx, uy = -qy, uz = -qz;                       // v = conj(q) * p * q
        const double cx = uy * p[2] - uz * p[1], cy = uz * p[0] - ux * p[2], cz = ux * p[1] - uy * p[0];
        const double dx = uy * cz - uz * cy, dy = uz * cx - ux * cz, dz = ux * cy - uy * cx;
        const double vx = p[0] + 2.0 * (qw * cx + dx), vy = p[1] + 2.0 * (qw * cy + dy), vz = p[2] + 2.0 * (qw * cz + dz);
        if (!(vz < -1e-4)) ok = false;                                   // beside / behind the eye, or not a number
        const double sx = vx / -vz * c.focal / c.aspect, sy = vy / -vz * c.focal;
        const double fx = (sx + 1.0) * 0.5 * width, fy = (sy + 1.0) * 0.5 * height;
        if (!(fx > -1e300 && fx < 1e300 && fy > -1e300 && fy < 1e300)) ok = false;      // an infinite or NaN box has no screen rectangle
        x0 = fx < x0 ? fx : x0; x1 = fx > x1 ? fx : x1; y0 = fy < y0 ? fy : y0; y1 = fy > y1 ? fy : y1;
    }
    if (!ok) { atomicOr(&mask[words], 1u); return; }
    const double margin = 2.0;
    auto lo = [&](double v, uint32_t n) { v = (v - margin) / 8.0; return v <= 0.0 ? 0u : (v >= n ? n : uint32_t(v)); };
    auto hi = [&](double v, uint32_t n) { v = (v + margin) / 8.0 + 1.0; return v <= 0.0 ? 0u : (v >= n ? n : uint32_t(v)); };
    const uint32_t tx0 = lo(x0, tiles_x), tx1 = hi(x1, tiles_x), ty0 = lo(y0, tiles_y), ty1 = hi(y1, tiles_y);
    if (tx0 >= tx1) return;
    for (uint32_t ty = ty0; ty < ty1; ++ty) {
        const uint32_t a = ty * tiles_x + tx0, b = ty * tiles_x + tx1;      // bits [a, b), b <= tiles_x * tiles_y <= 32 * words
        for (uint32_t w = a >> 5; w <= ((b - 1u) >> 5); ++w) {
            const uint32_t first = w == (a >> 5) ? (a & 31u) : 0u, last = w == ((b - 1u) >> 5) ? ((b - 1u) & 31u) : 31u;
            const uint32_t bits = (0xFFFFFFFFu << first) & (0xFFFFFFFFu >> (31u - last));
            if ((__hip_atomic_load(&mask[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bits) != bits) atomicOr(&mask[w], bits);   // most entries find their tiles set
        }
    }
}

} // namespace

hipError_t launch_tile_cut(const uint4* wide, uint32_t num_wide, uint32_t node_base16, uint32_t root_index, uint32_t* cut, hipStream_t stream) {
    hipLaunchKernelGGL(tile_cut_kernel, dim3(1), dim3(kCutBlock), 0, stream, wide, num_wide, node_base16, root_index, cut);
    return hipGetLastError();
}

hipError_t launch_tile_cover(const uint4* wide, const uint32_t* cut, uint32_t count, const CoverCams& cams, uint32_t num_cams, uint32_t width, uint32_t height,
                             uint32_t* mask, uint32_t words, hipStream_t stream) {
    if (count == 0u || num_cams == 0u) return hipSuccess;
    if (count > kCutMax || num_cams > kCoverCams) return hipErrorInvalidValue;
    const uint32_t tiles_x = (width + 7u) / 8u, tiles_y = (height + 7u) / 8u;
    if ((uint64_t)tiles_x * tiles_y > (uint64_t)words * 32u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tile_cover_kernel, dim3((count + kCoverBlock - 1u) / kCoverBlock, num_cams), dim3(kCoverBlock), 0, stream, wide, cut, count, cams, width, height, tiles_x, tiles_y, mask, words);
    return hipGetLastError();
}

} // namespace ptk
