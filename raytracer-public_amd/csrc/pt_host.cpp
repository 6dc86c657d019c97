// pt_host.cpp -- host-side scene build of libmi355pt: the steps the reference runs in
// JavaScript on the CPU (Morton codes + sort, LBVH2 -> BVH4 collapse) or as an offline tool
// (BVH4_wide), plus the re-layout of the reference's buffers into the device formats the
// HIP kernels read.  Strict f32/f64 (-ffp-contract=off); no HIP calls.
#include "pt_host.h"
#include "pt_expose.h"
#include "pt_closest.h"
#include "pt_raymath.h"
#include "pt_overlap.h"
#include "pt_tritri.h"
#include "pt_cut.h"
#include "pt_sweep.h"

#include <cmath>
#include <cstring>
#include <algorithm>
#include <array>
#include <limits>
#include <thread>

namespace pt {

// The box and build arithmetic -- the f16 codecs, the min / max flavours, the packers, the areas, the Morton pieces -- is pt_bounds.h's,
// the text the kernels compile.
using ptbd::bits_of;
using ptbd::Box; using ptbd::unpack_box; using ptbd::box_degenerate;
using ptbd::js_min_f; using ptbd::js_max_f; using ptbd::sel_min; using ptbd::sel_max;

// ------------------------------------------------------------------------------------
// Morton codes + sort (PathTracer.js:411-481).  Doubles throughout, like the JS.
// Sort key is (code, triangle index); triangles start in index order, so a stable sort on
// the 30-bit code alone gives the same permutation -> 3-pass LSD radix sort.
// ------------------------------------------------------------------------------------

void morton_codes_sorted(const float* tris, uint32_t n, uint32_t* morton, uint32_t* tri_index) {
    if (n == 0) return;
    std::vector<double> cen(size_t(n) * 3);
    double lo[3] = {1e30, 1e30, 1e30}, hi[3] = {-1e30, -1e30, -1e30};
    for (uint32_t t = 0; t < n; ++t) {
        const float* p = tris + size_t(t) * 9;
        for (int k = 0; k < 3; ++k) {
            const double c = ptbd::centroid_axis(p, k);
            cen[size_t(t) * 3 + k] = c;
            if (c < lo[k]) lo[k] = c;
            if (c > hi[k]) hi[k] = c;
        }
    }
    double ext[3];
    for (int k = 0; k < 3; ++k) { const double d = hi[k] - lo[k]; ext[k] = d > 1e-20 ? d : 1e-20; }
    std::vector<uint32_t> code(n), idxA(n), idxB(n);
    for (uint32_t t = 0; t < n; ++t) {
        uint32_t q[3];
        for (int k = 0; k < 3; ++k) q[k] = ptbd::quantize1023((cen[size_t(t) * 3 + k] - lo[k]) / ext[k]);
        code[t] = (ptbd::spread10(q[0]) << 2) | (ptbd::spread10(q[1]) << 1) | ptbd::spread10(q[2]);
        idxA[t] = t;
    }
    uint32_t* src = idxA.data(); uint32_t* dst = idxB.data();
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass * 10;
        uint32_t hist[1025] = {0};
        for (uint32_t i = 0; i < n; ++i) hist[((code[src[i]] >> shift) & 0x3ffu) + 1]++;
        for (int b = 0; b < 1024; ++b) hist[b + 1] += hist[b];
        for (uint32_t i = 0; i < n; ++i) dst[hist[(code[src[i]] >> shift) & 0x3ffu]++] = src[i];
        std::swap(src, dst);
    }
    for (uint32_t i = 0; i < n; ++i) { tri_index[i] = src[i]; morton[i] = code[src[i]]; }
}

// ------------------------------------------------------------------------------------
// Greedy collapse LBVH2 -> BVH4 (PathTracer.js:506-667), iterative:
//   pass 1 numbers the BVH4 nodes in DFS pre-order (children in slot order) and records the
//          greedy child sets; pass 2 walks the indices backwards (children always have larger
//          pre-order indices than their parent) and unions the already-final child boxes.
// ------------------------------------------------------------------------------------
// the union of the valid children's boxes of BVH4 node `node` in slot order (m: children at or beyond m are skipped), js_min_f / js_max_f
// from (+inf, -inf); returns the number of children taken
static uint32_t union_children4(const uint32_t* bvh4, uint32_t node, uint32_t m, Box& u) {
    const uint32_t* r = bvh4 + 1 + size_t(node) * kNode4Stride;
    u = {{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}};
    uint32_t valid = 0;
    for (int s = 0; s < 4; ++s) {
        const uint32_t c = r[3 + s];
        if (c == kInvalid || c >= m) continue;
        ++valid;
        const Box b = unpack_box(bvh4 + 1 + size_t(c) * kNode4Stride);
        for (int k = 0; k < 3; ++k) { u.mn[k] = js_min_f(u.mn[k], b.mn[k]); u.mx[k] = js_max_f(u.mx[k], b.mx[k]); }
    }
    return valid;
}

bool collapse_to_bvh4(const uint32_t* bvh2, uint32_t num_tris, std::vector<uint32_t>& out, std::string& err) {
    return collapse_to_bvh4(bvh2, num_tris, false, out, err);
}

bool collapse_to_bvh4(const uint32_t* bvh2, uint32_t num_tris, bool by_area, std::vector<uint32_t>& out, std::string& err) {
    out.clear();
    if (num_tris == 0) { out.push_back(0u); return true; }
    const uint32_t nn2 = 2 * num_tris - 1;
    auto word = [&](uint32_t node, uint32_t k) { return bvh2[1 + size_t(node) * kNode2Stride + k]; };
    auto leaf = [&](uint32_t node) { return (word(node, 5) & kLeafFlag) != 0u; };
    out.reserve(1 + size_t(nn2) * kNode4Stride);
    out.push_back(0u);
    struct Todo { uint32_t node2; uint32_t parent4; uint32_t slot; };
    std::vector<Todo> todo;
    todo.push_back({0u, kInvalid, 0u});
    uint32_t count4 = 0;
    while (!todo.empty()) {
        const Todo cur = todo.back(); todo.pop_back();
        if (cur.node2 >= nn2) { err = "BVH2 child index out of range"; return false; }
        if (count4 >= nn2) { err = "BVH2 is not a tree (more BVH4 nodes than BVH2 nodes)"; return false; }
        const uint32_t id = count4++;
        const size_t base = out.size();
        out.resize(base + kNode4Stride, 0u);
        if (cur.parent4 != kInvalid) out[1 + size_t(cur.parent4) * kNode4Stride + 3 + cur.slot] = id;
        if (leaf(cur.node2)) {
            out[base + 0] = word(cur.node2, 0); out[base + 1] = word(cur.node2, 1); out[base + 2] = word(cur.node2, 2);
            out[base + 3] = out[base + 4] = out[base + 5] = out[base + 6] = kInvalid;
            out[base + 7] = word(cur.node2, 5);
            continue;
        }
        // greedy: repeatedly replace the first internal entry (by_area: the first internal entry of largest area; strict >, so ties
        // and NaN keep the earlier slot) by its two children until 4 entries
        uint32_t kid[4]; uint32_t nk = 2;
        kid[0] = word(cur.node2, 3); kid[1] = word(cur.node2, 4);
        for (;;) {
            if (nk >= 4) break;
            uint32_t pos = nk;
            float best = 0.0f;
            for (uint32_t i = 0; i < nk; ++i) {
                if (kid[i] >= nn2) { err = "BVH2 child index out of range"; return false; }
                if (leaf(kid[i])) continue;
                if (!by_area) { pos = i; break; }
                const float a = ptbd::node_area2(word(kid[i], 0), word(kid[i], 1), word(kid[i], 2));
                if (pos == nk || a > best) { pos = i; best = a; }
            }
            if (pos == nk) break;
            const uint32_t k = kid[pos];
            for (uint32_t m = nk; m > pos + 1; --m) kid[m] = kid[m - 1];
            kid[pos] = word(k, 3); kid[pos + 1] = word(k, 4);
            ++nk;
        }
        out[base + 3] = out[base + 4] = out[base + 5] = out[base + 6] = kInvalid;
        out[base + 7] = 0u;
        for (uint32_t i = nk; i-- > 0;) todo.push_back({kid[i], id, i});   // slot 0 is numbered first
    }
    out[0] = count4;
    for (uint32_t id = count4; id-- > 0;) {
        const size_t base = 1 + size_t(id) * kNode4Stride;
        if (out[base + 7] & kLeafFlag) continue;
        Box u;
        union_children4(out.data(), id, kInvalid, u);
        ptbd::pack_trunc(u, &out[base]);
    }
    return true;
}

// ------------------------------------------------------------------------------------
// PLOC BVH2 (Meister & Bittner, "Parallel Locally-Ordered Clustering for BVH Construction", TVCG 2018), host twin of
// pt_build.hip's device build.  Clusters start as the Morton-sorted leaves with an f32 box (per-axis min / max of the three
// vertices); each iteration every cluster i picks the j in [i-R, i+R] minimising (area(box_i u box_j), min(i,j), max(i,j)),
// mutual pairs merge into a new internal node (ids counting down from N-2 in creation order: iteration, then position), and
// the survivors are compacted in order.  Then the LBVH's leaf words and the reference's refit (BVHBuilder.wgsl:242-306).
// ------------------------------------------------------------------------------------
namespace {
inline Box box_union(const Box& a, const Box& b) {                    // a = the cluster at the lower position
    Box u;
    for (int k = 0; k < 3; ++k) { u.mn[k] = sel_min(a.mn[k], b.mn[k]); u.mx[k] = sel_max(a.mx[k], b.mx[k]); }
    return u;
}
inline float union_area(const Box& a, const Box& b) {                 // PLOC's key
    return ptbd::ploc_area(ptbd::union_extent(a.mx[0], b.mx[0], a.mn[0], b.mn[0]), ptbd::union_extent(a.mx[1], b.mx[1], a.mn[1], b.mn[1]),
                           ptbd::union_extent(a.mx[2], b.mx[2], a.mn[2], b.mn[2]));
}
// the box of BVH2 nodes l and r united by `lo` / `hi` (js_min_f / js_max_f, or wmin / wmax), stepped outwards into node p
template <class Min, class Max>
inline void union_bounds2(uint32_t* p, const uint32_t* l, const uint32_t* r, Min lo, Max hi) {
    const Box a = unpack_box(l), b = unpack_box(r);
    Box u;
    for (int k = 0; k < 3; ++k) { u.mn[k] = lo(a.mn[k], b.mn[k]); u.mx[k] = hi(a.mx[k], b.mx[k]); }
    ptbd::store_bounds2(u, p);
}
} // namespace

bool build_bvh2_ploc(const float* tris, uint32_t n, std::vector<uint32_t>& out, std::string& err) {
    out.clear();
    if (n == 0) { out.push_back(0u); return true; }
    const uint32_t nn2 = 2 * n - 1, internal = n - 1;
    out.assign(1 + size_t(nn2) * kNode2Stride, 0u);
    out[0] = nn2;
    std::vector<uint32_t> morton(n), tri_index(n);
    morton_codes_sorted(tris, n, morton.data(), tri_index.data());
    std::vector<Box> box(n), box2(n);
    std::vector<uint32_t> node(n), node2(n), nn(n);
    for (uint32_t k = 0; k < n; ++k) {
        const float* t = tris + size_t(tri_index[k]) * 9;
        for (int a = 0; a < 3; ++a) {
            box[k].mn[a] = sel_min(sel_min(t[a], t[3 + a]), t[6 + a]);
            box[k].mx[a] = sel_max(sel_max(t[a], t[3 + a]), t[6 + a]);
        }
        node[k] = internal + k;
    }
    uint32_t count = n, created = 0;
    for (uint32_t iter = 0; count > 1; ++iter) {
        if (iter >= n) { err = "PLOC did not converge"; return false; }
        for (uint32_t i = 0; i < count; ++i) {
            const uint32_t lo = i >= kPlocRadius ? i - kPlocRadius : 0u, hi = std::min(count - 1, i + kPlocRadius);
            float bd = 0.0f; uint32_t bj = kInvalid, blo = 0, bhi = 0;
            for (uint32_t j = lo; j <= hi; ++j) {
                if (j == i) continue;
                const uint32_t a = std::min(i, j), b = std::max(i, j);
                const float d = union_area(box[a], box[b]);
                if (bj == kInvalid || d < bd || (d == bd && (a < blo || (a == blo && b < bhi)))) { bd = d; bj = j; blo = a; bhi = b; }
            }
            nn[i] = bj;
        }
        uint32_t kept = 0, merged = 0;
        for (uint32_t i = 0; i < count; ++i) {
            const uint32_t j = nn[i];
            const bool mutual = nn[j] == i;
            if (mutual && j < i) continue;                            // absorbed by cluster j
            if (mutual) {
                const uint32_t id = internal - 1u - (created + merged++);
                uint32_t* p = out.data() + 1 + size_t(id) * kNode2Stride;
                p[3] = node[i]; p[4] = node[j]; p[5] = 0u;
                box2[kept] = box_union(box[i], box[j]);
                node2[kept++] = id;
            } else {
                box2[kept] = box[i];
                node2[kept++] = node[i];
            }
        }
        if (merged == 0) { err = "PLOC iteration merged no pair"; return false; }
        created += merged;
        count = kept;
        std::swap(box, box2); std::swap(node, node2);
    }
    // leaves: writeLeaf2 (BVHBuilder.wgsl:124-132, 278-306), the LBVH's leaf words; min / max here are js_min_f / js_max_f over
    // (a, b), c (pt_bounds.h names the pair: lbvh2_leaves_kernel uses wmin / wmax over a, (b, c), equal except on NaN vertices)
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t ti = tri_index[k];
        const float* t = tris + size_t(ti) * 9;
        Box b;
        for (int a = 0; a < 3; ++a) { b.mn[a] = js_min_f(js_min_f(t[a], t[3 + a]), t[6 + a]); b.mx[a] = js_max_f(js_max_f(t[a], t[3 + a]), t[6 + a]); }
        uint32_t* p = out.data() + 1 + size_t(internal + k) * kNode2Stride;
        ptbd::store_bounds2(b, p);
        p[3] = 0u; p[4] = 0u; p[5] = kLeafFlag | (ti & 0x7fffffffu);
    }
    // refit (propagateUp, BVHBuilder.wgsl:242-275): children have larger ids than their parent, so descending ids see final children
    for (uint32_t id = internal; id-- > 0;) {
        uint32_t* p = out.data() + 1 + size_t(id) * kNode2Stride;
        union_bounds2(p, out.data() + 1 + size_t(p[3]) * kNode2Stride, out.data() + 1 + size_t(p[4]) * kNode2Stride, js_min_f, js_max_f);
    }
    return true;
}

// ------------------------------------------------------------------------------------
// BVH4_wide (tests/test.cpp:106-196): each internal node adopts its grandchildren (or the
// child itself when that child is a leaf); node indices and bounds are those of the BVH2.
// ------------------------------------------------------------------------------------
bool promote_to_bvh4_wide(const uint32_t* bvh2, uint64_t words, std::vector<uint32_t>& out, std::string& err) {
    if (words < 1) { err = "empty BVH2 buffer"; return false; }
    const uint32_t nn2 = bvh2[0];
    if (words < 1 + uint64_t(nn2) * kNode2Stride) { err = "BVH2 buffer shorter than its node count"; return false; }
    out.assign(1 + size_t(nn2) * kNode4Stride, 0u);
    out[0] = nn2;
    for (uint32_t n = 0; n < nn2; ++n) {
        const uint32_t* s = bvh2 + 1 + size_t(n) * kNode2Stride;
        uint32_t* d = out.data() + 1 + size_t(n) * kNode4Stride;
        d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
        if (s[5] & kLeafFlag) { d[3] = d[4] = d[5] = d[6] = kInvalid; d[7] = s[5]; continue; }
        uint32_t got = 0;
        for (int side = 0; side < 2; ++side) {
            const uint32_t c = s[3 + side];
            if (c == kInvalid) continue;
            const bool cleaf = (c >= nn2) || (bvh2[1 + size_t(c) * kNode2Stride + 5] & kLeafFlag);
            if (cleaf) { if (got < 4) d[3 + got++] = c; }
            else {
                const uint32_t* cs = bvh2 + 1 + size_t(c) * kNode2Stride;
                if (got < 4) d[3 + got++] = cs[3];
                if (got < 4) d[3 + got++] = cs[4];
            }
        }
        while (got < 4) d[3 + got++] = kInvalid;
        d[7] = 0u;
    }
    return true;
}

// ------------------------------------------------------------------------------------
// Device layouts
// ------------------------------------------------------------------------------------
bool build_wide_bvh(const uint32_t* bvh4, uint64_t words, uint32_t num_tris, uint32_t node_base16, WideBvh& out, std::string& err) {
    out = WideBvh();
    if (words < 1) { err = "empty BVH buffer"; return false; }
    const uint32_t m = bvh4[0];
    out.num_nodes4 = m;
    if (m == 0) return true;
    if (words < 1 + uint64_t(m) * kNode4Stride) { err = "BVH buffer shorter than its node count"; return false; }
    auto rec = [&](uint32_t i) { return bvh4 + 1 + size_t(i) * kNode4Stride; };
    // Reachability walk from the root; assigns wide indices to reachable internal nodes in
    // DFS pre-order so that a parent's first child record follows it in memory.
    std::vector<uint32_t> wide_index(m, kInvalid);
    std::vector<uint8_t> seen(m, 0);
    std::vector<uint32_t> stack;
    std::vector<uint32_t> order;   // reachable internal nodes in pre-order
    stack.push_back(0u); seen[0] = 1;
    while (!stack.empty()) {
        const uint32_t i = stack.back(); stack.pop_back();
        const uint32_t* r = rec(i);
        if (r[7] & kLeafFlag) continue;
        wide_index[i] = uint32_t(order.size());
        order.push_back(i);
        for (int s = 3; s >= 0; --s) {
            const uint32_t c = r[3 + s];
            if (c == kInvalid || c >= m) continue;          // skipped by every ray (renderer.wgsl:288)
            if (seen[c]) { err = "BVH node reachable twice (not a tree)"; return false; }
            seen[c] = 1;
            stack.push_back(c);
        }
    }
    const uint32_t* r0 = rec(0);
    out.root_box[0] = r0[0]; out.root_box[1] = r0[1]; out.root_box[2] = r0[2];
    out.root_degenerate = box_degenerate(r0[0], r0[1], r0[2]);
    out.root_ref = (r0[7] & kLeafFlag) ? packed_leaf_ref(r0[7] & 0x7fffffffu, num_tris) : node_base16;
    out.nodes.resize(order.size());
    for (size_t w = 0; w < order.size(); ++w) {
        const uint32_t* r = rec(order[w]);
        WideNode& wn = out.nodes[w];
        for (int s = 0; s < 4; ++s) {
            const uint32_t c = r[3 + s];
            WideNode::Child& ch = wn.child[s];
            ch.box[0] = kEmptyBox0; ch.box[1] = kEmptyBox1; ch.box[2] = kEmptyBox2;   // the inverted box (+inf, -inf) no ray enters
            ch.ref = kInvalid;
            if (c == kInvalid || c >= m) continue;
            const uint32_t* cr = rec(c);
            if (box_degenerate(cr[0], cr[1], cr[2])) { ch.ref = kDegenerate; continue; }   // renderer.wgsl:291: fetched, then skipped
            ch.box[0] = cr[0]; ch.box[1] = cr[1]; ch.box[2] = cr[2];
            ch.ref = (cr[7] & kLeafFlag) ? packed_leaf_ref(cr[7] & 0x7fffffffu, num_tris) : node_base16 + 4u * wide_index[c];
        }
    }
    return true;
}

// ------------------------------------------------------------------------------------
// Refit in place (host twins of pt_refit.hip)
// ------------------------------------------------------------------------------------
namespace {
using ptbd::wmin; using ptbd::wmax;     // the device's v_min_f32 / v_max_f32, spelt out for the host
// reachable nodes of a reference-layout BVH4 in pre-order (build_wide_bvh's walk)
bool reachable4(const uint32_t* bvh4, uint64_t words, std::vector<uint32_t>& order, std::string& err) {
    order.clear();
    if (words < 1) { err = "empty BVH buffer"; return false; }
    const uint32_t m = bvh4[0];
    if (m == 0) return true;
    if (words < 1 + uint64_t(m) * kNode4Stride) { err = "BVH buffer shorter than its node count"; return false; }
    std::vector<uint8_t> seen(m, 0);
    std::vector<uint32_t> stack;
    stack.push_back(0u); seen[0] = 1;
    while (!stack.empty()) {
        const uint32_t i = stack.back(); stack.pop_back();
        order.push_back(i);
        const uint32_t* r = bvh4 + 1 + size_t(i) * kNode4Stride;
        if (r[7] & kLeafFlag) continue;
        for (int s = 3; s >= 0; --s) {
            const uint32_t c = r[3 + s];
            if (c == kInvalid || c >= m) continue;
            if (seen[c]) { err = "BVH node reachable twice (not a tree)"; return false; }
            seen[c] = 1;
            stack.push_back(c);
        }
    }
    return true;
}
} // namespace

bool refit_bvh4(const float* tris, uint32_t n, uint32_t* bvh4, uint64_t words, std::string& err) {
    std::vector<uint32_t> order;
    if (!reachable4(bvh4, words, order, err)) return false;
    const uint32_t m = order.empty() ? 0u : bvh4[0];
    for (size_t k = order.size(); k-- > 0;) {                       // children come after their parent in pre-order
        uint32_t* r = bvh4 + 1 + size_t(order[k]) * kNode4Stride;
        if (r[7] & kLeafFlag) {
            const uint32_t t = r[7] & 0x7fffffffu;
            if (t < n) ptbd::leaf_box_words(tris + size_t(t) * 9, r);
            continue;
        }
        Box u;
        if (union_children4(bvh4, order[k], m, u)) ptbd::pack_trunc(u, r);
    }
    return true;
}

bool refit_bvh2(const float* tris, uint32_t n, uint32_t* bvh2, uint64_t words, std::string& err) {
    if (words < 1) { err = "empty BVH2 buffer"; return false; }
    const uint32_t nn2 = bvh2[0];
    if (words < 1 + uint64_t(nn2) * kNode2Stride) { err = "BVH2 buffer shorter than its node count"; return false; }
    std::vector<uint32_t> parent(nn2, kInvalid), arrive(nn2, 0u);
    auto rec = [&](uint32_t i) { return bvh2 + 1 + size_t(i) * kNode2Stride; };
    for (uint32_t i = 0; i < nn2; ++i) {
        const uint32_t* p = rec(i);
        if (p[5] & kLeafFlag) continue;
        const uint32_t l = p[3], r = p[4];
        if (l >= nn2 || r >= nn2 || l == r) continue;
        parent[l] = i; parent[r] = i;
    }
    for (uint32_t i = 0; i < nn2; ++i) {
        uint32_t* p = rec(i);
        if (!(p[5] & kLeafFlag)) continue;
        const uint32_t t = p[5] & 0x7fffffffu;
        if (t < n) ptbd::leaf_box_words(tris + size_t(t) * 9, p);
        for (uint32_t cur = i;;) {                                  // propagateUp (BVHBuilder.wgsl:242-275): the second child to arrive unions
            const uint32_t par = parent[cur];
            if (par >= nn2) break;
            if (arrive[par]++ == 0u) break;
            arrive[par] = 0u;
            uint32_t* pp = rec(par);
            union_bounds2(pp, rec(pp[3]), rec(pp[4]), wmin, wmax);
            cur = par;
        }
    }
    return true;
}

bool bvh4_cost(const uint32_t* bvh4, uint64_t words, double& cost, std::string& err) {
    cost = 0.0;
    std::vector<uint32_t> order;
    if (!reachable4(bvh4, words, order, err)) return false;
    if (order.empty()) return true;
    const double root = ptbd::half_area(bvh4[1], bvh4[2], bvh4[3]);
    if (!(root > 0.0) || root == double(INFINITY)) return true;
    std::sort(order.begin(), order.end());
    for (uint32_t i : order) {
        const uint32_t* r = bvh4 + 1 + size_t(i) * kNode4Stride;
        if (!(r[7] & kLeafFlag)) cost += ptbd::half_area(r[0], r[1], r[2]) / root;
    }
    return true;
}

bool refit_plan4(const uint32_t* bvh4, uint64_t words, uint32_t num_tris, uint32_t node_base16,
                 std::vector<uint32_t>& up, std::vector<uint32_t>& self, std::vector<uint32_t>& child_ref, std::string& err) {
    std::vector<uint32_t> order;
    if (!reachable4(bvh4, words, order, err)) return false;
    const uint32_t m = order.empty() ? 0u : bvh4[0];
    up.assign(size_t(m) * 2, 0u); self.assign(size_t(m) * 2, kInvalid); child_ref.clear();
    for (uint32_t i = 0; i < m; ++i) up[size_t(i) * 2] = kInvalid;
    uint32_t internal = 0;
    for (uint32_t i : order)                                        // wide indices: the reachable internal nodes in pre-order
        if (!(bvh4[1 + size_t(i) * kNode4Stride + 7] & kLeafFlag)) self[size_t(i) * 2 + 1] = internal++;
    child_ref.assign(size_t(internal) * 4, kInvalid);
    for (uint32_t i : order) {
        const uint32_t* r = bvh4 + 1 + size_t(i) * kNode4Stride;
        if (r[7] & kLeafFlag) { self[size_t(i) * 2] = kLeafFlag; continue; }
        uint32_t valid = 0;
        for (uint32_t s = 0; s < 4; ++s) {
            const uint32_t c = r[3 + s];
            if (c == kInvalid || c >= m) continue;
            const uint32_t w7 = bvh4[1 + size_t(c) * kNode4Stride + 7];
            child_ref[size_t(self[size_t(i) * 2 + 1]) * 4 + s] = (w7 & kLeafFlag) ? packed_leaf_ref(w7 & 0x7fffffffu, num_tris) : node_base16 + 4u * self[size_t(c) * 2 + 1];
            up[size_t(c) * 2] = i; up[size_t(c) * 2 + 1] = s;
            ++valid;
        }
        self[size_t(i) * 2] = valid;
    }
    return true;
}

void build_tri_records(const float* tris, uint32_t n, TriRecord* out) {
    for (uint32_t t = 0; t < n; ++t) {
        const float* p = tris + size_t(t) * 9;
        TriRecord& r = out[t];
        float e1[3], e2[3];
        for (int k = 0; k < 3; ++k) { e1[k] = p[3 + k] - p[k]; e2[k] = p[6 + k] - p[k]; }
        const float cx = e1[1] * e2[2] - e1[2] * e2[1];
        const float cy = e1[2] * e2[0] - e1[0] * e2[2];
        const float cz = e1[0] * e2[1] - e1[1] * e2[0];
        const float inv = 1.0f / std::sqrt((cx * cx + cy * cy) + cz * cz);
        const float n[3] = {cx * inv, cy * inv, cz * inv};
        for (int k = 0; k < 3; ++k) { r.axis[k][0] = p[k]; r.axis[k][1] = e1[k]; r.axis[k][2] = e2[k]; r.axis[k][3] = 0.0f; r.n[k] = n[k]; }
        r.n[3] = 0.0f;
    }
}

// ------------------------------------------------------------------------------------
// Closest-point queries (host twin of pt_pointquery.hip): the same records, operations, order and cap
// ------------------------------------------------------------------------------------
namespace {
constexpr int kStackCap = 64;
struct PointWalk {
    const TriRecord* rec; uint32_t num_tris;
    const WideBvh* wide; uint32_t node_base16;
};
struct WalkCounters { uint64_t nodes = 0, tris = 0, drops = 0, maxstack = 0; };

// d2 of one record with the u, v it was computed from
inline float record_uv_d2(const TriRecord& r, const float p[3], float& u, float& v) {
    const float ax = p[0] - r.axis[0][0], ay = p[1] - r.axis[1][0], az = p[2] - r.axis[2][0];
    ptcp::closest_uv(ax, ay, az, r.axis[0][1], r.axis[1][1], r.axis[2][1], r.axis[0][2], r.axis[1][2], r.axis[2][2], u, v);
    return ptcp::closest_d2(ax, ay, az, r.axis[0][1], r.axis[1][1], r.axis[2][1], r.axis[0][2], r.axis[1][2], r.axis[2][2], u, v);
}
// the record of an item that found nothing: {+inf bits, 0xFFFFFFFF, 0, 0}
inline void write_miss(uint32_t* o) { o[0] = 0x7F800000u; o[1] = kInvalid; o[2] = 0u; o[3] = 0u; }
// pt_pointquery.hip::box_bound2: per axis max(mn - (p + s), (p - s) - mx, 0), each difference rounded once
inline float box_bound2_h(const float hi[3], const float lo[3], const uint32_t w[3]) {
    const Box b = unpack_box(w);
    float g[3];
    for (int k = 0; k < 3; ++k) g[k] = wmax(wmax(b.mn[k] - hi[k], lo[k] - b.mx[k]), 0.0f);
    return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
}

// The walk of every twin, the point queries' and the ray queries': `best2` is what child keys and stacked entries are compared with, and
// `leaf(tri)` is called for every reached leaf with tri < num_tris, in visit order -- the closest-point query lowers best2 there, the
// radius query and the crossing counts leave it alone.  `key(box words, reference)` is what a child is ordered and stacked by: bound2 of
// a point, 0 / +inf of a box query (box_search), tmin / +inf of a sweep or a ray (sweep_spheres, walk_ray_h).  A child is visited iff its
// key is below best2, so a key of +inf is a child that is never visited.
template <class Key, class Leaf>
void walk_keys_h(const PointWalk& W, Key key, const float& best2, WalkCounters& cnt, Leaf leaf) {
    const WideBvh& wb = *W.wide;
    if (wb.root_ref == kInvalid || W.num_tris == 0u) return;
    cnt.nodes += 1; if (cnt.maxstack < 1u) cnt.maxstack = 1u;
    if (wb.root_degenerate) return;
    if (!(key(wb.root_box, wb.root_ref) < best2)) return;
    struct Entry { uint32_t ref; float b2; } stk[kStackCap];
    uint32_t cur = wb.root_ref;
    int sp = 0;
    for (;;) {
        bool need_pop = false;
        if (cur & kLeafFlag) {
            const uint32_t ti4 = cur & 0x7fffffffu;
            if (ti4 < 4u * W.num_tris) {
                cnt.tris += 1;
                leaf(ti4 >> 2);
            }
            need_pop = true;
        } else {
            const WideNode& nd = wb.nodes[(cur - W.node_base16) >> 2];
            float t[4]; bool h[4]; uint32_t r[4];
            for (int k = 0; k < 4; ++k) {
                r[k] = nd.child[k].ref; t[k] = key(nd.child[k].box, r[k]); h[k] = t[k] < best2;
                cnt.nodes += (r[k] != kInvalid);
            }
            int nslot = -1, fslot = -1;
            for (int k = 0; k < 4; ++k) if (h[k]) { if (nslot < 0 || t[k] < t[nslot]) nslot = k; if (fslot < 0) fslot = k; }
            if (nslot < 0) {
                need_pop = true;
            } else {
                // pushes far -> near; the slot the nearest child left holds the first passing child
                for (int k = 3; k >= 1; --k) {
                    if (!h[k] || fslot == k) continue;
                    const int src = (nslot == k) ? fslot : k;
                    if (sp < kStackCap) { stk[sp].ref = r[src]; stk[sp].b2 = t[src]; ++sp; } else cnt.drops += 1;
                }
                const uint64_t depth = uint64_t(sp) + (sp < kStackCap ? 1u : 0u);
                if (depth > cnt.maxstack) cnt.maxstack = depth;
                if (sp < kStackCap) cur = r[nslot];
                else { need_pop = true; cnt.drops += 1; }
            }
        }
        if (need_pop) {
            bool found = false;
            while (sp > 0) {
                --sp;
                if (stk[sp].b2 < best2) { cur = stk[sp].ref; found = true; break; }
            }
            if (!found) break;
        }
    }
}
template <class Leaf>
void walk_h(const PointWalk& W, const float p[3], const float& best2, WalkCounters& cnt, Leaf leaf) {
    const float hi[3] = {p[0] + ptcp::kSlack, p[1] + ptcp::kSlack, p[2] + ptcp::kSlack};
    const float lo[3] = {p[0] - ptcp::kSlack, p[1] - ptcp::kSlack, p[2] - ptcp::kSlack};
    walk_keys_h(W, [&](const uint32_t* w, uint32_t) { return box_bound2_h(hi, lo, w); }, best2, cnt, leaf);
}
void walk_point_h(const PointWalk& W, const float p[3], float& best2, uint32_t& best_tri, WalkCounters& cnt) {
    best_tri = kInvalid;
    walk_h(W, p, best2, cnt, [&](uint32_t tri) {
        float u, v;
        const float d2 = record_uv_d2(W.rec[tri], p, u, v);
        if (d2 < best2) { best2 = d2; best_tri = tri; }
    });
}

// What every *_bvh4 twin starts from: the wide tree (none with brute force: bvh4 = nullptr), the triangle records, the walk's view of
// both, and at most 16 workers with a counter block each.  Worker w of parallel() takes the items [n w / workers, n (w + 1) / workers).
struct TwinScene {
    WideBvh wide; std::vector<TriRecord> rec; PointWalk W;
    uint64_t n = 0, workers = 1; std::vector<WalkCounters> per;

    bool init(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, uint64_t items, std::string& err) {
        const uint32_t node_base16 = uint32_t((uint64_t(num_tris) + 1u) * 4u);
        if (bvh4 && !build_wide_bvh(bvh4, words, num_tris, node_base16, wide, err)) return false;
        rec.resize(num_tris);
        build_tri_records(tris, num_tris, rec.data());
        W.rec = rec.data(); W.num_tris = num_tris; W.wide = &wide; W.node_base16 = node_base16;
        const unsigned hw = std::thread::hardware_concurrency();
        n = items; workers = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(hw ? hw : 1u, 16u), n / 256u));
        per.assign(workers, WalkCounters());
        return true;
    }
    // run(w, first, end)
    template <class Run>
    void parallel(Run run) const {
        auto part = [&](uint64_t w) { run(w, n * w / workers, n * (w + 1) / workers); };
        if (workers == 1) { part(0); return; }
        std::vector<std::thread> pool;
        for (uint64_t w = 0; w < workers; ++w) pool.emplace_back(part, w);
        for (std::thread& t : pool) t.join();
    }
    // the five counters of PtStats: `items`, and the workers' blocks summed (the stack depth: their maximum)
    void reduce(uint64_t* counters, uint64_t items) const {
        if (!counters) return;
        counters[0] = items; counters[1] = counters[2] = counters[3] = counters[4] = 0;
        for (const WalkCounters& c : per) {
            counters[1] += c.nodes; counters[2] += c.tris; counters[3] += c.drops; counters[4] = std::max(counters[4], c.maxstack);
        }
    }
};

// The frame of a list query (radius_search, box_search, list_hits), the device's two walks around its scan.  query(i, cnt, accept) walks
// item i and calls accept(store) for every accepted leaf in visit order, store(o) writing the 16-byte entry at o.  The count walk leaves
// the count of item i in offsets[i + 1] until the prefix sum; the fill walk takes the same steps and stores entry k of item i at
// offsets[i] + k where that is below the capacity (its counters are dropped: the device counts over the count walk), then calls
// stored(worker, i) behind each list.
template <class Query, class Stored>
void list_twin(TwinScene& S, uint64_t* offsets, uint32_t* entries, uint64_t capacity, Query query, Stored stored) {
    offsets[0] = 0;
    S.parallel([&](uint64_t w, uint64_t first, uint64_t end) {
        for (uint64_t i = first; i < end; ++i) {
            uint64_t count = 0;
            query(i, S.per[w], [&](auto&&) { ++count; });
            offsets[i + 1] = count;
        }
    });
    for (uint64_t i = 0; i < S.n; ++i) offsets[i + 1] += offsets[i];
    if (!entries || !capacity) return;
    S.parallel([&](uint64_t w, uint64_t first, uint64_t end) {
        WalkCounters unused;
        for (uint64_t i = first; i < end; ++i) {
            uint64_t g = offsets[i];
            if (g >= capacity) break;                           // the offsets only grow
            query(i, unused, [&](auto&& store) { if (g < capacity) store(entries + g * 4); ++g; });
            stored(w, i);
        }
    });
}
} // namespace

bool closest_points(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const float* points, uint64_t n,
                    uint32_t* out, uint64_t* counters, std::string& err) {
    TwinScene S;
    if (!S.init(tris, num_tris, bvh4, words, n, err)) return false;
    const std::vector<TriRecord>& rec = S.rec;
    S.parallel([&](uint64_t w, uint64_t first, uint64_t end) {
        WalkCounters& cnt = S.per[w];
        for (uint64_t i = first; i < end; ++i) {
            const float* q = points + i * 4;
            float best2 = q[3] * q[3]; uint32_t tri = kInvalid;
            if (ptcp::point_walked(q[0], q[1], q[2], q[3])) {
                if (bvh4) walk_point_h(S.W, q, best2, tri, cnt);
                else {
                    for (uint32_t t = 0; t < num_tris; ++t) { float u, v; const float d2 = record_uv_d2(rec[t], q, u, v); if (d2 < best2) { best2 = d2; tri = t; } }
                    cnt.tris += num_tris;
                }
            }
            uint32_t* o = out + i * 4;
            if (tri == kInvalid) { write_miss(o); continue; }
            const TriRecord& r = rec[tri];
            float u, v;
            ptcp::closest_uv(q[0] - r.axis[0][0], q[1] - r.axis[1][0], q[2] - r.axis[2][0],
                             r.axis[0][1], r.axis[1][1], r.axis[2][1], r.axis[0][2], r.axis[1][2], r.axis[2][2], u, v);
            o[0] = bits_of(std::sqrt(best2)); o[1] = tri; o[2] = bits_of(u); o[3] = bits_of(v);
        }
    });
    S.reduce(counters, n);
    return true;
}

// ------------------------------------------------------------------------------------
// Radius queries (host twin of pt_radius.hip): the closest-point walk with best2 held at r_max^2, every accepted leaf counted and, in a
// second walk of the same steps, listed at offsets[i] + k -- the device's two walks around its scan
// ------------------------------------------------------------------------------------
bool radius_search(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const float* points, uint64_t n,
                   uint64_t* offsets, uint32_t* entries, uint64_t capacity, uint64_t* counters, std::string& err) {
    TwinScene S;
    if (!S.init(tris, num_tris, bvh4, words, n, err)) return false;
    // one point: the walk (or every triangle in index order)
    list_twin(S, offsets, entries, capacity, [&](uint64_t i, WalkCounters& cnt, auto accept) {
        const float* q = points + i * 4;
        if (!ptcp::point_walked(q[0], q[1], q[2], q[3])) return;
        const float r2 = q[3] * q[3];
        auto leaf = [&](uint32_t t) {
            float u, v;
            const float d2 = record_uv_d2(S.rec[t], q, u, v);
            if (d2 < r2) accept([&](uint32_t* o) { o[0] = bits_of(std::sqrt(d2)); o[1] = t; o[2] = bits_of(u); o[3] = bits_of(v); });
        };
        if (bvh4) { walk_h(S.W, q, r2, cnt, leaf); return; }    // r2 never moves: every stacked entry passes its re-validation
        for (uint32_t t = 0; t < num_tris; ++t) leaf(t);
        cnt.tris += num_tris;
    }, [](uint64_t, uint64_t) {});
    S.reduce(counters, n);
    return true;
}

// ------------------------------------------------------------------------------------
// Box-overlap queries (host twin of pt_overlap.hip): the walk with every key equal -- 0 for a child whose box meets the query box moved out
// by the slack, +inf for any other, against a bound of 1 -- every accepted leaf counted and, in a second walk of the same steps, listed at
// offsets[i] + k.  The arithmetic is pt_overlap.h, the text the kernels compile.
// ------------------------------------------------------------------------------------
bool box_search(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const float* boxes, uint64_t n,
                uint64_t* offsets, uint32_t* entries, uint64_t capacity, uint64_t* counters, std::string& err) {
    TwinScene S;
    if (!S.init(tris, num_tris, bvh4, words, n, err)) return false;
    // one box: the walk (or every triangle in index order)
    list_twin(S, offsets, entries, capacity, [&](uint64_t i, WalkCounters& cnt, auto accept) {
        const float* q = boxes + i * 8;
        if (!ptov::box_walked(q[0], q[1], q[2], q[4], q[5], q[6])) return;
        const ptov::Box b = ptov::make_box(q[0], q[1], q[2], q[4], q[5], q[6]);
        auto leaf = [&](uint32_t t) {
            const TriRecord& r = S.rec[t];
            uint32_t in;
            if (ptov::tri_overlaps(b, r.axis[0][0], r.axis[1][0], r.axis[2][0], r.axis[0][1], r.axis[1][1], r.axis[2][1],
                                   r.axis[0][2], r.axis[1][2], r.axis[2][2], in)) accept([&](uint32_t* o) { o[0] = t; o[1] = in; o[2] = 0u; o[3] = 0u; });
        };
        if (bvh4) {
            const float bound = 1.0f;
            walk_keys_h(S.W, [&](const uint32_t* w, uint32_t) {
                const Box c = unpack_box(w);
                const bool meets = ptov::node_overlaps(b, c.mn[0], c.mn[1], c.mn[2], c.mx[0], c.mx[1], c.mx[2]);
                return meets ? 0.0f : std::numeric_limits<float>::infinity();
            }, bound, cnt, leaf);
            return;
        }
        for (uint32_t t = 0; t < num_tris; ++t) leaf(t);
        cnt.tris += num_tris;
    }, [](uint64_t, uint64_t) {});
    S.reduce(counters, n);
    return true;
}

// ------------------------------------------------------------------------------------
// Triangle-overlap queries (host twin of pt_tritri.hip): box_search's walk on the caller triangle's exact bounding box, every accepted
// leaf counted and, in a second walk of the same steps, listed at offsets[i] + k.  The arithmetic is pt_tritri.h, the text the kernels
// compile; both walks compute all six bits (the device's count walk may stop at the first: the same accepted set).
// ------------------------------------------------------------------------------------
bool tri_search(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const float* in, uint64_t n,
                uint64_t* offsets, uint32_t* entries, uint64_t capacity, uint64_t* counters, std::string& err) {
    TwinScene S;
    if (!S.init(tris, num_tris, bvh4, words, n, err)) return false;
    // one caller triangle: the walk (or every triangle in index order)
    list_twin(S, offsets, entries, capacity, [&](uint64_t i, WalkCounters& cnt, auto accept) {
        const float* p = in + i * 12;
        const pttt::Tri q = {p[0], p[1], p[2], p[4], p[5], p[6], p[8], p[9], p[10]};
        if (!pttt::tri_walked(q)) return;
        const ptov::Box b = pttt::tri_box(q);
        auto leaf = [&](uint32_t t) {
            const TriRecord& r = S.rec[t];
            const uint32_t edges = pttt::tri_crosses<true>(b, q, r.axis[0][0], r.axis[1][0], r.axis[2][0], r.axis[0][1], r.axis[1][1], r.axis[2][1],
                                                           r.axis[0][2], r.axis[1][2], r.axis[2][2]);
            if (edges) accept([&](uint32_t* o) { o[0] = t; o[1] = edges; o[2] = 0u; o[3] = 0u; });
        };
        if (bvh4) {
            const float bound = 1.0f;
            walk_keys_h(S.W, [&](const uint32_t* w, uint32_t) {
                const Box c = unpack_box(w);
                const bool meets = ptov::node_overlaps(b, c.mn[0], c.mn[1], c.mn[2], c.mx[0], c.mx[1], c.mx[2]);
                return meets ? 0.0f : std::numeric_limits<float>::infinity();
            }, bound, cnt, leaf);
            return;
        }
        for (uint32_t t = 0; t < num_tris; ++t) leaf(t);
        cnt.tris += num_tris;
    }, [](uint64_t, uint64_t) {});
    S.reduce(counters, n);
    return true;
}

// ------------------------------------------------------------------------------------
// Plane-cut queries (host twin of pt_cut.hip): box_search's walk on the window, a child entered iff the window's node test passes and
// the plane separates two corners of the child's grown box; every accepted leaf counted and, in a second walk of the same steps, listed
// at offsets[i] + k with where the plane crosses its two crossing edges.  The arithmetic is pt_cut.h, the text the kernels compile; both
// walks compute t0 and t1 (the device's count walk classifies only: the same accepted set).
// ------------------------------------------------------------------------------------
bool cut_search(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const float* in, uint64_t n,
                uint64_t* offsets, uint32_t* entries, uint64_t capacity, uint64_t* counters, std::string& err) {
    TwinScene S;
    if (!S.init(tris, num_tris, bvh4, words, n, err)) return false;
    // one plane and its window: the walk (or every triangle in index order)
    list_twin(S, offsets, entries, capacity, [&](uint64_t i, WalkCounters& cnt, auto accept) {
        const float* q = in + i * 12;
        const ptct::Plane p = {q[0], q[1], q[2], q[3]};
        if (!ptct::plane_walked(p) || !ptov::box_walked(q[4], q[5], q[6], q[8], q[9], q[10])) return;
        const ptov::Box b = ptov::make_box(q[4], q[5], q[6], q[8], q[9], q[10]);
        auto leaf = [&](uint32_t t) {
            const TriRecord& r = S.rec[t];
            ptct::Cut c = {0u, 0.0f, 0.0f};
            if (ptct::tri_cut<true>(b, p, r.axis[0][0], r.axis[1][0], r.axis[2][0], r.axis[0][1], r.axis[1][1], r.axis[2][1],
                                    r.axis[0][2], r.axis[1][2], r.axis[2][2], c))
                accept([&](uint32_t* o) { o[0] = t; o[1] = c.code; std::memcpy(o + 2, &c.t0, 4); std::memcpy(o + 3, &c.t1, 4); });
        };
        if (bvh4) {
            const float bound = 1.0f;
            walk_keys_h(S.W, [&](const uint32_t* w, uint32_t) {
                const Box c = unpack_box(w);
                const bool meets = ptov::node_overlaps(b, c.mn[0], c.mn[1], c.mn[2], c.mx[0], c.mx[1], c.mx[2]) &&
                                   ptct::node_cut(p, c.mn[0], c.mn[1], c.mn[2], c.mx[0], c.mx[1], c.mx[2]);
                return meets ? 0.0f : std::numeric_limits<float>::infinity();
            }, bound, cnt, leaf);
            return;
        }
        for (uint32_t t = 0; t < num_tris; ++t) leaf(t);
        cnt.tris += num_tris;
    }, [](uint64_t, uint64_t) {});
    S.reduce(counters, n);
    return true;
}

// ------------------------------------------------------------------------------------
// Sphere-cast queries (host twin of pt_sweep.hip): the walk with the key of a child = tmin of the slab test on its box grown by r + s,
// +inf where that test fails, against `best`, which starts at t_max and shrinks to each accepted t_T.  The arithmetic is pt_sweep.h, the
// text the kernels compile.
// ------------------------------------------------------------------------------------
bool sweep_spheres(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const float* sweeps, uint64_t n,
                   uint32_t* out, uint64_t* counters, std::string& err) {
    TwinScene S;
    if (!S.init(tris, num_tris, bvh4, words, n, err)) return false;
    const std::vector<TriRecord>& rec = S.rec;
    S.parallel([&](uint64_t w, uint64_t first, uint64_t end) {
        WalkCounters& cnt = S.per[w];
        for (uint64_t i = first; i < end; ++i) {
            const float* q = sweeps + i * 8;
            const float o[3] = {q[0], q[1], q[2]}, d[3] = {q[4], q[5], q[6]}, r = q[7];
            float best = q[3]; uint32_t tri = kInvalid;
            if (ptsw::sweep_walked(o[0], o[1], o[2], q[3], d[0], d[1], d[2], r)) {
                const float inv[3] = {ptry::safe_inv(d[0]), ptry::safe_inv(d[1]), ptry::safe_inv(d[2])};
                auto leaf = [&](uint32_t t) {
                    const TriRecord& tr = rec[t];
                    const float tt = ptsw::tri_sweep(o[0], o[1], o[2], d[0], d[1], d[2], inv[0], inv[1], inv[2], r, best, tr.axis[0][0], tr.axis[1][0], tr.axis[2][0],
                                                     tr.axis[0][1], tr.axis[1][1], tr.axis[2][1], tr.axis[0][2], tr.axis[1][2], tr.axis[2][2]);
                    if (tt < best) { best = ptsw::bound_after(tt); tri = t; }
                };
                if (bvh4) {
                    const float R = r + ptcp::kSlack;
                    const float op[3] = {o[0] + R, o[1] + R, o[2] + R}, om[3] = {o[0] - R, o[1] - R, o[2] - R};
                    walk_keys_h(S.W, [&](const uint32_t* bw, uint32_t) {
                        const Box c = unpack_box(bw);
                        float tmin;
                        const bool pass = ptsw::node_pass(c.mn[0], c.mn[1], c.mn[2], c.mx[0], c.mx[1], c.mx[2],
                                                          op[0], op[1], op[2], om[0], om[1], om[2], inv[0], inv[1], inv[2], best, tmin);
                        return pass ? tmin : std::numeric_limits<float>::infinity();
                    }, best, cnt, leaf);
                } else {
                    for (uint32_t t = 0; t < num_tris; ++t) leaf(t);
                    cnt.tris += num_tris;
                }
            }
            uint32_t* po = out + i * 4;
            if (tri == kInvalid) { write_miss(po); continue; }
            const TriRecord& tr = rec[tri];
            float u, v;
            best = ptsw::time_of(best);
            ptsw::contact_uv(o[0], o[1], o[2], d[0], d[1], d[2], best, tr.axis[0][0], tr.axis[1][0], tr.axis[2][0],
                             tr.axis[0][1], tr.axis[1][1], tr.axis[2][1], tr.axis[0][2], tr.axis[1][2], tr.axis[2][2], u, v);
            po[0] = bits_of(best); po[1] = tri; po[2] = bits_of(u); po[3] = bits_of(v);
        }
    });
    S.reduce(counters, n);
    return true;
}

// ------------------------------------------------------------------------------------
// k-nearest queries (host twin of pt_knn.hip): the closest-point walk with best2 replaced by worst2 -- r_max^2 while the list holds fewer
// than k pairs, the d2 of its last pair after that -- and a list of at most k pairs (d2, triangle) in ascending order of d2, equal
// distances in visit order
// ------------------------------------------------------------------------------------
bool nearest_k(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const float* points, uint64_t n, uint32_t k,
               uint32_t* out, uint64_t* counters, std::string& err) {
    if (k == 0u || k > kNearestMaxK) { err = "nearest_k: k must be 1 .. 64"; return false; }
    TwinScene S;
    if (!S.init(tris, num_tris, bvh4, words, n, err)) return false;
    const std::vector<TriRecord>& rec = S.rec;
    S.parallel([&](uint64_t w, uint64_t first, uint64_t end) {
        WalkCounters& cnt = S.per[w];
        struct Pair { float d2; uint32_t tri; } lst[kNearestMaxK];
        for (uint64_t i = first; i < end; ++i) {
            const float* q = points + i * 4;
            float worst2 = q[3] * q[3];
            uint32_t count = 0;
            // pt_knn.hip::nk_insert: behind every pair with d2' <= d2, the tail shifted down from the end, the pair behind the k-th lost
            auto leaf = [&](uint32_t t) {
                float u, v;
                const float d2 = record_uv_d2(rec[t], q, u, v);
                if (!(d2 < worst2)) return;
                uint32_t j = count < k ? count : k - 1u;
                for (; j > 0u && lst[j - 1u].d2 > d2; --j) lst[j] = lst[j - 1u];
                lst[j].d2 = d2; lst[j].tri = t;
                if (count < k) ++count;
                if (count == k) worst2 = lst[k - 1u].d2;
            };
            if (ptcp::point_walked(q[0], q[1], q[2], q[3])) {
                if (bvh4) walk_h(S.W, q, worst2, cnt, leaf);
                else {
                    for (uint32_t t = 0; t < num_tris; ++t) leaf(t);
                    cnt.tris += num_tris;
                }
            }
            uint32_t* o = out + i * k * 4;
            for (uint32_t j = 0; j < count; ++j, o += 4) {
                float u, v;
                (void)record_uv_d2(rec[lst[j].tri], q, u, v);
                o[0] = bits_of(std::sqrt(lst[j].d2)); o[1] = lst[j].tri; o[2] = bits_of(u); o[3] = bits_of(v);
            }
            for (uint32_t j = count; j < k; ++j, o += 4) write_miss(o);
        }
    });
    S.reduce(counters, n);
    return true;
}

// ------------------------------------------------------------------------------------
// Tiles: 8x8 pixels; tile (tx,ty) belongs to rank (tx + ty) % count.  A rank's tiles are
// listed row-major; the list index is the tile's slot in the rank's compact buffer.
// ------------------------------------------------------------------------------------
void tile_list(uint32_t width, uint32_t height, uint32_t rank, uint32_t count, std::vector<uint32_t>& tiles) {
    tiles.clear();
    if (count == 0) count = 1;
    const uint32_t tx_n = (width + kTile - 1) / kTile, ty_n = (height + kTile - 1) / kTile;
    for (uint32_t ty = 0; ty < ty_n; ++ty)
        for (uint32_t tx = 0; tx < tx_n; ++tx)
            if ((tx + ty) % count == rank) tiles.push_back(ty * tx_n + tx);
}

uint32_t tile_count_of(uint32_t width, uint32_t height, uint32_t rank, uint32_t count) {
    if (count == 0) count = 1;
    const uint32_t tx_n = (width + kTile - 1) / kTile, ty_n = (height + kTile - 1) / kTile;
    uint32_t n = 0;
    for (uint32_t ty = 0; ty < ty_n; ++ty) {
        const uint32_t first = (rank + count - ty % count) % count;
        if (first < tx_n) n += (tx_n - first + count - 1) / count;
    }
    return n;
}

// the rank's tiles inside the tile rectangle rect = {tx0, ty0, tx1, ty1} (packed tile shares, pt_kernels.hip)
uint32_t rect_tile_count_of(uint32_t rank, uint32_t count, const uint32_t rect[4]) {
    if (count == 0) count = 1;
    if (rect[2] <= rect[0] || rect[3] <= rect[1]) return 0;
    uint32_t n = 0;
    for (uint32_t ty = rect[1]; ty < rect[3]; ++ty) {
        const uint32_t first = rect[0] + (rank + count - ((ty + rect[0]) % count)) % count;
        if (first < rect[2]) n += (rect[2] - first + count - 1) / count;
    }
    return n;
}

// ------------------------------------------------------------------------------------
// Procedural stand-in scenes
// ------------------------------------------------------------------------------------
namespace {

inline uint32_t hash_u32(uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }
inline double hash01(uint32_t a, uint32_t b, uint32_t c, uint32_t seed) {
    return double(hash_u32(hash_u32(hash_u32(a + 0x9E3779B9u * seed) ^ b) ^ c) >> 8) / 16777216.0;
}
// periodic value noise on a ku x kv lattice, u,v in [0,1)
double value_noise(double u, double v, uint32_t ku, uint32_t kv, uint32_t oct, uint32_t seed) {
    const double fu = u * ku, fv = v * kv;
    const double iu = std::floor(fu), iv = std::floor(fv);
    double a = fu - iu, b = fv - iv;
    a = a * a * (3 - 2 * a); b = b * b * (3 - 2 * b);
    const uint32_t u0 = uint32_t(iu) % ku, u1 = (u0 + 1) % ku, v0 = uint32_t(iv) % kv, v1 = (v0 + 1) % kv;
    const double h00 = hash01(u0, v0, oct, seed), h10 = hash01(u1, v0, oct, seed);
    const double h01 = hash01(u0, v1, oct, seed), h11 = hash01(u1, v1, oct, seed);
    return (h00 * (1 - a) + h10 * a) * (1 - b) + (h01 * (1 - a) + h11 * a) * b;
}

struct D3 { double x, y, z; };
inline D3 operator+(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline D3 operator-(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline D3 operator*(D3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
inline D3 crossd(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline double dotd(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline D3 normd(D3 a) { const double l = std::sqrt(dotd(a, a)); return l > 0 ? a * (1.0 / l) : D3{0, 0, 1}; }

// "normalize cube" of Scene.js:104-165: centre on the bounding-box centre, scale 2/maxDim
void normalize_cube(std::vector<D3>& v) {
    D3 lo = v[0], hi = v[0];
    for (const D3& p : v) {
        lo.x = std::min(lo.x, p.x); lo.y = std::min(lo.y, p.y); lo.z = std::min(lo.z, p.z);
        hi.x = std::max(hi.x, p.x); hi.y = std::max(hi.y, p.y); hi.z = std::max(hi.z, p.z);
    }
    const D3 c = {(lo.x + hi.x) * 0.5, (lo.y + hi.y) * 0.5, (lo.z + hi.z) * 0.5};
    const double scale = 2.0 / std::max(hi.x - lo.x, std::max(hi.y - lo.y, hi.z - lo.z));
    for (D3& p : v) p = (p - c) * scale;
}

struct TriList {
    float* out; uint32_t cap; uint32_t n = 0;
    void add(D3 a, D3 b, D3 c) {
        if (n >= cap) return;
        float* p = out + size_t(n) * 9;
        p[0] = float(a.x); p[1] = float(a.y); p[2] = float(a.z);
        p[3] = float(b.x); p[4] = float(b.y); p[5] = float(b.z);
        p[6] = float(c.x); p[7] = float(c.y); p[8] = float(c.z);
        ++n;
    }
};

// Dragon-class: a thick trefoil-knot tube with a swelling body and multi-octave "scale"
// bumps: closed, concave, self-occluding.  a x b quad grid -> 2ab triangles; the remainder up
// to num_tris is made by centroid-splitting evenly spaced triangles (+2 each), a last odd
// triangle by one edge-midpoint split (+1).
bool dragon_class(uint32_t seed, uint32_t num_tris, float* out, std::string& err) {
    if (num_tris < 24) { err = "dragon-class scene needs at least 24 triangles"; return false; }
    uint32_t b = uint32_t(std::floor(std::sqrt(double(num_tris) / 2.0 / 12.0)));
    if (b < 3) b = 3;
    uint32_t a = num_tris / 2 / b;
    if (a < 4) { a = 4; b = num_tris / 2 / a; if (b < 3) b = 3; }
    const uint32_t base_tris = 2 * a * b;
    if (base_tris > num_tris) { err = "internal: grid larger than request"; return false; }
    std::vector<D3> vert(size_t(a) * b);
    const double two_pi = 6.283185307179586476925286766559;
    for (uint32_t i = 0; i < a; ++i) {
        const double u = double(i) / a, t = two_pi * u;
        // trefoil centre line and its frame (analytic tangent, numeric-free normal via second derivative)
        const double c3 = std::cos(3 * t), s3 = std::sin(3 * t), c2 = std::cos(2 * t), s2 = std::sin(2 * t);
        const D3 pos = {(2 + c3) * c2, (2 + c3) * s2, s3 * 1.3};
        const D3 d1 = {-3 * s3 * c2 - 2 * (2 + c3) * s2, -3 * s3 * s2 + 2 * (2 + c3) * c2, 3 * c3 * 1.3};
        const D3 d2 = {-9 * c3 * c2 + 12 * s3 * s2 - 4 * (2 + c3) * c2, -9 * c3 * s2 - 12 * s3 * c2 - 4 * (2 + c3) * s2, -9 * s3 * 1.3};
        const D3 T = normd(d1);
        const D3 N = normd(d2 - T * dotd(d2, T));
        const D3 B = crossd(T, N);
        const double swell = 0.62 + 0.22 * std::sin(5 * t + 0.7) + 0.10 * std::sin(11 * t);
        for (uint32_t j = 0; j < b; ++j) {
            const double v = double(j) / b, phi = two_pi * v;
            double bump = 0.0;
            bump += 0.090 * (value_noise(u, v, 96, 12, 0, seed) - 0.5);
            bump += 0.050 * (value_noise(u, v, 288, 36, 1, seed) - 0.5);
            bump += 0.025 * (value_noise(u, v, 864, 108, 2, seed) - 0.5);
            const double ridge = 0.06 * std::fabs(std::sin(40 * t)) * (0.5 + 0.5 * std::cos(phi));   // dorsal scales
            const double r = swell * (1.0 + 0.18 * std::cos(2 * phi)) + bump + ridge;
            vert[size_t(i) * b + j] = pos + (N * std::cos(phi) + B * std::sin(phi)) * r;
        }
    }
    normalize_cube(vert);
    TriList tl{out, num_tris};
    uint32_t extra = num_tris - base_tris;
    const uint32_t splits = extra / 2; const bool odd = (extra & 1u) != 0;
    // evenly spaced triangle ids get the centroid split
    uint64_t acc = 0; uint32_t next_split = 0, done_splits = 0; bool odd_done = !odd;
    uint32_t tri_id = 0;
    auto emit = [&](D3 p0, D3 p1, D3 p2) {
        bool split = false;
        if (done_splits < splits) {
            acc += splits;
            if (acc >= base_tris) { acc -= base_tris; split = true; }
        }
        (void)next_split;
        if (split) {
            const D3 c = (p0 + p1 + p2) * (1.0 / 3.0);
            tl.add(p0, p1, c); tl.add(p1, p2, c); tl.add(p2, p0, c);
            ++done_splits;
        } else if (!odd_done) {
            const D3 m = (p0 + p1) * 0.5;
            tl.add(p0, m, p2); tl.add(m, p1, p2);
            odd_done = true;
        } else {
            tl.add(p0, p1, p2);
        }
        ++tri_id;
    };
    for (uint32_t i = 0; i < a; ++i) {
        const uint32_t i1 = (i + 1) % a;
        for (uint32_t j = 0; j < b; ++j) {
            const uint32_t j1 = (j + 1) % b;
            const D3 p00 = vert[size_t(i) * b + j], p10 = vert[size_t(i1) * b + j];
            const D3 p01 = vert[size_t(i) * b + j1], p11 = vert[size_t(i1) * b + j1];
            emit(p00, p10, p11);
            emit(p00, p11, p01);
        }
    }
    if (tl.n != num_tris) { err = "internal: dragon-class generator produced a wrong triangle count"; return false; }
    return true;
}

// Sponza-class: an atrium seen from inside -- floor, four walls, a roof open along the middle, two
// colonnades of fluted columns (long thin triangles) and hanging wavy drapes.  Nearly every camera ray hits.
bool sponza_class(uint32_t seed, uint32_t num_tris, float* out, std::string& err) {
    if (num_tris < 12000) { err = "sponza-class scene needs at least 12000 triangles"; return false; }
    TriList tl{out, num_tris};
    std::vector<D3> quads;   // 4 corners per quad, later normalised together
    std::vector<D3> all;
    auto quad = [&](D3 p00, D3 p10, D3 p11, D3 p01) { all.push_back(p00); all.push_back(p10); all.push_back(p11); all.push_back(p01); };
    // budget: columns+drapes+walls take ~55 %, the floor/ceiling grids absorb the rest
    const double X = 3.0, Y = 1.2, Z = 1.4;   // half extents: long hall along x
    const uint32_t ncol = 10;                 // per side
    const uint32_t flutes = 48, rings = std::max(2u, uint32_t(num_tris * 0.30 / (2.0 * ncol * 2 * flutes)));
    const double two_pi = 6.283185307179586476925286766559;
    for (uint32_t side = 0; side < 2; ++side)
        for (uint32_t c = 0; c < ncol; ++c) {
            const double cx = -X + (c + 0.5) * (2 * X / ncol), cz = (side ? 0.75 : -0.75);
            for (uint32_t r = 0; r < rings; ++r) {
                const double y0 = -Y + 2 * Y * double(r) / rings, y1 = -Y + 2 * Y * double(r + 1) / rings;
                for (uint32_t f = 0; f < flutes; ++f) {
                    const double a0 = two_pi * f / flutes, a1 = two_pi * (f + 1) / flutes;
                    const double r0 = 0.11 + 0.012 * std::cos(a0 * 12) , r1 = 0.11 + 0.012 * std::cos(a1 * 12);
                    quad({cx + r0 * std::cos(a0), y0, cz + r0 * std::sin(a0)}, {cx + r1 * std::cos(a1), y0, cz + r1 * std::sin(a1)},
                         {cx + r1 * std::cos(a1), y1, cz + r1 * std::sin(a1)}, {cx + r0 * std::cos(a0), y1, cz + r0 * std::sin(a0)});
                }
            }
        }
    // drapes: wavy sheets hanging between columns
    const uint32_t ndrape = 8, du = 40, dv = std::max(4u, uint32_t(num_tris * 0.20 / (2.0 * ndrape * du)));
    for (uint32_t d = 0; d < ndrape; ++d) {
        const double x0 = -X + 0.4 + d * (2 * X - 0.8) / ndrape, x1 = x0 + (2 * X - 0.8) / ndrape * 0.8;
        const double z = (d & 1) ? 0.35 : -0.35;
        for (uint32_t i = 0; i < du; ++i) for (uint32_t j = 0; j < dv; ++j) {
            auto P = [&](uint32_t ii, uint32_t jj) {
                const double u = double(ii) / du, v = double(jj) / dv;
                const double w = 0.08 * std::sin(u * 18 + d) * (0.3 + v) + 0.05 * (value_noise(u, v, 8, 8, d, seed) - 0.5);
                return D3{x0 + (x1 - x0) * u, Y - 0.1 - 1.3 * v, z + w};
            };
            quad(P(i, j), P(i + 1, j), P(i + 1, j + 1), P(i, j + 1));
        }
    }
    // walls (coarse long thin strips) : 4 walls x strips
    const uint32_t strips = 64;
    for (uint32_t s = 0; s < strips; ++s) {
        const double xa = -X + 2 * X * double(s) / strips, xb = -X + 2 * X * double(s + 1) / strips;
        quad({xa, -Y, -Z}, {xb, -Y, -Z}, {xb, Y, -Z}, {xa, Y, -Z});
        quad({xb, -Y, Z}, {xa, -Y, Z}, {xa, Y, Z}, {xb, Y, Z});
    }
    for (uint32_t s = 0; s < strips / 4; ++s) {
        const double za = -Z + 2 * Z * double(s) / (strips / 4), zb = -Z + 2 * Z * double(s + 1) / (strips / 4);
        quad({-X, -Y, zb}, {-X, -Y, za}, {-X, Y, za}, {-X, Y, zb});
        quad({X, -Y, za}, {X, -Y, zb}, {X, Y, zb}, {X, Y, za});
    }
    // floor + ceiling grids absorb the remaining budget
    const uint64_t used = all.size() / 4 * 2;
    if (used + 64 > num_tris) { err = "internal: sponza-class fixed parts exceed the request"; return false; }
    const uint64_t rest_quads = (num_tris - used) / 2;
    uint32_t gz = std::max(2u, uint32_t(std::floor(std::sqrt(double(rest_quads) / 2.0 / 2.2))));
    uint32_t gx = std::max(2u, uint32_t(rest_quads / 2 / gz));
    for (uint32_t pass = 0; pass < 2; ++pass) {
        const double y = pass ? Y : -Y;
        for (uint32_t i = 0; i < gx; ++i) for (uint32_t j = 0; j < gz; ++j) {
            // the roof is open along the middle of the hall (an atrium): the ceiling grid covers two side
            // strips, columns j < gz/2 the one at -z, the others the one at +z
            const uint32_t half = gz / 2;
            auto P = [&](uint32_t ii, uint32_t jj) {
                const double u = double(ii) / gx, v = double(jj) / gz;
                if (!pass) {
                    const double h = 0.01 * (value_noise(u, v, 64, 32, 9, seed) - 0.5);
                    return D3{-X + 2 * X * u, y + h, -Z + 2 * Z * v};
                }
                const bool left = j < half;
                const double w = left ? double(jj) / half : double(jj - half) / (gz - half);   // 0..1 across the strip
                const double z = left ? (-Z + 0.5 * Z * w) : (0.5 * Z + 0.5 * Z * w);
                return D3{-X + 2 * X * u, y + 0.06 * std::sin(u * 40) * std::sin(w * 9), z};
            };
            if (pass) quad(P(i, j), P(i + 1, j), P(i + 1, j + 1), P(i, j + 1));
            else      quad(P(i, j), P(i, j + 1), P(i + 1, j + 1), P(i + 1, j));
        }
    }
    normalize_cube(all);
    const uint64_t nq = all.size() / 4;
    uint64_t base_tris = nq * 2;
    if (base_tris > num_tris) { err = "internal: sponza-class generator overshoot"; return false; }
    uint64_t extra = num_tris - base_tris;   // made up by splitting the first `extra` triangles at an edge midpoint (+1 each)
    for (uint64_t q = 0; q < nq; ++q) {
        const D3 p00 = all[q * 4], p10 = all[q * 4 + 1], p11 = all[q * 4 + 2], p01 = all[q * 4 + 3];
        for (int h = 0; h < 2; ++h) {
            const D3 a0 = p00, a1 = h ? p11 : p10, a2 = h ? p01 : p11;
            if (extra > 0) { const D3 m = (a0 + a1) * 0.5; tl.add(a0, m, a2); tl.add(m, a1, a2); --extra; }
            else tl.add(a0, a1, a2);
        }
    }
    if (tl.n != num_tris) { err = "internal: sponza-class generator produced a wrong triangle count"; return false; }
    return true;
}

} // namespace

bool procedural_scene(uint32_t kind, uint32_t seed, uint32_t num_tris, float* out, std::string& err) {
    if (!out) { err = "null output"; return false; }
    if (kind == 0) return dragon_class(seed, num_tris, out, err);
    if (kind == 1) return sponza_class(seed, num_tris, out, err);
    err = "unknown procedural scene kind";
    return false;
}

// ---- ambient-occlusion sample rays: the sampling functions of pt_raymath.h, the text the kernels compile ----
void occlusion_rays(const float* surfels, uint64_t n, uint32_t samples, uint32_t seed, uint32_t index_base, float bias, float* rays) {
    for (uint64_t i = 0; i < n; ++i) {
        const float* sf = surfels + i * 8;
        const float* p = sf; const float r_max = sf[3]; const float* nr = sf + 4;
        const bool traced = ptry::surfel_walked(p[0], p[1], p[2], nr[0], nr[1], nr[2], r_max);
        const uint32_t pixel = index_base + uint32_t(i);
        for (uint32_t s = 0; s < samples; ++s) {
            float* r = rays + (i * samples + s) * 8;
            if (!traced) {
                r[0] = p[0]; r[1] = p[1]; r[2] = p[2]; r[3] = 0.0f; r[4] = nr[0]; r[5] = nr[1]; r[6] = nr[2]; r[7] = 0.0f;
                continue;
            }
            const uint32_t key = ptry::sample_key(seed, pixel, s);
            const float u1 = ptry::rnd(key, 0u, 2u), u2 = ptry::rnd(key, 0u, 3u);
            float l[3];
            ptry::cosine_local(u1, u2, l[0], l[1], l[2]);
            ptry::cosine_world(nr[0], nr[1], nr[2], l[0], l[1], l[2], r[4], r[5], r[6]);
            ptry::offset_origin(p[0], p[1], p[2], nr[0], nr[1], nr[2], bias, r[0], r[1], r[2]);
            r[3] = r_max; r[7] = 0.0f;
        }
    }
}

// ------------------------------------------------------------------------------------
// Crossing counts and containment (host twin of pt_crossings.hip): the same records, operations, order, cap and counters
// ------------------------------------------------------------------------------------
namespace {
struct RayH { float o[3], d[3], inv[3]; };

// pt_device.h::slab: the min / max form of the one-ray kernels (the sign-selected form of the persistent kernels gives the same bits)
inline bool slab_h(const RayH& r, const uint32_t w[3], float best, float& tmin_out) {
    const Box b = unpack_box(w);
    float t1[3], t2[3];
    for (int k = 0; k < 3; ++k) { t1[k] = (b.mn[k] - r.o[k]) * r.inv[k]; t2[k] = (b.mx[k] - r.o[k]) * r.inv[k]; }
    const float tmin = wmax(wmax(wmin(t1[0], t2[0]), wmin(t1[1], t2[1])), wmin(t1[2], t2[2]));
    const float tmax = wmin(wmin(wmax(t1[0], t2[0]), wmax(t1[1], t2[1])), wmax(t1[2], t2[2]));
    tmin_out = tmin;
    return (tmax >= wmax(tmin, 0.0f)) && (tmin < best);
}
// ptry::tri_hit and ptry::hit_uv on a triangle record
inline bool record_hit(const RayH& r, const TriRecord& rec, float& t) {
    return ptry::tri_hit(r.o[0], r.o[1], r.o[2], r.d[0], r.d[1], r.d[2], rec.axis[0][0], rec.axis[1][0], rec.axis[2][0],
                         rec.axis[0][1], rec.axis[1][1], rec.axis[2][1], rec.axis[0][2], rec.axis[1][2], rec.axis[2][2], t);
}
inline void record_hit_uv(const RayH& r, const TriRecord& rec, float& u, float& v) {
    ptry::hit_uv(r.o[0], r.o[1], r.o[2], r.d[0], r.d[1], r.d[2], rec.axis[0][0], rec.axis[1][0], rec.axis[2][0],
                 rec.axis[0][1], rec.axis[1][1], rec.axis[2][1], rec.axis[0][2], rec.axis[1][2], rec.axis[2][2], u, v);
}
// The ray walk: walk_keys_h with the key of a child = tmin of its slab test, +inf where that test fails or the child is a degenerate or
// empty slot (reference >= kDegenerate: its inverted box would pass the min / max form, pt_device.h::kEmptyBox*).  best <= 1e30 < +inf,
// so "key < best" is "the slab test passes"; `best` never moves, and every stacked entry passes its re-validation.
template <class Leaf>
void walk_ray_h(const PointWalk& W, const RayH& r, float best, WalkCounters& cnt, Leaf leaf) {
    walk_keys_h(W, [&](const uint32_t* w, uint32_t ref) {
        float tmin;
        return (ref < kDegenerate && slab_h(r, w, best, tmin)) ? tmin : std::numeric_limits<float>::infinity();
    }, best, cnt, leaf);
}
// a PtRay record (pt_rays.h::load_ray, ray_traced): whether the ray is walked, and then `best` = min(t_max, kInfT)
inline bool load_ray_h(const float* q, RayH& r, float& best) {
    for (int k = 0; k < 3; ++k) { r.o[k] = q[k]; r.d[k] = q[4 + k]; r.inv[k] = ptry::safe_inv(q[4 + k]); }
    best = wmin(q[3], ptry::kInfT);
    return ptry::ray_walked(r.o[0], r.o[1], r.o[2], r.d[0], r.d[1], r.d[2], q[3]);
}
// every crossing of a walked ray below `best`, handed to accept(t, triangle) in visit order (or in index order with brute force)
template <class Accept>
void ray_crossings(const TwinScene& S, bool walk, const RayH& r, float best, WalkCounters& cnt, Accept accept) {
    auto leaf = [&](uint32_t tri) { float t; if (record_hit(r, S.rec[tri], t) && t < best) accept(t, tri); };
    if (walk) { walk_ray_h(S.W, r, best, cnt, leaf); return; }
    for (uint32_t t = 0; t < S.W.num_tris; ++t) leaf(t);
    cnt.tris += S.W.num_tris;
}
} // namespace

bool count_hits(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const float* rays, uint64_t n,
                uint32_t* counts, uint64_t* counters, std::string& err) {
    TwinScene S;
    if (!S.init(tris, num_tris, bvh4, words, n, err)) return false;
    S.parallel([&](uint64_t w, uint64_t first, uint64_t end) {
        WalkCounters& cnt = S.per[w];
        for (uint64_t i = first; i < end; ++i) {
            RayH r; float best;
            uint32_t count = 0;
            if (load_ray_h(rays + i * 8, r, best)) ray_crossings(S, bvh4 != nullptr, r, best, cnt, [&](float, uint32_t) { ++count; });
            counts[i] = count;
        }
    });
    S.reduce(counters, n);
    return true;
}

bool contains(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const float* points, uint64_t n,
              uint32_t samples, uint32_t seed, uint32_t index_base, uint32_t* out, uint64_t* counters, std::string& err) {
    // the surfels whose sample rays these are: {p, +inf, (0, 0, 1)}; a point with a NaN in p stays untraced (r_max = 0: rays that are not walked)
    std::vector<float> surfels(size_t(n) * 8), rays(size_t(n) * samples * 8);
    uint64_t traced = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const float* p = points + i * 4; float* sf = surfels.data() + i * 8;
        const bool ok = !(std::isnan(p[0]) || std::isnan(p[1]) || std::isnan(p[2]));
        sf[0] = p[0]; sf[1] = p[1]; sf[2] = p[2]; sf[3] = ok ? std::numeric_limits<float>::infinity() : 0.0f;
        sf[4] = 0.0f; sf[5] = 0.0f; sf[6] = 1.0f; sf[7] = 0.0f;
        traced += ok;
    }
    occlusion_rays(surfels.data(), n, samples, seed, index_base, 0.0f, rays.data());
    std::vector<uint32_t> counts(size_t(n) * samples);
    if (!count_hits(tris, num_tris, bvh4, words, rays.data(), n * samples, counts.data(), counters, err)) return false;
    if (counters) counters[0] = traced * samples;
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t* o = out + i * 4;
        if (surfels[i * 8 + 3] == 0.0f) { o[0] = o[1] = o[2] = o[3] = 0u; continue; }
        uint32_t odd = 0;
        for (uint32_t s = 0; s < samples; ++s) odd += counts[i * samples + s] & 1u;
        o[0] = 2u * odd > samples ? 1u : 0u; o[1] = odd; o[2] = samples; o[3] = 0u;
    }
    return true;
}

// ------------------------------------------------------------------------------------
// Hit lists (host twin of pt_hitlist.hip): count_hits' walk twice around a scan, the second time storing entry k of ray i at
// offsets[i] + k, then each fully stored list sorted by (t bits << 32 | prim)
// ------------------------------------------------------------------------------------
bool list_hits(const float* tris, uint32_t num_tris, const uint32_t* bvh4, uint64_t words, const float* rays, uint64_t n,
               uint64_t* offsets, uint32_t* entries, uint64_t capacity, bool sorted, uint64_t* counters, std::string& err) {
    TwinScene S;
    if (!S.init(tris, num_tris, bvh4, words, n, err)) return false;
    using Entry = std::array<uint32_t, 4>;
    std::vector<std::vector<Entry>> lists(S.workers);
    // one ray: the walk (or every triangle in index order); behind a list that was stored in full, its sort
    list_twin(S, offsets, entries, capacity, [&](uint64_t i, WalkCounters& cnt, auto accept) {
        RayH r; float best;
        if (!load_ray_h(rays + i * 8, r, best)) return;
        ray_crossings(S, bvh4 != nullptr, r, best, cnt, [&](float t, uint32_t tri) {
            accept([&](uint32_t* o) {
                float u, v; record_hit_uv(r, S.rec[tri], u, v);
                o[0] = bits_of(t); o[1] = tri; o[2] = bits_of(u); o[3] = bits_of(v);
            });
        });
    }, [&](uint64_t w, uint64_t i) {
        if (!sorted || offsets[i + 1] > capacity || offsets[i + 1] - offsets[i] <= 1u) return;
        Entry* first = reinterpret_cast<Entry*>(entries + offsets[i] * 4);
        std::vector<Entry>& list = lists[w];                    // one buffer per worker
        list.assign(first, first + (offsets[i + 1] - offsets[i]));
        std::stable_sort(list.begin(), list.end(), [](const Entry& a, const Entry& b) { return ((uint64_t(a[0]) << 32) | a[1]) < ((uint64_t(b[0]) << 32) | b[1]); });
        std::memcpy(first, list.data(), list.size() * sizeof(Entry));
    });
    S.reduce(counters, n);
    return true;
}

// ---- exposed triangles: every pair, with the arithmetic of pt_expose.h (pt_expose.hip walks the tree instead) ----
uint32_t exposure_flags(const float* tris, uint32_t num_tris, double s_max, double d_max, double gate, uint32_t* mask) {
    const uint32_t words = ((num_tris + 63u) / 64u) * 2u;
    std::memset(mask, 0, size_t(words) * sizeof(uint32_t));
    std::vector<TriRecord> rec(num_tris);
    if (num_tris) build_tri_records(tris, num_tris, rec.data());
    // the light direction as the kernels hold it (pt_device.h::light_dir: normalize3 in f32)
    const float inv = 1.0f / std::sqrt((1.0f * 1.0f + 1.5f * 1.5f) + 1.0f * 1.0f);
    const ptex::Light g = ptex::make_light(1.0f * inv, 1.5f * inv, 1.0f * inv);
    const ptex::Bounds b = {s_max, d_max};
    auto load = [&](uint32_t t) {
        ptex::Tri r;
        for (int a = 0; a < 3; ++a) { r.v0[a] = rec[t].axis[a][0]; r.e1[a] = rec[t].axis[a][1]; r.e2[a] = rec[t].axis[a][2]; }
        return r;
    };
    std::vector<ptex::Tri> all(num_tris);
    for (uint32_t t = 0; t < num_tris; ++t) all[t] = load(t);
    uint32_t flagged = 0;
    for (uint32_t t = 0; t < num_tris; ++t) {
        const float n32[3] = {rec[t].n[0], rec[t].n[1], rec[t].n[2]};
        const ptex::Query q = ptex::make_query(all[t], n32, g, b, gate);
        bool blocked = !q.ok;
        for (uint32_t n = 0; n < num_tris && !blocked; ++n) blocked = ptex::blocks(q, all[n], g);
        if (!blocked) { mask[t >> 5] |= 1u << (t & 31u); ++flagged; }
    }
    return flagged;
}

} // namespace pt
