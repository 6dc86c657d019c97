// knn_sanitize.cpp -- the host twin of the k-nearest queries (pt_host.cpp::nearest_k, no HIP, no oracle) under AddressSanitizer + UBSan:
// the tetra (k beyond the number of triangles: padded rows) and a 1000-triangle soup under a PLOC tree, the walk and brute force, for
// k = 1, 5 and 64, with output buffers of exactly n * k records so that a store past them is a heap overflow.
// Built and run by tests/test_knn_sanitizers.py (CPU only).
#include "../../raytracer-public_amd/csrc/pt_host.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

static int fails = 0;
#define CHECK(c, what) do { if (!(c)) { std::printf("FAIL %s (line %d)\n", what, __LINE__); ++fails; } } while (0)

static const uint32_t kInf = 0x7F800000u, kNone = 0xFFFFFFFFu;

// rows of exactly n * k records: ascending dist, padding whole and last, walk and brute force agree on the dist bits
static void run(const std::vector<float>& tris, uint32_t n_tris, const std::vector<uint32_t>& bvh4, const std::vector<float>& pts, uint32_t n_pts,
                const std::vector<uint32_t>& unwalked) {
    std::string err;
    for (uint32_t k : {1u, 5u, 64u}) {
        std::vector<uint32_t> walk(size_t(n_pts) * k * 4, 0xA5A5A5A5u), brute(size_t(n_pts) * k * 4, 0xA5A5A5A5u);
        uint64_t counters[5] = {0, 0, 0, 0, 0};
        CHECK(pt::nearest_k(tris.data(), n_tris, bvh4.data(), bvh4.size(), pts.data(), n_pts, k, walk.data(), counters, err), "walk");
        CHECK(counters[0] == n_pts && counters[3] == 0, "counters");
        CHECK(pt::nearest_k(tris.data(), n_tris, nullptr, 0, pts.data(), n_pts, k, brute.data(), nullptr, err), "brute force");
        for (uint32_t i = 0; i < n_pts; ++i) {
            bool padded = false;
            for (uint32_t j = 0; j < k; ++j) {
                const uint32_t* w = &walk[(size_t(i) * k + j) * 4]; const uint32_t* b = &brute[(size_t(i) * k + j) * 4];
                CHECK(w[0] == b[0], "dist bits of the walk and of brute force");
                if (w[1] == kNone) { padded = true; CHECK(w[0] == kInf && w[2] == 0 && w[3] == 0, "padding record"); }
                else {
                    CHECK(!padded && w[1] < n_tris, "a listed entry behind the padding");
                    if (j) CHECK(w[-4] <= w[0], "ascending dist");       // bits of non-negative floats order as integers
                }
            }
            if (k > n_tris) CHECK(walk[(size_t(i) * k + n_tris) * 4 + 1] == kNone, "k beyond the number of triangles: a padded tail");
        }
        for (uint32_t i : unwalked) for (uint32_t j = 0; j < k; ++j) CHECK(walk[(size_t(i) * k + j) * 4 + 1] == kNone && brute[(size_t(i) * k + j) * 4 + 1] == kNone, "a point that is not walked");
    }
}

int main() {
    std::mt19937 rng(3);
    std::uniform_real_distribution<float> U(-1.f, 1.f);
    std::string err;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();

    // the tetra (the reference's default mesh): 4 triangles
    const std::vector<float> tetra = {0, 1, 0, -1, -1, 1, 1, -1, 1,   0, 1, 0, 1, -1, 1, 0, -1, -1,   0, 1, 0, 0, -1, -1, -1, -1, 1,   -1, -1, 1, 0, -1, -1, 1, -1, 1};
    std::vector<uint32_t> t2, t4;
    CHECK(pt::build_bvh2_ploc(tetra.data(), 4, t2, err), "PLOC BVH2 of the tetra");
    CHECK(pt::collapse_to_bvh4(t2.data(), 4, true, t4, err), "collapse of the tetra");
    std::vector<float> tp(size_t(64) * 4);
    for (uint32_t i = 0; i < 64; ++i) { for (int c = 0; c < 3; ++c) tp[size_t(i) * 4 + c] = 2.0f * U(rng); tp[size_t(i) * 4 + 3] = (i & 1) ? inf : 1.0f; }
    tp[4 * 5 + 3] = 0.0f; tp[4 * 6 + 3] = -1.0f; tp[4 * 7 + 3] = nan; tp[4 * 8 + 1] = nan;
    run(tetra, 4, t4, tp, 64, {5, 6, 7, 8});

    // soup1k
    const uint32_t n_tris = 1000, n_pts = 1024;
    std::vector<float> tris(size_t(n_tris) * 9);
    for (uint32_t t = 0; t < n_tris; ++t) {
        const float c[3] = {U(rng), U(rng), U(rng)};
        for (int v = 0; v < 3; ++v) for (int k = 0; k < 3; ++k) tris[size_t(t) * 9 + v * 3 + k] = c[k] + 0.15f * U(rng);
    }
    std::vector<uint32_t> bvh2, bvh4;
    CHECK(pt::build_bvh2_ploc(tris.data(), n_tris, bvh2, err), "PLOC BVH2");
    CHECK(pt::collapse_to_bvh4(bvh2.data(), n_tris, true, bvh4, err), "area-guided collapse");
    std::vector<float> pts(size_t(n_pts) * 4);
    for (uint32_t i = 0; i < n_pts; ++i) {
        for (int k = 0; k < 3; ++k) pts[size_t(i) * 4 + k] = 1.5f * U(rng);
        pts[size_t(i) * 4 + 3] = (i & 1) ? inf : 0.02f + 0.09f * (U(rng) + 1.0f);
    }
    pts[4 * 5 + 3] = 0.0f; pts[4 * 6 + 3] = -1.0f; pts[4 * 7 + 3] = nan; pts[4 * 8 + 1] = nan;
    run(tris, n_tris, bvh4, pts, n_pts, {5, 6, 7, 8});

    // k out of range and a malformed tree are rejected, not read or written out of bounds; an empty batch writes nothing
    std::vector<uint32_t> one(4, 0xA5A5A5A5u);
    CHECK(!pt::nearest_k(tris.data(), n_tris, bvh4.data(), bvh4.size(), pts.data(), 1, 0, one.data(), nullptr, err), "k = 0 rejected");
    CHECK(!pt::nearest_k(tris.data(), n_tris, bvh4.data(), bvh4.size(), pts.data(), 1, 65, one.data(), nullptr, err), "k = 65 rejected");
    CHECK(!pt::nearest_k(tris.data(), n_tris, bvh4.data(), bvh4.size() - 9, pts.data(), 1, 1, one.data(), nullptr, err), "short buffer rejected");
    CHECK(pt::nearest_k(tris.data(), n_tris, bvh4.data(), bvh4.size(), pts.data(), 0, 5, nullptr, nullptr, err), "empty batch");
    CHECK(one[0] == 0xA5A5A5A5u && one[3] == 0xA5A5A5A5u, "nothing written by the rejected calls");
    std::printf(fails ? "%d failures\n" : "knn_sanitize ok\n", fails);
    return fails ? 1 : 0;
}
