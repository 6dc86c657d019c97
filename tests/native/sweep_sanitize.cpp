// sweep_sanitize.cpp -- the host twin of the sphere-cast queries (pt_host.cpp::sweep_spheres, no HIP, no oracle) under AddressSanitizer +
// UBSan: a 1000-triangle soup under a PLOC tree, the walk and brute force over 1024 sweeps (enough for four workers), with an output
// buffer of exactly n records so that a store past it is a heap overflow; the items that are not walked, a sphere that holds everything,
// a malformed tree and an empty batch.
// Built and run by tests/test_sweep_sanitizers.py (CPU only).
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

int main() {
    const uint32_t n_tris = 1000, n = 1024;
    std::mt19937 rng(3);
    std::uniform_real_distribution<float> U(-1.f, 1.f);
    std::vector<float> tris(size_t(n_tris) * 9);
    for (uint32_t t = 0; t < n_tris; ++t) {
        const float c[3] = {U(rng), U(rng), U(rng)};
        for (int v = 0; v < 3; ++v) for (int k = 0; k < 3; ++k) tris[size_t(t) * 9 + v * 3 + k] = c[k] + 0.15f * U(rng);
    }
    std::string err;
    std::vector<uint32_t> bvh2, bvh4;
    CHECK(pt::build_bvh2_ploc(tris.data(), n_tris, bvh2, err), "PLOC BVH2");
    CHECK(pt::collapse_to_bvh4(bvh2.data(), n_tris, true, bvh4, err), "area-guided collapse");
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::vector<float> sw(size_t(n) * 8);
    for (uint32_t i = 0; i < n; ++i) {
        float* q = &sw[size_t(i) * 8];
        for (int k = 0; k < 3; ++k) { q[k] = 1.8f * U(rng); q[4 + k] = 0.7f * U(rng) - q[k]; }
        q[3] = (i % 4 == 3) ? 1.0f : inf;
        q[7] = 0.05f * float(i % 4);
    }
    sw[8 * 5 + 0] = nan; sw[8 * 6 + 5] = nan; sw[8 * 7 + 3] = 0.0f; sw[8 * 8 + 7] = -1.0f; sw[8 * 9 + 7] = nan;
    sw[8 * 10 + 4] = sw[8 * 10 + 5] = sw[8 * 10 + 6] = 0.0f;                             // not walked
    sw[8 * 11 + 7] = 8.0f; sw[8 * 11 + 3] = inf;                                          // holds the whole soup at the start
    sw[8 * 12 + 4] = inf;                                                                 // an infinite direction: walked, whatever it finds

    std::vector<uint32_t> walk(size_t(n) * 4), brute(size_t(n) * 4);
    uint64_t cw[5] = {0, 0, 0, 0, 0}, cb[5] = {0, 0, 0, 0, 0};
    CHECK(pt::sweep_spheres(tris.data(), n_tris, bvh4.data(), bvh4.size(), sw.data(), n, walk.data(), cw, err), "walk");
    CHECK(pt::sweep_spheres(tris.data(), n_tris, nullptr, 0, sw.data(), n, brute.data(), cb, err), "brute force");
    CHECK(cw[0] == n && cb[0] == n && cw[3] == 0 && cw[4] >= 1 && cw[4] <= 64 && cb[1] == 0 && cb[2] == uint64_t(n - 6) * n_tris, "counters");
    uint32_t hits = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (i == 12) continue;
        CHECK(walk[i * 4] == brute[i * 4], "walk = brute force on t");
        // several triangles may share the first contact time (all that overlap at the start do): u, v belong to prim
        CHECK(walk[i * 4 + 1] != brute[i * 4 + 1] || (walk[i * 4 + 2] == brute[i * 4 + 2] && walk[i * 4 + 3] == brute[i * 4 + 3]), "the same prim: the same u, v");
        CHECK((walk[i * 4 + 1] == 0xFFFFFFFFu) == (walk[i * 4] == 0x7F800000u) && (walk[i * 4 + 1] == 0xFFFFFFFFu || walk[i * 4 + 1] < n_tris), "prim");
        hits += walk[i * 4 + 1] != 0xFFFFFFFFu;
    }
    CHECK(hits > n / 4, "hits");
    for (uint32_t i = 5; i <= 10; ++i) CHECK(walk[i * 4] == 0x7F800000u && walk[i * 4 + 1] == 0xFFFFFFFFu && !walk[i * 4 + 2] && !walk[i * 4 + 3], "items that are not walked");
    CHECK(walk[11 * 4] == 0u && walk[11 * 4 + 1] < n_tris, "a sphere that holds everything: t = 0");
    // a malformed tree is rejected, not read out of bounds
    CHECK(!pt::sweep_spheres(tris.data(), n_tris, bvh4.data(), bvh4.size() - 9, sw.data(), n, walk.data(), nullptr, err), "short buffer rejected");
    CHECK(pt::sweep_spheres(tris.data(), n_tris, bvh4.data(), bvh4.size(), sw.data(), 0, nullptr, nullptr, err), "empty batch");
    std::printf(fails ? "%d failures\n" : "sweep_sanitize ok\n", fails);
    return fails ? 1 : 0;
}
