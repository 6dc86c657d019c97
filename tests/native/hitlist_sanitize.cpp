// hitlist_sanitize.cpp -- the host twin of the hit lists (pt_host.cpp::list_hits, no HIP, no oracle) under AddressSanitizer + UBSan: a deck
// of 300 parallel quads in shuffled order and a 1000-triangle soup, each under a PLOC tree, the walk and brute force, unsorted and sorted,
// each at the capacities 0 (no entry buffer), 1, total - 1, total and total + 7, with entry buffers of exactly the capacity so that a store
// past it is a heap overflow.
// Built and run by tests/test_hitlist_sanitizers.py (CPU only).
#include "../../raytracer-public_amd/csrc/pt_host.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <random>
#include <string>
#include <vector>

static int fails = 0;
#define CHECK(c, what) do { if (!(c)) { std::printf("FAIL %s (line %d)\n", what, __LINE__); ++fails; } } while (0)

static uint64_t key_of(const uint32_t* e) { return (uint64_t(e[0]) << 32) | e[1]; }

static void run(const std::vector<float>& tris, const std::vector<float>& rays, uint64_t want_per_ray) {
    const uint32_t n_tris = uint32_t(tris.size() / 9);
    const uint64_t n = rays.size() / 8;
    std::string err;
    std::vector<uint32_t> bvh2, bvh4;
    CHECK(pt::build_bvh2_ploc(tris.data(), n_tris, bvh2, err), "PLOC BVH2");
    CHECK(pt::collapse_to_bvh4(bvh2.data(), n_tris, true, bvh4, err), "area-guided collapse");
    for (int brute = 0; brute < 2; ++brute) {
        const uint32_t* tree = brute ? nullptr : bvh4.data();
        const uint64_t words = brute ? 0 : bvh4.size();
        std::vector<uint64_t> off0(n + 1, ~0ull), off(n + 1);
        uint64_t counters[5] = {0, 0, 0, 0, 0};
        CHECK(pt::list_hits(tris.data(), n_tris, tree, words, rays.data(), n, off0.data(), nullptr, 0, true, counters, err), "offsets only");
        const uint64_t total = off0[n];
        CHECK(off0[0] == 0 && total > 8 && counters[0] == n && counters[3] == 0, "offsets and counters");
        CHECK(off0[1] == 0 && off0[2] == 0 && off0[3] == 0, "rays that are not walked");
        if (want_per_ray) CHECK(off0[5] - off0[4] == want_per_ray, "every layer of the deck");
        std::vector<uint32_t> counts(n);
        CHECK(pt::count_hits(tris.data(), n_tris, tree, words, rays.data(), n, counts.data(), nullptr, err), "count_hits");
        for (uint64_t i = 0; i < n; ++i) if (off0[i + 1] - off0[i] != counts[i]) { CHECK(false, "list lengths are the crossing counts"); break; }
        std::vector<uint32_t> full(size_t(total) * 4);
        CHECK(pt::list_hits(tris.data(), n_tris, tree, words, rays.data(), n, off.data(), full.data(), total, false, nullptr, err) && off == off0, "capacity = total");
        for (int sorted = 0; sorted < 2; ++sorted)
            for (uint64_t cap : {uint64_t(1), total - 1, total, total + 7}) {
                std::vector<uint32_t> ent(size_t(cap) * 4, 0xA5A5A5A5u);
                CHECK(pt::list_hits(tris.data(), n_tris, tree, words, rays.data(), n, off.data(), ent.data(), cap, sorted != 0, nullptr, err) && off == off0, "truncated / roomy");
                const uint64_t held = cap < total ? cap : total;
                // what must be there: the visit-order entries, every list that ends at or below the capacity sorted by its key
                std::vector<uint32_t> want(full.begin(), full.begin() + size_t(held) * 4);
                if (sorted)
                    for (uint64_t i = 0; i < n; ++i) {
                        if (off0[i + 1] > held) break;
                        std::vector<uint64_t> order(off0[i + 1] - off0[i]);
                        std::iota(order.begin(), order.end(), off0[i]);
                        std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return key_of(&full[a * 4]) < key_of(&full[b * 4]); });
                        for (size_t k = 0; k < order.size(); ++k) std::memcpy(&want[(off0[i] + k) * 4], &full[order[k] * 4], 16);
                    }
                CHECK(std::memcmp(ent.data(), want.data(), size_t(held) * 16) == 0, "entries below min(total, capacity)");
                for (size_t w = size_t(held) * 4; w < ent.size(); ++w) if (ent[w] != 0xA5A5A5A5u) { CHECK(false, "guard behind the entries"); break; }
            }
    }
    std::vector<uint64_t> off(n + 1);
    CHECK(!pt::list_hits(tris.data(), n_tris, bvh4.data(), bvh4.size() - 9, rays.data(), n, off.data(), nullptr, 0, false, nullptr, err), "short buffer rejected");
    CHECK(pt::list_hits(tris.data(), n_tris, bvh4.data(), bvh4.size(), rays.data(), 0, off.data(), nullptr, 0, true, nullptr, err) && off[0] == 0, "empty batch");
}

int main() {
    std::mt19937 rng(3);
    std::uniform_real_distribution<float> U(-1.f, 1.f);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // rays 0 .. 2 of either set are not walked: t_max = 0, a NaN direction, a NaN t_max
    auto spoil = [&](std::vector<float>& rays) { rays[3] = 0.0f; rays[8 + 5] = nan; rays[16 + 3] = nan; };
    {
        const uint32_t layers = 300, n_rays = 512;
        std::vector<uint32_t> order(layers);
        std::iota(order.begin(), order.end(), 0u);
        std::shuffle(order.begin(), order.end(), rng);
        std::vector<float> tris;
        for (uint32_t k = 0; k < layers; ++k) {
            const float z = -2.0f + 4.0f * float(order[k]) / float(layers - 1);
            const float q[6][3] = {{-.5f, -.5f, z}, {.5f, -.5f, z}, {.5f, .5f, z}, {-.5f, -.5f, z}, {.5f, .5f, z}, {-.5f, .5f, z}};
            for (auto& v : q) tris.insert(tris.end(), v, v + 3);
        }
        std::vector<float> rays(size_t(n_rays) * 8, 0.0f);
        for (uint32_t i = 0; i < n_rays; ++i) {
            float x, y;
            do { x = 0.45f * U(rng); y = 0.45f * U(rng); } while (std::fabs(x - y) < 0.08f);
            float* r = &rays[size_t(i) * 8];
            r[0] = x; r[1] = y; r[2] = 3.0f; r[3] = (i % 3 == 2) ? 1.0f + 0.013f * float(i) : inf; r[6] = -1.0f;
        }
        spoil(rays);
        run(tris, rays, layers);
    }
    {
        const uint32_t n_tris = 1000, n_rays = 1024;
        std::vector<float> tris(size_t(n_tris) * 9);
        for (uint32_t t = 0; t < n_tris; ++t) {
            const float c[3] = {U(rng), U(rng), U(rng)};
            for (int v = 0; v < 3; ++v) for (int k = 0; k < 3; ++k) tris[size_t(t) * 9 + v * 3 + k] = c[k] + 0.15f * U(rng);
        }
        std::vector<float> rays(size_t(n_rays) * 8, 0.0f);
        for (uint32_t i = 0; i < n_rays; ++i) {
            float* r = &rays[size_t(i) * 8];
            for (int k = 0; k < 3; ++k) { r[k] = 1.5f * U(rng); r[4 + k] = U(rng) - r[k]; }
            r[3] = (i % 4 == 3) ? 1.0f : inf;
        }
        spoil(rays);
        run(tris, rays, 0);
    }
    std::printf(fails ? "%d failures\n" : "hitlist_sanitize ok\n", fails);
    return fails ? 1 : 0;
}
