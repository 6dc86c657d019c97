// tri_sanitize.cpp -- the host twin of the triangle-overlap queries (pt_host.cpp::tri_search, no HIP, no oracle) under AddressSanitizer +
// UBSan: a 1000-triangle soup under a PLOC tree, the walk and brute force, each at the capacities 0 (no entry buffer), total - 1, total and
// total + 7, with entry buffers of exactly the capacity so that a store past it is a heap overflow.
// Built and run by tests/test_tri_sanitizers.py (CPU only).
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
    const uint32_t n_tris = 1000, n_callers = 1024;
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
    std::vector<float> callers(size_t(n_callers) * 12, 0.0f);
    for (uint32_t i = 0; i < n_callers; ++i) {
        const float c[3] = {1.2f * U(rng), 1.2f * U(rng), 1.2f * U(rng)};
        for (int v = 0; v < 3; ++v) for (int k = 0; k < 3; ++k) callers[size_t(i) * 12 + v * 4 + k] = c[k] + 0.3f * U(rng);
    }
    // caller triangles that are not walked, a point, and one that spans everything
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    callers[12 * 5 + 0] = nan; callers[12 * 6 + 5] = nan; callers[12 * 7 + 1] = -inf; callers[12 * 8 + 10] = inf;
    for (int w = 0; w < 12; ++w) callers[12 * 9 + w] = 0.25f;
    const float span[12] = {-3.f, -3.f, -3.f, nan, 5.f, -3.f, 3.f, inf, -3.f, 5.f, 3.f, -inf};          // (the pads are ignored)
    std::memcpy(&callers[12 * 10], span, sizeof(span));

    for (int brute = 0; brute < 2; ++brute) {
        const uint32_t* tree = brute ? nullptr : bvh4.data();
        const uint64_t words = brute ? 0 : bvh4.size();
        std::vector<uint64_t> off0(n_callers + 1, ~0ull);
        uint64_t counters[5] = {0, 0, 0, 0, 0};
        CHECK(pt::tri_search(tris.data(), n_tris, tree, words, callers.data(), n_callers, off0.data(), nullptr, 0, counters, err), "offsets only");
        const uint64_t total = off0[n_callers];
        CHECK(off0[0] == 0 && total > 100 && counters[0] == n_callers && counters[3] == 0, "offsets and counters");
        CHECK(off0[6] == off0[5] && off0[7] == off0[6] && off0[8] == off0[7] && off0[9] == off0[8] && off0[10] == off0[9] && off0[11] - off0[10] > 16,
              "triangles that are not walked, the point and the spanning triangle");
        std::vector<uint32_t> full(size_t(total) * 4);
        std::vector<uint64_t> off(n_callers + 1);
        CHECK(pt::tri_search(tris.data(), n_tris, tree, words, callers.data(), n_callers, off.data(), full.data(), total, nullptr, err) && off == off0, "capacity = total");
        for (uint64_t e = 0; e < total; ++e) if (full[e * 4] >= n_tris || full[e * 4 + 1] == 0u || full[e * 4 + 1] > 63u || full[e * 4 + 2] || full[e * 4 + 3]) { CHECK(false, "entry words"); break; }
        for (uint64_t cap : {total - 1, total + 7}) {
            std::vector<uint32_t> ent(size_t(cap) * 4, 0xA5A5A5A5u);
            CHECK(pt::tri_search(tris.data(), n_tris, tree, words, callers.data(), n_callers, off.data(), ent.data(), cap, nullptr, err) && off == off0, "truncated / roomy");
            const uint64_t held = cap < total ? cap : total;
            CHECK(std::memcmp(ent.data(), full.data(), size_t(held) * 16) == 0, "entries below min(total, capacity)");
            for (size_t w = size_t(held) * 4; w < ent.size(); ++w) if (ent[w] != 0xA5A5A5A5u) { CHECK(false, "guard behind the entries"); break; }
        }
    }
    // a malformed tree is rejected, not read out of bounds
    std::vector<uint64_t> off(n_callers + 1);
    CHECK(!pt::tri_search(tris.data(), n_tris, bvh4.data(), bvh4.size() - 9, callers.data(), n_callers, off.data(), nullptr, 0, nullptr, err), "short buffer rejected");
    CHECK(pt::tri_search(tris.data(), n_tris, bvh4.data(), bvh4.size(), callers.data(), 0, off.data(), nullptr, 0, nullptr, err) && off[0] == 0, "empty batch");
    std::printf(fails ? "%d failures\n" : "tri_sanitize ok\n", fails);
    return fails ? 1 : 0;
}
