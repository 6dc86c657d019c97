// cut_sanitize.cpp -- the host twin of the plane-cut queries (pt_host.cpp::cut_search, no HIP, no oracle) under AddressSanitizer + UBSan:
// a 1000-triangle soup under a PLOC tree, the walk and brute force, each at the capacities 0 (no entry buffer), total - 1, total and
// total + 7, with entry buffers of exactly the capacity so that a store past it is a heap overflow.
// Built and run by tests/test_cut_sanitizers.py (CPU only).
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
    const uint32_t n_tris = 1000, n_planes = 1024;
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
    // records: (n.xyz, d, lo.xyz, pad, hi.xyz, pad); a plane through a point p of the scene with a window of half-size 0.4 around it
    std::vector<float> planes(size_t(n_planes) * 12, 0.0f);
    for (uint32_t i = 0; i < n_planes; ++i) {
        float* q = &planes[size_t(i) * 12];
        const float p[3] = {U(rng), U(rng), U(rng)};
        for (int k = 0; k < 3; ++k) { q[k] = U(rng); q[4 + k] = p[k] - 0.4f; q[8 + k] = p[k] + 0.4f; }
        q[3] = q[0] * p[0] + q[1] * p[1] + q[2] * p[2];
    }
    // records that are not walked, a zero-extent window, and one plane with a window that holds everything
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    planes[12 * 5 + 0] = nan; planes[12 * 6 + 3] = inf; planes[12 * 7 + 5] = -inf; planes[12 * 8 + 10] = nan;
    planes[12 * 9 + 0] = planes[12 * 9 + 1] = planes[12 * 9 + 2] = 0.0f;
    for (int k = 0; k < 3; ++k) planes[12 * 10 + 8 + k] = planes[12 * 10 + 4 + k] = 3.0f;
    const float span[12] = {0.3f, 0.5f, 0.9f, 0.0f, -3.f, -3.f, -3.f, nan, 3.f, 3.f, 3.f, -inf};          // (the pads are ignored)
    std::memcpy(&planes[12 * 11], span, sizeof(span));

    for (int brute = 0; brute < 2; ++brute) {
        const uint32_t* tree = brute ? nullptr : bvh4.data();
        const uint64_t words = brute ? 0 : bvh4.size();
        std::vector<uint64_t> off0(n_planes + 1, ~0ull);
        uint64_t counters[5] = {0, 0, 0, 0, 0};
        CHECK(pt::cut_search(tris.data(), n_tris, tree, words, planes.data(), n_planes, off0.data(), nullptr, 0, counters, err), "offsets only");
        const uint64_t total = off0[n_planes];
        CHECK(off0[0] == 0 && total > 100 && counters[0] == n_planes && counters[3] == 0, "offsets and counters");
        CHECK(off0[6] == off0[5] && off0[7] == off0[6] && off0[8] == off0[7] && off0[9] == off0[8] && off0[10] == off0[9] && off0[11] == off0[10] &&
              off0[12] - off0[11] > 16, "records that are not walked, the zero-extent window and the spanning window");
        std::vector<uint32_t> full(size_t(total) * 4);
        std::vector<uint64_t> off(n_planes + 1);
        CHECK(pt::cut_search(tris.data(), n_tris, tree, words, planes.data(), n_planes, off.data(), full.data(), total, nullptr, err) && off == off0, "capacity = total");
        for (uint64_t e = 0; e < total; ++e) {
            float t0, t1;
            std::memcpy(&t0, &full[e * 4 + 2], 4); std::memcpy(&t1, &full[e * 4 + 3], 4);
            const uint32_t edges = full[e * 4 + 1] & 7u;
            if (full[e * 4] >= n_tris || full[e * 4 + 1] > 63u || !(edges == 3u || edges == 5u || edges == 6u) || !(t0 >= 0.0f && t0 <= 1.0f) || !(t1 >= 0.0f && t1 <= 1.0f)) {
                CHECK(false, "entry words"); break;
            }
        }
        for (uint64_t cap : {total - 1, total + 7}) {
            std::vector<uint32_t> ent(size_t(cap) * 4, 0xA5A5A5A5u);
            CHECK(pt::cut_search(tris.data(), n_tris, tree, words, planes.data(), n_planes, off.data(), ent.data(), cap, nullptr, err) && off == off0, "truncated / roomy");
            const uint64_t held = cap < total ? cap : total;
            CHECK(std::memcmp(ent.data(), full.data(), size_t(held) * 16) == 0, "entries below min(total, capacity)");
            for (size_t w = size_t(held) * 4; w < ent.size(); ++w) if (ent[w] != 0xA5A5A5A5u) { CHECK(false, "guard behind the entries"); break; }
        }
    }
    // a malformed tree is rejected, not read out of bounds
    std::vector<uint64_t> off(n_planes + 1);
    CHECK(!pt::cut_search(tris.data(), n_tris, bvh4.data(), bvh4.size() - 9, planes.data(), n_planes, off.data(), nullptr, 0, nullptr, err), "short buffer rejected");
    CHECK(pt::cut_search(tris.data(), n_tris, bvh4.data(), bvh4.size(), planes.data(), 0, off.data(), nullptr, 0, nullptr, err) && off[0] == 0, "empty batch");
    std::printf(fails ? "%d failures\n" : "cut_sanitize ok\n", fails);
    return fails ? 1 : 0;
}
