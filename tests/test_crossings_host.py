"""Crossing counts and containment on the CPU: the host twins pt_count_hits_bvh4 and pt_contains_bvh4 (include/mi355pt.h, DESIGN.md
section 17) against a float32 restatement of the triangle test summed over all triangles, the tree walk against brute force (both on the
twin), the stack cap on the comb, containment against the float64 winding number (tests/crossref.py), the composition pt_contains is
specified as, and the error codes.  The GPU tests (tests/test_gpu_crossings.py) pin the kernels to these twins bit for bit.

Measured here (and written into DESIGN.md section 17): rays whose walk count differs from the brute-force count: 0 of 72,000 (6 scenes x
4 trees x 3,000 rays); single containment rays whose parity disagrees with the winding number: 0 of 35,994 (3 closed scenes x 3 rays x
the kept points of 4,000); points dropped as nearer than 1e-4 to the surface: 2 of 12,000."""
import numpy as np
import pytest

import closestref
import crossing_cases as cc
import crossref

N_RAYS = 3000
PT_ERR_BAD_BVH = 5                                # include/mi355pt.h PtStatus


@pytest.fixture(scope="module")
def cases(rt):
    """name -> (triangles, rays, float32 restatement of the brute-force counts): computed once, never written to."""
    memo = {}

    def get(name):
        if name not in memo:
            tris = cc.geometry(rt, name)
            rays = cc.ray_set(rt, tris, N_RAYS, 11)
            memo[name] = (tris, rays, crossref.crossings(rays, tris))
        return memo[name]
    return get


@pytest.mark.parametrize("name", cc.SCENES)
def test_brute_force_twin_equals_the_float32_restatement(rt, cases, name):
    tris, rays, ref = cases(name)
    got, st = rt.count_hits_bvh4(tris, None, rays, brute_force=True, stats=True)
    assert got.dtype == np.uint32 and np.array_equal(got, ref), np.flatnonzero(got != ref)[:10]
    walked = crossref.ray_walked(rays)
    assert walked.all() and ref.max() >= 2 and (ref == 0).any()          # the set sees misses and more than one surface
    assert st == dict(rays_closest=len(rays), rays_shadow=0, nodes_examined=0, tris_tested=int(walked.sum()) * (tris.size // 9),
                      stack_drops=0, max_stack=0, samples=0)


@pytest.mark.parametrize("name", cc.SCENES)
def test_walk_against_brute_force_on_every_tree(rt, orc, cases, name):
    base, _, _ = cases(name)
    differing = total = 0
    for label, tris, b4 in cc.forest(rt, orc, base):
        rays = cc.ray_set(rt, tris, N_RAYS, 11)
        brute = rt.count_hits_bvh4(tris, None, rays, brute_force=True)
        walk, st = rt.count_hits_bvh4(tris, b4, rays, stats=True)
        assert st["stack_drops"] == 0 and st["rays_closest"] == len(rays) and 1 <= st["max_stack"] <= 64, (label, st)
        assert st["tris_tested"] >= int(walk.sum()), (label, st)
        assert np.all(walk <= brute), (label, np.flatnonzero(walk > brute)[:10])
        bad = np.flatnonzero(walk != brute)
        for i in bad:           # a crossing lost to a box: the ray and the triangle whose leaf the ray's slab tests do not reach
            lost = [(int(t), crossref.reaches(b4, rays[i], int(t))) for t in crossref.crossed_triangles(rays[i], tris)]
            print("%s %s: ray %d %s walk %d brute %d; crossed triangles (reached, failing node): %s"
                  % (name, label, i, rays[i].tolist(), walk[i], brute[i], [l for l in lost if not l[1][0]]))
        differing += len(bad); total += len(rays)
    print("%s: %d of %d rays differ between walk and brute force" % (name, differing, total))
    assert differing * 10000 <= total, (name, differing, total)


def test_comb_drops_pushes_and_still_agrees_with_any_hit(rt, orc):
    tris, b4 = cc.geometry(rt, "comb"), cc.comb_tree()
    rays = cc.comb_rays(rt, 512, 3)
    walk, st = rt.count_hits_bvh4(tris, b4, rays, stats=True)
    brute = rt.count_hits_bvh4(tris, None, rays, brute_force=True)
    print("comb: counters %s; walk counts %d..%d, brute-force counts %d..%d" % (st, walk.min(), walk.max(), brute.min(), brute.max()))
    assert st["stack_drops"] > 0 and st["max_stack"] == 64
    assert np.all(walk <= brute) and np.any(walk < brute)                 # each triangle sits in one leaf; what is dropped is not counted
    # fact 1: count >= 1 exactly when the any-hit walk reports a hit (the oracle's orc_trace_ray(anyhit = 1) is its pinned statement)
    hit = np.array([orc.trace_ray(tris, b4, r[0:3], r[4:7], anyhit=True)[0] for r in rays])
    assert np.array_equal(walk >= 1, hit) and hit.any()
    # ... and on rays that miss the comb altogether
    away = rays.copy(); away[:, 6] = 1.0
    assert not rt.count_hits_bvh4(tris, b4, away).any()


@pytest.mark.parametrize("name", ["soup1k", "torus"])
def test_fact_one_against_the_oracle_on_ordinary_trees(rt, orc, cases, name):
    tris, rays, _ = cases(name)
    b4 = cc.host_trees(rt, orc, tris, 0)[1]
    sub = rays[np.isinf(rays[:, 3])][:600]                                # orc_trace_ray has no t_max
    walk = rt.count_hits_bvh4(tris, b4, sub)
    hit = np.array([orc.trace_ray(tris, b4, r[0:3], r[4:7], anyhit=True)[0] for r in sub])
    assert np.array_equal(walk >= 1, hit) and hit.any() and not hit.all()


@pytest.mark.parametrize("name", cc.CLOSED)
def test_containment_against_the_float64_winding_number(rt, orc, name):
    tris = cc.geometry(rt, name)
    b4 = cc.host_trees(rt, orc, tris, 0)[1]
    pts = cc.cube_points(4000, 21)
    samples = 3
    w = crossref.winding_number(pts, tris)
    inside_ref = np.abs(w) > 0.5
    keep = closestref.nearest(pts, tris)[0] >= 1e-4
    assert (~keep).sum() * 100 <= len(pts), (~keep).sum()
    assert np.all(np.abs(np.abs(w[keep]) - inside_ref[keep]) < 1e-6)       # a closed mesh: the winding number is an integer, 0 or +-1
    inside, odd, smp = rt.contains_bvh4(tris, b4, pts, samples=samples, seed=5)
    assert np.array_equal(smp, np.full(len(pts), samples, np.uint32))
    rays = cc.containment_rays(rt, pts, samples, seed=5)
    parity = (rt.count_hits_bvh4(tris, b4, rays) & 1).reshape(len(pts), samples).astype(bool)
    wrong = int((parity[keep] != inside_ref[keep][:, None]).sum())
    print("%s: %d of %d points dropped (closer than 1e-4); %d of %d single rays disagree with the winding number; %d inside"
          % (name, (~keep).sum(), len(pts), wrong, keep.sum() * samples, inside_ref[keep].sum()))
    assert inside_ref[keep].any() and not inside_ref[keep].all()
    assert np.array_equal(inside[keep].astype(bool), inside_ref[keep]), np.flatnonzero(keep & (inside.astype(bool) != inside_ref))[:10]
    assert wrong * 1000 <= keep.sum() * samples, wrong


@pytest.mark.parametrize("samples", [1, 3, 7])
def test_contains_is_the_composition(rt, orc, samples):
    tris = cc.geometry(rt, "torus")
    b4 = cc.host_trees(rt, orc, tris, 2)[1]
    pts = cc.cube_points(1500, 4, half=1.0)
    pts[7, 1] = np.nan                                                     # not traced: {0, 0, 0, 0}
    for seed, base in ((0, 0), (9, 4294966500)):                           # index_base + i wraps mod 2^32
        got = rt.contains_bvh4(tris, b4, pts, samples=samples, seed=seed, index_base=base, stats=True)
        rays = cc.containment_rays(rt, pts, samples, seed=seed, index_base=base)
        counts, st = rt.count_hits_bvh4(tris, b4, rays, stats=True)
        want = [a.copy() for a in cc.compose_contains(counts, len(pts), samples)]
        for a in want:
            a[7] = 0
        assert all(np.array_equal(g, w) for g, w in zip(got[:3], want))
        st["rays_closest"] = (len(pts) - 1) * samples                      # the rays of the traced points
        assert got[3] == st
        assert 0 < got[0].sum() < len(pts)
        # r_max of a PtPoint record is ignored
        rec = rt.pack_points(pts, 0.0)
        assert all(np.array_equal(g, w) for g, w in zip(rt.contains_bvh4(tris, b4, rec, samples=samples, seed=seed, index_base=base), want))
        # a batch split in two with index_base reproduces the unsplit batch
        k = 611
        lo = rt.contains_bvh4(tris, b4, pts[:k], samples=samples, seed=seed, index_base=base)
        hi = rt.contains_bvh4(tris, b4, pts[k:], samples=samples, seed=seed, index_base=base + k)
        assert all(np.array_equal(np.concatenate([a, b]), w) for a, b, w in zip(lo, hi, want))


def test_rays_that_are_not_walked_and_finite_t_max(rt, orc):
    tris = cc.geometry(rt, "box")
    b4 = cc.host_trees(rt, orc, tris, 0)[1]
    o = np.zeros((8, 3), np.float32); d = np.tile(np.float32([0.3, 0.2, 1.0]), (8, 1))
    rays = rt.pack_rays(o, d, [np.inf, 2.0, 0.5, 0.0, -1.0, np.nan, np.inf, np.inf])
    rays[6, 1] = np.nan; rays[7, 5] = np.nan
    for tree in (b4, None):
        got, st = rt.count_hits_bvh4(tris, tree, rays, stats=True, brute_force=tree is None)
        assert got.tolist() == [1, 1, 0, 0, 0, 0, 0, 0]                    # the wall at z = 1 is at t = 1
        assert st["rays_closest"] == 8
    assert np.array_equal(crossref.crossings(rays, tris), got)
    # from outside a closed box a ray crosses an even number of walls
    out = rt.pack_rays([[0.1, 0.2, 3.0]] * 2, [[0, 0, -1], [0, 0, 1]])
    assert rt.count_hits_bvh4(tris, b4, out).tolist() == [2, 0]
    # empty batch, and a leaf whose triangle index is out of range is skipped
    assert rt.count_hits_bvh4(tris, b4, np.zeros((0, 8), np.float32)).size == 0
    fewer = tris[:9 * 10]                                                  # the tree still names triangles 10 and 11 (the front)
    assert rt.count_hits_bvh4(fewer, b4, rays[:1]).tolist() == [0]


def test_arguments(rt, orc):
    import ctypes as C
    lib = rt.lib
    tris = cc.geometry(rt, "tetra")
    b4 = np.ascontiguousarray(cc.host_trees(rt, orc, tris, 0)[1], np.uint32)
    rays = rt.pack_rays([[0.2, 0.1, 3]], [[0.05, -0.02, -1]]); pts = rt.pack_points([[0, 0, 0]])
    counts = np.zeros(1, np.uint32); out = np.zeros((1, 4), np.uint32)
    tp, bp = tris.ctypes.data_as(C.POINTER(C.c_float)), b4.ctypes.data_as(C.POINTER(C.c_uint32))
    rp, cp = rays.ctypes.data_as(C.POINTER(rt.PtRay)), counts.ctypes.data_as(C.POINTER(C.c_uint32))
    pp, op = pts.ctypes.data_as(C.POINTER(rt.PtPoint)), out.ctypes.data_as(C.POINTER(rt.PtContainment))
    n4, w = C.c_uint32(4), C.c_uint64(b4.size)

    def count(tp=tp, bp=bp, w=w, rp=rp, n=1, flags=0, cp=cp):
        return lib.pt_count_hits_bvh4(tp, n4, bp, w, rp, C.c_uint64(n), C.c_uint32(flags), cp, None)
    assert count() == 0 and counts[0] == 2
    # what the two twins refuse, in which order and words: test_twin_query_errors.py
    assert count(bp=None, w=C.c_uint64(0), flags=rt.PT_COUNT_BRUTE_FORCE) == 0 and counts[0] == 2
    twice = b4.copy(); inner = next(i for i in range(int(b4[0])) if not b4[1 + 8 * i + 7] & 0x80000000)
    kids = [s for s in range(4) if twice[1 + 8 * inner + 3 + s] != 0xFFFFFFFF]
    twice[1 + 8 * inner + 3 + kids[1]] = twice[1 + 8 * inner + 3 + kids[0]]
    assert count(bp=twice.ctypes.data_as(C.POINTER(C.c_uint32))) == PT_ERR_BAD_BVH    # a node reachable twice

    def contains(samples=3, flags=0, n=1, pp=pp, op=op, bp=bp, params=True):
        p = rt.PtContainParams(samples, 0, 0, flags)
        return lib.pt_contains_bvh4(tp, n4, bp, w, pp, C.c_uint64(n), C.byref(p) if params else None, op, None)
    assert contains() == 0 and out[0].tolist() == [1, 3, 3, 0]
    assert contains(samples=255) == 0 and out[0].tolist() == [1, 255, 255, 0]
    nanp = rt.pack_points([[np.nan, 0, 0], [0, 0, 0]]); out2 = np.full((2, 4), 7, np.uint32)
    p = rt.PtContainParams(3, 0, 0, 0)
    assert lib.pt_contains_bvh4(tp, n4, bp, w, nanp.ctypes.data_as(C.POINTER(rt.PtPoint)), C.c_uint64(2), C.byref(p),
                                out2.ctypes.data_as(C.POINTER(rt.PtContainment)), None) == 0
    assert out2.tolist() == [[0, 0, 0, 0], [1, 3, 3, 0]]
    assert C.sizeof(rt.PtContainment) == 16 and C.sizeof(rt.PtContainParams) == 16
