"""Radius queries on the CPU: the host twin pt_radius_search_bvh4 (include/mi355pt.h) against a float32 restatement
of the brute-force list in numpy, the tree walk against brute force (both on the twin), whole-scene radii, the relations to the pinned
closest-point query, a float64 reference with a tolerance band, the stack cap on the comb, truncation at a capacity, and the error codes.
The GPU tests (tests/test_gpu_radius.py) pin the kernels to this twin bit for bit, order included.

Measured here (and written into DESIGN.md section 18): stack_drops = 0 on every scene and tree for the radii of radius_cases (max_stack up
to 32, dragon50k) and for the whole-scene radius (max_stack up to 44, dragon50k at level 0); point-triangle pairs left out of the float64
check because they lie inside the tolerance band: 124 of 410,387 listed entries over the 24 scene-tree pairs (0.03 %; the largest share
of one scene is tetra's, 4 of 1,435 = 0.28 %: one pair, seen in each of its four trees)."""
import ctypes as C

import numpy as np
import pytest

import closest_cases as clc
import closestref
import crossing_cases as cc
import radius_cases as rc

WHOLE_EXACT = ["tetra", "box", "cornell", "soup1k", "torus"]


@pytest.fixture(scope="module")
def cases(rt, orc):
    """name -> (triangles, [(label, triangles, bvh4)] of crossing_cases.forest): computed once, never written to."""
    memo = {}

    def get(name):
        if name not in memo:
            tris = cc.geometry(rt, name)
            memo[name] = (tris, cc.forest(rt, orc, tris))
        return memo[name]
    return get


@pytest.mark.parametrize("name", cc.SCENES)
def test_brute_force_twin_equals_the_float32_restatement(rt, cases, name):
    tris, _ = cases(name)
    pts = rc.point_records(rt, tris, name)
    got = rt.radius_search_bvh4(tris, None, pts, brute_force=True, stats=True)
    ref = rc.numpy_brute(pts, tris)
    assert got[0].dtype == np.uint64 and got[2].dtype == np.uint32
    rc.assert_same_lists(got, ref, ordered=True)                         # the set {d2 < r2} in index order, dist = sqrt(d2), u and v
    counts = np.diff(got[0].astype(np.int64))
    assert counts.max() >= 2 and (counts == 0).any()                     # the set sees empty lists and lists of several triangles
    assert got[5] == dict(rays_closest=len(pts), rays_shadow=0, nodes_examined=0, tris_tested=len(pts) * (tris.size // 9),
                          stack_drops=0, max_stack=0, samples=0)


@pytest.mark.parametrize("name", cc.SCENES)
def test_walk_against_brute_force_on_every_tree(rt, cases, name):
    for label, tris, b4 in cases(name)[1]:
        pts = rc.point_records(rt, tris, name)
        walk = rt.radius_search_bvh4(tris, b4, pts, stats=True)
        brute = rt.radius_search_bvh4(tris, None, pts, brute_force=True)
        st = walk[5]
        print("%s %s: %d entries, counters %s" % (name, label, int(walk[0][-1]), st))
        assert st["stack_drops"] == 0 and st["rays_closest"] == len(pts) and 1 <= st["max_stack"] <= 64, (label, st)
        assert st["tris_tested"] >= int(walk[0][-1]), (label, st)
        rc.assert_same_lists(walk, brute, ordered=False)
        # a second run gives the same order, and the counts alone agree with the lists
        again = rt.radius_search_bvh4(tris, b4, pts, simple=True)
        rc.assert_same_lists(walk, again, ordered=True)


@pytest.mark.parametrize("name", cc.SCENES)
def test_one_radius_that_covers_the_whole_scene(rt, cases, name):
    for label, tris, b4 in cases(name)[1]:
        n_tris = tris.size // 9
        radii = [np.float32(rc.WHOLE * rc.extent(tris))] + ([np.float32(np.inf)] if name == "tetra" else [])
        for r in radii:
            pts = rc.near_points(rt, tris, 16, r)
            walk = rt.radius_search_bvh4(tris, b4, pts, stats=True)
            st = walk[5]
            print("%s %s r_max %g: max_stack %d, stack_drops %d" % (name, label, r, st["max_stack"], st["stack_drops"]))
            counts = np.diff(walk[0].astype(np.int64))
            if name in WHOLE_EXACT:
                assert st["stack_drops"] == 0, (label, st)
                assert np.all(counts == int(clc.reachable_triangles(b4, n_tris).sum())) and counts[0] == n_tris, (label, counts)
            else:
                brute = rt.radius_search_bvh4(tris, None, pts, brute_force=True)
                missing = rc.assert_subset(walk, brute)
                if st["stack_drops"] == 0:
                    assert missing == 0
                    rc.assert_same_lists(walk, brute, ordered=False)


@pytest.mark.parametrize("name", cc.SCENES)
def test_relations_to_the_closest_point_query(rt, cases, name):
    label, tris, b4 = cases(name)[1][0]
    pts = rc.point_records(rt, tris, name)
    walk = rt.radius_search_bvh4(tris, b4, pts, stats=True)
    assert walk[5]["stack_drops"] == 0
    dist, prim, _, _, cst = rt.closest_points_bvh4(tris, b4, pts, stats=True)
    assert cst["stack_drops"] == 0
    off, ent = rc.words(walk)
    counts = np.diff(off)
    assert np.array_equal(counts == 0, prim == clc.MISS), np.flatnonzero((counts == 0) != (prim == clc.MISS))[:10]
    found = np.flatnonzero(counts > 0)
    assert len(found) and len(found) < len(pts)
    d = ent[:, 0].view(np.float32)
    low = np.minimum.reduceat(d, off[found])                             # empty lists between two starts take no part: starts of non-empty lists only
    assert clc.same_bits(low, dist[found])
    own = rc.owner(off)
    assert np.all(np.isin((found.astype(np.int64) << 32) | prim[found], (own.astype(np.int64) << 32) | ent[:, 1]))


@pytest.mark.parametrize("name", cc.SCENES)
def test_against_float64_with_a_tolerance_band(rt, cases, name):
    listed_total = band_total = 0
    for label, tris, b4 in cases(name)[1]:
        pts = rc.point_records(rt, tris, name)
        tol = clc.tolerance(pts, tris)
        walk = rt.radius_search_bvh4(tris, b4, pts)
        off, ent = rc.words(walk)
        own = rc.owner(off)
        p64 = pts[:, :3].astype(np.float64); r = pts[:, 3].astype(np.float64)
        # nothing beyond r + tol is listed
        d_listed = closestref.distance_to(p64[own], tris, ent[:, 1])
        assert np.all(d_listed <= r[own] + tol), (label, float((d_listed - r[own]).max()))
        # everything within r - tol is listed.  Candidates: a triangle lies inside the sphere around its centroid through its farthest
        # vertex, so one with |p - c| - rad >= r is at least r away and need not be evaluated.
        T = np.asarray(tris, np.float64).reshape(-1, 3, 3)
        cen = T.mean(1); rad = np.linalg.norm(T - cen[:, None, :], axis=2).max(1)
        have = (own.astype(np.int64) << 32) | ent[:, 1]
        band = 0
        for s in range(0, len(pts), 64):
            gap = np.linalg.norm(p64[s:s + 64, None, :] - cen[None, :, :], axis=2) - rad[None, :]
            pi, ti = np.nonzero(gap < r[s:s + 64, None])
            pi += s
            d = closestref.distance_to(p64[pi], tris, ti)
            must = d < r[pi] - tol
            assert np.all(np.isin((pi[must].astype(np.int64) << 32) | ti[must], have)), label
            band += int((np.abs(d - r[pi]) <= tol).sum())
        listed_total += len(ent); band_total += band
    print("%s: %d point-triangle pairs inside the band |d - r| <= tol, %d listed entries" % (name, band_total, listed_total))
    assert band_total * 200 <= listed_total, (band_total, listed_total)


def test_comb_drops_pushes_and_lists_a_subset(rt):
    tris, b4 = cc.geometry(rt, "comb"), cc.comb_tree()
    rng = np.random.default_rng(3)
    p = np.stack([rng.uniform(-0.9, 0.9, 64), rng.uniform(-0.9, 0.9, 64), rng.uniform(1.0, 2.0, 64)], axis=1).astype(np.float32)
    pts = rt.pack_points(p, np.inf)
    walk = rt.radius_search_bvh4(tris, b4, pts, stats=True)
    brute = rt.radius_search_bvh4(tris, None, pts, brute_force=True)
    st = walk[5]
    print("comb: counters %s; walk counts %s, brute-force counts %s" % (st, np.unique(np.diff(walk[0].astype(np.int64))), np.unique(np.diff(brute[0].astype(np.int64)))))
    assert st["stack_drops"] > 0 and st["max_stack"] == 64 and st["nodes_examined"] > 0 and st["tris_tested"] > 0
    assert rc.assert_subset(walk, brute) > 0                              # each triangle sits in one leaf; what is dropped is not listed
    assert np.all(np.diff(brute[0].astype(np.int64)) == tris.size // 9)


def test_truncation_at_a_capacity(rt, cases):
    label, tris, b4 = cases("soup1k")[1][0]
    pts = rc.point_records(rt, tris, "soup1k")
    tp = tris.ctypes.data_as(C.POINTER(C.c_float))
    tree = np.ascontiguousarray(b4, np.uint32)
    full = rt.radius_search_bvh4(tris, b4, pts)
    for bp, w, flags in ((tree.ctypes.data_as(C.POINTER(C.c_uint32)), tree.size, 0), (None, 0, rt.PT_RADIUS_BRUTE_FORCE)):
        head = (tp, C.c_uint32(tris.size // 9), bp, C.c_uint64(w))
        total = rc.assert_truncation(lambda cap, null: rc.raw_search(rt, rt.lib.pt_radius_search_bvh4, head, pts, flags, cap, null, (None,)),
                                     int(full[0][-1]))
        assert total == int(full[0][-1])
    # the binding: capacity given -> the first entries, offsets complete
    part = rt.radius_search_bvh4(tris, b4, pts, capacity=100)
    assert np.array_equal(part[0], full[0]) and len(part[2]) == 100
    assert all(clc.same_bits(a, b[:100]) for a, b in zip(part[1:5], full[1:5]))


def test_arguments_and_points_that_are_not_walked(rt, orc):
    lib = rt.lib
    tris = cc.geometry(rt, "box")
    b4 = np.ascontiguousarray(cc.host_trees(rt, orc, tris, 0)[1], np.uint32)
    r = np.float32([2.0, np.nan, 0.0, -1.0, 2.0, 2.0, 2.0, np.inf])
    pts = rt.pack_points(np.zeros((8, 3), np.float32), r)
    pts[4, 0] = np.nan; pts[5, 1] = np.nan; pts[6, 2] = np.nan
    for tree in (b4, None):
        res = rt.radius_search_bvh4(tris, tree, pts, brute_force=tree is None, stats=True)
        assert np.diff(res[0].astype(np.int64)).tolist() == [12, 0, 0, 0, 0, 0, 0, 12]      # the walls of the box are 1 away
        assert res[5]["rays_closest"] == 8
    # r2 is strict: the walls at distance exactly 1 are not within r_max = 1, and are within the next float
    edge = rt.pack_points(np.zeros((2, 3), np.float32), np.float32([1.0, np.nextafter(np.float32(1), np.float32(2))]))
    got = np.diff(rt.radius_search_bvh4(tris, b4, edge)[0].astype(np.int64)).tolist()
    assert got == np.diff(rt.radius_search_bvh4(tris, None, edge, brute_force=True)[0].astype(np.int64)).tolist() and got[0] == 0 and got[1] == 12
    # an empty batch: offsets = [0]; a leaf whose triangle index is out of range is skipped
    empty = rt.radius_search_bvh4(tris, b4, np.zeros((0, 4), np.float32))
    assert empty[0].tolist() == [0] and len(empty[2]) == 0
    fewer = tris[:9 * 10]
    assert np.diff(rt.radius_search_bvh4(fewer, b4, pts[:1])[0].astype(np.int64)).tolist() == [10]

    tp, bp = tris.ctypes.data_as(C.POINTER(C.c_float)), b4.ctypes.data_as(C.POINTER(C.c_uint32))
    one = rt.pack_points([[0, 0, 0]], 2.0)
    pp = one.ctypes.data_as(C.POINTER(rt.PtPoint))
    raw = np.zeros(4, np.uint64); off = raw[:2]
    ent = rt._aligned_zeros((16, 4), np.uint32)
    op, ep = off.ctypes.data_as(C.POINTER(C.c_uint64)), ent.ctypes.data_as(C.POINTER(rt.PtClosest))
    n12, w = C.c_uint32(12), C.c_uint64(b4.size)

    def search(tp=tp, bp=bp, w=w, pp=pp, n=1, flags=0, op=op, ep=ep, cap=16):
        return lib.pt_radius_search_bvh4(tp, n12, bp, w, pp, C.c_uint64(n), C.c_uint32(flags), op, ep, C.c_uint64(cap), None)
    assert search() == 0 and off.tolist() == [0, 12]
    assert search(ep=None, cap=0) == 0 and off.tolist() == [0, 12]
    assert search(bp=None, w=C.c_uint64(0), flags=rt.PT_RADIUS_BRUTE_FORCE) == 0 and off.tolist() == [0, 12]
    assert search(flags=rt.PT_RADIUS_SIMPLE_KERNEL | rt.PT_RADIUS_STATS) == 0
    assert search(pp=None, ep=None, n=0, cap=0) == 0 and off[0] == 0
    # what the twin refuses, in which order and words: test_twin_query_errors.py
    assert C.sizeof(rt.PtClosest) == 16 and C.sizeof(rt.PtPoint) == 16
