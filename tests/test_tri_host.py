"""Triangle-overlap queries on the CPU: the host twin pt_tri_search_bvh4 (include/mi355pt.h) against the float32
restatement of csrc/pt_tritri.h in numpy (tests/triref.py), the tree walk against brute force (both on the twin), the float64 sandwich with
its tolerance band, the relation to the crossing counts and to the box query, the audit of the small soups, the exact cases, truncation at
a capacity, the triangles that are not walked and the error codes.  The GPU tests (tests/test_gpu_tri.py) pin the kernels to this twin
word for word, order included.

Measured here (and written into DESIGN.md section 23): stack_drops = 0 on every scene and tree for the caller triangles of tri_cases
(max_stack up to 19, dragon50k at level 2); listed pairs inside the tolerance band |G| <= tol of the float64 check: 3 of 3,346 on each
built tree of dragon50k, 1 of 1,154 on each built tree of the torus, none on the other 18 scene-tree pairs (tol about 2e-6); and the
sandwich holds from K = 0 on (tri_cases.MEASURED_K): no listed pair has G < 0, no unlisted pair G > 0."""
import ctypes as C

import numpy as np
import pytest

import box_cases as bc
import crossing_cases as cc
import tri_cases as tc
import triref


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
    rec = tc.caller_records(rt, tris)
    got = rt.tri_search_bvh4(tris, None, rec, brute_force=True, stats=True)
    ref = triref.numpy_brute(rec, tris)
    assert got[0].dtype == np.uint64 and got[1].dtype == np.uint32 and got[2].dtype == np.uint32
    tc.assert_same_lists(got, ref, ordered=True)                         # the accepted set in index order, edges
    counts = np.diff(got[0].astype(np.int64))
    two = np.array([bin(int(e)).count("1") == 2 for e in got[2]])
    print("%s: %d listed pairs, %d of %d caller triangles empty, %d pairs without exactly two bits, edges values %s"
          % (name, int(got[0][-1]), int((counts == 0).sum()), len(rec), int((~two).sum()), np.unique(got[2])))
    # (a caller triangle of this size meets one of the large faces of tetra, box and cornell; the fine meshes give lists of several)
    assert counts.max() >= (2 if name in ("soup1k", "dragon50k", "torus") else 1) and np.all(got[2] != 0) and np.all(got[2] < 64)
    assert got[3] == dict(rays_closest=len(rec), rays_shadow=0, nodes_examined=0, tris_tested=len(rec) * (tris.size // 9),
                          stack_drops=0, max_stack=0, samples=0)


@pytest.mark.parametrize("name", cc.SCENES)
def test_walk_against_brute_force_on_every_tree(rt, cases, name):
    for label, tris, b4 in cases(name)[1]:
        rec = tc.caller_records(rt, tris)
        walk = rt.tri_search_bvh4(tris, b4, rec, stats=True)
        brute = rt.tri_search_bvh4(tris, None, rec, brute_force=True)
        st = walk[3]
        print("%s %s: %d entries, counters %s" % (name, label, int(walk[0][-1]), st))
        assert st["stack_drops"] == 0 and st["rays_closest"] == len(rec) and 1 <= st["max_stack"] <= 64, (label, st)
        assert st["tris_tested"] >= int(walk[0][-1]), (label, st)
        tc.assert_same_lists(walk, brute, ordered=False)
        counts = np.diff(rt.tri_search_bvh4(tris, b4, rec, capacity=0)[0].astype(np.int64))
        assert np.array_equal(counts, np.diff(walk[0].astype(np.int64)))
        tc.assert_same_lists(walk, rt.tri_search_bvh4(tris, b4, rec, simple=True), ordered=True)
        # every listed prim is in the box query's list of the caller triangle's bounding box
        boxes = rt.box_search_bvh4(tris, b4, tc.bounding_boxes(rt, rec))
        assert np.all(np.isin(tc.keys(walk), bc.keys(boxes)))


@pytest.mark.parametrize("name", cc.SCENES)
def test_against_float64_with_a_tolerance_band(rt, cases, name):
    listed_total = band_total = 0
    worst = 0.0
    for label, tris, b4 in cases(name)[1]:
        rec = tc.caller_records(rt, tris)
        walk = rt.tri_search_bvh4(tris, b4, rec)
        band, listed, k = tc.check_against_float64(rec, tris, walk)
        print("%s %s: %d listed pairs, %d of them inside the band |G| <= %.3g; the sandwich holds from K = %.3g" % (name, label, listed, band, tc.tolerance(rec, tris), k))
        assert band <= tc.BAND_CAP * listed, (label, band, listed)
        listed_total += listed; band_total += band; worst = max(worst, k)
    assert band_total <= tc.BAND_CAP * listed_total, (band_total, listed_total)
    assert worst <= max(tc.MEASURED_K, 1.0), worst                        # what DESIGN.md section 23 states, to within one unit


@pytest.mark.parametrize("name", cc.SCENES)
def test_caller_edge_bits_against_the_crossing_counts(rt, cases, name):
    """(edges & 7) != 0 exactly where count_hits, brute force, counts a crossing on one of the three edge rays with t_max = 1 -- on pairs
    outside the band: the two predicates round differently (count_hits divides, and has the absolute 1e-7 thresholds)."""
    tris, _ = cases(name)
    rec = tc.caller_records(rt, tris)
    got = rt.tri_search_bvh4(tris, None, rec, brute_force=True)
    k, G = tc.margins(rec, tris)
    tol = tc.tolerance(rec, tris)
    Q = triref.callers(rec)
    n_tris = tris.size // 9
    # one mesh triangle at a time would be 500 x m calls: count per caller edge over the whole mesh, and compare per caller triangle
    # where no pair of that caller triangle is inside the band
    clean = np.ones(len(rec), bool)
    clean[(k[np.abs(G) <= tol] >> 32).astype(np.int64)] = False
    rays = rt.pack_rays(Q.reshape(-1, 3), (np.roll(Q, -1, axis=1) - Q).reshape(-1, 3), 1.0)
    hits = rt.count_hits_bvh4(tris, None, rays, brute_force=True).reshape(-1, 3).astype(np.int64)
    off = got[0].astype(np.int64)
    own = tc.owner(off)
    for e in range(3):
        mine = np.bincount(own[(got[2] >> e) & 1 == 1], minlength=len(rec))
        # count_hits needs t > 1e-7 and |det| >= 1e-7: an edge that starts on a triangle, or a pair below its thresholds, may differ
        same = mine[clean] == hits[clean, e]
        print("%s edge %d: %d of %d clean caller triangles agree with count_hits" % (name, e, int(same.sum()), int(clean.sum())))
        assert np.all((mine[clean] > 0) == (hits[clean, e] > 0)), np.flatnonzero((mine > 0) != (hits[:, e] > 0))[:10]
    assert n_tris > 0 and clean.sum() >= 0.9 * len(rec)


@pytest.mark.parametrize("accel", [0, 2])
@pytest.mark.parametrize("name", ["soup1", "soup5", "soup65", "soup777"])
def test_every_triangle_is_listed_by_the_triangle_through_it(rt, orc, name, accel):
    from test_point_audit import scene
    tris = scene(rt, name)
    b4 = cc.host_trees(rt, orc, tris, accel)[1]
    rec, tri = tc.aimed_tris(rt, tris)
    res = rt.tri_search_bvh4(tris, b4, rec, stats=True)
    assert res[3]["stack_drops"] == 0
    G = triref.margin64(rec, tris, np.arange(len(tri)), tri)
    must = G > tc.tolerance(rec, tris)
    have = tc.keys(res)
    want = (np.arange(len(tri), dtype=np.int64) << 32) | np.asarray(tri, np.int64)
    lost = must & ~np.isin(want, have)
    print("%s accel %d: %d of %d aimed triangles beyond the tolerance, %d of those not listed" % (name, accel, int(must.sum()), len(tri), int(lost.sum())))
    assert not lost.any() and must.sum() >= 0.95 * len(tri)
    assert np.all(res[2][np.isin(have, want)] & 1)                        # by the edge p + eps n -> p - eps n


def test_exact_cases(rt, orc):
    rec = tc.exact_tris(rt)
    brute = rt.tri_search_bvh4(tc.EXACT_TRI, None, rec, brute_force=True)
    tc.assert_exact(brute)
    tc.assert_same_lists(brute, triref.numpy_brute(rec, tc.EXACT_TRI), ordered=True)
    # through a tree too: the triangle next to the walls of the closed box, moved away by 4
    tris = np.concatenate([tc.EXACT_TRI, cc.geometry(rt, "box") + np.float32(4.0)])
    for accel in (0, 2):
        walk = rt.tri_search_bvh4(tris, cc.host_trees(rt, orc, tris, accel)[1], rec, stats=True)
        assert walk[3]["stack_drops"] == 0
        tc.assert_exact(walk)


def test_intersecting_pairs_composition(rt, cases):
    """Context.intersecting_pairs is tri_search flattened; its composition is checked here on a stand-in that answers with the twin."""
    label, tris, b4 = cases("torus")[1][0]
    rec = tc.caller_records(rt, tris)
    full = rt.tri_search_bvh4(tris, b4, rec)

    class Stub:
        tri_search = staticmethod(lambda t, capacity=None: rt.tri_search_bvh4(tris, b4, t, capacity=capacity))
    for cap in (None, 100):
        pairs, edges = rt.Context.intersecting_pairs(Stub, rec, cap)
        m = len(full[1]) if cap is None else cap
        assert pairs.shape == (m, 2) and pairs.dtype == np.int64
        assert np.array_equal(pairs[:, 0], tc.owner(full[0].astype(np.int64))[:m]) and np.array_equal(pairs[:, 1], full[1][:m]) and np.array_equal(edges, full[2][:m])


def test_truncation_at_a_capacity(rt, cases):
    label, tris, b4 = cases("soup1k")[1][0]
    rec = tc.caller_records(rt, tris)
    tp = tris.ctypes.data_as(C.POINTER(C.c_float))
    tree = np.ascontiguousarray(b4, np.uint32)
    full = rt.tri_search_bvh4(tris, b4, rec)
    for bp, w, flags in ((tree.ctypes.data_as(C.POINTER(C.c_uint32)), tree.size, 0), (None, 0, rt.PT_TRI_BRUTE_FORCE)):
        head = (tp, C.c_uint32(tris.size // 9), bp, C.c_uint64(w))
        total = tc.assert_truncation(lambda cap, null: tc.raw_search(rt, rt.lib.pt_tri_search_bvh4, head, rec, flags, cap, null, (None,)),
                                     int(full[0][-1]))
        assert total == int(full[0][-1])
    st, off, ent = tc.raw_search(rt, rt.lib.pt_tri_search_bvh4, (tp, C.c_uint32(tris.size // 9), tree.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_uint64(tree.size)),
                                 rec, 0, total, False, (None,))
    assert st == 0 and np.array_equal(ent[:total], tc.records_of(full))      # the reserved words are written, as 0
    part = rt.tri_search_bvh4(tris, b4, rec, capacity=100)
    assert np.array_equal(part[0], full[0]) and len(part[1]) == 100
    assert np.array_equal(part[1], full[1][:100]) and np.array_equal(part[2], full[2][:100])


def test_arguments_and_triangles_that_are_not_walked(rt, orc):
    lib = rt.lib
    tris = cc.geometry(rt, "box")
    b4 = np.ascontiguousarray(cc.host_trees(rt, orc, tris, 0)[1], np.uint32)
    big = np.array([[-3, -3, -3], [5, -3, 3], [-3, 5, 3]], np.float64)       # cuts through the whole closed box
    Q = np.tile(big, (9, 1, 1))
    Q[1, 0, 0] = np.nan; Q[2, 1, 2] = np.inf; Q[3, 2, 1] = -np.inf
    Q[4] = [[-3, 0.1, 0.2], [3, 0.1, 0.2], [0, 0.1, 0.2]]                  # degenerate: a segment through two walls
    Q[5] = [[0.1, 0.2, 0.3]] * 3                                          # degenerate: a point inside the box
    Q[6] += 20.0                                                          # a valid triangle that meets nothing
    Q[7] = Q[0][::-1]                                                     # the other orientation: the same set
    rec = rt.pack_tris(Q)
    rec[8, 3] = np.nan; rec[8, 7] = np.inf; rec[8, 11] = -np.inf           # the pads are ignored
    assert np.array_equal(triref.walked(rec), [True, False, False, False, True, True, True, True, True])
    for tree in (b4, None):
        res = rt.tri_search_bvh4(tris, tree, rec, brute_force=tree is None, stats=True)
        counts = np.diff(res[0].astype(np.int64)).tolist()
        assert counts[0] >= 4 and counts[1:4] == [0, 0, 0] and counts[4] >= 2 and counts[5:7] == [0, 0] and counts[7:] == [counts[0]] * 2, counts
        assert res[3]["rays_closest"] == 9
        lists = [set(res[1][int(a):int(b)].tolist()) for a, b in zip(res[0][:-1], res[0][1:])]
        assert lists[7] == lists[0] == lists[8]
        own = tc.owner(res[0].astype(np.int64))
        assert np.all(res[2][own == 4] < 8)                              # a segment: every det against the caller's "triangle" is 0
    tc.assert_same_lists(rt.tri_search_bvh4(tris, None, rec, brute_force=True), triref.numpy_brute(rec, tris), ordered=True)
    # a NaN mesh triangle is never accepted, whatever the caller triangle
    bad = tris.copy(); bad[9 * 3 + 4] = np.nan
    assert 3 not in rt.tri_search_bvh4(bad, None, rec[:1], brute_force=True)[1]
    # an empty batch: offsets = [0]; the three input shapes give the same records
    empty = rt.tri_search_bvh4(tris, b4, np.zeros((0, 12), np.float32))
    assert empty[0].tolist() == [0] and len(empty[1]) == 0
    assert np.array_equal(rt.pack_tris(Q.reshape(-1, 9)).view(np.uint32), rt.pack_tris(Q).view(np.uint32)) and rt.pack_tris(Q).shape == (9, 12)
    assert rt.pack_tris(Q).ctypes.data % 16 == 0

    tp, bp = tris.ctypes.data_as(C.POINTER(C.c_float)), b4.ctypes.data_as(C.POINTER(C.c_uint32))
    one = rec[:1].copy()
    pp = one.ctypes.data_as(C.POINTER(rt.PtTri))
    raw = np.zeros(4, np.uint64); off = raw[:2]
    ent = rt._aligned_zeros((16, 4), np.uint32)
    op, ep = off.ctypes.data_as(C.POINTER(C.c_uint64)), ent.ctypes.data_as(C.POINTER(rt.PtCross))
    n12, w = C.c_uint32(12), C.c_uint64(b4.size)
    total = int(np.diff(rt.tri_search_bvh4(tris, b4, rec[:1])[0].astype(np.int64))[0])

    def search(tp=tp, bp=bp, w=w, pp=pp, n=1, flags=0, op=op, ep=ep, cap=16):
        return lib.pt_tri_search_bvh4(tp, n12, bp, w, pp, C.c_uint64(n), C.c_uint32(flags), op, ep, C.c_uint64(cap), None)
    assert search() == 0 and off.tolist() == [0, total]
    assert search(ep=None, cap=0) == 0 and off.tolist() == [0, total]
    assert search(bp=None, w=C.c_uint64(0), flags=rt.PT_TRI_BRUTE_FORCE) == 0 and off.tolist() == [0, total]
    assert search(flags=rt.PT_TRI_SIMPLE_KERNEL | rt.PT_TRI_STATS) == 0
    assert search(pp=None, ep=None, n=0, cap=0) == 0 and off[0] == 0
    # what the twin refuses, in which order and words: test_twin_query_errors.py
    assert C.sizeof(rt.PtCross) == 16 and C.sizeof(rt.PtTri) == 48
    assert (rt.PT_TRI_STATS, rt.PT_TRI_SIMPLE_KERNEL, rt.PT_TRI_BRUTE_FORCE) == (rt.PT_BOX_STATS, rt.PT_BOX_SIMPLE_KERNEL, rt.PT_BOX_BRUTE_FORCE)
