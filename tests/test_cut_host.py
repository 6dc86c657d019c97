"""Plane-cut queries on the CPU: the host twin pt_cut_search_bvh4 (include/mi355pt.h) against the float32
restatement of csrc/pt_cut.h in numpy (tests/cutref.py), the tree walk against brute force (both on the twin), the float64 sandwich with
its tolerance band, loop closure on the closed meshes, the end points, the audit of the small soups, the exact cases, truncation at a
capacity, the records that are not walked, and cross_section.  The GPU tests (tests/test_gpu_cut.py) pin the kernels to this twin word for
word, order included.

Measured here (and written into DESIGN.md section 24): stack_drops = 0 on every scene and tree for the planes of cut_cases (max_stack up
to 21 with their windows, dragon50k at level 1; 24 with the whole-scene window); listed pairs inside the tolerance band |G| <= tol of the
float64 check: 10 of 20,302 on each built tree of dragon50k, 12 of 20,831 on its refitted tree, none on the other scenes (tol about
1.7e-6); the sandwich holds from K = 0 on (cut_cases.MEASURED_K); the largest |n.p - d| of an end point is 1.84e-7 (cut_cases.END_TOL is
four times that)."""
import ctypes as C

import numpy as np
import pytest

import box_cases as bc
import closest_cases as clc
import crossing_cases as cc
import cut_cases as ctc
import cutref


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
    rec = ctc.plane_records(rt, tris)
    got = rt.cut_search_bvh4(tris, None, rec, brute_force=True, stats=True)
    ref = cutref.numpy_brute(rec, tris)
    assert [x.dtype for x in got[:5]] == [np.uint64, np.uint32, np.uint32, np.float32, np.float32]
    ctc.assert_same_lists(got, ref, ordered=True)                         # the accepted set in index order, code, the bits of t0 and t1
    counts = np.diff(got[0].astype(np.int64))
    print("%s: %d listed pairs, %d of %d planes empty, longest list %d, codes %s" % (name, int(got[0][-1]), int((counts == 0).sum()), len(rec), counts.max(), np.unique(got[2])))
    assert counts[:ctc.N_PLANES].max() >= 1 and not counts[ctc.N_PLANES:].any() and len(counts) == ctc.N_PLANES + ctc.N_BESIDE
    assert np.all(np.isin(got[2] & 7, (3, 5, 6))) and np.all(got[2] < 64)                  # exactly two crossing edges
    assert np.all((got[3] >= 0) & (got[3] <= 1) & (got[4] >= 0) & (got[4] <= 1))
    assert got[5] == dict(rays_closest=len(rec), rays_shadow=0, nodes_examined=0, tris_tested=len(rec) * (tris.size // 9),
                          stack_drops=0, max_stack=0, samples=0)


@pytest.mark.parametrize("name", cc.SCENES)
def test_walk_against_brute_force_on_every_tree(rt, cases, name):
    deepest = 0
    for label, tris, b4 in cases(name)[1]:
        rec = ctc.plane_records(rt, tris)
        walk = rt.cut_search_bvh4(tris, b4, rec, stats=True)
        brute = rt.cut_search_bvh4(tris, None, rec, brute_force=True)
        st = walk[5]
        print("%s %s: %d entries, counters %s" % (name, label, int(walk[0][-1]), st))
        assert st["stack_drops"] == 0 and st["rays_closest"] == len(rec) and st["max_stack"] <= 64, (label, st)
        assert st["tris_tested"] >= int(walk[0][-1]), (label, st)
        deepest = max(deepest, st["max_stack"])
        ctc.assert_same_lists(walk, brute, ordered=False)
        counts = np.diff(rt.cut_search_bvh4(tris, b4, rec, capacity=0)[0].astype(np.int64))
        assert np.array_equal(counts, np.diff(walk[0].astype(np.int64)))
        ctc.assert_same_lists(walk, rt.cut_search_bvh4(tris, b4, rec, simple=True), ordered=True)
        # The relation to the box query of the window.  The window filters on the triangle's BOUNDING BOX (stage (a) alone), the box
        # query on the triangle itself ((a) and a vertex inside or the separating axes), so its list is the smaller one: a large
        # triangle whose box meets a small window that the triangle misses is listed here and not there (most pairs of tetra).  What
        # holds, and is asserted: every triangle the box query lists for the window, and the plane test accepts, is listed; and every
        # listed triangle passes stage (a) (test_against_float64_with_a_tolerance_band: nothing outside the candidates).
        boxes = rt.box_search_bvh4(tris, b4, rt.pack_boxes(rec[:, 4:7], rec[:, 8:11]))
        bi, bt = ctc.owner(boxes[0].astype(np.int64)), boxes[1].astype(np.int64)
        cut = cutref.tri_cut(rec, tris, bi, bt)[0]
        assert cut.any() and np.all(np.isin((bi[cut] << 32) | bt[cut], ctc.keys(walk)))
        # the whole-scene window: the longest lists, and the deepest stacks
        wide = ctc.with_scene_window(rec[:64], tris)
        ww = rt.cut_search_bvh4(tris, b4, wide, stats=True)
        assert ww[5]["stack_drops"] == 0
        deepest = max(deepest, ww[5]["max_stack"])
        ctc.assert_same_lists(ww, rt.cut_search_bvh4(tris, None, wide, brute_force=True), ordered=False)
    print("%s: deepest stack %d" % (name, deepest))


def test_comb_lists_a_subset_and_the_deep_comb_overruns_the_cap(rt):
    """As the box query's: the whole-scene window and planes that hold the z direction through the middle of the comb, which cut every
    one of its triangles, so every leaf passes the node test.  The 30-level comb stays below the cap; the 64-level one overruns it and lists
    a subset."""
    for what, (tris, b4) in (("comb", (cc.geometry(rt, "comb"), cc.comb_tree())), ("deep comb", bc.deep_comb())):
        rec = ctc.vertical_planes(rt, tris, 64)
        walk = rt.cut_search_bvh4(tris, b4, rec, stats=True)
        brute = rt.cut_search_bvh4(tris, None, rec, brute_force=True)
        st = walk[5]
        print("%s: counters %s; walk counts %s, brute-force counts %s" % (what, st, np.unique(np.diff(walk[0].astype(np.int64))), np.unique(np.diff(brute[0].astype(np.int64)))))
        missing = ctc.assert_subset(walk, brute)
        assert int(brute[0][-1]) > 0 and st["nodes_examined"] > 0 and st["tris_tested"] > 0
        assert (missing > 0) == (st["stack_drops"] > 0)
        if what == "deep comb":
            assert st["stack_drops"] > 0 and st["max_stack"] == 64 and missing > 0


def test_spoiled_tree_lists_a_subset(rt, orc):
    tris = cc.geometry(rt, "spoiled")
    b4 = cc.spoiled_tree(rt, orc, tris)
    rec = ctc.plane_records(rt, tris)
    walk = rt.cut_search_bvh4(tris, b4, rec, stats=True)
    brute = rt.cut_search_bvh4(tris, None, rec, brute_force=True)
    missing = ctc.assert_subset(walk, brute)
    print("spoiled: %d of %d entries missing, counters %s" % (missing, int(brute[0][-1]), walk[5]))
    assert walk[5]["stack_drops"] == 0 and missing > 0 and int(walk[0][-1]) > 0


@pytest.mark.parametrize("name", cc.SCENES)
def test_against_float64_with_a_tolerance_band(rt, cases, name):
    listed_total = band_total = 0
    worst = 0.0
    for label, tris, b4 in cases(name)[1]:
        rec = ctc.plane_records(rt, tris)
        walk = rt.cut_search_bvh4(tris, b4, rec)
        band, listed, k, _ = ctc.check_against_float64(rec, tris, walk)
        print("%s %s: %d listed pairs, %d of them inside the band; the sandwich holds from K = %.3g" % (name, label, listed, band, k))
        assert band <= ctc.BAND_CAP * listed, (label, band, listed)
        listed_total += listed; band_total += band; worst = max(worst, k)
    assert band_total <= ctc.BAND_CAP * listed_total, (band_total, listed_total)
    assert worst <= max(ctc.MEASURED_K, 1.0), worst                       # what DESIGN.md section 24 states


@pytest.mark.parametrize("name", cc.CLOSED)
def test_segments_close_into_loops_on_closed_meshes(rt, cases, name):
    """Whole-scene window, the planes none of whose pairs is in the band: every mesh edge crossed appears in exactly two listed triangles
    (edges identified by exact vertex coordinates), and the classes of a shared vertex agree between the triangles that share it."""
    label, tris, b4 = cases(name)[1][0]
    rec = ctc.with_scene_window(ctc.plane_records(rt, tris)[:ctc.N_PLANES], tris)
    res = rt.cut_search_bvh4(tris, b4, rec)
    _, _, _, dirty = ctc.check_against_float64(rec, tris, res)
    clean = np.setdiff1d(np.arange(len(rec)), dirty)
    assert len(clean) >= 0.9 * len(rec)
    T = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    _, vid = np.unique(T.reshape(-1, 3), axis=0, return_inverse=True)
    vid = vid.reshape(-1, 3).astype(np.int64)                              # the vertex ids of every triangle, by exact coordinates
    off = res[0].astype(np.int64)
    checked = 0
    for i in clean:
        prim, code = res[1][off[i]:off[i + 1]].astype(np.int64), res[2][off[i]:off[i + 1]].astype(np.int64)
        if not len(prim):
            continue
        ids = vid[prim]
        edge_keys, classes = [], {}
        for e, (a, b) in enumerate(((0, 1), (1, 2), (0, 2))):
            on = (code >> e) & 1 == 1
            lo, hi = np.minimum(ids[on, a], ids[on, b]), np.maximum(ids[on, a], ids[on, b])
            edge_keys.append(lo * (vid.max() + 1) + hi)
        _, per_edge = np.unique(np.concatenate(edge_keys), return_counts=True)
        assert np.all(per_edge == 2), (name, i, per_edge)
        for v in range(3):
            for j, c in zip(ids[:, v], (code >> (3 + v)) & 1):
                assert classes.setdefault(int(j), int(c)) == int(c), (name, i, j)
        checked += 1
    print("%s: %d clean planes, %d of them with a loop" % (name, len(clean), checked))
    assert checked >= 100


@pytest.mark.parametrize("name", cc.SCENES)
def test_end_points_lie_on_the_plane(rt, cases, name):
    label, tris, b4 = cases(name)[1][0]
    rec = ctc.plane_records(rt, tris)
    off, prim, code, t0, t1 = rt.cut_search_bvh4(tris, b4, rec)
    assert np.all((t0 >= 0) & (t0 <= 1) & (t1 >= 0) & (t1 <= 1))
    seg = rt.cut_segments(tris, prim, code, t0, t1)
    assert seg.shape == (len(prim), 2, 3) and seg.dtype == np.float32
    r = rec.astype(np.float64)[ctc.owner(off.astype(np.int64))]
    err = np.abs(np.einsum("nec,nc->ne", seg.astype(np.float64), r[:, 0:3]) - r[:, 3:4])
    print("%s: largest |n.p - d| of an end point %.3g" % (name, err.max()))
    assert err.max() <= ctc.END_TOL
    # the end points lie in the triangle's own bounding box
    T = np.asarray(tris, np.float32).reshape(-1, 3, 3)[prim]
    assert np.all(seg >= T.min(1)[:, None, :]) and np.all(seg <= T.max(1)[:, None, :])


@pytest.mark.parametrize("accel", [0, 2])
@pytest.mark.parametrize("name", ["soup1", "soup5", "soup65", "soup777"])
def test_every_triangle_is_listed_by_the_plane_through_it(rt, orc, name, accel):
    from test_point_audit import scene
    tris = scene(rt, name)
    b4 = cc.host_trees(rt, orc, tris, accel)[1]
    rec, tri = ctc.aimed_planes(rt, tris)
    res = rt.cut_search_bvh4(tris, b4, rec, stats=True)
    assert res[5]["stack_drops"] == 0
    G = cutref.margin64(rec, tris, np.arange(len(tri)), tri)
    must = G > clc.TOL_K * ctc.scale(rec, tris)
    have = ctc.keys(res)
    want = (np.arange(len(tri), dtype=np.int64) << 32) | np.asarray(tri, np.int64)
    lost = must & ~np.isin(want, have)
    print("%s accel %d: %d of %d aimed planes straddled beyond the tolerance, %d of those not listed" % (name, accel, int(must.sum()), len(tri), int(lost.sum())))
    assert not lost.any() and must.sum() >= 0.9 * len(tri)


def test_exact_cases(rt, orc):
    rec = ctc.exact_planes(rt)
    brute = rt.cut_search_bvh4(ctc.EXACT_TRI, None, rec, brute_force=True)
    ctc.assert_exact(brute)
    ctc.assert_same_lists(brute, cutref.numpy_brute(rec, ctc.EXACT_TRI), ordered=True)
    seg = rt.cut_segments(ctc.EXACT_TRI, *brute[1:5])
    assert seg[0].tolist() == [[0.25, 0, 0], [0.25, 0.75, 0]] and seg[3].tolist() == [[0, 0, 0], [0, 0, 0]]      # the cut, the zero-length segment
    assert seg[4].tolist() == [[1, 0, 0], [0, 0, 0]]                                                          # the edge v0-v1
    # through a tree too: the triangle next to the walls of the closed box, moved away by 4
    tris = np.concatenate([ctc.EXACT_TRI, cc.geometry(rt, "box") + np.float32(4.0)])
    for accel in (0, 2):
        walk = rt.cut_search_bvh4(tris, cc.host_trees(rt, orc, tris, accel)[1], rec, stats=True)
        assert walk[5]["stack_drops"] == 0
        ctc.assert_exact(walk)


def test_node_test_restated_passes_wherever_the_leaf_does(rt):
    """ptct::node_cut on the f16 box of one triangle (its corners are exact in f16): a plane moved along its normal across the triangle
    is listed by brute force only where the node test passes the box, and the node test passes a little beyond -- the slack."""
    tri = np.float32([0.25, 0.25, 0.25, 0.75, 0.25, 0.25, 0.25, 0.75, 0.5])
    ds = np.float32(np.linspace(-0.2, 1.4, 4001))
    for nrm in ([1, 0, 0], [0.5, -0.25, 1], [-1, 1, 0.125]):
        rec = rt.pack_cuts(np.float32(nrm), ds)
        brute = np.diff(rt.cut_search_bvh4(tri, None, rec, brute_force=True)[0].astype(np.int64))
        mn, mx = tri.reshape(3, 3).min(0), tri.reshape(3, 3).max(0)
        node = np.array([cutref.node_cut(r, mn[None], mx[None])[0] for r in rec])
        assert (brute > 0).sum() > 100 and np.all(node[brute > 0]) and node.sum() > (brute > 0).sum()


def test_truncation_at_a_capacity(rt, cases):
    label, tris, b4 = cases("soup1k")[1][0]
    rec = ctc.plane_records(rt, tris)
    tp = tris.ctypes.data_as(C.POINTER(C.c_float))
    tree = np.ascontiguousarray(b4, np.uint32)
    full = rt.cut_search_bvh4(tris, b4, rec)
    for bp, w, flags in ((tree.ctypes.data_as(C.POINTER(C.c_uint32)), tree.size, 0), (None, 0, rt.PT_CUT_BRUTE_FORCE)):
        head = (tp, C.c_uint32(tris.size // 9), bp, C.c_uint64(w))
        total = ctc.assert_truncation(lambda cap, null: ctc.raw_search(rt, rt.lib.pt_cut_search_bvh4, head, rec, flags, cap, null, (None,)),
                                      int(full[0][-1]))
        assert total == int(full[0][-1])
    st, off, ent = ctc.raw_search(rt, rt.lib.pt_cut_search_bvh4, (tp, C.c_uint32(tris.size // 9), tree.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_uint64(tree.size)),
                                  rec, 0, total, False, (None,))
    assert st == 0 and np.array_equal(ent[:total], ctc.records_of(full))
    part = rt.cut_search_bvh4(tris, b4, rec, capacity=100)
    assert np.array_equal(part[0], full[0]) and len(part[1]) == 100
    assert all(np.array_equal(p.view(np.uint32), f[:100].view(np.uint32)) for p, f in zip(part[1:5], full[1:5]))


def test_records_that_are_not_walked(rt, orc):
    tris = cc.geometry(rt, "box")
    b4 = np.ascontiguousarray(cc.host_trees(rt, orc, tris, 0)[1], np.uint32)
    c = np.asarray(tris, np.float32).reshape(-1, 3).mean(0)
    base = rt.pack_cuts([0.3, 0.5, 0.9], np.float32(np.dot(np.float32([0.3, 0.5, 0.9]), c)), *ctc.scene_window(tris))[0]
    rec = rt.pack_cuts(np.tile(base[0:3], (20, 1)), base[3], base[4:7], base[8:11])
    nan, inf = np.nan, np.inf
    rec[1, 0] = nan; rec[2, 1] = inf; rec[3, 2] = -inf; rec[4, 3] = nan; rec[5, 3] = inf                 # n and d
    rec[6, 4] = nan; rec[7, 5] = -inf; rec[8, 9] = inf; rec[9, 10] = nan                                 # lo and hi
    rec[10, 0:3] = 0.0; rec[11, 0:3] = [-0.0, 0.0, -0.0]                                                 # n = 0
    rec[12, 4] = rec[12, 8] + 1.0                                                                        # lo > hi
    rec[13, 7] = nan; rec[13, 11] = inf                                                                  # the pads are ignored
    rec[14, 4:7] = rec[14, 8:11] = c                                                                     # a zero-extent window is valid (inside the box: nothing)
    v0 = np.asarray(tris, np.float32).reshape(-1, 3, 3)[0]
    mid = ((v0[0].astype(np.float64) + v0[1]) * 0.5).astype(np.float32)                                  # a zero-extent window on an edge of triangle 0
    rec[15, 4:7] = rec[15, 8:11] = mid
    rec[15, 3] = np.float32(np.dot(rec[15, 0:3].astype(np.float64), mid.astype(np.float64)) + 1e-3)
    rec[16, 0:4] *= np.float32(-2.0)                                                                     # the other orientation, not normalised: the same set
    rec[17, 0:4] *= np.float32(2.0 ** 90)                                                                # |n_k|, |d| near 2^100: nothing overflows
    walked = [True] + [False] * 12 + [True] * 7
    assert np.array_equal(cutref.walked(rec), walked)
    for tree in (b4, None):
        res = rt.cut_search_bvh4(tris, tree, rec, brute_force=tree is None, stats=True)
        counts = np.diff(res[0].astype(np.int64)).tolist()
        assert counts[0] >= 4 and counts[1:13] == [0] * 12 and counts[13] == counts[0] and counts[14] == 0 and counts[15] >= 1, counts
        assert counts[16:] == [counts[0]] * 4, counts
        assert res[5]["rays_closest"] == 20
        lists = [set(res[1][int(a):int(b)].tolist()) for a, b in zip(res[0][:-1], res[0][1:])]
        assert lists[16] == lists[0] == lists[17] == lists[13]
        ctc.assert_same_lists(res, cutref.numpy_brute(rec, tris), ordered=tree is None)
        own = ctc.owner(res[0].astype(np.int64))
        flipped, plain = res[2][own == 16], res[2][own == 0]
        order = (np.argsort(res[1][own == 16]), np.argsort(res[1][own == 0]))
        assert np.array_equal(flipped[order[0]] & 7, plain[order[1]] & 7)            # the same crossing edges, the classes mirrored
    # a NaN mesh triangle is never accepted
    bad = tris.copy(); bad[9 * 3 + 4] = np.nan
    assert 3 not in rt.cut_search_bvh4(bad, None, rec[:1], brute_force=True)[1]
    empty = rt.cut_search_bvh4(tris, b4, np.zeros((0, 12), np.float32))
    assert empty[0].tolist() == [0] and len(empty[1]) == 0
    assert C.sizeof(rt.PtCut) == 16 and C.sizeof(rt.PtCutPlane) == 48
    assert (rt.PT_CUT_STATS, rt.PT_CUT_SIMPLE_KERNEL, rt.PT_CUT_BRUTE_FORCE) == (rt.PT_BOX_STATS, rt.PT_BOX_SIMPLE_KERNEL, rt.PT_BOX_BRUTE_FORCE)


@pytest.mark.parametrize("name", ["torus", "soup1k"])
def test_cross_section_tiles_one_plane(rt, cases, name):
    """Context.cross_section on a stand-in that answers with the twin: the same prim set for grid 1, 3 and 8, equal to brute force's."""
    label, tris, b4 = cases(name)[1][0]

    class Stub:
        calls = 0

        @classmethod
        def cut_search(cls, normal, d, lo, hi):
            cls.calls += 1
            return rt.cut_search_bvh4(tris, b4, normal, d, lo, hi)
    nrm, c = np.float32([0.2, -0.3, 0.9]), np.asarray(tris, np.float32).reshape(-1, 3).mean(0)
    d = np.float32(np.dot(nrm, c))
    brute = rt.cut_search_bvh4(tris, None, nrm, d, brute_force=True)
    assert len(brute[1]) > 20
    for grid in (1, 3, 8):
        prim, code, seg = rt.Context.cross_section(Stub, tris, nrm, d, grid)
        assert len(np.unique(prim)) == len(prim) and seg.shape == (len(prim), 2, 3)
        assert np.array_equal(np.sort(prim), np.sort(brute[1])), grid
        order = np.argsort(prim)
        assert np.array_equal(code[order], brute[2][np.argsort(brute[1])])
        assert np.array_equal(seg[order], rt.cut_segments(tris, *brute[1:5])[np.argsort(brute[1])])
    assert Stub.calls == 3                                                # one cut_search call per cross_section
    with pytest.raises(ValueError):
        rt.Context.cross_section(Stub, tris, nrm, d, 0)
