"""Box-overlap queries on the CPU: the host twin pt_box_search_bvh4 (include/mi355pt.h) against a float32
restatement of csrc/pt_overlap.h in numpy, the tree walk against brute force (both on the twin), whole-scene boxes, a float64
separating-axis reference with a tolerance band, the exact cases, the relation to the radius query, the stack cap on the comb, truncation at
a capacity, the boxes that are not walked and the error codes.  The GPU tests (tests/test_gpu_box.py) pin the kernels to this twin word for
word, order included.

Measured here (and written into DESIGN.md section 21): stack_drops = 0 on every scene and tree for the boxes of box_cases (max_stack up to
24, dragon50k at level 2) and for the whole-scene box on every tree (max_stack up to 27, dragon50k at level 2); box-triangle pairs inside
the tolerance band |g| <= tol of the float64 check: 1 of the 50,532 listed pairs over the 20 scene-tree pairs of tetra, box, cornell,
soup1k and torus (the refitted torus: 1 of 10,354; tol about 2.5e-6)."""
import ctypes as C

import numpy as np
import pytest

import box_cases as bc
import closest_cases as clc
import crossing_cases as cc
import radius_cases as rc

FLOAT64_SCENES = ["tetra", "box", "cornell", "soup1k", "torus"]
WHOLE_EXACT = FLOAT64_SCENES


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
    boxes = bc.box_records(rt, tris)
    got = rt.box_search_bvh4(tris, None, boxes, brute_force=True, stats=True)
    ref = bc.numpy_brute(boxes, tris)
    assert got[0].dtype == np.uint64 and got[1].dtype == np.uint32 and got[2].dtype == np.uint32
    bc.assert_same_lists(got, ref, ordered=True)                         # the accepted set in index order, verts_inside
    counts = np.diff(got[0].astype(np.int64))
    print("%s: %d listed pairs, %d of %d boxes empty, verts_inside values %s" % (name, int(got[0][-1]), int((counts == 0).sum()), len(boxes), np.unique(got[2])))
    assert counts.max() >= 2 and (counts == 0).any()                     # the set sees empty lists and lists of several triangles
    assert got[3] == dict(rays_closest=len(boxes), rays_shadow=0, nodes_examined=0, tris_tested=len(boxes) * (tris.size // 9),
                          stack_drops=0, max_stack=0, samples=0)


@pytest.mark.parametrize("name", cc.SCENES)
def test_walk_against_brute_force_on_every_tree(rt, cases, name):
    for label, tris, b4 in cases(name)[1]:
        boxes = bc.box_records(rt, tris)
        walk = rt.box_search_bvh4(tris, b4, boxes, stats=True)
        brute = rt.box_search_bvh4(tris, None, boxes, brute_force=True)
        st = walk[3]
        print("%s %s: %d entries, counters %s" % (name, label, int(walk[0][-1]), st))
        assert st["stack_drops"] == 0 and st["rays_closest"] == len(boxes) and 1 <= st["max_stack"] <= 64, (label, st)
        assert st["tris_tested"] >= int(walk[0][-1]), (label, st)
        bc.assert_same_lists(walk, brute, ordered=False)
        # count = 0 exactly when the list is empty, and a second run gives the same order
        counts = np.diff(rt.box_search_bvh4(tris, b4, boxes, capacity=0)[0].astype(np.int64))
        assert np.array_equal(counts, np.diff(walk[0].astype(np.int64)))
        assert np.array_equal(counts == 0, ~np.isin(np.arange(len(boxes)), bc.owner(bc.words(walk)[0])))
        bc.assert_same_lists(walk, rt.box_search_bvh4(tris, b4, boxes, simple=True), ordered=True)


@pytest.mark.parametrize("name", cc.SCENES)
def test_one_box_that_holds_the_whole_scene(rt, cases, name):
    for label, tris, b4 in cases(name)[1]:
        n_tris = tris.size // 9
        boxes = bc.whole_scene_box(rt, tris, 4)
        walk = rt.box_search_bvh4(tris, b4, boxes, stats=True)
        st = walk[3]
        print("%s %s whole-scene box: max_stack %d, stack_drops %d" % (name, label, st["max_stack"], st["stack_drops"]))
        counts = np.diff(walk[0].astype(np.int64))
        if name in WHOLE_EXACT:
            assert st["stack_drops"] == 0, (label, st)
            assert np.all(counts == int(clc.reachable_triangles(b4, n_tris).sum())) and counts[0] == n_tris, (label, counts)
            assert np.all(walk[2] == 7)
        else:
            brute = rt.box_search_bvh4(tris, None, boxes, brute_force=True)
            missing = bc.assert_subset(walk, brute)
            if st["stack_drops"] == 0:
                assert missing == 0
                bc.assert_same_lists(walk, brute, ordered=False)


@pytest.mark.parametrize("name", FLOAT64_SCENES)
def test_against_float64_with_a_tolerance_band(rt, cases, name):
    listed_total = band_total = 0
    for label, tris, b4 in cases(name)[1]:
        boxes = bc.box_records(rt, tris)
        walk = rt.box_search_bvh4(tris, b4, boxes)
        band, listed = bc.check_against_float64(boxes, tris, walk)
        print("%s %s: %d listed pairs, %d pairs inside the band |g| <= %.3g" % (name, label, listed, band, bc.tolerance(boxes, tris)))
        assert band <= bc.BAND_CAP * listed, (label, band, listed)
        listed_total += listed; band_total += band
    assert band_total <= bc.BAND_CAP * listed_total, (band_total, listed_total)


def test_exact_cases(rt, orc):
    boxes = bc.exact_boxes(rt)
    brute = rt.box_search_bvh4(bc.EXACT_TRI, None, boxes, brute_force=True)
    bc.assert_exact(brute)
    bc.assert_same_lists(brute, bc.numpy_brute(boxes, bc.EXACT_TRI), ordered=True)
    # through a tree too: the triangle in front of the walls of the closed box, moved away by 4
    tris = np.concatenate([bc.EXACT_TRI, cc.geometry(rt, "box") + np.float32(4.0)])
    for accel in (0, 2):
        walk = rt.box_search_bvh4(tris, cc.host_trees(rt, orc, tris, accel)[1], boxes, stats=True)
        assert walk[3]["stack_drops"] == 0
        bc.assert_exact(walk)


@pytest.mark.parametrize("name", ["soup1k", "torus"])
def test_every_triangle_of_a_radius_list_is_in_the_box_around_it(rt, cases, name):
    label, tris, b4 = cases(name)[1][0]
    pts = rc.point_records(rt, tris, name)
    found = rt.radius_search_bvh4(tris, b4, pts)
    p, r = pts[:, :3].astype(np.float64), pts[:, 3:4].astype(np.float64)
    boxes = rt.pack_boxes((p - 1.01 * r).astype(np.float32), (p + 1.01 * r).astype(np.float32))
    walk = rt.box_search_bvh4(tris, b4, boxes, stats=True)
    assert walk[3]["stack_drops"] == 0 and len(found[2]) > len(pts)
    off = found[0].astype(np.int64)
    near = (rc.owner(off).astype(np.int64) << 32) | found[2]
    assert np.all(np.isin(near, bc.keys(walk)))


def test_comb_lists_a_subset_and_the_deep_comb_overruns_the_cap(rt):
    """crossing_cases.comb_tree(): the walk's list is a subset of brute force's.  Its 30 levels do not reach the cap in slot order
    (box_cases.DEEP_COMB_LEVELS says why: max_stack 50 for the box that holds all of it), so the overrun is shown on the same comb with 64."""
    for what, (tris, b4) in (("comb", (cc.geometry(rt, "comb"), cc.comb_tree())), ("deep comb", bc.deep_comb())):
        boxes = bc.whole_scene_box(rt, tris, 64)
        walk = rt.box_search_bvh4(tris, b4, boxes, stats=True)
        brute = rt.box_search_bvh4(tris, None, boxes, brute_force=True)
        st = walk[3]
        print("%s: counters %s; walk counts %s, brute-force counts %s" % (what, st, np.unique(np.diff(walk[0].astype(np.int64))), np.unique(np.diff(brute[0].astype(np.int64)))))
        missing = bc.assert_subset(walk, brute)                           # each triangle sits in one leaf; what is dropped is not listed
        assert np.all(np.diff(brute[0].astype(np.int64)) == tris.size // 9)
        assert st["nodes_examined"] > 0 and st["tris_tested"] > 0
        assert (missing > 0) == (st["stack_drops"] > 0)
        if what == "deep comb":
            assert st["stack_drops"] > 0 and st["max_stack"] == 64 and missing > 0


def test_truncation_at_a_capacity(rt, cases):
    label, tris, b4 = cases("soup1k")[1][0]
    boxes = bc.box_records(rt, tris)
    tp = tris.ctypes.data_as(C.POINTER(C.c_float))
    tree = np.ascontiguousarray(b4, np.uint32)
    full = rt.box_search_bvh4(tris, b4, boxes)
    for bp, w, flags in ((tree.ctypes.data_as(C.POINTER(C.c_uint32)), tree.size, 0), (None, 0, rt.PT_BOX_BRUTE_FORCE)):
        head = (tp, C.c_uint32(tris.size // 9), bp, C.c_uint64(w))
        total = bc.assert_truncation(lambda cap, null: bc.raw_search(rt, rt.lib.pt_box_search_bvh4, head, boxes, flags, cap, null, (None,)),
                                     int(full[0][-1]))
        assert total == int(full[0][-1])
    st, off, ent = bc.raw_search(rt, rt.lib.pt_box_search_bvh4, (tp, C.c_uint32(tris.size // 9), tree.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_uint64(tree.size)),
                                 boxes, 0, total, False, (None,))
    assert st == 0 and np.array_equal(ent[:total], bc.records_of(full))      # the reserved words are written, as 0
    # the binding: capacity given -> the first entries, offsets complete
    part = rt.box_search_bvh4(tris, b4, boxes, capacity=100)
    assert np.array_equal(part[0], full[0]) and len(part[1]) == 100
    assert np.array_equal(part[1], full[1][:100]) and np.array_equal(part[2], full[2][:100])


def test_arguments_and_boxes_that_are_not_walked(rt, orc):
    lib = rt.lib
    tris = cc.geometry(rt, "box")
    b4 = np.ascontiguousarray(cc.host_trees(rt, orc, tris, 0)[1], np.uint32)
    lo = np.full((10, 3), -2, np.float32); hi = np.full((10, 3), 2, np.float32)
    lo[1, 0] = np.nan; hi[2, 1] = np.nan; lo[3, 2] = -np.inf; hi[4, 0] = np.inf; lo[5, 1] = np.inf
    lo[6, 0] = 2.5                                                       # lo > hi on one axis
    lo[7], hi[7] = [1, 0, 0], [1, 0, 0]                                   # a point on a wall: zero extent is valid
    lo[8], hi[8] = [5, 5, 5], [6, 6, 6]                                   # a valid box that meets nothing
    boxes = rt.pack_boxes(lo, hi)
    boxes[9, 3] = np.nan; boxes[9, 7] = np.inf                            # the pads are ignored
    for tree in (b4, None):
        res = rt.box_search_bvh4(tris, tree, boxes, brute_force=tree is None, stats=True)
        counts = np.diff(res[0].astype(np.int64)).tolist()
        assert counts[:7] == [12, 0, 0, 0, 0, 0, 0] and counts[7] >= 1 and counts[8:] == [0, 12], counts
        assert res[3]["rays_closest"] == 10
    assert np.array_equal(bc.walked(boxes), [True, False, False, False, False, False, False, True, True, True])
    # a NaN triangle is never accepted, whatever the box
    bad = tris.copy(); bad[9 * 3 + 4] = np.nan
    assert 3 not in rt.box_search_bvh4(bad, None, boxes[:1], brute_force=True)[1]
    assert len(rt.box_search_bvh4(bad, None, boxes[:1], brute_force=True)[1]) == 11
    # an empty batch: offsets = [0]; a leaf whose triangle index is out of range is skipped
    empty = rt.box_search_bvh4(tris, b4, np.zeros((0, 8), np.float32))
    assert empty[0].tolist() == [0] and len(empty[1]) == 0
    fewer = tris[:9 * 10]
    assert np.diff(rt.box_search_bvh4(fewer, b4, boxes[:1])[0].astype(np.int64)).tolist() == [10]

    tp, bp = tris.ctypes.data_as(C.POINTER(C.c_float)), b4.ctypes.data_as(C.POINTER(C.c_uint32))
    one = boxes[:1].copy()
    pp = one.ctypes.data_as(C.POINTER(rt.PtBox))
    raw = np.zeros(4, np.uint64); off = raw[:2]
    ent = rt._aligned_zeros((16, 4), np.uint32)
    op, ep = off.ctypes.data_as(C.POINTER(C.c_uint64)), ent.ctypes.data_as(C.POINTER(rt.PtOverlap))
    n12, w = C.c_uint32(12), C.c_uint64(b4.size)

    def search(tp=tp, bp=bp, w=w, pp=pp, n=1, flags=0, op=op, ep=ep, cap=16):
        return lib.pt_box_search_bvh4(tp, n12, bp, w, pp, C.c_uint64(n), C.c_uint32(flags), op, ep, C.c_uint64(cap), None)
    assert search() == 0 and off.tolist() == [0, 12]
    assert search(ep=None, cap=0) == 0 and off.tolist() == [0, 12]
    assert search(bp=None, w=C.c_uint64(0), flags=rt.PT_BOX_BRUTE_FORCE) == 0 and off.tolist() == [0, 12]
    assert search(flags=rt.PT_BOX_SIMPLE_KERNEL | rt.PT_BOX_STATS) == 0
    assert search(pp=None, ep=None, n=0, cap=0) == 0 and off[0] == 0
    # what the twin refuses, in which order and words: test_twin_query_errors.py
    assert C.sizeof(rt.PtOverlap) == 16 and C.sizeof(rt.PtBox) == 32
    assert (rt.PT_BOX_STATS, rt.PT_BOX_SIMPLE_KERNEL, rt.PT_BOX_BRUTE_FORCE) == (rt.PT_RADIUS_STATS, rt.PT_RADIUS_SIMPLE_KERNEL, rt.PT_RADIUS_BRUTE_FORCE)
