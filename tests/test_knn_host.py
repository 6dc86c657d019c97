"""k-nearest queries on the CPU: the host twin pt_nearest_k_bvh4 (include/mi355pt.h) against a float32 restatement of
the brute-force rows in numpy, the tree walk against brute force (both on the twin) with no exemptions, k = 1 against the pinned
closest-point query, the relation to the radius lists, exact ties in visit order, short and empty rows, the stack cap on the comb, the
error codes, and a float64 statement of the k smallest distances.  Every result is an integer or a bit pattern, so every check but the
last is an equality.  The GPU tests (tests/test_gpu_knn.py) pin the kernels to this twin bit for bit, order included."""
import ctypes as C

import numpy as np
import pytest

import closest_cases as clc
import closestref
import crossing_cases as cc
import knn_cases as kc
import radius_cases as rc
from scenes import TETRA


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
    for radii in kc.RADII:
        pts = kc.point_records(rt, tris, radii)
        ref = kc.numpy_rows(pts, tris)                                    # the 64 smallest d2 < r2, sorted; u, v per prim
        for k in kc.KS:
            got = rt.nearest_k_bvh4(tris, None, pts, k, brute_force=True, stats=True)
            assert got[0].shape == (len(pts), k) and got[1].dtype == np.uint32
            w = kc.words(got)
            assert np.array_equal(w, ref[:, :k]), (radii, k, np.flatnonzero((w != ref[:, :k]).any(axis=(1, 2)))[:10])
            assert got[4] == dict(rays_closest=len(pts), rays_shadow=0, nodes_examined=0, tris_tested=len(pts) * (tris.size // 9),
                                  stack_drops=0, max_stack=0, samples=0)
        assert bool((~kc.listed(ref)).all(1).any()) == (radii == "drawn")                                # empty rows with radii only


@pytest.mark.parametrize("name", cc.SCENES)
def test_walk_against_brute_force_on_every_tree(rt, cases, name):
    for label, tris, b4 in cases(name)[1]:
        for radii in kc.RADII:
            pts = kc.point_records(rt, tris, radii)
            rows = []
            for k in kc.KS:
                walk = rt.nearest_k_bvh4(tris, b4, pts, k, stats=True)
                brute = rt.nearest_k_bvh4(tris, None, pts, k, brute_force=True)
                st = walk[4]
                print("%s %s %s k=%d: counters %s" % (name, label, radii, k, st))
                assert st["stack_drops"] == 0 and st["rays_closest"] == len(pts) and 1 <= st["max_stack"] <= 64, (label, st)
                w, b = kc.words(walk), kc.words(brute)
                assert np.array_equal(w[:, :, 0], b[:, :, 0]), (label, radii, k, np.flatnonzero((w[:, :, 0] != b[:, :, 0]).any(1))[:10])
                kc.listed(w)
                kc.assert_distinct_prims(w)
                kc.assert_same_rows(walk, rt.nearest_k_bvh4(tris, b4, pts, k, simple=True))       # the twin is deterministic, and takes the flag
                rows.append(w)
            kc.assert_entries_are_radius_entries(rt, tris, pts, rows)


@pytest.mark.parametrize("name", cc.SCENES)
def test_k_1_is_the_closest_point_query(rt, cases, name):
    for label, tris, b4 in cases(name)[1]:
        for radii in kc.RADII:
            pts = kc.point_records(rt, tris, radii)
            for tree in (b4, None):
                one = rt.nearest_k_bvh4(tris, tree, pts, 1, brute_force=tree is None, stats=True)
                cp = rt.closest_points_bvh4(tris, tree, pts, brute_force=tree is None, stats=True)
                assert all(clc.same_bits(a[:, 0], b) for a, b in zip((one[0], one[2], one[3]), (cp[0], cp[2], cp[3]))), (label, radii)
                assert np.array_equal(one[1][:, 0], cp[1]), (label, radii)
                assert one[4] == cp[4], (label, radii, one[4], cp[4])       # the same walk: the same counters


@pytest.mark.parametrize("name", cc.SCENES)
def test_relation_to_the_radius_lists(rt, cases, name):
    for label, tris, b4 in cases(name)[1]:
        pts = kc.point_records(rt, tris, "drawn")
        off, ent = rc.words(rt.radius_search_bvh4(tris, b4, pts))
        counts = np.diff(off)
        assert counts.max() >= 2 and (counts == 0).any()                  # both branches below are taken
        for k in kc.KS:
            w = kc.words(rt.nearest_k_bvh4(tris, b4, pts, k))
            held = kc.listed(w).sum(1)
            assert np.array_equal(held, np.minimum(counts, k)), (label, k)
            for i in range(len(pts)):
                lst = ent[off[i]:off[i + 1]]
                row = w[i, :held[i]]
                if counts[i] <= k:                                        # the row without its padding is the radius list, as a set
                    assert np.array_equal(row[np.argsort(row[:, 1])], lst[np.argsort(lst[:, 1])]), (label, k, i)
                else:                                                     # the k smallest dist of the list (bits of dist >= 0 sort as integers)
                    assert np.array_equal(row[:, 0], np.sort(lst[:, 0])[:k]), (label, k, i)


def test_exact_ties_keep_visit_order(rt, orc):
    tris = kc.DOUBLED_TETRA
    b4 = cc.host_trees(rt, orc, tris, 0)[1]
    pts = kc.point_records(rt, tris, "inf", n=400)
    off, ent = rc.words(rt.radius_search_bvh4(tris, b4, pts))            # r_max = +inf: every triangle, in visit order
    assert np.all(np.diff(off) == 8)
    d2_of = clc.product_d2(np.repeat(pts, 8, axis=0), tris, ent[:, 1].astype(np.int64)).reshape(-1, 8)
    for k in (1, 2, 3, 8):
        walk = kc.words(rt.nearest_k_bvh4(tris, b4, pts, k, stats=True))
        brute = kc.words(rt.nearest_k_bvh4(tris, None, pts, k, brute_force=True))
        assert np.array_equal(walk[:, :, 0], brute[:, :, 0])
        if k >= 2:
            assert (walk[:, 0, 0] == walk[:, 1, 0]).all()                # every triangle twice: adjacent entries with equal dist bits
        for i in range(len(pts)):
            seq = [(d2_of[i, j], int(ent[8 * i + j, 1])) for j in range(8)]
            want = [t for _, t in kc.list_rule(seq, k)]
            assert walk[i, :, 1].tolist() == want, (k, i, walk[i, :, 1].tolist(), want)
        # brute force: ties in index order
        for row in brute[:, :, 1].tolist():                               # (equal dist bits may hide unequal d2: only the twins are compared)
            assert all(t - 4 in row and row.index(t - 4) < row.index(t) for t in row if t >= 4), (k, row)


def test_short_and_empty_rows(rt, orc):
    tris = TETRA.reshape(-1)
    b4 = cc.host_trees(rt, orc, tris, 0)[1]
    r = np.float32([np.inf, np.nan, 0.0, -1.0, np.inf, np.inf, np.inf, 2.0])
    pts = rt.pack_points(np.full((8, 3), 0.1, np.float32), r)
    pts[4, 0] = np.nan; pts[5, 1] = np.nan; pts[6, 2] = np.nan
    for k in (5, 64):
        for tree in (b4, None):
            w = kc.words(rt.nearest_k_bvh4(tris, tree, pts, k, brute_force=tree is None))
            held = kc.listed(w).sum(1)
            assert held.tolist() == [4, 0, 0, 0, 0, 0, 0, 4], (k, held)    # k > num_tris: a padded tail; not walked: fully padded
            assert np.all(w[0, 4:] == kc.PAD) and np.all(w[1:7] == kc.PAD)
            assert sorted(w[0, :4, 1].tolist()) == [0, 1, 2, 3] and np.all(np.diff(w[0, :4, 0].view(np.float32)) >= 0)
    # an empty batch, and a leaf whose triangle index is out of range is skipped
    assert rt.nearest_k_bvh4(tris, b4, np.zeros((0, 4), np.float32), 3)[0].shape == (0, 3)
    w = kc.words(rt.nearest_k_bvh4(tris[:18], b4, pts[:1], 4))
    assert sorted(w[0, :2, 1].tolist()) == [0, 1] and np.all(w[0, 2:] == kc.PAD)


def test_comb_drops_pushes_and_lists_true_candidates(rt):
    tris, b4 = cc.geometry(rt, "comb"), cc.comb_tree()
    pts = kc.comb_points(rt, 64)
    rows = []
    for k in kc.KS:
        walk = rt.nearest_k_bvh4(tris, b4, pts, k, stats=True)
        st = walk[4]
        print("comb k=%d: counters %s" % (k, st))
        assert st["stack_drops"] > 0 and st["max_stack"] == 64 and st["nodes_examined"] > 0 and st["tris_tested"] > 0
        w = kc.words(walk)
        kc.assert_distinct_prims(w)
        rows.append(w)
    kc.assert_entries_are_radius_entries(rt, tris, pts, rows)             # a subset of brute force's candidates


def test_arguments(rt, orc):
    lib = rt.lib
    tris = cc.geometry(rt, "box")
    b4 = np.ascontiguousarray(cc.host_trees(rt, orc, tris, 0)[1], np.uint32)
    tp, bp = tris.ctypes.data_as(C.POINTER(C.c_float)), b4.ctypes.data_as(C.POINTER(C.c_uint32))
    one = rt.pack_points([[0, 0, 0]], 2.0)
    pp = one.ctypes.data_as(C.POINTER(rt.PtPoint))
    out = rt._aligned_zeros((64, 4), np.uint32)
    op = out.ctypes.data_as(C.POINTER(rt.PtClosest))
    n12, w = C.c_uint32(12), C.c_uint64(b4.size)

    def call(tp=tp, bp=bp, w=w, pp=pp, n=1, k=3, flags=0, op=op):
        return lib.pt_nearest_k_bvh4(tp, n12, bp, w, pp, C.c_uint64(n), C.c_uint32(k), C.c_uint32(flags), op, None)
    assert call() == 0 and np.all(out[:3, 1] < 12)
    assert call(k=64) == 0
    assert call(flags=rt.PT_NEAREST_SIMPLE_KERNEL | rt.PT_NEAREST_STATS) == 0
    # what the twin refuses, in which order and words: test_twin_query_errors.py
    with pytest.raises(rt.PtError):
        rt.nearest_k_bvh4(tris, b4, one, 0)
    with pytest.raises(rt.PtError):
        rt.nearest_k_bvh4(tris, b4, one, 65)
    assert rt.PT_NEAREST_MAX_K == 64 and (rt.PT_NEAREST_STATS, rt.PT_NEAREST_SIMPLE_KERNEL, rt.PT_NEAREST_BRUTE_FORCE) == (1, 2, 4)


@pytest.mark.parametrize("name", cc.SCENES)
def test_against_float64(rt, cases, name):
    """For every entry j the float64 distance of the listed prim lies within 2 * tolerance of the j-th smallest float64 distance: one
    tolerance bounds each f32 distance, order statistics move by no more than their inputs, the second covers the listed triangle itself."""
    smallest = {}
    worst = 0.0
    for label, tris, b4 in cases(name)[1]:
        for radii in kc.RADII:
            pts = kc.point_records(rt, tris, radii)
            tol = clc.tolerance(pts, tris)
            key = (id(tris), radii)
            if key not in smallest:
                smallest[key] = kc.smallest_float64(pts, tris)
            ref = smallest[key]
            for k in kc.KS:
                w = kc.words(rt.nearest_k_bvh4(tris, b4, pts, k))
                pi, j = np.nonzero(kc.listed(w))
                d = closestref.distance_to(pts[pi, :3].astype(np.float64), tris, w[pi, j, 1])
                dev = np.abs(d - ref[pi, j])
                worst = max(worst, float(dev.max(initial=0.0)) / tol)
                assert np.all(dev <= 2 * tol), (label, radii, k, float(dev.max()), tol)
                if radii == "inf":
                    assert len(pi) == len(pts) * min(k, tris.size // 9)
    print("%s: largest deviation %.3f tolerances" % (name, worst))
