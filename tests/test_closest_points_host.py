"""Closest-point queries on the CPU: the host twin pt_closest_points_bvh4 (include/mi355pt.h) against the independent
float64 reference (tests/closestref.py), the tree walk against brute force (both on the twin), r_max, the points that are not walked, the
error codes, the counters and the record layouts.  The GPU tests (tests/test_gpu_closest_points.py) pin the kernels to this twin bit for bit.

The largest deviation from the float64 reference measured here is written next to closest_cases.TOL_K."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import closest_cases as cc
import closestref
from refit_cases import host_trees, wave
from scenes import TETRA, comb_bvh4, random_soup, spoil_bvh4

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SCENE_SEED = 20260109
N_POINTS = 20000
PT_ERR_INVALID_ARG, PT_ERR_BAD_BVH = 1, 5        # include/mi355pt.h PtStatus
SCENES = ["tetra", "soup1k", "soup120k", "dragon50k", "sponza_slice", "comb", "spoiled"]


def geometry(rt, name):
    if name == "tetra":
        return TETRA
    if name == "soup1k":
        return random_soup(1000, 3)
    if name == "soup120k":
        return random_soup(120000, 5, size=0.02)
    if name == "dragon50k":        # straddles every coordinate plane: internal boxes with bounds flushed to +-0
        return rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 50000, SCENE_SEED)
    if name == "sponza_slice":     # the first 30,000 triangles of the sponza-class mesh: large flat walls next to small detail
        return np.ascontiguousarray(rt.procedural_scene(rt.SCENE_SPONZA_CLASS, 262144, SCENE_SEED)[:9 * 30000])
    if name == "comb":
        return comb_bvh4(30, 5)[0]
    assert name == "spoiled"
    return random_soup(3000, 23)


def trees(rt, orc, name, tris):
    """[(label, bvh4)] over `tris`."""
    if name == "comb":
        return [("comb", comb_bvh4(30, 5)[1])]
    if name == "spoiled":
        b4, n_oob, n_deg = spoil_bvh4(host_trees(rt, orc, tris, 0)[1], 9)
        assert n_oob > 0 and n_deg > 0
        return [("spoiled", b4)]
    return [("accel%d" % a, host_trees(rt, orc, tris, a)[1]) for a in (0, 1, 2)]


@pytest.mark.parametrize("name", SCENES)
def test_twin_against_float64_and_tree_against_brute_force(rt, orc, name):
    base = geometry(rt, name)
    worst = []
    for moved in (False, True):
        tris = wave(base, 0.02, 3) if moved else base
        # after a refit the topology is the one built over the base geometry, the boxes are those of the displaced vertices
        forest = [(label + ("+refit" if moved else ""), rt.refit_bvh4(tris, b4) if moved else b4) for label, b4 in trees(rt, orc, name, base)]
        pts = cc.query_points(tris, N_POINTS, 7 + moved)
        brute = rt.closest_points_bvh4(tris, None, pts, brute_force=True)
        ref_all = closestref.nearest(pts, tris)[0]
        cc.check_against_float64(pts, tris, brute, ref_all, worst)                       # the brute-force route: every triangle
        # the arithmetic of DESIGN.md section 15, restated in numpy float32: the same bits
        u, v, d2 = cc.product_uv_d2(pts, tris, brute[1])
        assert cc.same_bits(np.sqrt(d2), brute[0]) and cc.same_bits(u, brute[2]) and cc.same_bits(v, brute[3])
        for label, b4 in forest:
            res = rt.closest_points_bvh4(tris, b4, pts, stats=True)
            st = res[4]
            found = res[1] != cc.MISS
            assert st["rays_closest"] == len(pts) and st["tris_tested"] >= found.sum() and 1 <= st["max_stack"] <= 64, (label, st)
            assert (st["stack_drops"] > 0) == (name == "comb"), (label, st)             # the cap is reached on the comb only
            u, v, d2 = cc.product_uv_d2(pts[found], tris, res[1][found])
            assert cc.same_bits(np.sqrt(d2), res[0][found]) and cc.same_bits(u, res[2][found]) and cc.same_bits(v, res[3][found])
            if name == "comb":
                # pushes were dropped: the walk may miss the minimum, but what it returns is a real triangle at its real distance
                assert np.all(res[0] >= brute[0])
                continue
            if name == "spoiled":
                # the damaged tree cannot reach every triangle: brute force and the float64 reference over the ones it can
                mask = cc.reachable_triangles(b4, tris.size // 9)
                assert 0 < mask.sum() < mask.size
                hidden = np.array(tris, np.float32).reshape(-1, 9); hidden[~mask] = np.nan      # a NaN triangle is never accepted
                want = rt.closest_points_bvh4(hidden.reshape(-1), None, pts, brute_force=True)
                ref = closestref.nearest(pts, tris, mask=mask)[0]
            else:
                want, ref = brute, ref_all
            cc.check_same_minimum(pts, tris, res, want, lambda p, prim: cc.product_d2(p, tris, prim))
            cc.check_against_float64(pts, tris, res[:4], ref, worst)
    print("%s: largest deviation from float64 %.3f units (MEASURED_K = %g, TOL_K = %g)" % (name, max(worst), cc.MEASURED_K, cc.TOL_K))


def test_r_max_prunes_and_nothing_else(rt, orc):
    tris = random_soup(1000, 3)
    b4 = host_trees(rt, orc, tris, 0)[1]
    pts = cc.query_points(tris, N_POINTS, 11)
    dist, prim, u, v = rt.closest_points_bvh4(tris, b4, pts)
    rng = np.random.default_rng(5)
    r_max = np.maximum(dist * rng.choice(np.float32([0.5, 1.5]), len(pts)), np.float32(1e-6)).astype(np.float32)
    for kw in ({}, {"brute_force": True}):
        d2, p2, u2, v2 = rt.closest_points_bvh4(tris, b4, pts, r_max=r_max, **kw)
        want = dist < r_max
        assert 0 < want.sum() < len(pts)
        assert np.array_equal(p2 != cc.MISS, want)
        assert cc.same_bits(d2[want], dist[want]) and np.array_equal(p2[want], prim[want]) and cc.same_bits(u2[want], u[want]) and cc.same_bits(v2[want], v[want])
        assert np.all(np.isposinf(d2[~want])) and np.all(u2[~want] == 0) and np.all(v2[~want] == 0)


def test_points_that_are_not_walked(rt, orc):
    tris = random_soup(1000, 3)
    b4 = host_trees(rt, orc, tris, 0)[1]
    good = np.float32([0.1, 0.2, -0.3, np.inf])
    bad = np.tile(good, (7, 1))
    bad[0, 0] = np.nan; bad[1, 1] = np.nan; bad[2, 2] = np.nan; bad[3, 3] = np.nan; bad[4, 3] = 0.0; bad[5, 3] = -1.0
    for kw in ({}, {"brute_force": True}):
        dist, prim, u, v, st = rt.closest_points_bvh4(tris, b4, bad, stats=True, **kw)
        assert list(prim[:6]) == [cc.MISS] * 6 and np.all(np.isposinf(dist[:6])) and np.all(u[:6] == 0) and np.all(v[:6] == 0)
        assert prim[6] != cc.MISS and np.isfinite(dist[6])
        one = rt.closest_points_bvh4(tris, b4, good[None, :], stats=True, **kw)[4]
        assert st["rays_closest"] == 7 and st["tris_tested"] == one["tris_tested"] and st["nodes_examined"] == one["nodes_examined"]


def test_empty_scene_no_points_and_error_codes(rt, orc):
    import ctypes as C
    pts = cc.query_points(TETRA, 64, 3)
    empty = np.zeros(0, np.float32)
    for b4, kw in ((np.array([0], np.uint32), {}), (None, {"brute_force": True})):
        dist, prim, u, v = rt.closest_points_bvh4(empty, b4, pts, **kw)
        assert np.all(prim == cc.MISS) and np.all(np.isposinf(dist)) and np.all(u == 0) and np.all(v == 0)
    b4 = host_trees(rt, orc, TETRA, 0)[1]
    assert all(len(x) == 0 for x in rt.closest_points_bvh4(TETRA, b4, np.zeros((0, 3), np.float32)))
    with pytest.raises(rt.PtError) as e:
        rt.closest_points_bvh4(TETRA, None, pts)                                       # no tree without PT_CLOSEST_BRUTE_FORCE
    assert e.value.code == PT_ERR_INVALID_ARG
    out = np.zeros((64, 4), np.uint32)
    p4 = rt.pack_points(pts)
    args = (TETRA.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint32(4), b4.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_uint64(b4.size))
    rc = rt.lib.pt_closest_points_bvh4(*args, p4.ctypes.data_as(C.POINTER(rt.PtPoint)), C.c_uint64(64), C.c_uint32(8), out.ctypes.data_as(C.POINTER(rt.PtClosest)), None)
    assert rc == PT_ERR_INVALID_ARG                                                  # an unknown flag
    rc = rt.lib.pt_closest_points_bvh4(*args, None, C.c_uint64(64), C.c_uint32(0), out.ctypes.data_as(C.POINTER(rt.PtClosest)), None)
    assert rc == PT_ERR_INVALID_ARG
    with pytest.raises(rt.PtError) as e:
        rt.closest_points_bvh4(TETRA, b4[:9], pts)                                     # shorter than its node count
    assert e.value.code == PT_ERR_BAD_BVH


def test_a_single_triangle_every_region(rt):
    """One triangle, its root a leaf: points over every region of its plane and off it, against float64."""
    tri = np.float32([0.1, 0.0, 0.0, 1.0, 0.2, 0.0, 0.3, 0.9, 0.1])
    b4 = np.array([1, 0, 0, 0, cc.INVALID, cc.INVALID, cc.INVALID, cc.INVALID, cc.LEAF | 0], np.uint32)
    b4[1:4] = np.array(__import__("scenes").pack_box((0.1, 0.0, 0.0), (1.0, 0.9, 0.1)), np.uint32)
    rng = np.random.default_rng(2)
    pts = rng.uniform(-2, 3, (N_POINTS, 3)).astype(np.float32)
    res = rt.closest_points_bvh4(tri, b4, pts)
    brute = rt.closest_points_bvh4(tri, None, pts, brute_force=True)
    for a, b in zip(res, brute):
        assert cc.same_bits(a, b)
    dist, prim, u, v = res
    assert np.all(prim == 0)
    for lo, hi in ((0, 0), (1, 0), (0, 1)):                                            # the three vertex regions are met exactly
        assert np.any((u == lo) & (v == hi))
    assert np.any((u > 0) & (v > 0) & (u + v < 1)) and np.any((u > 0) & (u < 1) & (v == 0)) and np.any((v > 0) & (v < 1) & (u == 0))
    cc.check_against_float64(pts, tri, res, closestref.nearest(pts, tri)[0])


HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")


@pytest.mark.skipif(HIPCC is None and shutil.which("cc") is None and shutil.which("gcc") is None, reason="no C compiler")
def test_header_records_are_16_bytes(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stddef.h>\n#include "mi355pt.h"\n'
        "_Static_assert(sizeof(PtPoint) == 16 && offsetof(PtPoint, r_max) == 12, \"PtPoint\");\n"
        "_Static_assert(sizeof(PtClosest) == 16, \"PtClosest\");\n"
        "_Static_assert(offsetof(PtClosest, prim) == 4 && offsetof(PtClosest, u) == 8 && offsetof(PtClosest, v) == 12, \"PtClosest fields\");\n"
        "_Static_assert(PT_CLOSEST_STATS == 1 && PT_CLOSEST_SIMPLE_KERNEL == 2 && PT_CLOSEST_BRUTE_FORCE == 4, \"flags\");\n")
    cc_ = shutil.which("cc") or shutil.which("gcc") or os.path.join(os.path.dirname(HIPCC), "..", "llvm", "bin", "clang")
    subprocess.run([cc_, "-std=c11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], check=True, capture_output=True, timeout=120)


def test_python_records_match_the_header(rt):
    import ctypes as C
    assert C.sizeof(rt.PtPoint) == 16 and C.sizeof(rt.PtClosest) == 16
    assert rt.PtPoint.r_max.offset == 12 and rt.PtClosest.prim.offset == 4 and rt.PtClosest.u.offset == 8 and rt.PtClosest.v.offset == 12
    assert (rt.PT_CLOSEST_STATS, rt.PT_CLOSEST_SIMPLE_KERNEL, rt.PT_CLOSEST_BRUTE_FORCE) == (1, 2, 4)
    p = rt.pack_points(np.float32([[1, 2, 3], [4, 5, 6]]), r_max=[0.5, 2.0])
    assert p.shape == (2, 4) and p.ctypes.data % 16 == 0 and list(p[1]) == [4, 5, 6, 2.0]
    assert np.all(np.isposinf(rt.pack_points(np.zeros((3, 3), np.float32))[:, 3]))
