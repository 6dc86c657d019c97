"""Batched closest-point queries on the GPU (pt_closest_points / pt_closest_points_host) against the host twin
pt_closest_points_bvh4, bit for bit: dist, prim, u, v of the persistent and of the simple kernel on every point, and the counters of
PT_CLOSEST_STATS.  The twin itself is pinned to an independent float64 reference on the CPU (tests/test_closest_points_host.py)."""

import numpy as np
import pytest

import closest_cases as cc
import closestref
from refit_cases import host_trees, wave
from routecheck import run_case
from scenes import TETRA, comb_bvh4, random_soup, spoil_bvh4

pytestmark = pytest.mark.gpu

SCENE_SEED = 20260109
KERNELS = [False, True]       # simple=False: the persistent kernel; True: the one-point-per-thread kernel
COUNTERS = ("rays_closest", "rays_shadow", "nodes_examined", "tris_tested", "stack_drops", "max_stack", "samples")


def soup(name):
    return {"tetra": lambda: TETRA, "soup1k": lambda: random_soup(1000, 3), "soup120k": lambda: random_soup(120000, 5, size=0.02)}[name]()


def check_against_twin(rt, ctx, tris, bvh4, pts, r_max=None):
    """Both kernels, the counting variant and its counters against the twin over the same tree."""
    want = rt.closest_points_bvh4(tris, bvh4, pts, r_max=r_max, stats=True)
    for simple in KERNELS:
        got = ctx.closest_points(pts, r_max=r_max, simple=simple)
        for k, (a, b) in enumerate(zip(got, want[:4])):
            assert cc.same_bits(a, b), (simple, "dist prim u v".split()[k], np.flatnonzero(cc.bits(a) != cc.bits(b))[:10])
    got = ctx.closest_points(pts, r_max=r_max, stats=True)
    st = ctx.stats()
    for a, b in zip(got, want[:4]):
        assert cc.same_bits(a, b)
    assert {k: st[k] for k in COUNTERS} == {k: want[4][k] for k in COUNTERS}
    return want


@pytest.mark.parametrize("accel", [0, 1, 2])
@pytest.mark.parametrize("name", ["tetra", "soup1k", "soup120k"])
def test_device_equals_twin_on_built_installed_and_refitted_trees(rt, orc, gpu_ctx, name, accel):
    tris = soup(name)
    pts = cc.query_points(tris, 20000, 7)
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh(accel)                  # device-built
    built = gpu_ctx.read_bvh4()
    check_against_twin(rt, gpu_ctx, tris, built, pts)
    moved = wave(tris, 0.02, 3)
    gpu_ctx.update_triangles(moved)                                         # refitted in place
    pts2 = cc.query_points(moved, 20000, 8)
    refit = gpu_ctx.read_bvh4()
    assert np.array_equal(refit, rt.refit_bvh4(moved, built))
    check_against_twin(rt, gpu_ctx, moved, refit, pts2)
    host = host_trees(rt, orc, tris, accel)[1]
    gpu_ctx.set_triangles(tris); gpu_ctx.set_bvh4(host)                     # installed
    want = check_against_twin(rt, gpu_ctx, tris, host, pts)
    rng = np.random.default_rng(5)
    r_max = np.maximum(want[0] * rng.choice(np.float32([0.5, 1.5]), len(pts)), np.float32(1e-6)).astype(np.float32)
    check_against_twin(rt, gpu_ctx, tris, host, pts, r_max=r_max)
    brute = gpu_ctx.closest_points(pts, brute_force=True)
    for a, b in zip(brute, rt.closest_points_bvh4(tris, None, pts, brute_force=True)):
        assert cc.same_bits(a, b)


def test_stack_cap_comb(rt, gpu_ctx):
    tris, bvh4 = comb_bvh4(30, 5)
    gpu_ctx.set_triangles(tris); gpu_ctx.set_bvh4(bvh4)
    pts = cc.query_points(tris, 20000, 9)
    want = check_against_twin(rt, gpu_ctx, tris, bvh4, pts)
    assert want[4]["stack_drops"] > 0 and want[4]["max_stack"] == 64
    moved = wave(tris, 0.02, 3)
    gpu_ctx.update_triangles(moved)
    check_against_twin(rt, gpu_ctx, moved, gpu_ctx.read_bvh4(), cc.query_points(moved, 20000, 10))


def test_spoiled_tree(rt, orc, gpu_ctx):
    tris = random_soup(3000, 23)
    bvh4, n_oob, n_deg = spoil_bvh4(host_trees(rt, orc, tris, 0)[1], 9)
    assert n_oob > 0 and n_deg > 0
    gpu_ctx.set_triangles(tris); gpu_ctx.set_bvh4(bvh4)
    pts = cc.query_points(tris, 20000, 11)
    check_against_twin(rt, gpu_ctx, tris, bvh4, pts)
    moved = wave(tris, 0.02, 3)
    gpu_ctx.update_triangles(moved)
    check_against_twin(rt, gpu_ctx, moved, gpu_ctx.read_bvh4(), cc.query_points(moved, 20000, 12))


def test_points_that_are_not_walked_and_batch_shapes(rt, gpu_ctx):
    tris = random_soup(1000, 3)
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh()
    bvh4 = gpu_ctx.read_bvh4()
    bad = np.tile(np.float32([0.1, 0.2, -0.3, np.inf]), (7, 1))
    bad[0, 0] = np.nan; bad[1, 1] = np.nan; bad[2, 2] = np.nan; bad[3, 3] = np.nan; bad[4, 3] = 0.0; bad[5, 3] = -1.0
    want = check_against_twin(rt, gpu_ctx, tris, bvh4, bad)
    assert list(want[1][:6]) == [cc.MISS] * 6 and want[1][6] != cc.MISS
    for n in (0, 1, 63, 65, (1 << 20) + 3):
        pts = cc.query_points(tris, max(n, 8), 41)[:n]
        a, b = gpu_ctx.closest_points(pts), gpu_ctx.closest_points(pts, simple=True)
        want = rt.closest_points_bvh4(tris, bvh4, pts)
        for x, y, z in zip(a, b, want):
            assert len(x) == n and cc.same_bits(x, y) and cc.same_bits(x, z)


def test_full_size_dragon(rt, gpu_ctx):
    """C2, 871,414 triangles: persistent == simple on 200,000 points; the tree's dist bits == the brute-force kernel's on 20,000 of them
    (prim equal or the same d2 bits); 500 of them against the float64 reference."""
    tris = rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 871414, SCENE_SEED)
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh()
    pts = cc.query_points(tris, 200000, 13)
    a, b = gpu_ctx.closest_points(pts), gpu_ctx.closest_points(pts, simple=True)
    for x, y in zip(a, b):
        assert cc.same_bits(x, y)
    gpu_ctx.closest_points(pts, stats=True)
    assert gpu_ctx.stats()["stack_drops"] == 0
    sub = np.sort(np.random.default_rng(1).choice(len(pts), 20000, replace=False))
    brute = gpu_ctx.closest_points(pts[sub], brute_force=True)
    cc.check_same_minimum(pts[sub], tris, [x[sub] for x in a], brute, lambda p, prim: cc.product_d2(p, tris, prim))
    few = sub[:: len(sub) // 500][:500]
    cc.check_against_float64(pts[few], tris, [x[few] for x in a], closestref.nearest(pts[few], tris)[0])


@pytest.mark.parametrize("case", ["torch_route_equals_the_host_route", "ordering_with_batched_frames_and_scene_changes", "errors"])
def test_torch_route(case):
    """The zero-copy torch route vs the host route, ordering behind pt_set_batch frames and before scene changes, every error code:
    tests/closest_torch_cases.py in a child process (torch is imported before the package there)."""
    run_case("closest_torch_cases", case)
