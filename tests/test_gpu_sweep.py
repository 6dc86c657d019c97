"""Sphere-cast queries on the GPU (pt_sweep_spheres / pt_sweep_spheres_host) against the host twin
pt_sweep_spheres_bvh4, word for word: t, prim, u, v of the persistent, the simple and the brute-force kernel on every item, and the counters
of PT_SWEEP_STATS.  The twin itself is pinned to the numpy restatement and to a float64 reference on the CPU (tests/test_sweep_host.py)."""

import numpy as np
import pytest

import crossing_cases as xc
import sweep_cases as sc
from refit_cases import host_trees, wave
from routecheck import run_case
from scenes import comb_bvh4

pytestmark = pytest.mark.gpu

N = 2048
COUNTERS = ("rays_closest", "rays_shadow", "nodes_examined", "tris_tested", "stack_drops", "max_stack", "samples")
f32 = np.float32


def same(got, want, what):
    for k, (a, b) in enumerate(zip(got, want)):
        assert sc.same_bits(a, b), (what, "t prim u v".split()[k], np.flatnonzero(sc.bits(a) != sc.bits(b))[:10])


def check_against_twin(rt, ctx, tris, bvh4, sweeps):
    """The three kernels, the counting variants and their counters against the twin over the same tree."""
    want = rt.sweep_spheres_bvh4(tris, bvh4, sweeps, stats=True)
    same(ctx.sweep_spheres(sweeps), want[:4], "persistent")
    same(ctx.sweep_spheres(sweeps, simple=True), want[:4], "simple")
    same(ctx.sweep_spheres(sweeps, stats=True), want[:4], "stats")
    st = ctx.stats()
    assert {k: st[k] for k in COUNTERS} == {k: want[4][k] for k in COUNTERS}
    brute = rt.sweep_spheres_bvh4(tris, None, sweeps, brute_force=True, stats=True)
    same(ctx.sweep_spheres(sweeps, brute_force=True), brute[:4], "brute")
    same(ctx.sweep_spheres(sweeps, brute_force=True, stats=True), brute[:4], "brute + stats")
    st = ctx.stats()
    assert {k: st[k] for k in COUNTERS} == {k: brute[4][k] for k in COUNTERS}
    return want


@pytest.mark.parametrize("name,accel", [("tetra", 0), ("torus", 0), ("soup1k", 1), ("dragon50k", 0), ("dragon50k", 2)])
def test_device_equals_twin_on_built_trees(rt, gpu_ctx, name, accel):
    tris = xc.geometry(rt, name)
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh(accel)
    want = check_against_twin(rt, gpu_ctx, tris, gpu_ctx.read_bvh4(), sc.sweep_set(rt, tris, N, 21))
    assert (want[1] != sc.MISS).sum() > N // 2 and want[4]["stack_drops"] == 0


def test_device_equals_twin_on_a_refitted_and_on_an_installed_tree(rt, orc, gpu_ctx):
    tris = xc.geometry(rt, "torus")
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh(0)
    built = gpu_ctx.read_bvh4()
    moved = wave(tris, 0.02, 3)
    gpu_ctx.update_triangles(moved)                                         # refitted in place
    refit = gpu_ctx.read_bvh4()
    assert np.array_equal(refit, rt.refit_bvh4(moved, built))
    check_against_twin(rt, gpu_ctx, moved, refit, sc.sweep_set(rt, moved, N, 22))
    soup = xc.geometry(rt, "soup1k")
    gpu_ctx.set_triangles(soup); gpu_ctx.set_bvh2(host_trees(rt, orc, soup, 0)[0])      # a BVH2 installed: collapsed on the way in
    check_against_twin(rt, gpu_ctx, soup, gpu_ctx.read_bvh4(), sc.sweep_set(rt, soup, N, 23))


@pytest.mark.parametrize("tree", ["comb", "sparse comb", "spoiled"])
def test_device_equals_twin_at_the_cap_and_on_a_spoiled_tree(rt, orc, gpu_ctx, tree):
    if tree == "spoiled":
        tris = xc.geometry(rt, "spoiled")
        b4 = xc.spoiled_tree(rt, orc, tris)
        sweeps = sc.sweep_set(rt, tris, N, 24)
    else:
        tris, b4 = comb_bvh4(xc.COMB_LEVELS, xc.COMB_SEED, all_hit=tree == "comb")
        rng = np.random.default_rng(3)
        org = np.stack([rng.uniform(-0.9, 0.9, N), rng.uniform(-0.9, 0.9, N), np.full(N, 2.0)], axis=1).astype(f32)
        d = np.stack([rng.uniform(-0.02, 0.02, N), rng.uniform(-0.02, 0.02, N), np.full(N, -1.0)], axis=1).astype(f32)
        sweeps = rt.pack_sweeps(org, d, rng.choice([0.0, 0.01, 0.05], N).astype(f32))
    gpu_ctx.set_triangles(tris); gpu_ctx.set_bvh4(b4)
    want = check_against_twin(rt, gpu_ctx, tris, gpu_ctx.read_bvh4(), sweeps)
    assert (want[4]["stack_drops"] > 0) == (tree == "comb")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batch_sizes(rt, gpu_ctx, n):
    tris = xc.geometry(rt, "soup1k")
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh()
    sweeps = sc.sweep_set(rt, tris, n, 30 + n)
    want = rt.sweep_spheres_bvh4(tris, gpu_ctx.read_bvh4(), sweeps)
    for kw in ({}, {"simple": True}, {"brute_force": True}):
        same(gpu_ctx.sweep_spheres(sweeps, **kw), want if not kw.get("brute_force") else rt.sweep_spheres_bvh4(tris, None, sweeps, brute_force=True), kw)


def test_one_wavefront_of_mixed_items(rt, gpu_ctx):
    """Items that are not walked, misses, overlaps at t = 0 and one sphere of four scene extents' radius in one wavefront."""
    tris = xc.geometry(rt, "torus")
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh()
    ext = sc.extent_of(tris)
    S = sc.sweep_set(rt, tris, 64, 9)
    S[0::8, 0] = np.nan; S[1::16, 3] = 0.0; S[2::16, 7] = -1.0; S[3::16, 4:7] = 0.0; S[9::16, 7] = np.nan      # not walked
    S[4::8, 0:3] = [5, 5, 5]; S[4::8, 4:7] = [1, 0, 0]                                  # misses: moving away, outside the scene
    centroids = np.asarray(tris, f32).reshape(-1, 3, 3).mean(axis=1)
    S[5::8, 0:3] = centroids[:8]; S[5::8, 7] = 0.05 * ext; S[5::8, 3] = np.inf           # overlapping at the start
    S[6, 7] = 4 * ext                                                                   # holds the whole scene
    want = check_against_twin(rt, gpu_ctx, tris, gpu_ctx.read_bvh4(), S)
    assert np.all(want[1][0::8] == sc.MISS) and np.all(want[1][4::8] == sc.MISS) and np.all(want[0][5::8] == 0) and want[0][6] == 0


@pytest.mark.parametrize("case", ["torch_route_equals_the_host_route", "device_route_into_guarded_tensors", "no_host_synchronisation_then_a_scene_change", "errors"])
def test_torch_route(case):
    """The device route: tests/sweep_torch_cases.py in a child process (torch is imported before the package there)."""
    run_case("sweep_torch_cases", case)
