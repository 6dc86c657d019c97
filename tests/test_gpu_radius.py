"""Radius queries on the GPU (pt_radius_count / pt_radius_search).  Every result is an integer or a bit pattern, so
every check is an equality: of the persistent, the one-point-per-thread and the brute-force kernels with the host twin
(tests/test_radius_host.py pins that to a float32 restatement, to brute force and to float64) -- counts, offsets, the entries' bits and their
ORDER, and the counters of PT_RADIUS_STATS; of truncated results with the full one; of the counts with the offsets; of the nearest entry with
the closest-point query."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import closest_cases as clc
import crossing_cases as cc
import radius_cases as rc
from radius_cases import install
from routecheck import run_case

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N_POINTS = 2048
SCENES = ["tetra", "torus", "soup1k", "dragon50k_l0", "dragon50k_l2", "refit", "bvh2", "comb", "spoiled"]
COUNTERS = ("rays_closest", "rays_shadow", "nodes_examined", "tris_tested", "stack_drops", "max_stack", "samples")


def points_for(rt, name, tris, n=N_POINTS):
    if name != "comb":
        return rc.point_records(rt, tris, n=n)
    # above the comb with radii that reach every level: the walk runs into the 64-entry cap; a quarter too far away to reach anything
    rng = np.random.default_rng(3)
    p = np.stack([rng.uniform(-0.9, 0.9, n), rng.uniform(-0.9, 0.9, n), rng.uniform(1.0, 2.0, n)], axis=1).astype(np.float32)
    r = np.full(n, np.inf, np.float32); r[-(n // 4):] = 0.05
    return rt.pack_points(p, r)


@pytest.mark.parametrize("name", SCENES)
def test_search_equals_the_host_twin(rt, orc, gpu_ctx, name):
    tris, b4 = install(rt, orc, gpu_ctx, name)
    pts = points_for(rt, name, tris)
    want = rt.radius_search_bvh4(tris, b4, pts, stats=True)
    counts = np.diff(want[0].astype(np.int64)).astype(np.uint32)
    assert counts.max() >= 2 and (counts == 0).any()
    for simple in (False, True):
        got = gpu_ctx.radius_search(pts, simple=simple)
        assert got[0].dtype == np.uint64 and got[2].dtype == np.uint32
        rc.assert_same_lists(got, want, ordered=True)
        assert np.array_equal(gpu_ctx.radius_count(pts, simple=simple), counts)
    got = gpu_ctx.radius_search(pts, stats=True)
    st = gpu_ctx.stats()
    rc.assert_same_lists(got, want, ordered=True)
    assert {k: st[k] for k in COUNTERS} == want[5], (st, want[5])
    assert (st["stack_drops"] > 0) == (name == "comb")
    assert np.array_equal(gpu_ctx.radius_count(pts, stats=True), counts)
    st = gpu_ctx.stats()
    assert {k: st[k] for k in COUNTERS} == want[5], (st, want[5])
    brute = rt.radius_search_bvh4(tris, None, pts, brute_force=True, stats=True)
    rc.assert_same_lists(gpu_ctx.radius_search(pts, brute_force=True), brute, ordered=True)
    rc.assert_same_lists(gpu_ctx.radius_search(pts, brute_force=True, stats=True), brute, ordered=True)
    st = gpu_ctx.stats()
    assert {k: st[k] for k in COUNTERS} == brute[5], (st, brute[5])
    assert np.array_equal(gpu_ctx.radius_count(pts, brute_force=True), np.diff(brute[0].astype(np.int64)).astype(np.uint32))
    if name in ("comb", "spoiled"):
        rc.assert_subset(want, brute)
    else:
        rc.assert_same_lists(want, brute, ordered=False)                 # completeness: nothing dropped, every triangle reachable


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batch_sizes_at_the_chunk_edges(rt, orc, gpu_ctx, n):
    tris, b4 = install(rt, orc, gpu_ctx, "soup1k")
    pts = rc.point_records(rt, tris, n=8400)[2100:2100 + n].copy()       # on the surface (the second quarter): every list has entries
    want = rt.radius_search_bvh4(tris, b4, pts)
    assert len(want[0]) == n + 1 and int(want[0][-1]) >= n
    for simple in (False, True):
        rc.assert_same_lists(gpu_ctx.radius_search(pts, simple=simple), want, ordered=True)
        assert np.array_equal(gpu_ctx.radius_count(pts, simple=simple), np.diff(want[0].astype(np.int64)))
    empty = gpu_ctx.radius_search(pts[:0])                               # n = 0: offsets = [0], no kernel
    assert empty[0].tolist() == [0] and len(empty[2]) == 0 and gpu_ctx.radius_count(pts[:0]).size == 0


def test_long_and_empty_lists_in_one_wavefront(rt, orc, gpu_ctx):
    tris, b4 = install(rt, orc, gpu_ctx, "dragon50k_l0")
    pts = rc.point_records(rt, tris, n=512)
    pts[0::4, 3] = 0.4 * rc.extent(tris)                                 # long lists
    pts[1::8, 3] = 0.0; pts[3::16, 3] = -1.0; pts[5::16, 3] = np.nan; pts[7::16, 0] = np.nan      # not walked
    want = rt.radius_search_bvh4(tris, b4, pts, stats=True)
    counts = np.diff(want[0].astype(np.int64))
    assert want[5]["stack_drops"] == 0
    assert (counts[0:512:4] > 1000).sum() >= 32 and not counts[1::8].any() and not counts[3::16].any() and not counts[5::16].any() and not counts[7::16].any()
    for kw in ({}, {"simple": True}, {"stats": True}):
        rc.assert_same_lists(gpu_ctx.radius_search(pts, **kw), want, ordered=True)
        assert np.array_equal(gpu_ctx.radius_count(pts, **kw), counts)
    assert gpu_ctx.stats()["rays_closest"] == len(pts)
    rc.assert_same_lists(gpu_ctx.radius_search(pts, brute_force=True), rt.radius_search_bvh4(tris, None, pts, brute_force=True), ordered=True)
    # the (points, r_max) form packs the same records
    rc.assert_same_lists(gpu_ctx.radius_search(pts[:, :3], pts[:, 3]), want, ordered=True)


@pytest.mark.parametrize("kernel", ["persistent", "simple", "brute"])
def test_truncation_at_a_capacity_on_the_host_route(rt, orc, gpu_ctx, kernel):
    """pt_radius_search_host: the staging and the copy back.  What the kernels themselves do with `capacity` is checked on the device route,
    with the guard in the memory they write: radius_torch_cases.py::truncation_on_the_device_route."""
    tris, b4 = install(rt, orc, gpu_ctx, "soup1k")
    pts = rc.point_records(rt, tris, n=1000)
    flags = {"persistent": 0, "simple": rt.PT_RADIUS_SIMPLE_KERNEL, "brute": rt.PT_RADIUS_BRUTE_FORCE}[kernel]
    want = rt.radius_search_bvh4(tris, b4 if kernel != "brute" else None, pts, brute_force=kernel == "brute")
    total = rc.assert_truncation(lambda cap, null: rc.raw_search(rt, rt.lib.pt_radius_search_host, (gpu_ctx.h,), pts, flags, cap, null), int(want[0][-1]))
    rc_, off, ent = rc.raw_search(rt, rt.lib.pt_radius_search_host, (gpu_ctx.h,), pts, flags, total)
    assert rc_ == 0 and np.array_equal(off, want[0]) and np.array_equal(ent[:total], rc.words(want)[1])
    part = gpu_ctx.radius_search(pts, capacity=total - 5, simple=kernel == "simple", brute_force=kernel == "brute")
    assert np.array_equal(part[0], want[0]) and len(part[2]) == total - 5 and np.array_equal(part[2], want[2][:total - 5])


def test_nearest_entry_is_the_closest_point(rt, orc, gpu_ctx):
    tris, b4 = install(rt, orc, gpu_ctx, "torus")
    pts = rc.point_records(rt, tris, n=N_POINTS)
    off, ent = rc.words(gpu_ctx.radius_search(pts))
    dist, prim, _, _ = gpu_ctx.closest_points(pts)
    counts = np.diff(off)
    assert np.array_equal(counts == 0, prim == clc.MISS)
    found = np.flatnonzero(counts > 0)
    assert 0 < len(found) < len(pts)
    assert clc.same_bits(np.minimum.reduceat(ent[:, 0].view(np.float32), off[found]), dist[found])
    assert np.all(np.isin((found.astype(np.int64) << 32) | prim[found], (rc.owner(off).astype(np.int64) << 32) | ent[:, 1]))


@pytest.mark.parametrize("case", ["torch_route_equals_the_host_route", "truncation_on_the_device_route", "no_host_synchronisation_with_a_capacity",
                                  "ordering_with_batched_frames_and_scene_changes", "errors"])
def test_torch_route(case):
    """The device route: tests/radius_torch_cases.py in a child process (torch is imported before the package there)."""
    run_case("radius_torch_cases", case)


NODE = "/usr/bin/node" if os.path.exists("/usr/bin/node") else "node"
JS = os.path.join(os.path.dirname(HERE), "raytracer-public_amd", "js")


def test_node_radius_queries(tmp_path, rt, gpu_ctx):
    """PathTracer.radiusSearch, radiusCount and within give the Python results bit for bit, in the same order."""
    tris = rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 20000, 7)
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh()
    pts = rc.point_records(rt, tris, n=N_POINTS)
    pts.tofile(str(tmp_path / "points.f32"))
    script = tmp_path / "radius.js"
    script.write_text("""
const fs = require("fs");
const PT = require(%r);
const f32 = (p) => { const raw = fs.readFileSync(p); return new Float32Array(raw.buffer, raw.byteOffset, raw.byteLength / 4); };
(async () => {
  const pt = new PT.PathTracer({ width: 64, height: 48 });
  await pt.initialize();
  await pt.buildBVH(PT.native().proceduralScene(0, 20000, 7));
  const points = f32(%r);
  const s = await pt.radiusSearch(points);
  const fixed = await pt.radiusSearch(points, 0.05, { simple: true });
  const counts = await pt.radiusCount(points);
  const brute = await pt.radiusCount(points, undefined, { bruteForce: true });
  const one = await pt.within(points[4 * 600], points[4 * 600 + 1], points[4 * 600 + 2], 0.1);
  const out = { offsets: s.offsets, dist: s.dist, prim: s.prim, u: s.u, v: s.v, fixed_offsets: fixed.offsets, fixed_prim: fixed.prim,
                counts: counts, brute: brute, one_prim: one.prim, one_dist: one.dist, one_count: Uint32Array.of(one.count) };
  for (const [k, v] of Object.entries(out)) fs.writeFileSync(%r + k, Buffer.from(v.buffer, v.byteOffset, v.byteLength));
  pt.destroy();
})().catch((e) => { console.error(e); process.exit(1); });
""" % (os.path.join(JS, "PathTracer.js"), str(tmp_path / "points.f32"), str(tmp_path / "out_")))
    r = subprocess.run([NODE, str(script)], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr

    def out(k, dt=np.uint32):
        return np.fromfile(str(tmp_path / ("out_" + k)), dt)
    want = gpu_ctx.radius_search(pts)
    got = (out("offsets", np.float64).astype(np.uint64), out("dist", np.float32), out("prim"), out("u", np.float32), out("v", np.float32))
    rc.assert_same_lists(got, want, ordered=True)
    assert int(want[0][-1]) > len(pts)
    fixed = gpu_ctx.radius_search(pts, 0.05)
    assert np.array_equal(out("fixed_offsets", np.float64).astype(np.uint64), fixed[0]) and np.array_equal(out("fixed_prim"), fixed[2])
    assert np.array_equal(out("counts"), gpu_ctx.radius_count(pts)) and np.array_equal(out("brute"), gpu_ctx.radius_count(pts, brute_force=True))
    one = gpu_ctx.radius_search(pts[600:601, :3], 0.1)
    assert out("one_count")[0] == len(one[2]) > 0 and np.array_equal(out("one_prim"), one[2]) and clc.same_bits(out("one_dist", np.float32), one[1])
