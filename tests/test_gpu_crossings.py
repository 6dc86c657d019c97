"""Crossing counts, containment and signed distance on the GPU (pt_count_hits / pt_contains / pt_signed_distance).
Every result is an integer or a bit pattern, so every check is an equality: of the three count kernels and their counters with the host
twin (tests/test_crossings_host.py pins that to a float32 restatement and to brute force), of count >= 1 with the any-hit ray query, of
both containment kernels with the composition occlusion_rays -> count_hits -> parity -> majority, of the signed distance with
closest_points and contains; and containment against the float64 winding number on a closed mesh."""
import os
import subprocess

import numpy as np
import pytest

import closestref
import crossing_cases as cc
import crossref
from refit_cases import wave
from routecheck import code, run_case
from scenes import random_soup

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MISS = 0xFFFFFFFF
N_RAYS, N_POINTS = 4096, 2048
KERNELS = [False, True]       # simple=False: the persistent kernel; True: the one-ray-per-thread kernel
SCENES = ["tetra", "torus", "soup1k", "dragon50k_l0", "dragon50k_l2", "refit", "bvh2", "comb", "spoiled"]
COUNTERS = ("rays_closest", "rays_shadow", "nodes_examined", "tris_tested", "stack_drops", "max_stack", "samples")


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def install(rt, orc, ctx, name):
    """Sets the scene `name` on the context; returns (triangles, the BVH4 the context holds: what the host twin walks)."""
    if name == "comb":
        tris = cc.geometry(rt, "comb")
        ctx.set_triangles(tris); ctx.set_bvh4(cc.comb_tree())
    elif name == "spoiled":
        tris = cc.geometry(rt, "spoiled")
        ctx.set_triangles(tris); ctx.set_bvh4(cc.spoiled_tree(rt, orc, tris))
    elif name == "bvh2":
        tris = random_soup(2000, 31)
        ctx.set_triangles(tris); ctx.set_bvh2(orc.build_bvh4(tris)[0])
    elif name == "refit":
        base = cc.geometry(rt, "soup1k")
        ctx.set_triangles(base); ctx.build_bvh(1)
        tris = wave(base, 0.02, 3)
        ctx.update_triangles(tris)
    else:
        tris = cc.geometry(rt, name.split("_")[0])
        ctx.set_triangles(tris); ctx.build_bvh(2 if name.endswith("_l2") else 0)
    return tris, ctx.read_bvh4()


def rays_for(rt, name, tris, n=N_RAYS):
    if name != "comb":
        return cc.ray_set(rt, tris, n, 11)
    rays = cc.comb_rays(rt, n, 3)
    rays[-(n // 4):, 6] = 1.0                                               # a quarter points away from the comb: misses
    return rays


@pytest.mark.parametrize("name", SCENES)
def test_count_hits_equals_the_host_twin(rt, orc, gpu_ctx, name):
    tris, b4 = install(rt, orc, gpu_ctx, name)
    rays = rays_for(rt, name, tris)
    want, want_st = rt.count_hits_bvh4(tris, b4, rays, stats=True)
    assert want.max() >= 1 and (want == 0).any()
    for simple in KERNELS:
        got = gpu_ctx.count_hits(rays, simple=simple)
        assert got.dtype == np.uint32 and np.array_equal(got, want), (simple, np.flatnonzero(got != want)[:8])
    got = gpu_ctx.count_hits(rays, stats=True)
    st = gpu_ctx.stats()
    assert np.array_equal(got, want)
    assert {k: st[k] for k in COUNTERS} == want_st, (st, want_st)
    assert (st["stack_drops"] > 0) == (name == "comb")
    if name in ("comb", "spoiled"):
        return
    brute, brute_st = rt.count_hits_bvh4(tris, None, rays, brute_force=True, stats=True)
    assert np.array_equal(gpu_ctx.count_hits(rays, brute_force=True), brute)
    assert np.array_equal(gpu_ctx.count_hits(rays, brute_force=True, stats=True), brute)
    st = gpu_ctx.stats()
    assert {k: st[k] for k in COUNTERS} == brute_st, (st, brute_st)
    assert np.array_equal(want, brute)                                      # fact 3: nothing dropped, nothing lost to a box


@pytest.mark.parametrize("name", SCENES)
def test_count_is_positive_exactly_where_any_hit_hits(rt, orc, gpu_ctx, name):
    tris, _ = install(rt, orc, gpu_ctx, name)
    rays = rays_for(rt, name, tris)
    for simple in KERNELS:
        counts = gpu_ctx.count_hits(rays, simple=simple)
        _, prim, _, _ = gpu_ctx.trace_rays(rays, any_hit=True, simple=simple)
        assert np.array_equal(counts >= 1, prim != MISS), (simple, np.flatnonzero((counts >= 1) != (prim != MISS))[:8])
    assert 0 < (counts >= 1).sum() < len(rays)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batch_sizes_at_the_chunk_edges(rt, orc, gpu_ctx, n):
    tris, b4 = install(rt, orc, gpu_ctx, "soup1k")
    rays = cc.ray_set(rt, tris, 8400, 17)[100:100 + n]                      # aimed rays (the first half): most of them cross something
    want = rt.count_hits_bvh4(tris, b4, rays)
    assert len(want) == n
    for simple in KERNELS:
        assert np.array_equal(gpu_ctx.count_hits(rays, simple=simple), want)
    assert gpu_ctx.count_hits(rays[:0]).size == 0                           # n = 0: nothing is launched


def test_rays_that_are_not_walked_among_others(rt, orc, gpu_ctx):
    tris, b4 = install(rt, orc, gpu_ctx, "soup1k")
    rays = cc.ray_set(rt, tris, N_RAYS, 19).copy()
    rays[3::13, 3] = np.resize(np.float32([0.5, 2.0, 0.05, 1.0]), len(rays[3::13]))    # finite t_max
    rays[5::17, 3] = 0.0; rays[6::17, 3] = -1.0; rays[7::17, 3] = np.nan; rays[8::17, 3] = -np.inf
    rays[9::17, 0] = np.nan; rays[10::17, 5] = np.nan; rays[11::17, 6] = np.nan
    walked = crossref.ray_walked(rays)
    want = rt.count_hits_bvh4(tris, b4, rays)
    assert not want[~walked].any() and 0 < (~walked).sum() < len(rays) and want[walked].any()
    for kw in ({}, {"simple": True}, {"brute_force": True}, {"stats": True}):
        assert np.array_equal(gpu_ctx.count_hits(rays, **kw), want), kw
    assert gpu_ctx.stats()["rays_closest"] == len(rays)
    # the (origins, directions, t_max) form packs the same records
    assert np.array_equal(gpu_ctx.count_hits(rays[:, 0:3], rays[:, 4:7], rays[:, 3]), want)


@pytest.mark.parametrize("samples", [1, 3, 7])
@pytest.mark.parametrize("name", ["torus", "soup1k", "comb"])
def test_contains_equals_the_composition_and_the_twin(rt, orc, gpu_ctx, name, samples):
    tris, b4 = install(rt, orc, gpu_ctx, name)
    lo, hi = cc.box_of(tris)
    pts = (lo + np.random.default_rng(5).random((N_POINTS, 3)) * (hi - lo)).astype(np.float32)
    if name == "comb":
        pts[:, 2] = -1.0                                                    # below the comb: the rays go up through every level
    pts[11, 0] = np.nan; pts[12, 2] = np.nan                                # not traced: {0, 0, 0, 0}
    kw = dict(seed=samples, index_base=0xFFFFFF00)
    rays = cc.containment_rays(rt, pts, samples, **kw)
    want = [a.copy() for a in cc.compose_contains(gpu_ctx.count_hits(rays), len(pts), samples)]
    for a in want:
        a[[11, 12]] = 0
    twin = rt.contains_bvh4(tris, b4, pts, samples=samples, stats=True, **kw)
    assert all(np.array_equal(t, w) for t, w in zip(twin[:3], want))
    for simple in KERNELS:
        got = gpu_ctx.contains(pts, samples=samples, simple=simple, **kw)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), (simple, [np.flatnonzero(g != w)[:8] for g, w in zip(got, want)])
    got = gpu_ctx.contains(pts, samples=samples, stats=True, **kw)
    st = gpu_ctx.stats()
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert {k: st[k] for k in COUNTERS} == twin[3], (st, twin[3])
    assert st["rays_closest"] == (len(pts) - 2) * samples
    assert 0 < want[1].sum()


@pytest.mark.parametrize("samples", [1, 3, 7])
def test_closed_box_inside_and_outside(rt, gpu_ctx, samples):
    gpu_ctx.set_triangles(cc.geometry(rt, "box")); gpu_ctx.build_bvh()
    rng = np.random.default_rng(samples)
    inner = rng.uniform(-0.95, 0.95, (N_POINTS // 2, 3)).astype(np.float32)
    outer = rng.uniform(-0.95, 0.95, (N_POINTS // 2, 3)).astype(np.float32)
    axis = rng.integers(0, 3, len(outer))
    outer[np.arange(len(outer)), axis] = (rng.choice([-1.0, 1.0], len(outer)) * rng.uniform(1.05, 3.0, len(outer))).astype(np.float32)
    for simple in KERNELS:
        inside, odd, smp = gpu_ctx.contains(inner, samples=samples, seed=3, simple=simple)
        assert np.all(inside == 1) and np.all(odd == samples) and np.all(smp == samples)
        inside, odd, smp = gpu_ctx.contains(outer, samples=samples, seed=3, simple=simple)
        assert np.all(inside == 0) and np.all(odd == 0) and np.all(smp == samples)


def test_torus_against_the_float64_winding_number(rt, gpu_ctx):
    tris = cc.geometry(rt, "torus")
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh()
    pts = cc.cube_points(N_POINTS, 33)
    inside_ref = np.abs(crossref.winding_number(pts, tris)) > 0.5
    keep = closestref.nearest(pts, tris)[0] >= 1e-4
    assert (~keep).sum() * 100 <= len(pts) and 20 < inside_ref[keep].sum() < keep.sum()
    for simple in KERNELS:
        inside, odd, smp = gpu_ctx.contains(pts, samples=3, seed=1, simple=simple)
        assert np.array_equal(inside[keep].astype(bool), inside_ref[keep]), np.flatnonzero(keep & (inside.astype(bool) != inside_ref))[:8]
        wrong = int(np.where(inside_ref[keep], 3 - odd[keep], odd[keep]).sum())      # single rays that disagree
        print("torus: %d of %d single rays disagree with the winding number (simple=%s)" % (wrong, 3 * keep.sum(), simple))
        assert wrong * 1000 <= 3 * keep.sum()


@pytest.mark.parametrize("name", ["tetra", "torus"])
def test_signed_distance(rt, gpu_ctx, name):
    tris = cc.geometry(rt, name)
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh()
    pts = cc.cube_points(N_POINTS, 41, half=1.0)
    if name == "torus":
        pts[: N_POINTS // 2] = tris.reshape(-1, 3)[::6][: N_POINTS // 2] * np.float32(0.97) + np.float32([0.0, 0.003, 0.0])    # near the surface, either side
    for r_max in (None, 0.05):
        dist, prim, u, v = gpu_ctx.closest_points(pts, r_max)
        inside, _, _ = gpu_ctx.contains(pts, samples=3, seed=2)
        for simple in KERNELS:
            sd, sprim, su, sv = gpu_ctx.signed_distance(pts, r_max, samples=3, seed=2, simple=simple)
            assert same_bits(np.abs(sd), dist) and np.array_equal(sprim, prim) and same_bits(su, u) and same_bits(sv, v)
            assert np.array_equal(np.signbit(sd), inside.astype(bool))
        assert 0 < inside.sum() < len(pts)
        if r_max is not None:       # inside, and nothing within r_max: -inf; outside and nothing: +inf
            assert np.any(np.isneginf(sd)) and np.any(np.isposinf(sd)) and np.any(np.isfinite(sd) & (sd < 0)) and np.any(np.isfinite(sd) & (sd > 0))
            assert np.all(prim[np.isinf(sd)] == MISS)


def test_argument_errors(rt, gpu_ctx):
    pts = np.zeros((3, 3), np.float32); rays = rt.pack_rays(pts, pts + 1)
    assert code(rt, lambda: gpu_ctx.count_hits(rays)) == 4 and code(rt, lambda: gpu_ctx.contains(pts)) == 4 and code(rt, lambda: gpu_ctx.signed_distance(pts)) == 4
    gpu_ctx.set_triangles(cc.geometry(rt, "tetra")); gpu_ctx.build_bvh()
    for bad in (0, 2, 256):
        assert code(rt, lambda: gpu_ctx.contains(pts, samples=bad)) == 1 and code(rt, lambda: gpu_ctx.signed_distance(pts, samples=bad)) == 1
    import ctypes as C
    p = rt.PtContainParams(3, 0, 0, 0); out = rt._aligned_zeros((4, 4), np.uint32); rec = rt.pack_points(pts)
    assert rt.lib.pt_contains_host(gpu_ctx.h, rec.ctypes.data_as(C.POINTER(rt.PtPoint)), C.c_uint64((1 << 32) // 3 + 1), C.byref(p),
                                   out.ctypes.data_as(C.POINTER(rt.PtContainment))) == 1
    assert b"n * samples" in rt.lib.pt_last_error(gpu_ctx.h)
    p.flags = 4
    assert rt.lib.pt_contains_host(gpu_ctx.h, rec.ctypes.data_as(C.POINTER(rt.PtPoint)), C.c_uint64(3), C.byref(p),
                                   out.ctypes.data_as(C.POINTER(rt.PtContainment))) == 1
    assert rt.lib.pt_count_hits_host(gpu_ctx.h, rays.ctypes.data_as(C.POINTER(rt.PtRay)), C.c_uint64(3), C.c_uint32(8), out.ctypes.data_as(C.POINTER(C.c_uint32))) == 1
    assert gpu_ctx.contains(pts)[0].tolist() == [1, 1, 1] and gpu_ctx.contains(pts, samples=255)[1].tolist() == [255] * 3      # still usable


@pytest.mark.parametrize("case", ["torch_route_equals_the_host_route", "device_composition", "no_host_synchronisation",
                                  "ordering_with_batched_frames_and_scene_changes", "errors"])
def test_torch_route(case):
    """The device route: tests/crossings_torch_cases.py in a child process (torch is imported before the package there)."""
    run_case("crossings_torch_cases", case)


NODE = "/usr/bin/node" if os.path.exists("/usr/bin/node") else "node"
JS = os.path.join(os.path.dirname(HERE), "raytracer-public_amd", "js")


def test_node_crossings(tmp_path, rt, gpu_ctx):
    """PathTracer.countHits, contains, signedDistance and inside give the Python results bit for bit; a scene change after a call does not
    reach its result (the promise was resolved from the first scene)."""
    tris = rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 20000, 7)
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh()
    rays = cc.ray_set(rt, tris, N_RAYS, 23)
    pts = rt.pack_points(cc.cube_points(N_POINTS, 29, half=1.0), 0.25)
    rays.tofile(str(tmp_path / "rays.f32")); pts.tofile(str(tmp_path / "points.f32"))
    script = tmp_path / "crossings.js"
    script.write_text("""
const fs = require("fs");
const PT = require(%r);
const f32 = (p) => { const raw = fs.readFileSync(p); return new Float32Array(raw.buffer, raw.byteOffset, raw.byteLength / 4); };
(async () => {
  const pt = new PT.PathTracer({ width: 64, height: 48 });
  await pt.initialize();
  await pt.buildBVH(PT.native().proceduralScene(0, 20000, 7));
  const rays = f32(%r), points = f32(%r);
  const counts = await pt.countHits(rays);
  const brute = await pt.countHits(rays, { bruteForce: true });
  const c = await pt.contains(points, { samples: 3, seed: 5 });
  const s = await pt.signedDistance(points, { samples: 3, seed: 5 });
  const one = await pt.inside(points[0], points[1], points[2], { seed: 5, indexBase: 0 });
  await pt.buildBVH(PT.native().proceduralScene(0, 5000, 9));      // after the calls: their results stay those of the first scene
  const later = await pt.countHits(rays);
  const out = { counts: counts, brute: brute, inside: c.inside, odd: c.odd, samples: c.samples, dist: s.dist, prim: s.prim, u: s.u, v: s.v, later: later,
                one: Uint32Array.of(one.inside ? 1 : 0, one.odd, one.samples) };
  for (const [k, v] of Object.entries(out)) fs.writeFileSync(%r + k, Buffer.from(v.buffer, v.byteOffset, v.byteLength));
  pt.destroy();
})().catch((e) => { console.error(e); process.exit(1); });
""" % (os.path.join(JS, "PathTracer.js"), str(tmp_path / "rays.f32"), str(tmp_path / "points.f32"), str(tmp_path / "out_")))
    r = subprocess.run([NODE, str(script)], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr

    def out(k, dt=np.uint32):
        return np.fromfile(str(tmp_path / ("out_" + k)), dt)
    want = gpu_ctx.count_hits(rays)
    assert np.array_equal(out("counts"), want) and np.array_equal(out("brute"), gpu_ctx.count_hits(rays, brute_force=True))
    inside, odd, smp = gpu_ctx.contains(pts, samples=3, seed=5)
    assert np.array_equal(out("inside"), inside) and np.array_equal(out("odd"), odd) and np.array_equal(out("samples"), smp)
    assert 0 < inside.sum() < len(pts)
    sd = gpu_ctx.signed_distance(pts, samples=3, seed=5)
    assert same_bits(out("dist"), sd[0]) and np.array_equal(out("prim"), sd[1]) and same_bits(out("u"), sd[2]) and same_bits(out("v"), sd[3])
    assert out("one").tolist() == [int(inside[0]), int(odd[0]), 3]
    other = rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 5000, 9)
    gpu_ctx.set_triangles(other); gpu_ctx.build_bvh()
    later = gpu_ctx.count_hits(rays)
    assert np.array_equal(out("later"), later) and not np.array_equal(later, want)
