"""k-nearest queries on the GPU (pt_nearest_k).  Every result is an integer or a bit pattern, so every check is an
equality: of the persistent kernel (each capacity tier, both sides of each tier boundary), the one-point-per-thread kernel and the
brute-force kernel with the host twin (tests/test_knn_host.py pins that to a float32 restatement, to brute force and to float64) -- every
bit of every record, the order of the prims included, and the counters of PT_NEAREST_STATS; of the guard behind the n * k records; of
k = 1 with the closest-point query."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import closest_cases as clc
import knn_cases as kc
import radius_cases as rc
from routecheck import run_case

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N_POINTS = 1024
N_BRUTE = 256
KS = (1, 4, 5, 16, 17, 64)           # both sides of the tier boundaries 4 | 16 | 64 of nearest_k_kernel<KCAP>
SCENES = ["tetra", "doubled", "torus", "soup1k", "dragon50k_l0", "dragon50k_l2", "refit", "bvh2", "comb", "spoiled"]
COUNTERS = ("rays_closest", "rays_shadow", "nodes_examined", "tris_tested", "stack_drops", "max_stack", "samples")


def install(rt, orc, ctx, name):
    if name == "doubled":
        ctx.set_triangles(kc.DOUBLED_TETRA); ctx.build_bvh(0)
        return kc.DOUBLED_TETRA, ctx.read_bvh4()
    return rc.install(rt, orc, ctx, name)


def points_for(rt, name, tris, n=N_POINTS):
    """every other point without a radius (full rows), the others with a radius of 1-10 % of the extent (short and empty rows)"""
    if name == "comb":
        return kc.comb_points(rt, n)
    pts = rc.point_records(rt, tris, n=n)
    pts[0::2, 3] = np.inf
    return pts


@pytest.mark.parametrize("name", SCENES)
def test_kernels_equal_the_host_twin(rt, orc, gpu_ctx, name):
    tris, b4 = install(rt, orc, gpu_ctx, name)
    pts = points_for(rt, name, tris)
    for k in KS:
        want = rt.nearest_k_bvh4(tris, b4, pts, k, stats=True)
        for kw in ({}, {"simple": True}):
            got = gpu_ctx.nearest_k(pts, k, **kw)
            assert got[0].shape == (len(pts), k) and got[1].dtype == np.uint32
            kc.assert_same_rows(got, want)
        kc.assert_same_rows(gpu_ctx.nearest_k(pts, k, stats=True), want)
        st = gpu_ctx.stats()
        assert {c: st[c] for c in COUNTERS} == want[4], (k, st, want[4])
        assert (st["stack_drops"] > 0) == (name == "comb")
    few = np.ascontiguousarray(pts[:N_BRUTE])
    for k in (5, 64):
        brute = rt.nearest_k_bvh4(tris, None, few, k, brute_force=True, stats=True)
        kc.assert_same_rows(gpu_ctx.nearest_k(few, k, brute_force=True), brute)
        kc.assert_same_rows(gpu_ctx.nearest_k(few, k, brute_force=True, stats=True), brute)
        st = gpu_ctx.stats()
        assert {c: st[c] for c in COUNTERS} == brute[4], (k, st, brute[4])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batch_sizes_at_the_chunk_edges(rt, orc, gpu_ctx, n):
    tris, b4 = install(rt, orc, gpu_ctx, "soup1k")
    pts = rc.point_records(rt, tris, n=8400)[2100:2100 + n].copy()       # on the surface (the second quarter): every row has entries
    pts[0::3, 3] = np.inf
    for k in (4, 17, 64):
        want = rt.nearest_k_bvh4(tris, b4, pts, k)
        assert kc.listed(kc.words(want))[:, 0].all()
        for simple in (False, True):
            kc.assert_same_rows(gpu_ctx.nearest_k(pts, k, simple=simple), want)
    assert gpu_ctx.nearest_k(pts[:0], 5)[0].shape == (0, 5)              # n = 0: no kernel


def test_empty_short_and_full_rows_in_one_wavefront(rt, orc, gpu_ctx):
    tris, b4 = install(rt, orc, gpu_ctx, "dragon50k_l0")
    pts = rc.point_records(rt, tris, n=512)
    pts[0::4, 3] = np.inf                                                # full rows
    pts[1::8, 3] = 0.0; pts[3::16, 3] = -1.0; pts[5::16, 3] = np.nan; pts[7::16, 0] = np.nan      # not walked
    pts[2::8, 3] *= 0.1                                                  # a few triangles only: short rows also for k = 4
    for k in (4, 16, 64):
        want = rt.nearest_k_bvh4(tris, b4, pts, k, stats=True)
        held = kc.listed(kc.words(want)).sum(1)
        assert want[4]["stack_drops"] == 0
        assert np.all(held[0::4] == k) and not held[1::8].any() and not held[3::16].any() and not held[5::16].any() and not held[7::16].any()
        assert ((held > 0) & (held < k)).sum() >= 8                      # short rows in the same wavefronts
        for kw in ({}, {"simple": True}, {"stats": True}):
            kc.assert_same_rows(gpu_ctx.nearest_k(pts, k, **kw), want)
        assert gpu_ctx.stats()["rays_closest"] == len(pts)
        kc.assert_same_rows(gpu_ctx.nearest_k(pts, k, brute_force=True), rt.nearest_k_bvh4(tris, None, pts, k, brute_force=True))
    # the (points, r_max) form packs the same records
    kc.assert_same_rows(gpu_ctx.nearest_k(pts[:, :3], 16, pts[:, 3]), rt.nearest_k_bvh4(tris, b4, pts, 16))


@pytest.mark.parametrize("kernel", ["persistent", "simple", "brute"])
def test_host_route_writes_n_times_k_records_and_nothing_behind_them(rt, orc, gpu_ctx, kernel):
    """pt_nearest_k_host: the staging and the copy back.  The same on the memory the kernels write: knn_torch_cases.py::guard_on_the_device_route."""
    tris, b4 = install(rt, orc, gpu_ctx, "soup1k")
    pts = points_for(rt, "soup1k", tris, n=1000)
    flags = {"persistent": 0, "simple": rt.PT_NEAREST_SIMPLE_KERNEL, "brute": rt.PT_NEAREST_BRUTE_FORCE}[kernel]
    for k in KS:
        want = kc.words(rt.nearest_k_bvh4(tris, b4 if kernel != "brute" else None, pts, k, brute_force=kernel == "brute"))
        buf = kc.guarded(rt, len(pts), k)
        assert rt.lib.pt_nearest_k_host(gpu_ctx.h, pts.ctypes.data_as(C.POINTER(rt.PtPoint)), C.c_uint64(len(pts)), C.c_uint32(k), C.c_uint32(flags),
                                        buf.ctypes.data_as(C.POINTER(rt.PtClosest))) == 0
        kc.assert_guard(buf, len(pts), k)
        assert np.array_equal(buf[:len(pts) * k].reshape(len(pts), k, 4), want), k


def test_k_1_is_the_closest_point_query(rt, orc, gpu_ctx):
    tris, b4 = install(rt, orc, gpu_ctx, "torus")
    pts = points_for(rt, "torus", tris, n=2048)
    one = gpu_ctx.nearest_k(pts, 1)
    dist, prim, u, v = gpu_ctx.closest_points(pts)
    assert (prim == clc.MISS).any() and (prim != clc.MISS).any()
    assert clc.same_bits(one[0][:, 0], dist) and np.array_equal(one[1][:, 0], prim) and clc.same_bits(one[2][:, 0], u) and clc.same_bits(one[3][:, 0], v)


def test_arguments(rt, orc, gpu_ctx):
    pts = rt.pack_points(np.zeros((4, 3), np.float32), 10.0)
    with pytest.raises(rt.PtError) as e:
        gpu_ctx.nearest_k(pts, 3)
    assert e.value.code == 4                                             # no scene
    install(rt, orc, gpu_ctx, "tetra")
    for k in (0, 65):
        with pytest.raises(rt.PtError) as e:
            gpu_ctx.nearest_k(pts, k)
        assert e.value.code == 1
    buf = kc.guarded(rt, 4, 3)
    pp, op = pts.ctypes.data_as(C.POINTER(rt.PtPoint)), buf.ctypes.data_as(C.POINTER(rt.PtClosest))
    odd = C.cast(C.c_void_p(buf.ctypes.data + 8), C.POINTER(rt.PtClosest))
    host = rt.lib.pt_nearest_k_host
    assert host(gpu_ctx.h, pp, C.c_uint64(4), C.c_uint32(3), C.c_uint32(8), op) == 1       # unknown flag
    assert host(gpu_ctx.h, None, C.c_uint64(4), C.c_uint32(3), C.c_uint32(0), op) == 1
    assert host(gpu_ctx.h, pp, C.c_uint64(4), C.c_uint32(3), C.c_uint32(0), None) == 1
    assert host(gpu_ctx.h, pp, C.c_uint64(4), C.c_uint32(3), C.c_uint32(0), odd) == 1      # 16-byte alignment
    assert host(gpu_ctx.h, pp, C.c_uint64(1 << 32), C.c_uint32(3), C.c_uint32(0), op) == 1
    assert host(gpu_ctx.h, pp, C.c_uint64(0), C.c_uint32(3), C.c_uint32(0), op) == 0 and np.all(buf == rc.GUARD)
    assert np.all(gpu_ctx.nearest_k(pts, 4)[1] < 4)                     # the context is still usable


@pytest.mark.parametrize("case", ["torch_route_equals_the_host_route", "guard_on_the_device_route", "no_host_synchronisation",
                                  "ordering_with_batched_frames_and_scene_changes", "errors"])
def test_torch_route(case):
    """The device route: tests/knn_torch_cases.py in a child process (torch is imported before the package there)."""
    run_case("knn_torch_cases", case)


NODE = "/usr/bin/node" if os.path.exists("/usr/bin/node") else "node"
JS = os.path.join(os.path.dirname(HERE), "raytracer-public_amd", "js")


def test_node_nearest_k(tmp_path, rt, gpu_ctx):
    """PathTracer.nearestK and kNearest give the Python results bit for bit, in the same order."""
    tris = rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 20000, 7)
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh()
    pts = points_for(rt, "dragon", tris, n=N_POINTS)
    pts.tofile(str(tmp_path / "points.f32"))
    script = tmp_path / "knn.js"
    script.write_text("""
const fs = require("fs");
const PT = require(%r);
const f32 = (p) => { const raw = fs.readFileSync(p); return new Float32Array(raw.buffer, raw.byteOffset, raw.byteLength / 4); };
(async () => {
  const pt = new PT.PathTracer({ width: 64, height: 48 });
  await pt.initialize();
  await pt.buildBVH(PT.native().proceduralScene(0, 20000, 7));
  const points = f32(%r);
  const a = await pt.nearestK(points, 5);
  const b = await pt.nearestK(points, 17, { rMax: 0.05, simple: true });
  const c = await pt.nearestK(points.subarray(0, 4 * 64), 3, { bruteForce: true });
  const one = await pt.kNearest(points[4 * 300], points[4 * 300 + 1], points[4 * 300 + 2], 8);
  let threw = 0;
  try { await pt.nearestK(points, 65); } catch (e) { threw = 1; }
  const out = { a_dist: a.dist, a_prim: a.prim, a_u: a.u, a_v: a.v, b_dist: b.dist, b_prim: b.prim, c_prim: c.prim, c_dist: c.dist,
                one_prim: one.prim, one_dist: one.dist, misc: Uint32Array.of(one.count, a.k, threw) };
  for (const [k, v] of Object.entries(out)) fs.writeFileSync(%r + k, Buffer.from(v.buffer, v.byteOffset, v.byteLength));
  pt.destroy();
})().catch((e) => { console.error(e); process.exit(1); });
""" % (os.path.join(JS, "PathTracer.js"), str(tmp_path / "points.f32"), str(tmp_path / "out_")))
    r = subprocess.run([NODE, str(script)], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr

    def out(k, dt=np.uint32):
        return np.fromfile(str(tmp_path / ("out_" + k)), dt)
    n = len(pts)
    a = gpu_ctx.nearest_k(pts, 5)
    kc.assert_same_rows(tuple(out("a_" + c, t).reshape(n, 5) for c, t in (("dist", np.float32), ("prim", np.uint32), ("u", np.float32), ("v", np.float32))), a)
    b = gpu_ctx.nearest_k(pts, 17, 0.05)
    assert np.array_equal(out("b_prim").reshape(n, 17), b[1]) and clc.same_bits(out("b_dist", np.float32), b[0].reshape(-1))
    assert (b[1] == clc.MISS).any() and (b[1] != clc.MISS).any()
    c = gpu_ctx.nearest_k(pts[:64], 3, brute_force=True)
    assert np.array_equal(out("c_prim").reshape(64, 3), c[1]) and clc.same_bits(out("c_dist", np.float32), c[0].reshape(-1))
    one = gpu_ctx.nearest_k(pts[300:301, :3], 8)
    assert out("misc").tolist() == [8, 5, 1]
    assert np.array_equal(out("one_prim"), one[1][0]) and clc.same_bits(out("one_dist", np.float32), one[0][0])
