"""Animated geometry on the device (pt_update_triangles, pt_bvh_cost; include/mi355pt.h): the refit in place
equals its host twins word for word whatever installed the tree; every renderer and the ray queries traverse the refitted tree exactly
as the oracle does (the read-back BVH4 is a BVH4 in the reference's layout); updates are ordered with queued frames, restart an
accumulation, leave the context untouched when refused; groups, the torch route, the Node host and the driver pass them on."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import orc as orc_mod
from refit_cases import host_trees, wave
from routecheck import code, run_case
from scenes import TETRA, random_soup, quat_yaw_pitch, spoil_bvh4
from test_accel_host import DEGENERATE, degenerate
from test_gpu_rayquery import MISS, oracle_batch, random_rays

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NODE = shutil.which("node")
JS = os.path.join(ROOT, "raytracer-public_amd", "js")
ADDON = os.path.join(ROOT, "raytracer-public_amd", "napi", "mi355pt.node")
SCENE_SEED = 20260109
KEYS_REF = ("rays_closest", "nodes_examined", "tris_tested", "stack_drops", "max_stack", "samples")
KEYS_PATH = ("rays_closest", "rays_shadow", "nodes_examined", "tris_tested", "stack_drops", "max_stack", "samples")
CAMS = [((0, 0, 2.5), (0, 0, 0, 1)), ((0.4, 0.3, 1.7), quat_yaw_pitch(0.2, -0.15))]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def small_scene(rt, name):
    if name == "soup":
        return random_soup(3000, 11)
    if name == "dragon":
        return rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 20000)
    if name == "tetra":
        return TETRA
    return degenerate(name)


def update_and_compare(rt, ctx, moved, b4, b2=None):
    """update_triangles(moved) on a context whose tree had the words b4 (and BVH2 b2): the device's words are the host twins'."""
    ctx.update_triangles(moved)
    got4 = ctx.read_bvh4()
    assert np.array_equal(got4, rt.refit_bvh4(moved, b4))
    if b2 is not None:
        assert np.array_equal(ctx.read_bvh2(), rt.refit_bvh2(moved, b2))
    return got4


def check_render(rt, orc, ctx, tris, bvh4, mode, simple, w=160, h=96, cam=CAMS[1]):
    """One frame with counters against the oracle on the read-back tree: image and all seven counters."""
    n = tris.size // 9
    kw = dict(spp=3, max_bounces=6, seed=7, frame=3) if mode == rt.PT_MODE_PATH else {}
    ctx.render(ctx.make_params(w, h, cam[0], cam[1], mode=mode, stats=True, simple_kernel=simple, **kw))
    omode = {rt.PT_MODE_REFERENCE_PACKET: orc_mod.MODE_PACKET, rt.PT_MODE_REFERENCE: orc_mod.MODE_SINGLE, rt.PT_MODE_PATH: orc_mod.MODE_PATH}[mode]
    ref, _, ost = orc.render(orc.make_params(w, h, n, cam[0], cam[1], mode=omode, **kw), tris, bvh4)
    assert same_bits(ctx.read_radiance(), ref), (mode, simple)
    st = ctx.stats()
    for k in KEYS_PATH:
        assert st[k] == ost[k], (k, mode, simple, st[k], ost[k])


@pytest.mark.parametrize("accel", [0, 1, 2])
@pytest.mark.parametrize("name", ["soup", "dragon", "tetra"] + DEGENERATE)
def test_device_refit_equals_the_host_twins(rt, orc, gpu_ctx, name, accel):
    tris = small_scene(rt, name)
    gpu_ctx.set_triangles(tris)
    gpu_ctx.build_bvh(accel)
    b4, b2 = gpu_ctx.read_bvh4(), gpu_ctx.read_bvh2()
    update_and_compare(rt, gpu_ctx, tris, b4, b2)                          # unchanged triangles: the built tree, word for word
    assert np.array_equal(gpu_ctx.read_bvh4(), b4) and np.array_equal(gpu_ctx.read_bvh2(), b2)
    for amp, frame in ((0.1, 3), (0.3, 7)):
        update_and_compare(rt, gpu_ctx, wave(tris, amp, frame), b4, b2)
    if name == "soup":                                                     # infinite and NaN vertices: word equality only, nothing is traced
        odd = wave(tris, 0.1, 1).reshape(-1, 3, 3)
        odd[5, 0, 1] = np.inf; odd[17, 1, 0] = np.nan; odd[40, :, 2] = -np.inf
        update_and_compare(rt, gpu_ctx, odd.reshape(-1), b4, b2)
        update_and_compare(rt, gpu_ctx, tris, b4, b2)
        assert np.array_equal(gpu_ctx.read_bvh4(), b4)


@pytest.mark.parametrize("how", ["set_bvh4", "set_bvh4_wide", "set_bvh4_spoiled", "set_bvh2", "set_bvh2_ploc"])
def test_installed_trees_are_refitted_too(rt, orc, gpu_ctx, how):
    tris = small_scene(rt, "dragon")
    n = tris.size // 9
    gpu_ctx.set_triangles(tris)
    b2 = None
    if how == "set_bvh4":
        b4 = host_trees(rt, orc, tris, 1)[1]
        gpu_ctx.set_bvh4(b4)
    elif how == "set_bvh4_wide":                                           # BVH2 ids, nodes no path from the root reaches, boxes by the BVH2's rule
        b4 = rt.bvh2_to_bvh4_wide(orc.build_lbvh2(tris))
        gpu_ctx.set_bvh4(b4)
    elif how == "set_bvh4_spoiled":
        # children the reference skips: indices beyond the node count (their subtrees are no longer reachable and keep their words), and
        # leaves beyond the triangle count with an inverted box, which keep it: "fetched, never entered" in the wide records, also after the refit
        b4 = spoil_bvh4(host_trees(rt, orc, tris, 0)[1], 5)[0]
        rec = b4[1:].reshape(-1, 8)
        for i in np.nonzero(rec[:, 7] & 0x80000000)[0][10:400:40]:
            w0, w1 = int(rec[i, 0]), int(rec[i, 1])
            rec[i, 0] = (w0 & 0xFFFF0000) | (w1 >> 16); rec[i, 1] = (w1 & 0xFFFF) | ((w0 & 0xFFFF) << 16); rec[i, 7] = 0x80000000 | (n + 3)
        gpu_ctx.set_bvh4(b4)
    else:                                                                  # no parent[] on the device: derived from the child words
        b2 = rt.build_bvh2_ploc(tris) if how == "set_bvh2_ploc" else orc.build_lbvh2(tris)
        gpu_ctx.set_bvh2(b2)
        b4 = rt.collapse_lbvh2_to_bvh4(b2, n)[0]
    assert np.array_equal(gpu_ctx.read_bvh4(), b4)
    moved = wave(tris, 0.1, 2)
    got4 = update_and_compare(rt, gpu_ctx, moved, b4, b2)
    for mode in (rt.PT_MODE_REFERENCE_PACKET, rt.PT_MODE_REFERENCE, rt.PT_MODE_PATH):
        check_render(rt, orc, gpu_ctx, moved, got4, mode, False)
    cost = gpu_ctx.bvh_cost()
    want = rt.bvh4_cost(got4)
    assert abs(cost - want) <= int(got4[0]) * 2.0 ** -51 * want and want > 1.0


@pytest.mark.parametrize("accel", [0, 2])
@pytest.mark.parametrize("simple", [False, True])
@pytest.mark.parametrize("name", ["soup", "dragon"])
def test_renders_after_an_update_are_the_oracles(rt, orc, gpu_ctx, name, simple, accel):
    tris = small_scene(rt, name)
    gpu_ctx.set_triangles(tris)
    gpu_ctx.build_bvh(accel)
    gpu_ctx.render(gpu_ctx.make_params(160, 96, mode=rt.PT_MODE_PATH, spp=1))       # a frame of the old geometry first
    moved = wave(tris, 0.1, 5)
    gpu_ctx.update_triangles(moved)
    bvh4 = gpu_ctx.read_bvh4()
    for mode in (rt.PT_MODE_REFERENCE_PACKET, rt.PT_MODE_REFERENCE, rt.PT_MODE_PATH):
        if simple and mode == rt.PT_MODE_REFERENCE_PACKET:
            continue                                                       # the packet kernel has one form
        for cam in CAMS:
            check_render(rt, orc, gpu_ctx, moved, bvh4, mode, simple, cam=cam)


def test_vertices_beyond_the_f16_range_and_back(rt, orc, gpu_ctx):
    """Vertices beyond the f16 range give leaves boxes with an infinite side and a NaN pattern above it; frames equal the oracle's on the
    read-back tree, and the next update brings the built tree back."""
    tris = small_scene(rt, "soup")
    gpu_ctx.set_triangles(tris)
    gpu_ctx.build_bvh(2)
    b4 = gpu_ctx.read_bvh4()
    odd = tris.reshape(-1, 3, 3).copy()
    odd[100:110, :, 0] = np.float32(70000.0)                               # rounds to f16 infinity: the box's min steps down to 65504, its max up past +inf
    got = update_and_compare(rt, gpu_ctx, odd.reshape(-1), b4)
    check_render(rt, orc, gpu_ctx, odd.reshape(-1), got, rt.PT_MODE_REFERENCE, False)
    check_render(rt, orc, gpu_ctx, odd.reshape(-1), got, rt.PT_MODE_PATH, False)
    back = update_and_compare(rt, gpu_ctx, tris, b4)
    assert np.array_equal(back, b4)
    check_render(rt, orc, gpu_ctx, tris, b4, rt.PT_MODE_PATH, False)


@pytest.mark.parametrize("config", ["C2", "C4"])
def test_full_size_refit_words_and_frames(rt, orc, gpu_ctx, config):
    """C2 (871,414 triangles, PLOC tree) and C4 (262,144-triangle interior, reference tree) at full size: words against the host twins,
    then 1920x1080 / 4 spp / 8 bounces on every 4th pixel in x and y against the oracle on the read-back tree."""
    if config == "C2":
        tris, accel, cam, quat = rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 871414, SCENE_SEED), 2, (0, 0, 2.5), (0, 0, 0, 1)
    else:
        tris, accel, cam, quat = rt.procedural_scene(rt.SCENE_SPONZA_CLASS, 262144, SCENE_SEED), 0, (0.55, -0.05, 0.05), (0.0, 0.6630, 0.0, 0.7486)
    gpu_ctx.set_triangles(tris)
    gpu_ctx.build_bvh(accel)
    b4, b2 = gpu_ctx.read_bvh4(), gpu_ctx.read_bvh2()
    moved = wave(tris, 0.02, 4)
    got4 = update_and_compare(rt, gpu_ctx, moved, b4, b2)
    cost, want = gpu_ctx.bvh_cost(), rt.bvh4_cost(got4)
    print(config, "bvh_cost device", cost, "host", want)
    assert abs(cost - want) <= int(got4[0]) * 2.0 ** -51 * want
    w, h = 1920, 1080
    gpu_ctx.render(gpu_ctx.make_params(w, h, cam, quat, mode=rt.PT_MODE_PATH, spp=4, max_bounces=8, seed=1))
    img = gpu_ctx.read_radiance()
    ref, _ = orc.render_mt(orc.make_params(w, h, tris.size // 9, cam, quat, mode=orc_mod.MODE_PATH, spp=4, max_bounces=8, seed=1, step=(4, 4)), moved, got4)
    assert same_bits(img[::4, ::4], ref[::4, ::4])


@pytest.mark.parametrize("anyhit", [False, True])
def test_ray_queries_after_an_update(rt, orc, gpu_ctx, anyhit):
    tris = small_scene(rt, "dragon")
    gpu_ctx.set_triangles(tris)
    gpu_ctx.build_bvh(2)
    moved = wave(tris, 0.1, 6)
    gpu_ctx.update_triangles(moved)
    bvh4 = gpu_ctx.read_bvh4()
    O, D = random_rays(moved, 4000, 61)
    hit, ot, oprim = oracle_batch(orc, moved, bvh4, O, D, anyhit=anyhit)
    for simple in (False, True):
        t, prim, _, _ = gpu_ctx.trace_rays(O, D, any_hit=anyhit, simple=simple)
        assert np.array_equal(prim != MISS, hit) and np.array_equal(prim[hit], oprim[hit]) and same_bits(t[hit], ot[hit])
    assert hit.sum() > 200


def test_eight_updates_and_back_restore_tree_and_frame(rt, orc, gpu_ctx):
    tris = small_scene(rt, "dragon")
    gpu_ctx.set_triangles(tris)
    gpu_ctx.build_bvh(2)
    b4, b2 = gpu_ctx.read_bvh4(), gpu_ctx.read_bvh2()
    p = gpu_ctx.make_params(160, 96, mode=rt.PT_MODE_PATH, spp=2, max_bounces=4, seed=3)
    gpu_ctx.render(p)
    first = gpu_ctx.read_radiance().copy()
    for k in range(8):
        moved = wave(tris, 0.04 * (k + 1), k)
        gpu_ctx.update_triangles(moved)
    assert np.array_equal(gpu_ctx.read_bvh4(), rt.refit_bvh4(moved, b4))    # one refit with the last triangles: no memory of the others
    gpu_ctx.update_triangles(tris)
    assert np.array_equal(gpu_ctx.read_bvh4(), b4) and np.array_equal(gpu_ctx.read_bvh2(), b2)
    gpu_ctx.render(p)
    assert same_bits(gpu_ctx.read_radiance(), first)


def test_accumulation_restarts_after_an_update(rt, orc, gpu_ctx):
    tris = small_scene(rt, "dragon")
    n = tris.size // 9
    gpu_ctx.set_triangles(tris)
    gpu_ctx.build_bvh()
    w, h = 128, 72
    kw = dict(mode=rt.PT_MODE_PATH, spp=2, max_bounces=3, seed=9)
    for f in range(3):
        gpu_ctx.render(gpu_ctx.make_params(w, h, frame=f, accumulate=True, **kw))
    assert gpu_ctx.accum_info().samples == 6
    moved = wave(tris, 0.1, 1)
    gpu_ctx.update_triangles(moved)
    bvh4 = gpu_ctx.read_bvh4()
    for f in range(2):
        gpu_ctx.render(gpu_ctx.make_params(w, h, frame=10 + f, accumulate=True, **kw))
    assert gpu_ctx.accum_info().samples == 4
    want, _, _ = orc.render(orc.make_params(w, h, n, mode=orc_mod.MODE_PATH, spp=2, max_bounces=3, seed=9, frame=10, accum_frames=2), moved, bvh4)
    assert same_bits(gpu_ctx.read_radiance(), want)


def test_update_without_a_tree_only_replaces_the_triangles(rt, orc, gpu_ctx):
    tris = small_scene(rt, "soup")
    moved = wave(tris, 0.1, 2)
    gpu_ctx.set_triangles(tris)
    gpu_ctx.update_triangles(moved)                                        # no tree yet
    gpu_ctx.build_bvh()
    assert np.array_equal(gpu_ctx.read_bvh4(), orc.build_bvh4(moved)[1])
    check_render(rt, orc, gpu_ctx, moved, gpu_ctx.read_bvh4(), rt.PT_MODE_PATH, False)


def test_refused_updates_leave_the_context_as_it_was(rt, orc, gpu_ctx):
    tris = small_scene(rt, "soup")
    n = tris.size // 9
    moved = wave(tris, 0.2, 1)
    fp = C.POINTER(C.c_float)

    assert code(rt, lambda: gpu_ctx.update_triangles(moved)) == 4              # PT_ERR_NO_SCENE: no triangles yet
    assert code(rt, lambda: gpu_ctx.bvh_cost()) == 4
    gpu_ctx.set_triangles(tris)
    assert code(rt, lambda: gpu_ctx.bvh_cost()) == 4                           # triangles without a tree
    gpu_ctx.build_bvh(2)
    b4, b2 = gpu_ctx.read_bvh4(), gpu_ctx.read_bvh2()
    p = gpu_ctx.make_params(128, 72, mode=rt.PT_MODE_PATH, spp=2, max_bounces=4, seed=2)
    gpu_ctx.render(p)
    frame = gpu_ctx.read_radiance().copy()
    assert code(rt, lambda: gpu_ctx.update_triangles(moved[:-9])) == 1         # another count
    assert code(rt, lambda: gpu_ctx.update_triangles(np.concatenate([moved, moved[:9]]))) == 1
    assert rt.lib.pt_update_triangles(gpu_ctx.h, None, C.c_uint32(n)) == 1                  # NULL
    assert rt.lib.pt_update_triangles_device(gpu_ctx.h, None, C.c_uint32(n)) == 1
    assert code(rt, lambda: gpu_ctx.update_triangles_device(0x1000 + 4, n)) == 1                # not 16-byte aligned: refused before it is read
    assert rt.lib.pt_bvh_cost(gpu_ctx.h, None) == 1
    assert np.array_equal(gpu_ctx.read_bvh4(), b4) and np.array_equal(gpu_ctx.read_bvh2(), b2)
    gpu_ctx.render(p)
    assert same_bits(gpu_ctx.read_radiance(), frame)
    empty = rt.Context(0)                                                  # an empty scene: PT_OK, nothing to launch
    try:
        empty.set_triangles(np.zeros(0, np.float32))
        assert rt.lib.pt_update_triangles(empty.h, moved.ctypes.data_as(fp), C.c_uint32(0)) == 0
    finally:
        empty.close()


def test_group_update_triangles(rt, orc):
    tris = rt.procedural_scene(0, 20000)
    moved = wave(tris, 0.1, 3)
    one = rt.Context(0)
    g = rt.Group([0, 0], rt.PT_GROUP_TRANSPORT_COPY)
    try:
        one.set_triangles(tris); one.build_bvh(rt.PT_ACCEL_PLOC); one.update_triangles(moved)
        g.set_triangles(tris); g.build_bvh(rt.PT_ACCEL_PLOC)
        w, h = 200, 120
        kw = dict(mode=rt.PT_MODE_PATH, spp=2, max_bounces=4, seed=5, frame=1)
        g.render(g.make_params(w, h, **kw))                                # the old geometry first
        g.update_triangles(moved)
        g.render(g.make_params(w, h, **kw))
        ref, _, _ = orc.render(orc.make_params(w, h, tris.size // 9, mode=orc_mod.MODE_PATH, spp=2, max_bounces=4, seed=5, frame=1), moved, one.read_bvh4())
        assert same_bits(g.read_radiance(), ref)
        with pytest.raises(rt.PtError):
            g.update_triangles(moved[:-9])
    finally:
        g.close(); one.close()


@pytest.mark.parametrize("case", ["device_route_equals_the_host_route", "ordering_with_batched_frames", "device_route_on_c2"])
def test_torch_route(case):
    """The zero-copy device route (a torch tensor of vertices), its ordering with queued frames and with torch's streams:
    tests/refit_torch_cases.py in a child process (torch has to be imported before the package)."""
    run_case("refit_torch_cases", case, timeout=900)


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_node_update_triangles_and_the_animated_driver(tmp_path, rt, orc):
    """pathTracer.updateTriangles / bvhCost through the addon equal the ctypes route; `main.js --animate 0.1 --frames 3 --out f.ppm` writes,
    byte for byte, the oracle's tonemapper over the oracle's frame of the displaced scene on the refitted tree."""
    import json
    n = 5000
    script = tmp_path / "refit.js"
    script.write_text("""
const PT = require(%r);
(async () => {
  const tris = require(%r).proceduralScene(0, %d, 7);
  const pt = new PT.PathTracer({ width: 32, height: 32 }, { accel: 2 });
  await pt.initialize();
  await pt.buildBVH(tris);
  const moved = Float32Array.from(tris);
  for (let i = 1; i < moved.length; i += 3) moved[i] = Math.fround(moved[i] + Math.fround(0.0625 * moved[i - 1]));
  const before = pt.bvhCost();
  pt.updateTriangles(moved);
  const after = pt.bvhCost();
  const b2 = await pt.readBVH2(4 * (1 + 6 * (2 * %d - 1)));
  const fs = require("fs");
  fs.writeFileSync(%r, Buffer.from(b2.buffer, b2.byteOffset, b2.byteLength));
  fs.writeFileSync(%r, Buffer.from(tris.buffer, tris.byteOffset, tris.byteLength));
  fs.writeFileSync(%r, Buffer.from(moved.buffer, moved.byteOffset, moved.byteLength));
  fs.writeFileSync(%r, JSON.stringify({ before, after }));
  let refused = false;
  try { pt.updateTriangles(moved.subarray(9)); } catch (e) { refused = true; }
  if (!refused) throw new Error("a shorter array was accepted");
})().catch((e) => { console.error(e); process.exit(1); });
""" % (os.path.join(JS, "PathTracer.js"), ADDON, n, n, str(tmp_path / "b2.bin"), str(tmp_path / "t.bin"), str(tmp_path / "m.bin"), str(tmp_path / "cost.json")))
    r = subprocess.run([NODE, str(script)], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    tris, moved = np.fromfile(str(tmp_path / "t.bin"), np.float32), np.fromfile(str(tmp_path / "m.bin"), np.float32)
    b2 = np.fromfile(str(tmp_path / "b2.bin"), np.uint32)
    costs = json.loads((tmp_path / "cost.json").read_text())
    ctx = rt.Context(0)
    try:
        ctx.set_triangles(tris); ctx.build_bvh(rt.PT_ACCEL_PLOC)
        m = ctx.scene_info()["numNodes4"]
        built = rt.bvh4_cost(ctx.read_bvh4())
        assert abs(costs["before"] - built) <= m * 2.0 ** -51 * built
        ctx.update_triangles(moved)
        assert np.array_equal(b2, ctx.read_bvh2()) and np.array_equal(b2, rt.refit_bvh2(moved, rt.build_bvh2_ploc(tris)))
        want = rt.bvh4_cost(ctx.read_bvh4())
        assert abs(costs["after"] - want) <= m * 2.0 ** -51 * want
    finally:
        ctx.close()
    # the driver: before render() number f (1-based, the frame count it sets) the scene as built is displaced with the wave of frame f
    w, h, n, frames, amp = 320, 180, 20000, 3, 0.1
    ppm = tmp_path / "f.ppm"
    r = subprocess.run([NODE, os.path.join(JS, "main.js"), "--tris", str(n), "--accel", "2", "--mode", "1", "--frames", str(frames), "--animate", str(amp),
                        "--width", str(w), "--height", str(h), "--out", str(ppm), "--radiance", str(tmp_path / "img.f32"),
                        "--triangles", str(tmp_path / "tris.f32")], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    base = rt.procedural_scene(rt.SCENE_DRAGON_CLASS, n, SCENE_SEED)            # the stand-in scene the driver builds its tree over
    moved = wave(base, amp, frames)
    assert same_bits(np.fromfile(str(tmp_path / "tris.f32"), np.float32), moved)     # the driver's displacement is the restated one, bit for bit
    built = rt.collapse_bvh2_to_bvh4_accel(rt.build_bvh2_ploc(base), n, rt.PT_ACCEL_PLOC)[0]
    bvh4 = rt.refit_bvh4(moved, built)
    ref, _, _ = orc.render(orc.make_params(w, h, n, mode=orc_mod.MODE_SINGLE, frame=frames), moved, bvh4)
    assert same_bits(np.fromfile(str(tmp_path / "img.f32"), np.float32).reshape(h, w, 4), ref)
    head = ("P6\n%d %d\n255\n" % (w, h)).encode()
    assert ppm.read_bytes() == head + np.ascontiguousarray(orc.tonemap(ref, quantize=True)[..., :3]).astype(np.uint8).tobytes()
