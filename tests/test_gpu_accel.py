"""Opt-in tree quality on the device (pt_build_bvh_accel, include/mi355pt.h PT_ACCEL_*): level 0 is
pt_build_bvh word for word; levels 1 and 2 equal their host twins word for word (BVH2 and BVH4); every renderer traverses the new
trees exactly as the oracle does (image and counters, bit for bit); groups, the Node host and the driver pass the option on."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import orc as orc_mod
from scenes import TETRA, random_soup, quat_yaw_pitch
from test_accel_host import DEGENERATE, degenerate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
MAIN_JS = os.path.join(ROOT, "raytracer-public_amd", "js", "main.js")
SCENE_SEED = 20260109
KEYS_REF = ("rays_closest", "nodes_examined", "tris_tested", "stack_drops", "max_stack", "samples")
KEYS_PATH = ("rays_closest", "rays_shadow", "nodes_examined", "tris_tested", "samples")


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def host_trees(rt, orc, tris, accel):
    """(BVH2, BVH4) that the host twins give for build level `accel`."""
    n = tris.size // 9
    b2 = rt.build_bvh2_ploc(tris) if accel == rt.PT_ACCEL_PLOC else orc.build_lbvh2(tris)
    return b2, rt.collapse_bvh2_to_bvh4_accel(b2, n, accel)[0]


def build_and_compare(rt, orc, ctx, tris, accel):
    ctx.set_triangles(tris)
    ctx.build_bvh(accel)
    b2, b4 = host_trees(rt, orc, tris, accel)
    got4 = ctx.read_bvh4()
    got2 = ctx.read_bvh2()
    assert np.array_equal(got4, b4), accel
    assert np.array_equal(got2, b2), accel
    return b4


@pytest.mark.parametrize("n,seed", [(1, 0), (2, 1), (4, 0), (3, 2), (1000, 3), (20000, 4), (120000, 5)])
def test_accel_0_is_pt_build_bvh(rt, orc, gpu_ctx, n, seed):
    tris = TETRA if n == 4 else random_soup(n, seed)
    gpu_ctx.set_triangles(tris)
    gpu_ctx.build_bvh()
    b2, b4 = gpu_ctx.read_bvh2(), gpu_ctx.read_bvh4()
    assert rt.lib.pt_build_bvh_accel(gpu_ctx.h, 0) == 0
    assert np.array_equal(gpu_ctx.read_bvh4(), b4) and np.array_equal(gpu_ctx.read_bvh2(), b2)


@pytest.mark.parametrize("accel", [1, 2])
@pytest.mark.parametrize("n,seed", [(1, 0), (2, 1), (4, 0), (3, 2), (1000, 3), (20000, 4), (120000, 5)])
def test_device_trees_equal_the_host_twins(rt, orc, gpu_ctx, n, seed, accel):
    tris = TETRA if n == 4 else random_soup(n, seed)
    build_and_compare(rt, orc, gpu_ctx, tris, accel)


@pytest.mark.parametrize("accel", [1, 2])
@pytest.mark.parametrize("kind", DEGENERATE)
def test_device_trees_on_degenerate_inputs(rt, orc, gpu_ctx, kind, accel):
    tris = degenerate(kind)
    b4 = build_and_compare(rt, orc, gpu_ctx, tris, accel)
    p = gpu_ctx.make_params(64, 48, (0, 0, 2.5), (0, 0, 0, 1), mode=rt.PT_MODE_REFERENCE)
    gpu_ctx.render(p)
    want, _, _ = orc.render(orc.make_params(64, 48, tris.size // 9, (0, 0, 2.5), (0, 0, 0, 1), mode=orc_mod.MODE_SINGLE), tris, b4)
    assert same_bits(gpu_ctx.read_radiance(), want)


@pytest.mark.parametrize("accel", [1, 2])
@pytest.mark.parametrize("config", ["C2", "C4"])
def test_full_size_trees_equal_the_host_twins(rt, orc, gpu_ctx, config, accel):
    kind, n = (rt.SCENE_DRAGON_CLASS, 871414) if config == "C2" else (rt.SCENE_SPONZA_CLASS, 262144)
    tris = rt.procedural_scene(kind, n, SCENE_SEED)
    build_and_compare(rt, orc, gpu_ctx, tris, accel)


CAMS = [((0, 0, 2.5), (0, 0, 0, 1)), ((0.4, 0.3, 1.7), quat_yaw_pitch(0.2, -0.15)), ((0, 0, 0), quat_yaw_pitch(2.0, 0.4))]


@pytest.mark.parametrize("accel", [1, 2])
@pytest.mark.parametrize("kind", ["soup", "dragon"])
def test_renders_on_accel_trees_bit_exact(rt, orc, gpu_ctx, kind, accel):
    tris = random_soup(3000, 11) if kind == "soup" else rt.procedural_scene(0, 20000)
    n = tris.size // 9
    gpu_ctx.set_triangles(tris)
    gpu_ctx.build_bvh(accel)
    bvh4 = gpu_ctx.read_bvh4()
    w, h = 160, 96
    for cam, quat in CAMS:
        gpu_ctx.render(gpu_ctx.make_params(w, h, cam, quat, mode=rt.PT_MODE_REFERENCE, stats=True))
        ref, _, ost = orc.render(orc.make_params(w, h, n, cam, quat, mode=orc_mod.MODE_SINGLE), tris, bvh4)
        assert same_bits(gpu_ctx.read_radiance(), ref)
        st = gpu_ctx.stats()
        for k in KEYS_REF:
            assert st[k] == ost[k], (k, cam)
    cam, quat = CAMS[1]
    gpu_ctx.render(gpu_ctx.make_params(w, h, cam, quat, mode=rt.PT_MODE_REFERENCE_PACKET, stats=True))
    ref, _, ost = orc.render(orc.make_params(w, h, n, cam, quat, mode=orc_mod.MODE_PACKET), tris, bvh4)
    assert same_bits(gpu_ctx.read_radiance(), ref)
    st = gpu_ctx.stats()
    for k in KEYS_REF:
        assert st[k] == ost[k], k
    cam, quat = CAMS[0] if kind != "soup" else CAMS[2]
    gpu_ctx.render(gpu_ctx.make_params(w, h, cam, quat, mode=rt.PT_MODE_PATH, spp=3, max_bounces=6, seed=7, frame=3, stats=True))
    ref, _, ost = orc.render(orc.make_params(w, h, n, cam, quat, mode=orc_mod.MODE_PATH, spp=3, max_bounces=6, seed=7, frame=3), tris, bvh4)
    assert same_bits(gpu_ctx.read_radiance(), ref)
    st = gpu_ctx.stats()
    for k in KEYS_PATH:
        assert st[k] == ost[k], k


@pytest.mark.parametrize("accel", [1, 2])
def test_c2_full_size_on_a_sixteenth_grid(rt, orc, gpu_ctx, accel):
    """C2 at full size (871,414 triangles, 1920x1080, 4 spp, 8 bounces) on an accel tree: every 4th pixel in x and y against the oracle."""
    tris = rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 871414, SCENE_SEED)
    gpu_ctx.set_triangles(tris)
    gpu_ctx.build_bvh(accel)
    bvh4 = gpu_ctx.read_bvh4()
    w, h = 1920, 1080
    gpu_ctx.render(gpu_ctx.make_params(w, h, mode=rt.PT_MODE_PATH, spp=4, max_bounces=8, seed=1))
    img = gpu_ctx.read_radiance()
    ref, _ = orc.render_mt(orc.make_params(w, h, tris.size // 9, mode=orc_mod.MODE_PATH, spp=4, max_bounces=8, seed=1, step=(4, 4)), tris, bvh4)
    assert same_bits(img[::4, ::4], ref[::4, ::4])


def test_c4_full_frame_at_accel_2(rt, orc, gpu_ctx):
    """C4 (262,144-triangle interior, camera inside) on the PLOC tree: the whole 1920x1080 frame and its counters against the oracle."""
    tris = rt.procedural_scene(rt.SCENE_SPONZA_CLASS, 262144, SCENE_SEED)
    gpu_ctx.set_triangles(tris)
    gpu_ctx.build_bvh(rt.PT_ACCEL_PLOC)
    bvh4 = gpu_ctx.read_bvh4()
    w, h = 1920, 1080
    cam, quat = (0.55, -0.05, 0.05), (0.0, 0.6630, 0.0, 0.7486)
    gpu_ctx.render(gpu_ctx.make_params(w, h, cam, quat, mode=rt.PT_MODE_PATH, spp=4, max_bounces=8, seed=1, stats=True))
    img = gpu_ctx.read_radiance()
    st = gpu_ctx.stats()
    ref, ost = orc.render_mt(orc.make_params(w, h, tris.size // 9, cam, quat, mode=orc_mod.MODE_PATH, spp=4, max_bounces=8, seed=1), tris, bvh4)
    assert same_bits(img, ref)
    for k in KEYS_PATH:
        assert st[k] == ost[k], k


def test_group_members_build_the_same_ploc_tree(rt, orc):
    tris = rt.procedural_scene(0, 20000)
    one = rt.Context(0)
    g = rt.Group([0, 0], rt.PT_GROUP_TRANSPORT_COPY)
    try:
        one.set_triangles(tris); one.build_bvh(rt.PT_ACCEL_PLOC)
        g.set_triangles(tris); g.build_bvh(rt.PT_ACCEL_PLOC)
        w, h = 200, 120
        kw = dict(mode=rt.PT_MODE_PATH, spp=2, max_bounces=4, seed=5, frame=1)
        one.render(one.make_params(w, h, **kw))
        g.render(g.make_params(w, h, **kw))
        assert same_bits(g.read_radiance(), one.read_radiance())
        ref, _, _ = orc.render(orc.make_params(w, h, tris.size // 9, mode=orc_mod.MODE_PATH, spp=2, max_bounces=4, seed=5, frame=1), tris, one.read_bvh4())
        assert same_bits(one.read_radiance(), ref)
        with pytest.raises(rt.PtError):
            g.build_bvh(7)
    finally:
        g.close(); one.close()


def test_invalid_accel_leaves_the_context_usable(rt, orc, gpu_ctx):
    tris = random_soup(500, 2)
    gpu_ctx.set_triangles(tris)
    gpu_ctx.build_bvh(rt.PT_ACCEL_PLOC)
    for bad in (3, 0xFFFFFFFF):
        with pytest.raises(rt.PtError) as e:
            gpu_ctx.build_bvh(bad)
        assert e.value.code == 1                                          # PT_ERR_INVALID_ARG
        assert rt.lib.pt_build_bvh_accel(gpu_ctx.h, bad) == 1
    bvh4 = gpu_ctx.read_bvh4()
    assert np.array_equal(bvh4, host_trees(rt, orc, tris, rt.PT_ACCEL_PLOC)[1])   # the tree built before is still installed
    gpu_ctx.render(gpu_ctx.make_params(64, 48, mode=rt.PT_MODE_REFERENCE))
    ref, _, _ = orc.render(orc.make_params(64, 48, 500, mode=orc_mod.MODE_SINGLE), tris, bvh4)
    assert same_bits(gpu_ctx.read_radiance(), ref)


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_node_host_and_driver_pass_accel_on(tmp_path, rt, orc):
    """new PathTracer(canvas, { accel: 2 }) builds the tree the ctypes binding builds; `main.js --accel 2 --out frame.ppm` writes the
    oracle's tonemapper over the oracle's frame on that tree."""
    script = tmp_path / "accel.js"
    script.write_text("""
const PT = require(%r);
(async () => {
  const tris = require(%r).proceduralScene(0, 5000, 7);
  const pt = new PT.PathTracer({ width: 32, height: 32 }, { accel: 2 });
  await pt.initialize();
  await pt.buildBVH(tris);
  const b2 = await pt.readBVH2(4 * (1 + 6 * (2 * 5000 - 1)));
  require("fs").writeFileSync(%r, Buffer.from(b2.buffer, b2.byteOffset, b2.byteLength));
  require("fs").writeFileSync(%r, Buffer.from(tris.buffer, tris.byteOffset, tris.byteLength));
})().catch((e) => { console.error(e); process.exit(1); });
""" % (os.path.join(ROOT, "raytracer-public_amd", "js", "PathTracer.js"), os.path.join(ROOT, "raytracer-public_amd", "napi", "mi355pt.node"),
       str(tmp_path / "b2.bin"), str(tmp_path / "t.bin")))
    r = subprocess.run([NODE, str(script)], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    tris = np.fromfile(str(tmp_path / "t.bin"), np.float32)
    b2 = np.fromfile(str(tmp_path / "b2.bin"), np.uint32)
    ctx = rt.Context(0)
    try:
        ctx.set_triangles(tris); ctx.build_bvh(rt.PT_ACCEL_PLOC)
        assert np.array_equal(b2, ctx.read_bvh2())
    finally:
        ctx.close()
    assert np.array_equal(b2, rt.build_bvh2_ploc(tris))
    # the driver
    w, h, n = 320, 180, 20000
    ppm = tmp_path / "frame.ppm"
    r = subprocess.run([NODE, MAIN_JS, "--tris", str(n), "--accel", "2", "--mode", "1", "--frames", "2", "--width", str(w), "--height", str(h),
                        "--dump", str(tmp_path / "d" / "BVH2.bin"), "--out", str(ppm), "--radiance", str(tmp_path / "img.f32"),
                        "--triangles", str(tmp_path / "tris.f32")], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    tris = np.fromfile(str(tmp_path / "tris.f32"), np.float32)
    dumped = np.fromfile(str(tmp_path / "d" / "BVH2.bin"), np.uint32)
    assert np.array_equal(dumped, rt.build_bvh2_ploc(tris))              # data/BVH2.bin holds the PLOC BVH2
    bvh4, _ = rt.collapse_bvh2_to_bvh4_accel(dumped, n, rt.PT_ACCEL_PLOC)
    ref, _, _ = orc.render(orc.make_params(w, h, n, mode=orc_mod.MODE_SINGLE, frame=2), tris, bvh4)
    assert same_bits(np.fromfile(str(tmp_path / "img.f32"), np.float32).reshape(h, w, 4), ref)
    raw = ppm.read_bytes()
    head = ("P6\n%d %d\n255\n" % (w, h)).encode()
    assert raw.startswith(head) and len(raw) == len(head) + w * h * 3
    assert np.array_equal(np.frombuffer(raw[len(head):], np.uint8).reshape(h, w, 3), orc.tonemap(ref, quantize=True)[..., :3])
