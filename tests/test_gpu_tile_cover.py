"""The tile cover (pt_cover.hip): launches trace only the tiles that the live boxes of a breadth-first cut of the
tree reach from the launch's cameras.  The cover is conservative (every tile with a hit pixel is traced), not vacuous (it drops tiles
the root box's rectangle keeps), and invisible in the result: every frame equals the oracle's, and the rectangle-only launch's
(knob CULL = 1), bit for bit.  Dragon-class scene, 20,000 triangles, 256x144; the oracle renders the read-back device tree."""
import ctypes as C
import functools

import numpy as np
import pytest

import orc as orc_mod
from refit_cases import wave
from scenes import quat_yaw_pitch

pytestmark = pytest.mark.gpu

W, H, NTRIS = 256, 144, 20000
DEFAULT = ((0, 0, 2.5), (0, 0, 0, 1))
ROTATED = [((0.4, 0.3, 1.7), quat_yaw_pitch(0.2, -0.15)), ((2.2, 0.6, 1.6), quat_yaw_pitch(0.9, -0.2))]
PATH = dict(spp=2, max_bounces=3, seed=5)
COUNTERS = ("rays_closest", "rays_shadow", "nodes_examined", "tris_tested", "stack_drops", "max_stack", "samples")


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@functools.lru_cache(maxsize=None)
def _tris():
    import importlib
    t = importlib.import_module("raytracer-public_amd").procedural_scene(0, NTRIS)
    t.setflags(write=False)
    return t


_REF = {}


def oracle(orc, bvh4, tris_key, tris, w, h, cam, quat, mode, **kw):
    """One oracle frame per (geometry, camera, mode, ...), shared by the tests; the device tree of a geometry is the same in every context."""
    key = (tris_key, w, h, cam, tuple(float(v) for v in quat), mode, tuple(sorted(kw.items())))
    if key not in _REF:
        img, ids, st = orc.render(orc.make_params(w, h, tris.size // 9, cam, quat, mode=mode, **kw), tris, bvh4, want_tri_ids=(mode == orc_mod.MODE_SINGLE))
        for a in (img, ids):
            if a is not None: a.setflags(write=False)
        _REF[key] = (img, ids, st)
    return _REF[key]


def hit_tiles(ids, w, h):
    t = np.zeros(((h + 7) // 8, (w + 7) // 8), bool)
    ys, xs = np.nonzero(ids != 0xFFFFFFFF)
    t[ys // 8, xs // 8] = True
    return t


def settle(ctx, *cams, w=W, h=H):
    """A launch computes the cover of a view when it sees the view the second time (the first keeps the rectangle); the diagnostics call
    computes it at once, so the launches that follow use it."""
    for cam, quat in cams:
        ctx.debug_traced_tiles(ctx.make_params(w, h, cam, quat))


def scene(ctx):
    ctx.set_triangles(_tris()); ctx.build_bvh()
    return _tris(), ctx.read_bvh4()


@pytest.mark.parametrize("w,h,cam,quat", [(W, H) + DEFAULT, (W, H) + ROTATED[0], (W, H) + ROTATED[1], (250, 141) + DEFAULT])
def test_cover_holds_every_hit_tile_and_drops_some(rt, orc, gpu_ctx, w, h, cam, quat):
    """Every tile with a hit pixel of the oracle's mode-1 frame (every pixel centre) is traced; the cover is a subset of the rectangle's tiles
    and a proper one.  Default camera: the CPU simulation of the design (cut of 2,270 entries) drops 70 of the rectangle's 196 tiles and 99
    tiles hold a hit, so at least 40 must go."""
    tris, bvh4 = scene(gpu_ctx)
    p = gpu_ctx.make_params(w, h, cam, quat, mode=rt.PT_MODE_REFERENCE)
    mask, rect_tiles, traced = gpu_ctx.debug_traced_tiles(p)
    _, ids, _ = oracle(orc, bvh4, "rest", tris, w, h, cam, quat, orc_mod.MODE_SINGLE)
    hits = hit_tiles(ids, w, h)
    print("rect %d traced %d hit tiles %d" % (rect_tiles, traced, int(hits.sum())))
    assert hits.any() and not (hits & ~mask).any()
    assert traced == int(mask.sum()) and traced < rect_tiles
    r = gpu_ctx.traced_tile_rect(p)
    inside = np.zeros_like(mask); inside[r[1]:r[3], r[0]:r[2]] = True
    assert rect_tiles == int(inside.sum()) and not (mask & ~inside).any()
    if (w, h, cam) == (W, H, DEFAULT[0]) and tuple(quat) == DEFAULT[1]:
        assert rect_tiles - traced >= 40
    # knob CULL = 1 is the rectangle, 0 is every tile, an instrumented launch keeps the rectangle
    gpu_ctx.debug_set_tune("CULL", 1)
    m1, r1, t1 = gpu_ctx.debug_traced_tiles(p)
    assert np.array_equal(m1, inside) and r1 == t1 == rect_tiles
    gpu_ctx.debug_set_tune("CULL", 0)
    m0, r0, t0 = gpu_ctx.debug_traced_tiles(p)
    assert m0.all() and r0 == t0 == m0.size
    gpu_ctx.debug_set_tune("CULL", None)
    ms, rs, ts = gpu_ctx.debug_traced_tiles(gpu_ctx.make_params(w, h, cam, quat, mode=rt.PT_MODE_REFERENCE, stats=True))
    assert np.array_equal(ms, inside) and rs == ts == rect_tiles


def test_camera_beside_a_root_corner_traces_todays_set(rt, orc, gpu_ctx):
    """A root-box corner beside or behind the eye: no rectangle, no cover -- every tile, as before; the frame is the oracle's."""
    tris, bvh4 = scene(gpu_ctx)
    cam, quat = (0, 0, 0.2), (0, 0, 0, 1)
    p = gpu_ctx.make_params(W, H, cam, quat, mode=rt.PT_MODE_PATH, **PATH)
    mask, rect_tiles, traced = gpu_ctx.debug_traced_tiles(p)
    assert gpu_ctx.traced_tile_rect(p) == (0, 0, W // 8, H // 8)
    assert mask.all() and rect_tiles == traced == mask.size
    gpu_ctx.debug_set_tune("CULL", 1)
    m1, r1, t1 = gpu_ctx.debug_traced_tiles(p)
    gpu_ctx.debug_set_tune("CULL", None)
    assert np.array_equal(m1, mask) and (r1, t1) == (rect_tiles, traced)
    gpu_ctx.render(p)
    assert same_bits(gpu_ctx.read_radiance(), oracle(orc, bvh4, "rest", tris, W, H, cam, quat, orc_mod.MODE_PATH, **PATH)[0])


@pytest.mark.parametrize("cam,quat", [DEFAULT, ROTATED[1]])
def test_images_and_counters_unchanged(rt, orc, gpu_ctx, cam, quat):
    """CULL 2 and CULL 1: mode 2 and mode 1 give byte-identical frames, both the oracle's on every pixel; an instrumented launch counts the
    same with either knob (it keeps the rectangle)."""
    tris, bvh4 = scene(gpu_ctx)
    want2 = oracle(orc, bvh4, "rest", tris, W, H, cam, quat, orc_mod.MODE_PATH, **PATH)[0]
    want1 = oracle(orc, bvh4, "rest", tris, W, H, cam, quat, orc_mod.MODE_SINGLE)[0]
    got, counters = {}, {}
    settle(gpu_ctx, (cam, quat))
    for knob in (2, 1):
        gpu_ctx.debug_set_tune("CULL", knob)
        gpu_ctx.render(gpu_ctx.make_params(W, H, cam, quat, mode=rt.PT_MODE_PATH, **PATH))
        got[knob, 2] = gpu_ctx.read_radiance().copy()
        gpu_ctx.render(gpu_ctx.make_params(W, H, cam, quat, mode=rt.PT_MODE_REFERENCE))
        got[knob, 1] = gpu_ctx.read_radiance().copy()
        gpu_ctx.render(gpu_ctx.make_params(W, H, cam, quat, mode=rt.PT_MODE_PATH, stats=True, **PATH))
        st = gpu_ctx.stats()
        counters[knob] = tuple(st[k] for k in COUNTERS)
        assert same_bits(gpu_ctx.read_radiance(), want2)
    gpu_ctx.debug_set_tune("CULL", None)
    assert got[2, 2].tobytes() == got[1, 2].tobytes() and got[2, 1].tobytes() == got[1, 1].tobytes()
    assert same_bits(got[2, 2], want2) and same_bits(got[2, 1], want1)
    assert counters[2] == counters[1]
    gpu_ctx.render(gpu_ctx.make_params(W, H, cam, quat, mode=rt.PT_MODE_PATH, **PATH))      # the automatic default is the cover
    assert same_bits(gpu_ctx.read_radiance(), want2)


def test_three_cameras_in_one_launch(rt, orc, gpu_ctx):
    """The cover of a batch is the union over its cameras: three frames with three cameras in one launch equal three single launches (and the oracle)."""
    tris, bvh4 = scene(gpu_ctx)
    hip = C.CDLL("libamdhip64.so")
    cams = [DEFAULT] + ROTATED
    floats = W * H * 4
    single = []
    settle(gpu_ctx, *cams)
    for cam, quat in cams:
        gpu_ctx.render(gpu_ctx.make_params(W, H, cam, quat, mode=rt.PT_MODE_PATH, frame=7, **PATH))
        single.append(gpu_ctx.read_radiance().copy())
        assert same_bits(single[-1], oracle(orc, bvh4, "rest", tris, W, H, cam, quat, orc_mod.MODE_PATH, frame=7, **PATH)[0])
    bufs = []
    try:
        for _ in cams:
            b = C.c_void_p(); assert hip.hipMalloc(C.byref(b), C.c_size_t(floats * 4)) == 0; bufs.append(b)
        gpu_ctx.set_batch(len(cams))
        for attempt in range(3):              # the first launch of this set of cameras keeps the rectangle, the second takes their cover, the third finds it
            for (cam, quat), b in zip(cams, bufs):
                gpu_ctx.set_output_buffer(b.value, floats)
                gpu_ctx.render(gpu_ctx.make_params(W, H, cam, quat, mode=rt.PT_MODE_PATH, frame=7, **PATH))
            gpu_ctx.synchronize()
            for i, b in enumerate(bufs):
                host = np.zeros((H, W, 4), np.float32)
                assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), b, C.c_size_t(floats * 4), 2) == 0
                assert same_bits(host, single[i]), (attempt, i)
                assert hip.hipMemset(b, 0, C.c_size_t(floats * 4)) == 0 and hip.hipDeviceSynchronize() == 0
    finally:
        gpu_ctx.set_output_buffer(0, 0); gpu_ctx.set_batch(1)
        for b in bufs: hip.hipFree(b)


def test_two_accumulated_frames(rt, orc, gpu_ctx):
    tris, bvh4 = scene(gpu_ctx)
    settle(gpu_ctx, DEFAULT)
    for f in range(2):
        gpu_ctx.render(gpu_ctx.make_params(W, H, *DEFAULT, mode=rt.PT_MODE_PATH, frame=20 + f, accumulate=True, **PATH))
    assert gpu_ctx.accum_info().samples == 2 * PATH["spp"]
    want = oracle(orc, bvh4, "rest", tris, W, H, *DEFAULT, orc_mod.MODE_PATH, frame=20, accum_frames=2, **PATH)[0]
    assert same_bits(gpu_ctx.read_radiance(), want)


def test_tile_shares_rebuild_the_frame(rt, orc, gpu_ctx):
    """Tile shares of 3 (rank 1 among them) through the compact buffer, packed by the rectangle and unpacked: the oracle's frame.  A share's traced
    tiles are its own tiles under the cover."""
    tris, bvh4 = scene(gpu_ctx)
    hip = C.CDLL("libamdhip64.so")
    world = 3
    kw = dict(mode=rt.PT_MODE_PATH, **PATH)
    whole, _, traced_all = gpu_ctx.debug_traced_tiles(gpu_ctx.make_params(W, H, *DEFAULT, **kw))
    rect = gpu_ctx.traced_tile_rect(gpu_ctx.make_params(W, H, *DEFAULT, **kw))
    stride = max(rt.tile_layout(W, H, r, world)[1] for r in range(world))
    max_tiles, pstride = rt.packed_layout(W, H, world, rect)
    c_ptr, p_ptr = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(c_ptr), C.c_size_t(stride * 4)) == 0
    assert hip.hipMalloc(C.byref(p_ptr), C.c_size_t(world * pstride * 4)) == 0
    try:
        shares = np.zeros_like(whole)
        for r in (1, 0, 2):
            p = gpu_ctx.make_params(W, H, *DEFAULT, tile_rank=r, tile_count=world, **kw)
            m, _, t = gpu_ctx.debug_traced_tiles(p)
            owned = np.zeros(whole.size, bool); owned[rt.tile_ids(W, H, r, world)] = True
            assert np.array_equal(m, whole & owned.reshape(whole.shape)) and t == int(m.sum())
            shares |= m
            gpu_ctx.set_compact_buffer(c_ptr.value, stride)
            gpu_ctx.render(p)
            gpu_ctx.pack_shares(c_ptr.value, stride, 1, W, H, r, world, rect, p_ptr.value + r * pstride * 4, pstride)
            gpu_ctx.synchronize()
        assert np.array_equal(shares, whole) and int(shares.sum()) == traced_all
        gpu_ctx.unpack_batch(p_ptr.value, pstride, pstride, 1, W, H, world, rect, PATH["spp"])
        assert same_bits(gpu_ctx.read_radiance(W, H), oracle(orc, bvh4, "rest", tris, W, H, *DEFAULT, orc_mod.MODE_PATH, **PATH)[0])
    finally:
        gpu_ctx.set_compact_buffer(0, 0)
        hip.hipFree(c_ptr); hip.hipFree(p_ptr)


def test_moving_geometry_takes_a_new_cover(rt, orc, gpu_ctx):
    """pt_update_triangles carries the surface into tiles the cover of the rest pose had dropped: the cut names places in the arena, so the
    next launch projects the refitted boxes -- a cover kept from before, or a copy of the old boxes, would leave those tiles at the miss value."""
    tris, _ = scene(gpu_ctx)
    kw = dict(mode=rt.PT_MODE_PATH, **PATH)
    p = gpu_ctx.make_params(W, H, *DEFAULT, **kw)
    old, _, _ = gpu_ctx.debug_traced_tiles(p)
    gpu_ctx.render(p)                                          # the rest pose's cover is the one in use (and kept)
    moved = wave(tris, 0.3, 3)
    gpu_ctx.update_triangles(moved)
    bvh4 = gpu_ctx.read_bvh4()
    _, ids, _ = oracle(orc, bvh4, "wave 0.3 3", moved, W, H, *DEFAULT, orc_mod.MODE_SINGLE)
    hits = hit_tiles(ids, W, H)
    print("hit tiles the rest pose's cover had dropped: %d" % int((hits & ~old).sum()))
    assert (hits & ~old).any()                                 # the displacement does what this test is about
    want = oracle(orc, bvh4, "wave 0.3 3", moved, W, H, *DEFAULT, orc_mod.MODE_PATH, **PATH)[0]
    for launch in range(3):                                    # the first launch after the update keeps the rectangle, the second takes the new cover
        gpu_ctx.render(p)
        assert same_bits(gpu_ctx.read_radiance(), want), launch
    new, _, _ = gpu_ctx.debug_traced_tiles(p)
    assert not (hits & ~new).any() and (new & ~old).any()
    gpu_ctx.render(p)
    assert same_bits(gpu_ctx.read_radiance(), oracle(orc, bvh4, "wave 0.3 3", moved, W, H, *DEFAULT, orc_mod.MODE_PATH, **PATH)[0])
    gpu_ctx.render(gpu_ctx.make_params(W, H, *DEFAULT, mode=rt.PT_MODE_REFERENCE))
    assert same_bits(gpu_ctx.read_radiance(), oracle(orc, bvh4, "wave 0.3 3", moved, W, H, *DEFAULT, orc_mod.MODE_SINGLE)[0])


def test_nothing_left_to_trace(rt, orc, gpu_ctx):
    """The root box's rectangle reaches into the frame, no box of the cut does: nothing is traced, the frame is the miss frame."""
    tris, bvh4 = scene(gpu_ctx)
    cam, quat = (0, 0, 4.0), quat_yaw_pitch(1.14, 0.4)
    p = gpu_ctx.make_params(W, H, cam, quat, mode=rt.PT_MODE_PATH, **PATH)
    mask, rect_tiles, traced = gpu_ctx.debug_traced_tiles(p)
    assert rect_tiles > 0 and traced == 0 and not mask.any()
    gpu_ctx.render(p)
    got = gpu_ctx.read_radiance().copy()
    _, ids, _ = oracle(orc, bvh4, "rest", tris, W, H, cam, quat, orc_mod.MODE_SINGLE)
    assert not (ids != 0xFFFFFFFF).any()
    assert same_bits(got, oracle(orc, bvh4, "rest", tris, W, H, cam, quat, orc_mod.MODE_PATH, **PATH)[0])
    assert (got.reshape(-1, 4) == got[0, 0]).all()
    gpu_ctx.render(gpu_ctx.make_params(W, H, *DEFAULT, mode=rt.PT_MODE_PATH, **PATH))          # and the slot goes on to an ordinary launch
    assert same_bits(gpu_ctx.read_radiance(), oracle(orc, bvh4, "rest", tris, W, H, *DEFAULT, orc_mod.MODE_PATH, **PATH)[0])
