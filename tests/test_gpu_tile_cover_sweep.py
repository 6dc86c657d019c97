"""The tile cover (pt_cover.hip, tile_cover / traced_tiles / stage_traced_tiles in pt_api.cpp) pinned to
tests/coverref.py, the float64 restatement that tests/test_cover_reference.py validates against the oracle.

Part one states what the mask of a launch IS: for every tree that binds another rule of the cut and 150 seeded cameras each -- roll,
three resolutions, focal and aspect off their defaults, a near shell where the cover has to be given up -- inner <= mask <= outer, where
the two differ only on a tile seam within 1e-6 px of a box edge.  Part two drives what decides WHICH mask a launch gets: the four-entry
cover cache, the per-slot staging key, the rectangle -> cover transition inside an accumulation, batches beyond one group of cameras,
the launches large enough to take a cover at first sight.  There the expected frame is always the one-pixel-per-lane kernel's frame of
the same params (PT_FLAG_SIMPLE_KERNEL), which no launch planning touches: a tile dropped wrongly shows as miss-valued pixels."""
import ctypes as C

import numpy as np
import pytest

import coverref
import orc as orc_mod
from refit_cases import host_trees, wave
from scenes import INVALID, LEAF, comb_bvh4, pack_box, random_soup, spoil_bvh4

pytestmark = pytest.mark.gpu

RES = [(200, 120), (250, 141), (64, 40)]
CAMERAS = 150
TREES = ["soup300", "soup6000-level0", "soup6000-level1", "soup6000-level2", "soup6000-wave", "comb90", "bvh4-wide", "spoiled"]
PATH = dict(spp=2, max_bounces=2, seed=7)
LW, LH = 128, 80                       # the launch-path tests


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def clone(p, **fields):
    q = type(p).from_buffer_copy(p)
    for k, v in fields.items():
        setattr(q, k, v)
    return q


def simple_frame(rt, ctx, p):
    """The frame of these params by the one-pixel-per-lane kernel: no tile list, no rectangle, no cover."""
    ctx.render(clone(p, flags=p.flags | rt.PT_FLAG_SIMPLE_KERNEL, tile_rank=0, tile_count=1, accumulate=0))
    return ctx.read_radiance(p.width, p.height).copy()


def install(rt, ctx, name):
    """-> the triangles the context holds."""
    if name == "comb90":
        tris, b = comb_bvh4(90, 2, all_hit=False)
        ctx.set_triangles(tris); ctx.set_bvh4(b)
        return tris
    tris = random_soup(300 if name == "soup300" else 6000, 3)
    ctx.set_triangles(tris)
    ctx.build_bvh(int(name[-1]) if name.startswith("soup6000-level") else 0)
    if name == "soup6000-wave":
        tris = wave(tris, 0.3, 3)
        ctx.update_triangles(tris)
    elif name == "bvh4-wide":
        ctx.set_bvh4(rt.bvh2_to_bvh4_wide(ctx.read_bvh2()))
    elif name == "spoiled":
        ctx.set_bvh4(spoil_bvh4(ctx.read_bvh4(), 5)[0])
    return tris


def all_tiles(p):
    tx, ty = coverref._tiles(p)
    return np.ones((ty, tx), bool)


def judge_mask(ctx, bvh4, p, owned=None):
    """debug_traced_tiles(p) against the reference.  -> (band, state): does inner differ from outer; "cover", "rectangle" or "all"."""
    mask, rect_tiles, traced = ctx.debug_traced_tiles(p)
    own = all_tiles(p) if owned is None else owned
    assert traced == int(mask.sum())
    r_in, r_out = coverref.root_rect(bvh4, p, coverref.MARGIN - coverref.BAND), coverref.root_rect(bvh4, p, coverref.MARGIN + coverref.BAND)
    if r_in is None:                                   # the root box has no rectangle: every tile
        assert np.array_equal(mask, own) and rect_tiles == traced == int(own.sum())
        return False, "all"
    if np.array_equal(r_in, r_out):
        assert rect_tiles == int((r_in & own).sum())
    inner, outer = coverref.expected(bvh4, p)
    if inner is None:                                  # no cover: the rectangle
        assert not (r_in & own & ~mask).any() and not (mask & ~(r_out & own)).any() and traced == rect_tiles
        return False, "rectangle"
    assert not (inner & own & ~mask).any(), "tiles of the reference's cover that the launch leaves out: %s" % np.argwhere(inner & own & ~mask)[:8].tolist()
    assert not (mask & ~(outer & own)).any(), "tiles the launch traces beyond the reference's cover: %s" % np.argwhere(mask & ~(outer & own))[:8].tolist()
    return not np.array_equal(inner, outer), "cover"


def lit_tiles(img, miss, p):
    return coverref.hit_tiles((img != miss).any(-1), p.width, p.height)


@pytest.mark.parametrize("name", TREES)
def test_mask_is_the_reference_cover(rt, gpu_ctx, name):
    ctx = gpu_ctx
    install(rt, ctx, name)
    bvh4 = ctx.read_bvh4()
    cams = coverref.cameras(np.random.default_rng(2000 + TREES.index(name)), CAMERAS, coverref.extent_of(bvh4))
    rng = np.random.default_rng(77)
    miss = simple_frame(rt, ctx, ctx.make_params(16, 8, (0, 0, 50), (0, 1, 0, 0), mode=rt.PT_MODE_REFERENCE))[0, 0]      # looks away from the scene
    count = dict(cover=0, rectangle=0, all=0, band=0, frames=0, proper=0)
    for i, (pos, quat) in enumerate(cams):
        w, h = RES[i % 3]
        p = ctx.make_params(w, h, pos, quat, mode=rt.PT_MODE_PATH, **PATH)
        if i % 10 == 2:                                # a lens of its own, and the aspect of another frame
            p.focal = float(np.float32(p.focal * rng.uniform(0.5, 2.0)))
            p.aspect = float(rt.focal_aspect(*RES[(i + 1) % 3])[1])
        p1 = clone(p, mode=rt.PT_MODE_REFERENCE)
        if i % 6 == 0:
            # three launches of a view nobody has seen: the rectangle, the cover computed, the cover found; then mode 1 with the same cover
            want2, want1 = simple_frame(rt, ctx, p), simple_frame(rt, ctx, p1)
            for launch in range(3):
                ctx.render(p)
                assert same_bits(ctx.read_radiance(), want2), (i, launch)
            ctx.render(p1)
            assert same_bits(ctx.read_radiance(), want1), i
            count["frames"] += 1
        if name == "spoiled":
            # children beyond the node count become slots of the device's tree in a way the words do not show: hits <= mask <= rectangle
            mask, rect_tiles, traced = ctx.debug_traced_tiles(p)
            hits = lit_tiles(simple_frame(rt, ctx, p1), miss, p)
            r = ctx.traced_tile_rect(p)
            inside = np.zeros_like(mask); inside[r[1]:r[3], r[0]:r[2]] = True
            assert not (hits & ~mask).any() and not (mask & ~inside).any() and traced == int(mask.sum()) and rect_tiles == int(inside.sum())
            count["cover" if traced < rect_tiles else "rectangle"] += 1
            count["proper"] += traced < rect_tiles
            continue
        band, state = judge_mask(ctx, bvh4, p)
        count[state] += 1; count["band"] += band
        if state == "cover":
            count["proper"] += int(coverref.cover(bvh4, p).sum()) < int(coverref.root_rect(bvh4, p).sum())
    print("%s: %d cameras: cover %d (smaller than the rectangle %d), rectangle kept %d, every tile %d; inner != outer on %d; frames compared on %d" % (
        name, len(cams), count["cover"], count["proper"], count["rectangle"], count["all"], count["band"], count["frames"]))
    assert 2 * count["proper"] >= len(cams) and count["band"] * 100 <= len(cams)
    if name != "spoiled":
        assert count["all"] > 0


def test_a_cut_box_beside_the_eye_keeps_the_rectangle(rt, gpu_ctx):
    """A hand-made tree whose root box has a rectangle while a box of the cut reaches behind the eye (its triangle sticks out of the root
    box: a tree as set_bvh4 takes it): no cover, the rectangle, frames as the plain kernel's."""
    ctx = gpu_ctx
    tris = np.array([-0.4, -0.4, 0, 0.4, -0.4, 0, 0, 0.4, 0,   -0.3, -0.2, -0.3, 0.3, -0.2, 6.0, 0, 0.3, 0.1], np.float32)
    recs = [pack_box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)) + [1, 2, INVALID, INVALID, 0],
            pack_box((-0.4, -0.4, -0.01), (0.4, 0.4, 0.01)) + [INVALID] * 4 + [LEAF | 0],
            pack_box((-0.3, -0.2, -0.3), (0.3, 0.3, 6.0)) + [INVALID] * 4 + [LEAF | 1]]
    ctx.set_triangles(tris); ctx.set_bvh4(np.array([3] + [w for r in recs for w in r], np.uint32))
    bvh4 = ctx.read_bvh4()
    p = ctx.make_params(LW, LH, (0.1, 0.05, 2.5), (0, 0, 0, 1), mode=rt.PT_MODE_PATH, **PATH)
    assert coverref.root_rect(bvh4, p) is not None and not coverref.root_rect(bvh4, p).all() and coverref.cover(bvh4, p) is None
    want = simple_frame(rt, ctx, p)
    for launch in range(3):
        ctx.render(p)
        assert same_bits(ctx.read_radiance(), want), launch
    assert judge_mask(ctx, bvh4, p) == (False, "rectangle")


# ---- the launch path ------------------------------------------------------------------------------------------------------------------
def soup(ctx, n=6000, seed=3):
    tris = random_soup(n, seed)
    ctx.set_triangles(tris); ctx.build_bvh()
    return tris


def covered_views(ctx, bvh4, n, w=LW, h=LH, draw=31, **kw):
    """n views of the generator whose cover exists and leaves out part of the rectangle: the ones where a wrong mask shows."""
    out = []
    for pos, quat in coverref.cameras(np.random.default_rng(draw), 8 * n, coverref.extent_of(bvh4)):
        p = ctx.make_params(w, h, pos, quat, **kw)
        c = coverref.cover(bvh4, p)
        if c is not None and c.any() and int(c.sum()) < int(coverref.root_rect(bvh4, p).sum()):
            out.append(p)
        if len(out) == n:
            return out
    raise AssertionError("the generator gave too few covered views")


def test_six_views_through_a_cache_of_four(rt, gpu_ctx):
    """Six views in rotation, three rounds: the cache holds four, so each view is evicted before it returns.  Then every view twice in
    a row (noted, computed) while the others push it out again.  Every frame is right; afterwards every view's mask is the reference's."""
    ctx = gpu_ctx
    soup(ctx)
    bvh4 = ctx.read_bvh4()
    views = covered_views(ctx, bvh4, 6, mode=rt.PT_MODE_PATH, **PATH)
    want = [simple_frame(rt, ctx, p) for p in views]
    for rnd in range(3):
        for k, p in enumerate(views):
            ctx.render(p)
            assert same_bits(ctx.read_radiance(), want[k]), (rnd, k)
    for rnd in range(2):
        for k, p in enumerate(views):
            for again in range(2):
                ctx.render(p)
                assert same_bits(ctx.read_radiance(), want[k]), (rnd, k, again)
    for p in views:
        assert judge_mask(ctx, bvh4, p)[1] == "cover"
    for k, p in enumerate(views):                      # and with every cover computed and four of them kept
        ctx.render(p)
        assert same_bits(ctx.read_radiance(), want[k]), k


def render_shares(rt, ctx, p, world):
    """The frame as `world` tile shares through one gathered compact buffer and deinterleave."""
    hip = C.CDLL("libamdhip64.so")
    stride = max(rt.tile_layout(p.width, p.height, r, world)[1] for r in range(world))
    g = C.c_void_p()
    assert hip.hipMalloc(C.byref(g), C.c_size_t(stride * 4 * world)) == 0
    try:
        for r in range(world):
            ctx.set_compact_buffer(g.value + r * stride * 4, stride)
            ctx.render(clone(p, tile_rank=r, tile_count=world))
        ctx.synchronize()
        ctx.set_compact_buffer(0, 0)
        ctx.deinterleave(g.value, stride, p.width, p.height, world)
        return ctx.read_radiance(p.width, p.height).copy()
    finally:
        ctx.set_compact_buffer(0, 0)
        hip.hipFree(g)


def test_one_change_at_a_time(rt, orc, gpu_ctx):
    """One camera; the resolution, the focal length, the aspect ratio, the tile share, the tree and the triangles change one at a time.
    After each change three launches (rectangle, cover computed, cover found -- none of them with anything kept from before the change):
    every frame is the plain kernel's, and the mask is the reference's for the new state."""
    ctx = gpu_ctx
    tris = soup(ctx)
    base = covered_views(ctx, ctx.read_bvh4(), 1, mode=rt.PT_MODE_PATH, **PATH)[0]
    pos, quat = tuple(base.cam_pos), tuple(base.cam_quat)

    def params(w=LW, h=LH, focal=None, aspect=None):
        p = ctx.make_params(w, h, pos, quat, mode=rt.PT_MODE_PATH, **PATH)
        if focal: p.focal = float(np.float32(p.focal * focal))
        if aspect: p.aspect = float(np.float32(aspect))
        return p

    def three(p, what, world=1):
        bvh4 = ctx.read_bvh4()
        want = simple_frame(rt, ctx, p)
        for launch in range(3):
            if world == 1:
                ctx.render(p); got = ctx.read_radiance()
            else:
                got = render_shares(rt, ctx, p, world)
            assert same_bits(got, want), (what, launch)
        for r in range(world):
            owned = None
            if world > 1:
                owned = np.zeros(all_tiles(p).size, bool); owned[rt.tile_ids(p.width, p.height, r, world)] = True
                owned = owned.reshape(all_tiles(p).shape)
            assert judge_mask(ctx, bvh4, clone(p, tile_rank=r, tile_count=world), owned)[1] == "cover", what

    three(params(), "start")
    three(params(136, 88), "resolution")
    three(params(), "resolution back")
    three(params(focal=1.3), "focal")
    three(params(), "focal back")
    three(params(aspect=1.25), "aspect")
    three(params(), "aspect back")
    three(params(), "three tile shares", world=3)
    three(params(), "whole frames again")
    ctx.set_bvh4(host_trees(rt, orc, tris, rt.PT_ACCEL_PLOC)[1])
    three(params(), "the level-2 tree of the same triangles")
    ctx.set_triangles(random_soup(6000, 11)); ctx.build_bvh()
    three(params(), "another soup of the same size")


def test_accumulation_across_the_transition(rt, orc, gpu_ctx):
    """Frames 0..3 of one accumulation of a view nobody has seen: frame 0 traces the rectangle, frame 1 computes the cover, the later ones
    find it.  After each frame the radiance is the oracle's accumulation of f + 1 frames, bit for bit."""
    ctx = gpu_ctx
    tris = soup(ctx)
    bvh4 = ctx.read_bvh4()
    p = covered_views(ctx, bvh4, 1, draw=32, mode=rt.PT_MODE_PATH, accumulate=True, **PATH)[0]
    for f in range(4):
        ctx.render(clone(p, frame=f))
        got = ctx.read_radiance().copy()
        want, _ = orc.render_mt(orc.make_params(LW, LH, tris.size // 9, tuple(p.cam_pos), tuple(p.cam_quat), mode=orc_mod.MODE_PATH, frame=0, accum_frames=f + 1, **PATH), tris, bvh4)
        assert same_bits(got, want), f
        assert ctx.accum_info().samples == (f + 1) * PATH["spp"]
    assert judge_mask(ctx, bvh4, clone(p, accumulate=0))[1] == "cover"


def test_twenty_cameras_in_one_launch(rt, gpu_ctx):
    """set_batch(20) with 20 distinct cameras: two groups of kCoverCams = 16 for the cover kernel, one union.  Three times over (rectangle,
    cover computed, cover found), each frame the plain kernel's; then 20 frames of two alternating cameras (one group of two)."""
    ctx = gpu_ctx
    soup(ctx)
    bvh4 = ctx.read_bvh4()
    views = covered_views(ctx, bvh4, 20, draw=33, mode=rt.PT_MODE_PATH, **PATH)
    want = [simple_frame(rt, ctx, p) for p in views]
    hip = C.CDLL("libamdhip64.so")
    floats = LW * LH * 4
    bufs = []

    def batch(order, what):
        for attempt in range(3):
            for slot, k in enumerate(order):
                ctx.set_output_buffer(bufs[slot].value, floats)
                ctx.render(views[k])
            ctx.synchronize()
            for slot, k in enumerate(order):
                host = np.zeros((LH, LW, 4), np.float32)
                assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), bufs[slot], C.c_size_t(floats * 4), 2) == 0
                assert same_bits(host, want[k]), (what, attempt, slot)
                assert hip.hipMemset(bufs[slot], 0, C.c_size_t(floats * 4)) == 0
            assert hip.hipDeviceSynchronize() == 0

    try:
        for _ in range(20):
            b = C.c_void_p(); assert hip.hipMalloc(C.byref(b), C.c_size_t(floats * 4)) == 0; bufs.append(b)
        ctx.set_batch(20)
        batch(list(range(20)), "twenty cameras")
        batch([3 + (i & 1) * 9 for i in range(20)], "two alternating cameras")
    finally:
        ctx.set_output_buffer(0, 0); ctx.set_batch(1)
        for b in bufs: hip.hipFree(b)


def test_first_sight_at_two_to_the_24_segments(rt, gpu_ctx):
    """512 x 256 x 8 spp x (15 + 1) bounces = 2^24 ray segments: the launch takes a new view's cover at once, and its first frame is
    right.  One bounce fewer stays below: noted, computed, found -- right on launches 1, 2 and 3."""
    ctx = gpu_ctx
    soup(ctx, 300)
    bvh4 = ctx.read_bvh4()
    w, h = 512, 256
    big, small = covered_views(ctx, bvh4, 2, w=w, h=h, draw=34, mode=rt.PT_MODE_PATH, spp=8, max_bounces=15)
    assert (w // 8) * (h // 8) * 64 * 8 * 16 == 1 << 24
    want = simple_frame(rt, ctx, big)
    ctx.render(big)
    assert same_bits(ctx.read_radiance(), want)
    small = clone(small, max_bounces=14)
    want = simple_frame(rt, ctx, small)
    for launch in range(3):
        ctx.render(small)
        assert same_bits(ctx.read_radiance(), want), launch
    for p in (big, small):
        assert judge_mask(ctx, bvh4, p)[1] == "cover"
