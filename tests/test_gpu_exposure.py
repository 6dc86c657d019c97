"""Exposed triangles on the GPU: the device's mask against the float64 reference of tests/exposeref.py (validated on the
CPU by tests/test_exposure_reference.py), and frames with and without the skipped shadow rays against each other, the one-pixel-per-lane kernel
and the oracle, bit for bit."""
import ctypes as C
import importlib

import numpy as np
import pytest

import exposeref
import exposure_cases as xc
import orc as orc_mod
from scenes import comb_bvh4, random_soup, spoil_bvh4

pytestmark = pytest.mark.gpu
SLACK = 1e-11
W, H = 128, 72


@pytest.fixture(scope="module")
def rt():
    return importlib.import_module("raytracer-public_amd")


@pytest.fixture(scope="module")
def orc():
    return orc_mod.load()


def make(rt, tris, bvh4=None):
    ctx = rt.Context(0)
    ctx.set_triangles(np.ascontiguousarray(tris, np.float32).reshape(-1))
    if bvh4 is None:
        ctx.build_bvh()
    else:
        ctx.set_bvh4(bvh4)
    return ctx


def params(rt, ctx, w=W, h=H, spp=4, bounces=5, **kw):
    kw.setdefault("cam_pos", (0.3, 0.2, 2.5))
    return ctx.make_params(w, h, mode=rt.PT_MODE_PATH, spp=spp, max_bounces=bounces, seed=7, **kw)


def bits(img):
    return np.ascontiguousarray(img).view(np.uint32)


def band(tris, info):
    return (exposeref.flags(tris, info["s_max"], info["d_max"], slack=SLACK), exposeref.flags(tris, info["s_max"], info["d_max"], slack=-SLACK))


def oracle_frame(orc, tris, bvh4, w=W, h=H, spp=4, bounces=5, frame=0, cam=(0.3, 0.2, 2.5)):
    flat = np.ascontiguousarray(tris, np.float32).reshape(-1)
    p = orc.make_params(w, h, flat.size // 9, cam_pos=cam, mode=orc_mod.MODE_PATH, spp=spp, max_bounces=bounces, seed=7, frame=frame)
    img, _, st = orc.render(p, flat, bvh4)
    return img, st


@pytest.mark.parametrize("name", sorted(xc.SCENES))
def test_device_mask_lies_in_the_band(rt, name):
    tris = xc.scene(name)
    ctx = make(rt, tris)
    info = ctx.debug_exposure(params(rt, ctx))
    inner, outer = band(tris, info)
    m = info["mask"][: len(tris)]
    print(name, "flagged", info["flagged"], "gave up", info["gave_up"], "listed", info["listed"], "inner", int(inner.sum()), "outer", int(outer.sum()), "ms", info["kernel_ms"])
    assert info["valid"] and info["gave_up"] == 0 and info["flagged"] == int(m.sum())
    assert not (inner & ~m).any() and not (m & ~outer).any()
    assert not info["mask"][len(tris):].any()
    ctx.close()


def test_mask_on_a_comb_after_an_update_and_on_a_spoiled_tree(rt, orc):
    # a pt_set_bvh4 comb of 30 levels: every triangle reachable, the full band
    ctris, cb = comb_bvh4(30, 3, all_hit=False)
    ctx = make(rt, ctris, cb)
    info = ctx.debug_exposure(params(rt, ctx))
    inner, outer = band(ctris.reshape(-1, 3, 3), info)
    m = info["mask"][: ctris.size // 9]
    assert info["gave_up"] == 0 and not (inner & ~m).any() and not (m & ~outer).any()
    ctx.close()
    # after pt_update_triangles (the torus, waved): the mask of the refitted tree
    tris = np.array(xc.scene("torus"))
    ctx = make(rt, tris)
    ctx.debug_exposure(params(rt, ctx))
    moved = tris.copy(); moved[..., 2] += (0.05 * np.sin(4.0 * moved[..., 0])).astype(np.float32)
    ctx.update_triangles(moved.reshape(-1))
    assert not ctx.debug_exposure(None, want_mask=False)["valid"]
    info = ctx.debug_exposure(params(rt, ctx))
    inner, outer = band(moved, info)
    m = info["mask"][: len(moved)]
    assert info["valid"] and info["gave_up"] == 0 and not (inner & ~m).any() and not (m & ~outer).any()
    ctx.close()
    # a spoiled tree hides triangles from the traversal and from the walk alike: the mask holds at least the inner reference, and the frame is the oracle's
    soup = random_soup(2000, 5)
    _, b4 = orc.build_bvh4(soup)
    sp, _, _ = spoil_bvh4(b4, 2)
    ctx = make(rt, soup, sp)
    p = params(rt, ctx)
    info = ctx.debug_exposure(p)
    inner, _ = band(soup.reshape(-1, 3, 3), info)
    assert not (inner & ~info["mask"][: soup.size // 9]).any()
    ctx.render(p); img = ctx.read_radiance()
    ref, _ = oracle_frame(orc, soup, sp)
    assert np.array_equal(bits(img), bits(ref))
    ctx.close()


@pytest.mark.parametrize("quad,fork", [(16, 2), (5, 2), (1, 2), (16, 0), (5, 0)])
def test_frames_are_bit_identical(rt, orc, quad, fork):
    tris = xc.scene("torus")
    ctx = make(rt, tris)
    bvh4 = ctx.read_bvh4()
    ctx.debug_set_tune("QUAD", quad); ctx.debug_set_tune("FORK", fork)
    p = params(rt, ctx)
    ctx.debug_set_tune("EXPOSE", 0)
    ctx.render(p); off = ctx.read_radiance().copy()
    ctx.debug_set_tune("EXPOSE", None)
    assert ctx.debug_exposure(p, want_mask=False)["flagged"] > 0
    ctx.render(p); on = ctx.read_radiance().copy()
    assert ctx.debug_exposure(None, want_mask=False)["used"]                 # the production launch did read the mask ...
    ctx.debug_set_tune("EXPOSE", 0); ctx.render(p); ctx.synchronize()
    assert not ctx.debug_exposure(None, want_mask=False)["used"]             # ... and with the knob at 0 it does not
    ctx.debug_set_tune("EXPOSE", None)
    ctx.render(params(rt, ctx, simple_kernel=True)); simple = ctx.read_radiance().copy()
    ref, _ = oracle_frame(orc, tris, bvh4)
    assert np.array_equal(bits(off), bits(on)) and np.array_equal(bits(on), bits(simple)) and np.array_equal(bits(on), bits(ref))
    ctx.close()


def test_accumulation_batch_of_cameras_and_tile_shares(rt, orc):
    tris = xc.scene("plates")
    ctx = make(rt, tris)
    bvh4 = ctx.read_bvh4()
    ctx.debug_exposure(params(rt, ctx))
    hip = C.CDLL("libamdhip64.so")
    out = {}
    for knob in (0, None):
        ctx.debug_set_tune("EXPOSE", knob)
        for f in range(4):                                                   # four accumulated frames
            ctx.render(params(rt, ctx, frame=f, accumulate=True))
        acc = ctx.read_radiance().copy()
        ctx.set_batch(3)                                                     # three cameras in one launch
        cams = [(0.3, 0.2, 2.5), (-0.5, 0.4, 2.2), (0.1, -0.6, 2.8)]
        for c in cams:
            ctx.render(params(rt, ctx, cam_pos=c))
        ctx.flush(); last = ctx.read_radiance().copy()
        ctx.set_batch(1)
        shares = []
        for r in range(2):                                                   # two tile shares
            ctx.render(params(rt, ctx, tile_rank=r, tile_count=2))
            ptr, floats = ctx.compact_radiance(); ctx.synchronize()
            host = np.zeros(floats, np.float32)
            assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(floats * 4), 2) == 0
            shares.append(host)
        out[knob] = (acc, last, shares)
    assert np.array_equal(bits(out[0][0]), bits(out[None][0]))
    assert np.array_equal(bits(out[0][1]), bits(out[None][1]))
    for a, b in zip(out[0][2], out[None][2]):
        assert np.array_equal(bits(a), bits(b))
    ref, _ = oracle_frame(orc, tris, bvh4, cam=(0.1, -0.6, 2.8))
    assert np.array_equal(bits(out[None][1]), bits(ref))
    ctx.close()


def test_counters_and_the_skipped_count(rt, orc):
    tris = xc.scene("torus")
    ctx = make(rt, tris)
    bvh4 = ctx.read_bvh4()
    p = params(rt, ctx, stats=True)
    ctx.debug_exposure(p)
    ref, st = oracle_frame(orc, tris, bvh4)
    ctx.render(p); img = ctx.read_radiance().copy(); s1 = ctx.stats()       # EXPOSE 1: an instrumented launch traces every shadow ray
    assert np.array_equal(bits(img), bits(ref))
    for k in ("rays_closest", "rays_shadow", "nodes_examined", "tris_tested", "stack_drops", "max_stack", "samples"):
        assert s1[k] == st[k], k
    assert not ctx.debug_exposure(None, want_mask=False)["used"]
    ctx.debug_set_tune("EXPOSE", 2)
    ctx.render(p); img2 = ctx.read_radiance().copy(); s2 = ctx.stats()
    skipped = ctx.debug_exposure(None, want_mask=False)["skipped"]
    print("shadow rays", s1["rays_shadow"], "skipped", skipped)
    assert np.array_equal(bits(img2), bits(ref))
    assert skipped > 0 and s2["rays_shadow"] == s1["rays_shadow"] - skipped
    # a camera beyond the distance the mask was computed for: nothing is skipped
    far = params(rt, ctx, stats=True, cam_pos=(0.3, 0.2, 3.6))
    ctx.render(far); img3 = ctx.read_radiance().copy()
    far_info = ctx.debug_exposure(None, want_mask=False)
    assert far_info["skipped"] == 0 and not far_info["used"]
    ref3, _ = oracle_frame(orc, tris, bvh4, cam=(0.3, 0.2, 3.6))
    assert np.array_equal(bits(img3), bits(ref3))
    ctx.close()


def test_a_refit_voids_the_mask_and_a_budget_leaves_triangles_unflagged(rt, orc):
    tris = np.array(xc.scene("plates"))
    ctx = make(rt, tris)
    bvh4_before = ctx.read_bvh4()
    p = params(rt, ctx, stats=True)
    ctx.debug_set_tune("EXPOSE", 2)
    before = ctx.debug_exposure(p)["mask"][: len(tris)]
    moved = tris.copy(); moved[128:, :, :2] += np.float32(0.8)               # the upper plate slides over a part of the lower one that was flagged
    ctx.update_triangles(moved.reshape(-1))
    ctx.render(p); img = ctx.read_radiance().copy()
    info = ctx.debug_exposure(None, want_mask=False)
    assert not info["valid"] and info["skipped"] == 0                        # the first launch after the update skips nothing
    ref, _ = oracle_frame(orc, moved, ctx.read_bvh4())
    assert np.array_equal(bits(img), bits(ref))
    after = ctx.debug_exposure(p)["mask"][: len(tris)]
    assert (before[:128] & ~after[:128]).any()                               # triangles of the lower plate lost their flag
    ctx.render(p); img = ctx.read_radiance().copy()
    assert ctx.debug_exposure(None, want_mask=False)["skipped"] > 0 and np.array_equal(bits(img), bits(ref))
    # no budget: every query that reaches a leaf gives up, and its triangle stays unflagged
    ctx.debug_set_tune("EXBUDGET", 0)
    info = ctx.debug_exposure(p)
    assert info["gave_up"] > 0 and info["flagged"] == 0 and not info["mask"].any()
    assert bvh4_before[0] == ctx.read_bvh4()[0]
    ctx.close()


def test_the_mask_is_taken_by_the_first_large_launch_and_after_an_update_by_the_second(rt):
    tris = np.array(xc.scene("torus"))
    ctx = make(rt, tris)
    small, large = params(rt, ctx), params(rt, ctx, w=512, h=512, spp=8, bounces=7)      # 2^24 ray segments
    ctx.render(small); ctx.synchronize()
    assert not ctx.debug_exposure(None, want_mask=False)["valid"]
    ctx.render(large); img1 = ctx.read_radiance().copy()
    assert ctx.debug_exposure(None, want_mask=False)["valid"]
    ctx.debug_set_tune("EXPOSE", 0)
    ctx.render(large); img0 = ctx.read_radiance().copy()
    ctx.debug_set_tune("EXPOSE", None)
    assert np.array_equal(bits(img0), bits(img1))
    # a large launch from beyond the camera distance the mask holds for takes the mask again, for the wider bounds
    near = ctx.debug_exposure(None, want_mask=False)
    far = params(rt, ctx, w=512, h=512, spp=8, bounces=7, cam_pos=(0.3, 0.2, 6.0))
    ctx.render(far); ctx.synchronize()
    wide = ctx.debug_exposure(None, want_mask=False)
    assert near["cam_max"] < 6.0 <= wide["cam_max"] and wide["used"] and wide["valid"]
    ctx.update_triangles((tris * np.float32(1.01)).reshape(-1))
    ctx.render(large); ctx.synchronize()
    assert not ctx.debug_exposure(None, want_mask=False)["valid"]
    ctx.render(large); ctx.synchronize()
    assert ctx.debug_exposure(None, want_mask=False)["valid"]
    ctx.close()


def test_a_recompute_for_a_farther_camera_is_waited_for_by_the_next_launch_on_another_slot(rt):
    """A large production launch from beyond the mask's camera distance takes the mask again on its own side stream; the launch submitted
    right behind it, with no host wait, runs on another frame slot and has to wait for that pass (the tree version is the same: the slots
    compare the mask's generation).  Both frames equal the ones traced with every shadow ray."""
    tris = np.array(xc.scene("torus"))
    near = dict(w=512, h=512, spp=8, bounces=7)
    far = dict(w=512, h=512, spp=8, bounces=7, cam_pos=(0.3, 0.2, 6.0))
    ref = {}
    ctx = make(rt, tris)
    ctx.debug_set_tune("EXPOSE", 0)
    for f in (1, 2):
        ctx.render(params(rt, ctx, frame=f, **far)); ref[f] = ctx.read_radiance().copy()
    ctx.close()
    for last in (1, 2):                                  # read the recomputing launch's own frame, then the one behind it
        ctx = make(rt, tris)
        ctx.render(params(rt, ctx, **near)); ctx.synchronize()
        before = ctx.debug_exposure(None, want_mask=False)
        assert before["valid"] and before["cam_max"] < 6.0
        for f in range(1, last + 1):
            ctx.render(params(rt, ctx, frame=f, **far))          # no synchronize in between
        img = ctx.read_radiance().copy()
        after = ctx.debug_exposure(None, want_mask=False)
        assert after["cam_max"] >= 6.0 and after["used"] and after["flagged"] > 0
        assert np.array_equal(bits(img), bits(ref[last]))
        ctx.close()

