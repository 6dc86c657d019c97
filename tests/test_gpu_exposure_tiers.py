"""The two exposure tiers on the GPU: one pass computes a mask for hits at |n . d| >= 0.1002 (the first tier, what
tests/test_gpu_exposure.py pins) and one for hits at |n . d| >= 0.3008 (the second: a third of the in-plane margin, a superset).  Both masks
against the float64 reference at their gates, the first tier unchanged by the second, and frames, counters and ordering with both tiers in
use against the first tier alone (knob EXPOSE + 4), every shadow ray traced (EXPOSE 0), the one-pixel-per-lane kernel and the oracle, bit for
bit.  The bumpy plate of tests/exposure_tier_cases.py is the scene on which the tiers differ by a quarter of the triangles."""
import importlib

import numpy as np
import pytest

import exposure_tier_cases as tc
import orc as orc_mod
from scenes import comb_bvh4

pytestmark = pytest.mark.gpu
W, H = 96, 64
CAM = (0.3, 0.2, 2.5)
# a camera low over the plate, aimed at its centre: primary hits at |n . d| around 0.2, between the two gates
LOW = (0.6, 0.0, 0.12)
_yaw = np.arctan2(LOW[0], LOW[2])            # the camera looks along -z: a yaw about y turns that to (-sin, 0, -cos)
LOW_QUAT = (0.0, float(np.sin(_yaw / 2)), 0.0, float(np.cos(_yaw / 2)))
VIEWS = {"torus": ("torus", CAM, (0, 0, 0, 1)), "plate": ("bumpy_plate", CAM, (0, 0, 0, 1)), "plate_low": ("bumpy_plate", LOW, LOW_QUAT)}


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


def params(rt, ctx, w=W, h=H, spp=4, bounces=5, cam=CAM, quat=(0, 0, 0, 1), **kw):
    return ctx.make_params(w, h, cam, quat, mode=rt.PT_MODE_PATH, spp=spp, max_bounces=bounces, seed=7, **kw)


def bits(img):
    return np.ascontiguousarray(img).view(np.uint32)


_oracle = {}


def oracle_frame(orc, key, tris, bvh4, w=W, h=H, spp=4, bounces=5, frame=0, cam=CAM, quat=(0, 0, 0, 1)):
    """(radiance, counters) of the oracle, computed once per view (the device's tree of a scene is the same in every test: same triangles, same build)"""
    at = (key, w, h, spp, bounces, frame, tuple(cam), tuple(quat))
    if at not in _oracle:
        flat = np.ascontiguousarray(tris, np.float32).reshape(-1)
        p = orc.make_params(w, h, flat.size // 9, cam_pos=cam, cam_quat=quat, mode=orc_mod.MODE_PATH, spp=spp, max_bounces=bounces, seed=7, frame=frame)
        img, _, st = orc.render(p, flat, bvh4)
        _oracle[at] = (img, st)
    return _oracle[at]


def in_band(mask, inner, outer):
    return not (inner & ~mask).any() and not (mask & ~outer).any()


@pytest.mark.parametrize("k", (1, 2))
@pytest.mark.parametrize("name", tc.NAMES)
def test_device_masks_lie_in_their_bands(rt, name, k):
    tris = tc.scene(name)
    ctx = make(rt, tris)
    info = ctx.debug_exposure(params(rt, ctx))
    n = len(tris)
    m1, m2 = info["mask"][:n], info["mask2"][:n]
    inner, outer = tc.band(tris, k, info["s_max"], info["d_max"], key=name)
    print(name, "tier", k, "flagged", info["flagged"], info["flagged2"], "gave up", info["gave_up"], info["gave_up2"], "inner", int(inner.sum()), "outer", int(outer.sum()), "ms", info["kernel_ms"])
    assert info["valid"] and info["gave_up"] == 0 and info["gave_up2"] == 0
    assert info["flagged"] == int(m1.sum()) and info["flagged2"] == int(m2.sum())
    assert in_band(m1 if k == 1 else m2, inner, outer)
    assert not (m1 & ~m2).any()                                              # tier 1 is a subset of tier 2
    assert not info["mask"][n:].any() and not info["mask2"][n:].any()
    ctx.close()


def test_both_masks_on_a_comb(rt):
    ctris, cb = comb_bvh4(30, 3, all_hit=False)          # a pt_set_bvh4 comb of 30 levels: every triangle reachable, the full band
    ctx = make(rt, ctris, cb)
    info = ctx.debug_exposure(params(rt, ctx))
    n = ctris.size // 9
    for k, m in ((1, info["mask"][:n]), (2, info["mask2"][:n])):
        inner, outer = tc.band(ctris.reshape(-1, 3, 3), k, info["s_max"], info["d_max"])
        assert in_band(m, inner, outer), k
    assert info["gave_up"] == 0 and info["gave_up2"] == 0 and not (info["mask"] & ~info["mask2"]).any()
    ctx.close()


@pytest.mark.parametrize("k", (1, 2))
def test_both_masks_of_a_refitted_tree(rt, k):
    tris = np.array(tc.scene("torus"))
    ctx = make(rt, tris)
    ctx.debug_exposure(params(rt, ctx))
    moved = tris.copy(); moved[..., 2] += (0.05 * np.sin(4.0 * moved[..., 0])).astype(np.float32)
    ctx.update_triangles(moved.reshape(-1))
    assert not ctx.debug_exposure(None, want_mask=False)["valid"]
    info = ctx.debug_exposure(params(rt, ctx))
    inner, outer = tc.band(moved, k, info["s_max"], info["d_max"], key="torus_waved")
    m1, m2 = info["mask"][: len(moved)], info["mask2"][: len(moved)]
    assert info["valid"] and info["gave_up"] == 0 and info["gave_up2"] == 0
    assert in_band(m1 if k == 1 else m2, inner, outer) and not (m1 & ~m2).any()
    ctx.close()


@pytest.mark.parametrize("name", ("torus", "bumpy_plate"))
def test_the_first_tier_does_not_depend_on_the_knob_and_no_budget_empties_both(rt, name):
    tris = tc.scene(name)
    ctx = make(rt, tris)
    p = params(rt, ctx)
    keys = ("flagged", "gave_up", "listed", "s_max", "d_max", "cam_max")
    both = ctx.debug_exposure(p)
    ctx.debug_set_tune("EXPOSE", 5)                      # launches use the first tier only; the pass is the same one
    first = ctx.debug_exposure(p)
    assert np.array_equal(both["mask"], first["mask"]) and all(both[k] == first[k] for k in keys)
    assert np.array_equal(both["mask2"], first["mask2"]) and both["flagged2"] == first["flagged2"]
    assert both["flagged2"] > both["flagged"] > 0
    # the first tier is the host twin's at the first gate, the second the twin's at the second, up to the band (no walk gave up)
    twin1, twin2 = (rt.exposure_flags_host(tris, both["s_max"], both["d_max"], gate=g) for g in rt.EXPOSE_GATES)
    n = len(tris)
    assert (both["mask"][:n] != twin1).sum() <= 2 and (both["mask2"][:n] != twin2).sum() <= 2
    ctx.debug_set_tune("EXPOSE", None)
    ctx.debug_set_tune("EXBUDGET", 0)                    # every walk that reaches a leaf gives up: nothing is flagged in either tier
    info = ctx.debug_exposure(p)
    assert info["gave_up"] > 0 and info["flagged"] == 0 and info["flagged2"] == 0 and not info["mask"].any() and not info["mask2"].any()
    ctx.close()


def test_a_walk_that_runs_out_after_the_first_tier_is_settled_gives_up_for_the_second_only(rt):
    """EXBUDGET b: a walk may test b leaves.  A triangle that one of them blocks for tier 1 and none for tier 2 goes on and, with more leaves in
    reach, gives up for tier 2 alone: it is counted apart, tier 1's counts keep their meaning, and the triangle stays unflagged in the second tier."""
    tris = tc.scene("bumpy_plate")
    ctx = make(rt, tris)
    p = params(rt, ctx)
    full = ctx.debug_exposure(p)
    n = len(tris)
    second_only = 0
    for budget in (1, 2, 4, 8):
        ctx.debug_set_tune("EXBUDGET", budget)
        info = ctx.debug_exposure(p)
        print("EXBUDGET", budget, "gave up", info["gave_up"], info["gave_up2"], "flagged", info["flagged"], info["flagged2"])
        assert info["gave_up"] + info["gave_up2"] <= n
        assert not (info["mask"] & ~info["mask2"]).any()
        assert not (info["mask"] & ~full["mask"]).any() and not (info["mask2"] & ~full["mask2"]).any()      # a budget only takes flags away
        # a triangle the full walk flags in the second tier alone and this one in neither gave up after its first tier was settled
        lost = full["mask2"][:n] & ~full["mask"][:n] & ~info["mask2"][:n]
        assert info["gave_up2"] >= lost.sum() - info["gave_up"]
        second_only += info["gave_up2"]
    assert second_only > 0
    ctx.close()


@pytest.mark.parametrize("quad,fork", [(16, 2), (1, 2), (5, 0)])
@pytest.mark.parametrize("view", sorted(VIEWS))
def test_frames_are_bit_identical(rt, orc, view, quad, fork):
    name, cam, quat = VIEWS[view]
    tris = tc.scene(name)
    ctx = make(rt, tris)
    bvh4 = ctx.read_bvh4()
    ctx.debug_set_tune("QUAD", quad); ctx.debug_set_tune("FORK", fork)
    p = params(rt, ctx, cam=cam, quat=quat)
    ctx.debug_set_tune("EXPOSE", 0)
    ctx.render(p); off = ctx.read_radiance().copy()
    ctx.debug_set_tune("EXPOSE", None)
    info = ctx.debug_exposure(p, want_mask=False)
    assert info["flagged2"] > info["flagged"] > 0
    ctx.render(p); on = ctx.read_radiance().copy()
    assert ctx.debug_exposure(None, want_mask=False)["used"]
    ctx.debug_set_tune("EXPOSE", 5)
    ctx.render(p); first = ctx.read_radiance().copy()
    assert ctx.debug_exposure(None, want_mask=False)["used"]
    ctx.debug_set_tune("EXPOSE", None)
    ctx.render(params(rt, ctx, cam=cam, quat=quat, simple_kernel=True)); simple = ctx.read_radiance().copy()
    ref, st = oracle_frame(orc, view, tris, bvh4, cam=cam, quat=quat)
    assert st["rays_shadow"] >= 100                                        # the view does look at the scene (a run: torus 7,099, plate 101, plate_low 362)
    assert np.array_equal(bits(off), bits(on)) and np.array_equal(bits(first), bits(on))
    assert np.array_equal(bits(on), bits(simple)) and np.array_equal(bits(on), bits(ref))
    ctx.close()


@pytest.mark.parametrize("view", sorted(VIEWS))
def test_counters_with_both_tiers_and_with_the_first_alone(rt, orc, view):
    name, cam, quat = VIEWS[view]
    tris = tc.scene(name)
    ctx = make(rt, tris)
    bvh4 = ctx.read_bvh4()
    p = params(rt, ctx, cam=cam, quat=quat, stats=True)
    ctx.debug_exposure(p)
    ref, st = oracle_frame(orc, view, tris, bvh4, cam=cam, quat=quat)
    skipped = {}
    for knob in (6, 2):
        ctx.debug_set_tune("EXPOSE", knob)
        ctx.render(p); img = ctx.read_radiance().copy(); s = ctx.stats()
        info = ctx.debug_exposure(None, want_mask=False)
        skipped[knob] = info["skipped"]
        assert info["used"] and np.array_equal(bits(img), bits(ref))
        assert s["rays_shadow"] == st["rays_shadow"] - skipped[knob] and s["rays_closest"] == st["rays_closest"] and s["samples"] == st["samples"]
    print(view, "shadow rays", st["rays_shadow"], "skipped by the first tier", skipped[6], "by both", skipped[2])
    assert skipped[2] >= skipped[6] > 0
    if view == "plate":                                  # seen from above every hit passes both gates: the second tier's triangles add their rays
        assert skipped[2] > skipped[6]
    ctx.close()


def test_a_recompute_for_a_farther_camera_is_waited_for_by_the_next_launch_on_another_slot(rt, orc):
    """As the test of this name in tests/test_gpu_exposure.py, with both masks at stake (one pass writes them, one event follows it): a large
    production launch from beyond the masks' camera distance takes them again on its own side stream, and the launch submitted right behind
    it, with no host wait, runs on another frame slot and has to wait for that pass.  Both frames are the oracle's."""
    tris = np.array(tc.scene("torus"))
    near = dict(w=512, h=512, spp=8, bounces=7)
    far = dict(w=512, h=512, spp=8, bounces=7, cam=(0.3, 0.2, 6.0))
    for last in (1, 2):                                  # read the recomputing launch's own frame, then the one behind it
        ctx = make(rt, tris)
        bvh4 = ctx.read_bvh4()
        ctx.render(params(rt, ctx, **near)); ctx.synchronize()
        before = ctx.debug_exposure(None, want_mask=False)
        assert before["valid"] and before["cam_max"] < 6.0
        for f in range(1, last + 1):
            ctx.render(params(rt, ctx, frame=f, **far))          # no synchronize in between
        img = ctx.read_radiance().copy()
        after = ctx.debug_exposure(None, want_mask=False)
        assert after["cam_max"] >= 6.0 and after["used"] and after["flagged2"] >= after["flagged"] > 0
        ref, _ = oracle_frame(orc, "torus_far", tris, bvh4, 512, 512, 8, 7, frame=last, cam=(0.3, 0.2, 6.0))
        assert np.array_equal(bits(img), bits(ref))
        ctx.close()
