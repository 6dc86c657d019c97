"""The HIP kernels against tests/pathref.py -- the independent float64 brute-force restatement of DESIGN.md sections 4 and 13 -- with no
oracle in between: every other GPU test compares the kernels with oracle/pt_oracle.cpp walking the same tree, so a tree that loses a
hit, or an estimator mistake both sides share, stays invisible to them.  Same assertions as tests/test_path_reference.py: every pixel
(ray) the reference does not flag as fragile within pathref.TOL, fragile ones at most 2 % of a case.

This file does not use the `orc` fixture.  (`random_rays` is imported from tests/test_gpu_rayquery.py, as the ray generator every query
test shares; that module imports the oracle's ctypes wrapper at its top, nothing here calls it.)

Sizes: the 120,000-triangle cases compare 200 fixed pseudo-random pixels each (4 spp, 8 bounces: about 2,000 to 2,700 rays against
every triangle, 8 to 12 s of reference work on 8 cores); the query case is 6,000 rays against 20,000 triangles, four brute-force
passes of about 5 s."""
import ctypes as C

import numpy as np
import pytest

import pathref
from scenes import quat_yaw_pitch, random_soup
from test_gpu_rayquery import random_rays
from test_path_reference import closed_form_check, dark_box_check, roulette_bias_check, check_claims

pytestmark = pytest.mark.gpu

MISS = 0xFFFFFFFF
ACCELS = [0, 1, 2]            # the reference's tree, the area-guided collapse, device PLOC
KERNELS = [False, True]       # simple=False: the persistent megakernel; True: one pixel (ray) per lane


def gpu_render(rt, ctx, name, simple=False, stats=False, **extra):
    """A case of pathref.case() through pt_render (accumulating sequences frame by frame); the scene must be set."""
    tris, sph, w, h, kw = pathref.case(name)
    kw = dict(kw)
    frames, frame = kw.pop("accum_frames", 1), kw.pop("frame", 0)
    if frames > 1:
        ctx.render(ctx.make_params(w, h, mode=rt.PT_MODE_REFERENCE))          # a non-accumulating render ends any running sum
    for f in range(frames):
        ctx.render(ctx.make_params(w, h, frame=frame + f, accumulate=frames > 1, simple_kernel=simple, stats=stats, brute_force=sph is not None, **dict(kw, **extra)))
    return ctx.read_radiance()


def check_gpu_counters(st, ref, max_bounces):
    assert st["samples"] == ref.samples
    slack = int(ref.frag.sum()) * (max_bounces + 1)
    assert abs(st["rays_closest"] - ref.rays_closest) <= slack and abs(st["rays_shadow"] - ref.rays_shadow) <= slack, (st, ref.rays_closest, ref.rays_shadow, slack)


@pytest.mark.parametrize("name", pathref.PATH_CASES)
def test_kernels_equal_the_reference(rt, gpu_ctx, name):
    """Every CPU case, both kernels, on the tree of every accel level; counters of the instrumented megakernel; and the three
    estimator checks that do not lean on the reference's reading of the spec (closed form, roulette bias, dark box)."""
    tris, _, w, h, kw = pathref.case(name)
    ref = pathref.reference(name)
    check_claims(name, ref)
    gpu_ctx.set_triangles(tris)
    for accel in ACCELS:
        gpu_ctx.build_bvh(accel)
        for simple in KERNELS:
            img = gpu_render(rt, gpu_ctx, name, simple=simple)
            pathref.check_image(img, ref, pathref.TOL, "%s accel %d simple %d" % (name, accel, simple))
            assert np.all(img[..., 3] == 1)
            if name in ("tetra", "big_triangle"):
                closed_form_check(img, name, pathref.TOL)
            if name in ("soup300", "soup_inside", "room"):
                roulette_bias_check(img, name)
            if name == "closed_box":
                dark_box_check(img)
        if kw.get("accum_frames", 1) == 1:
            for simple in KERNELS:
                gpu_render(rt, gpu_ctx, name, simple=simple, stats=True)
                check_gpu_counters(gpu_ctx.stats(), ref, kw["max_bounces"])


def test_cornell_spheres_brute_force(rt, gpu_ctx):
    name = "cornell_spheres"
    tris, sph, w, h, kw = pathref.case(name)
    ref = pathref.reference(name)
    check_claims(name, ref)
    gpu_ctx.set_triangles(tris); gpu_ctx.set_spheres(sph)
    img = gpu_render(rt, gpu_ctx, name)
    pathref.check_image(img, ref, pathref.TOL_SPHERES, name)
    gpu_render(rt, gpu_ctx, name, stats=True)
    check_gpu_counters(gpu_ctx.stats(), ref, kw["max_bounces"])


@pytest.mark.parametrize("name", pathref.MODE01_CASES)
def test_modes_0_and_1(rt, gpu_ctx, name):
    tris, _, w, h, kw = pathref.case(name)
    ref = pathref.reference(name)
    gpu_ctx.set_triangles(tris)
    for accel in ACCELS:
        gpu_ctx.build_bvh(accel)
        for simple in KERNELS:
            img = gpu_render(rt, gpu_ctx, name, simple=simple)
            pathref.check_image(img, ref, pathref.TOL, "%s accel %d simple %d" % (name, accel, simple))


def test_four_frame_batch_accumulated(rt, gpu_ctx):
    """pt_set_batch(4): four accumulating frames traced by one launch are the reference's running sum over frames 2..5."""
    name = "room_frame2"
    tris, _, w, h, kw = pathref.case(name)
    ref = pathref.reference(name, accum_frames=4)
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh()
    kw = dict(kw); frame = kw.pop("frame")
    gpu_ctx.set_batch(4)
    for f in range(4):
        gpu_ctx.render(gpu_ctx.make_params(w, h, frame=frame + f, accumulate=True, **kw))
    img = gpu_ctx.read_radiance()
    gpu_ctx.set_batch(1)
    pathref.check_image(img, ref, pathref.TOL, name + " batch of 4")
    assert gpu_ctx.accum_info().samples == 4 * kw["spp"]
    one = pathref.reference(name)
    assert pathref.deviation(one.img, ref.img).max() > 0.05              # the sum is not the first frame alone


def test_three_tile_shares_reassembled(rt, gpu_ctx):
    """Three tile shares (tile_rank r of 3), each read from its compact buffer and put back with pt_tile_ids' order on the host."""
    name = "soup300_frame3_accum2"                                        # 75 x 41: edge tiles stick out of the image
    tris, _, w, h, kw = pathref.case(name)
    kw = dict(kw, accum_frames=1)
    ref = pathref.reference(name, accum_frames=1)
    kw.pop("accum_frames")
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh()
    hip = C.CDLL("libamdhip64.so")
    img = np.full((h, w, 4), np.nan, np.float32)
    tiles_x = (w + 7) // 8
    seen = 0
    for r in range(3):
        gpu_ctx.render(gpu_ctx.make_params(w, h, tile_rank=r, tile_count=3, **kw))
        ptr, floats = gpu_ctx.compact_radiance(); gpu_ctx.synchronize()
        ids = rt.tile_ids(w, h, r, 3)
        assert floats >= len(ids) * 256
        host = np.zeros(floats, np.float32)
        assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(floats * 4), 2) == 0
        d = host[: len(ids) * 256].reshape(len(ids), 8, 8, 4)
        for s, t in enumerate(ids):
            x0, y0 = (int(t) % tiles_x) * 8, (int(t) // tiles_x) * 8
            ny, nx = min(8, h - y0), min(8, w - x0)
            img[y0:y0 + ny, x0:x0 + nx] = d[s, :ny, :nx]
            seen += 1
    assert seen == tiles_x * ((h + 7) // 8) and not np.isnan(img).any()
    pathref.check_image(img, ref, pathref.TOL, name + " as 3 tile shares")


BIG = {   # 120,000 triangles: a real tree.  Cameras chosen (from the reference alone) so that at most 2 % of the pixels are fragile; at this
          # triangle size (edges about 0.013) a camera inside the sponza-class hall gives 7 %, because every long path meets some edge within f32 reach.
    "dragon120k": dict(kind=0, cam_pos=(0.1, 0.2, 1.4), cam_quat=(0, 0, 0, 1)),
    "sponza120k": dict(kind=1, cam_pos=(1.6, 0.6, 1.2), cam_quat=tuple(float(x) for x in quat_yaw_pitch(0.9, -0.3))),
}
BIG_W, BIG_H, BIG_PIXELS = 160, 96, 200


def big_case(rt, name):
    c = BIG[name]
    tris = rt.procedural_scene(c["kind"], 120000, 20260109)
    rng = np.random.default_rng(5)
    pix = np.stack([rng.integers(BIG_W // 4, 3 * BIG_W // 4, BIG_PIXELS), rng.integers(BIG_H // 4, 3 * BIG_H // 4, BIG_PIXELS)], 1)
    kw = dict(mode=pathref.MODE_PATH, spp=4, max_bounces=8, seed=7, cam_pos=c["cam_pos"], cam_quat=c["cam_quat"])
    return tris, pix, kw


@pytest.mark.parametrize("name", sorted(BIG))
def test_large_scene_pixels(rt, gpu_ctx, name):
    tris, pix, kw = big_case(rt, name)
    assert np.abs(tris).max() <= 4
    ref = pathref.render(tris, BIG_W, BIG_H, pixels=pix, **kw)
    assert ref.rays_closest > 3 * len(pix) * 4 // 2 and ref.rays_shadow > 400         # the subset does bounce
    gpu_ctx.set_triangles(tris)
    for accel in ACCELS:
        gpu_ctx.build_bvh(accel)
        for simple in KERNELS:
            gpu_ctx.render(gpu_ctx.make_params(BIG_W, BIG_H, simple_kernel=simple, **kw))
            img = gpu_ctx.read_radiance()[pix[:, 1], pix[:, 0]]
            pathref.check_image(img, ref, pathref.TOL, "%s accel %d simple %d" % (name, accel, simple))


# ---- ray queries ----------------------------------------------------------------------------------------------------------------------
QN = 6000


def query_scene():
    return random_soup(20000, 5, size=0.3)


def deform(tris):
    """A smooth warp of up to 0.35 per axis: the same triangles somewhere else, so a refitted tree must find other hits."""
    v = np.asarray(tris, np.float64).reshape(-1, 3)
    return (v + 0.35 * np.sin(3.0 * v[:, [1, 2, 0]] + np.array([0.3, 1.1, 2.0]))).astype(np.float32).reshape(-1)


class QueryRef:
    """The reference's answers for one scene and ray set (with and without t_max), and which rays each bound is asked of."""

    def __init__(self, tris, O, D, t_max=None, surface_starts=True):
        self.tris, self.O, self.D, self.t_max = tris, O, D, t_max
        r = self.r = pathref.query(tris, O, D, t_max)
        k = len(O) // 4
        self.surface = np.zeros(len(O), bool)
        if surface_starts:
            self.surface[2 * k:3 * k] = True        # random_rays' third quarter starts ON a triangle: its own t sits at the 1e-7 threshold, a coin toss in f32
        # values: u, v, t are asked to pathref.TOL where plain f32 can deliver it -- where the reference's own f32 evaluation of the winning pair is within TOL / 4
        h = r["hit"]
        self.poor = np.zeros(len(O), bool)
        if h.any():
            _, u32, v32, t32 = pathref.pair(tris, O[h], D[h], r["prim"][h], np.float32)
            q = pathref.TOL / 4
            self.poor[h] = ~((np.abs(u32 - r["u"][h]) <= q) & (np.abs(v32 - r["v"][h]) <= q) & (np.abs(t32 - r["t"][h]) <= q * np.maximum(r["t"][h], 1)))
        free = ~self.surface
        self.share = float((r["fragile"] | self.poor)[free].mean()); self.any_share = float(r["any_fragile"][free].mean())
        print("query reference: %d rays, hit %.2f, fragile %.3f %% + ill-conditioned %.3f %% of the rays not started on a surface (any hit: %.3f %%); fragile among surface starts %.1f %%"
              % (len(O), h.mean(), 100 * r["fragile"][free].mean(), 100 * (self.poor & ~r["fragile"])[free].mean(), 100 * self.any_share, 100 * r["fragile"][self.surface].mean() if surface_starts else 0.0))
        assert self.share <= pathref.FRAGILE_CAP and self.any_share <= pathref.FRAGILE_CAP

    def check_closest(self, got, what):
        t, prim, u, v = got
        r = self.r
        got_hit = prim != MISS
        ok = ~r["fragile"]
        assert np.array_equal(got_hit[ok], r["hit"][ok]), (what, np.flatnonzero(ok & (got_hit != r["hit"]))[:10])
        hh = ok & r["hit"]
        assert np.array_equal(prim[hh].astype(np.int64), r["prim"][hh]), (what, np.flatnonzero(hh & (prim.astype(np.int64) != r["prim"]))[:10])
        val = hh & ~self.poor
        tol = pathref.TOL
        assert np.all(np.abs(t[val] - r["t"][val]) <= tol * np.maximum(r["t"][val], 1)), what
        assert np.all(np.abs(u[val] - r["u"][val]) <= tol) and np.all(np.abs(v[val] - r["v"][val]) <= tol), what
        assert np.all(np.isposinf(t[~got_hit])) and np.all(u[~got_hit] == 0) and np.all(v[~got_hit] == 0)
        # fragile rays cannot be compared, but they can be explained: a hit is a triangle the reference could accept, no farther than the
        # closest one it accepts for certain; a miss means it accepts none for certain
        f = np.flatnonzero(~ok)
        fh = f[got_hit[f]]
        acc, tt = pathref.loosely_accepts(self.tris, self.O[fh], self.D[fh], prim[fh], None if self.t_max is None else self.t_max[fh])
        assert np.all(acc), (what, fh[~acc][:10])
        assert np.all(tt <= r["t_sure"][fh] + 1e-4 * np.maximum(np.abs(tt), 1)), what
        assert np.all(np.isinf(r["t_sure"][f[~got_hit[f]]])), what

    def check_any(self, got, what):
        t, prim, u, v = got
        r = self.r
        got_hit = prim != MISS
        ok = ~r["any_fragile"]
        assert np.array_equal(got_hit[ok], r["any"][ok]), (what, np.flatnonzero(ok & (got_hit != r["any"]))[:10])
        h = np.flatnonzero(got_hit)                                                   # its prim depends on the order: the reference must accept that triangle
        acc, tt = pathref.loosely_accepts(self.tris, self.O[h], self.D[h], prim[h], None if self.t_max is None else self.t_max[h])
        assert np.all(acc), (what, h[~acc][:10])
        assert np.all(np.abs(t[h] - tt) <= 1e-4 * np.maximum(np.abs(tt), 1)), what


def run_queries(ctx, refs, what):
    for label, q in refs.items():
        for simple in KERNELS:
            w = "%s %s simple %d" % (what, label, simple)
            q.check_closest(ctx.trace_rays(q.O, q.D, t_max=q.t_max, simple=simple), w)
            q.check_any(ctx.trace_rays(q.O, q.D, t_max=q.t_max, any_hit=True, simple=simple), w + " any")


def make_refs(tris, seed):
    O, D = random_rays(tris, QN, seed)
    plain = QueryRef(tris, O, D)
    rng = np.random.default_rng(3)
    h = plain.r["hit"]
    tmax = np.where(h, plain.r["t"] * rng.choice(np.float32([0.5, 1.5]), QN), rng.uniform(0.1, 10, QN)).astype(np.float32)
    bounded = QueryRef(tris, O, D, tmax)
    assert 0 < bounded.r["hit"].sum() < h.sum()                                    # t_max does cut hits off
    return {"unbounded": plain, "t_max": bounded}


def test_ray_queries_on_built_and_refitted_trees(rt, gpu_ctx):
    """ctx.trace_rays, closest and any hit, both kernels, with and without t_max, against float64 brute force: on the device-built tree
    of every accel level, and on that tree refitted by update_triangles after a warp that moves most hits to another triangle."""
    tris = query_scene()
    moved = deform(tris)
    assert np.abs(moved).max() <= 4
    before, after = make_refs(tris, 7), make_refs(moved, 7)
    # the rays made for the scene before the warp, answered in the scene after it (their surface starts no longer lie on a surface)
    a, b = before["unbounded"].r, QueryRef(moved, before["unbounded"].O, before["unbounded"].D, surface_starts=False)
    for accel in ACCELS:
        gpu_ctx.set_triangles(tris)
        gpu_ctx.build_bvh(accel)
        run_queries(gpu_ctx, before, "accel %d built" % accel)
        gpu_ctx.trace_rays(before["unbounded"].O, before["unbounded"].D, stats=True)
        assert gpu_ctx.stats()["stack_drops"] == 0                                 # nothing is lost at the 64-entry cap, so brute force is the answer
        gpu_ctx.update_triangles(moved)
        run_queries(gpu_ctx, after, "accel %d refitted" % accel)
        run_queries(gpu_ctx, {"old rays": b}, "accel %d refitted" % accel)
        gpu_ctx.trace_rays(after["unbounded"].O, after["unbounded"].D, stats=True)
        assert gpu_ctx.stats()["stack_drops"] == 0
    both = ~a["fragile"] & ~b.r["fragile"] & a["hit"] & b.r["hit"]
    assert (a["prim"][both] != b.r["prim"][both]).mean() > 0.5                       # the warp changes which triangle most rays meet
    assert ((a["hit"] != b.r["hit"]) & ~a["fragile"] & ~b.r["fragile"]).sum() > 100
