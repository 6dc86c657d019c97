"""The CPU oracle's path tracer against tests/pathref.py: an independent float64 restatement, brute force over
every triangle.  The bit-exact GPU <-> oracle tests cannot see a mistake both sides share; these can: each case compares every pixel
whose decisions are not on a knife edge (pathref's "fragile" flag, at most 2 % of a case) to pathref.TOL, the counters to the
reference's counts, and asserts from the reference's own diagnostics that the case exercises what it claims.  Three checks do not
depend on the reference's reading of the spec at all: a closed form on convex bodies, the unbiasedness of Russian roulette, and
darkness inside a closed box."""
import numpy as np
import pytest

import pathref
from pathref import END_LIMIT, END_MISS, END_ROULETTE
from scenes import random_soup


def oracle_render(orc, name, **override):
    tris, sph, w, h, kw = pathref.case(name)
    p = orc.make_params(w, h, tris.size // 9, **dict(kw, **override))
    if sph is None:
        _, bvh4 = orc.build_bvh4(tris)
        img, _, st = orc.render(p, tris, bvh4)
    else:
        img, st = orc.render_brute(p, tris, sph)
    return img, st


def test_rnd_equals_the_oracle_bit_for_bit(orc):
    n = 0
    for seed in (0, 1, 7, 0xFFFFFFFF, 0x61C88647):
        for pixel in (0, 1, 95, 96, 6143, 2073599, 0xFFFFFFFF):
            for sidx in (0, 1, 3, 4, 255, 65536):
                k = pathref.key(np.uint32(seed), np.uint32(pixel), np.uint32(sidx))
                for bounce in (0, 1, 2, 3, 8, 16, 31):
                    for dim in range(5):
                        want = np.float32(orc.lib.orc_rnd(seed, pixel, sidx, bounce, dim))
                        for dt in (np.float32, np.float64):
                            got = pathref.rnd(k, bounce, dim, dt)
                            assert got.dtype == dt and np.float32(got).view(np.uint32) == want.view(np.uint32) and float(got) == float(want)
                        n += 1
    assert n == 5 * 7 * 6 * 7 * 5


def check_counters(st, ref, max_bounces):
    """Equal where no sample is fragile; otherwise each ray counter is within (fragile samples) x (max_bounces + 1)."""
    assert st["samples"] == ref.samples
    slack = int(ref.frag.sum()) * (max_bounces + 1)
    print("counters: oracle closest %d shadow %d, reference %d %d, fragile samples %d" % (st["rays_closest"], st["rays_shadow"], ref.rays_closest, ref.rays_shadow, int(ref.frag.sum())))
    assert abs(st["rays_closest"] - ref.rays_closest) <= slack and abs(st["rays_shadow"] - ref.rays_shadow) <= slack


def check_claims(name, ref):
    """What a case is there for, from the reference's diagnostics (never from the code under test)."""
    ends = np.bincount(ref.end.ravel(), minlength=3)
    ok = ~ref.frag
    if name in ("soup300", "soup_inside", "room", "room_b3", "back_faces", "soup300_frame3_accum2", "room_frame2", "cornell_spheres"):
        assert ends[END_MISS] > 0 and ends[END_LIMIT] > 0 and ends[END_ROULETTE] > 0, ends
        assert ref.shadow_clear.sum() > 0 and ref.shadow_occluded.sum() > 0
    if name in ("room_b0", "room_b1", "room_b2"):            # roulette starts at bounce 2 and a path at its limit stops before it
        assert ends[END_ROULETTE] == 0 and ends[END_LIMIT] > 0 and (ends[END_MISS] > 0) == (name != "room_b0")
        assert ref.length.max() == int(name[6:]) + 1
    if name == "room_b3":
        assert ref.length.max() == 4
    if name == "room":
        assert (ref.length >= 4).mean() >= 0.25                # a quarter of the samples reach bounce 3
    if name == "closed_box":
        assert ends[END_MISS] == 0 and ends[END_LIMIT] > 0 and ends[END_ROULETTE] > 0
        assert ref.shadow_clear[ok].sum() == 0 and ref.shadow_occluded.sum() > 0
    if name == "back_faces":
        hit = ref.primary_tri >= 0
        assert hit.sum() > 1000 and np.all(ref.primary_back[hit])
    if name in ("tetra", "big_triangle"):
        assert ref.shadow_occluded[ok].sum() == 0 and ref.length[ok].max() == 2 and ends[END_MISS] == ref.end.size


@pytest.mark.parametrize("name", pathref.PATH_CASES)
def test_oracle_path_mode_equals_the_reference(orc, name):
    ref = pathref.reference(name)
    img, st = oracle_render(orc, name)
    pathref.check_image(img, ref, pathref.TOL, name)
    assert np.all(img[..., 3] == 1)
    check_counters(st, ref, pathref.case(name)[4]["max_bounces"])
    check_claims(name, ref)


@pytest.mark.parametrize("name", pathref.SPHERE_CASES)
def test_oracle_brute_force_spheres_equal_the_reference(orc, name):
    ref = pathref.reference(name)
    img, st = oracle_render(orc, name)
    pathref.check_image(img, ref, pathref.TOL_SPHERES, name)
    check_counters(st, ref, pathref.case(name)[4]["max_bounces"])
    check_claims(name, ref)
    assert (ref.primary_tri >= 10).sum() > 500                 # both spheres are seen


@pytest.mark.parametrize("name", pathref.MODE01_CASES)
def test_oracle_modes_0_and_1_equal_the_reference(orc, name):
    ref = pathref.reference(name)
    img, st = oracle_render(orc, name)
    pathref.check_image(img, ref, pathref.TOL, name)
    assert st["rays_closest"] == ref.rays_closest == img.shape[0] * img.shape[1] and st["rays_shadow"] == 0 and st["samples"] == ref.samples
    hit = ref.primary_tri[:, 0] >= 0
    assert 0.1 < hit.mean() < 0.9


def closed_form_check(img, name, tol):
    """Convex body or lone triangle, max_bounces >= 1: a sample that hits is base (max(nf.L, 0) + 0.15) exactly (NEE unoccluded, the bounce
    leaves), a miss 0.01.  Per pixel whose samples all hit one face (or all miss): from that triangle's normal alone."""
    tris, _, w, h, kw = pathref.case(name)
    ref = pathref.reference(name)
    T = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    n = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]); n /= np.linalg.norm(n, axis=1, keepdims=True)
    o, d = pathref.camera_rays(*(np.divmod(np.arange(w * h), w)[::-1]), w, h, *pathref.focal_aspect(w, h), kw.get("cam_pos", (0, 0, 2.5)), kw.get("cam_quat", (0, 0, 0, 1)))
    tri = ref.primary_tri
    one = (tri == tri[:, :1]).all(1) & ~ref.fragile.ravel()
    t0 = tri[:, 0]
    nd = (n[np.maximum(t0, 0)] * d).sum(1)                     # which side faces the camera (the pixel's corner ray; no knife edge: fragile pixels are out)
    nf = np.where((nd < 0)[:, None], n[np.maximum(t0, 0)], -n[np.maximum(t0, 0)])
    want = np.where((t0 >= 0)[:, None], pathref.BASE[None, :] * (np.maximum(nf @ pathref.LDIR, 0) + pathref.SKY)[:, None], pathref.BG_PRIMARY)
    dev = pathref.deviation(img.reshape(-1, 4), want)
    assert one.sum() > 0.9 * w * h and (t0[one] >= 0).sum() > 500 and (t0[one] < 0).sum() > 500
    print("%s closed form: %d pixels, worst %.3g" % (name, one.sum(), dev[one].max()))
    assert dev[one].max() <= tol, np.argwhere(one & (dev > tol))[:5]


@pytest.mark.parametrize("name", ["tetra", "big_triangle"])
def test_closed_form_on_convex_bodies(orc, name):
    img, _ = oracle_render(orc, name)
    closed_form_check(img, name, pathref.TOL)


def roulette_bias_check(img, name):
    """Roulette on (code under test) against the float64 reference with roulette off, same seed and bounce limit, paired per pixel."""
    ref = pathref.reference(name, roulette=False)
    D = (np.asarray(img, np.float64)[..., :3] - ref.img).mean(-1).ravel()
    n = D.size
    se = D.std() / np.sqrt(n)
    print("%s roulette: mean(D) %.3g, standard error %.3g, z %.2f" % (name, D.mean(), se, D.mean() / se if se else 0.0))
    assert abs(D.mean()) <= max(4 * se, 1e-6 * ref.img.mean())
    assert (pathref.reference(name).end == END_ROULETTE).sum() > 100          # roulette does act in this case


@pytest.mark.parametrize("name", ["soup300", "soup_inside", "room"])
def test_roulette_is_unbiased(orc, name):
    img, _ = oracle_render(orc, name)
    roulette_bias_check(img, name)


def dark_box_check(img):
    ref = pathref.reference("closed_box")
    assert ref.fragile.mean() <= pathref.FRAGILE_CAP
    assert np.all(ref.img[~ref.fragile] == 0)
    assert np.all(img[..., :3][~ref.fragile] == 0), np.argwhere((img[..., :3] != 0).any(-1) & ~ref.fragile)[:5]


def test_no_light_through_closed_geometry(orc):
    img, _ = oracle_render(orc, "closed_box")
    dark_box_check(img)


def test_oracle_traversal_against_brute_force_float64(orc):
    """orc.trace_ray (the BVH walk) against the reference's closest / any hit on rays from inside, outside and far away."""
    tris = random_soup(800, 13, size=0.4)
    _, bvh4 = orc.build_bvh4(tris)
    rng = np.random.default_rng(2)
    n = 1500
    O = rng.uniform(-1.5, 1.5, (n, 3)).astype(np.float32)
    D = rng.normal(size=(n, 3)).astype(np.float32)
    sc = pathref.Scene(tris)
    hit, prim, t, u, v, frag = pathref.closest_hit(sc, O, D)
    occ, afrag = pathref.any_hit(sc, O, D)
    assert frag.mean() <= pathref.FRAGILE_CAP and afrag.mean() <= pathref.FRAGILE_CAP and 0.2 < hit.mean() < 0.98
    for i in range(n):
        h, tt, nn, tri = orc.trace_ray(tris, bvh4, O[i], D[i])
        if not frag[i]:
            assert h == hit[i]
            if h:
                assert tri == prim[i] and abs(tt - t[i]) <= pathref.TOL * max(t[i], 1) and np.abs(nn - sc.n[tri]).max() <= pathref.TOL
        h, _, _, tri = orc.trace_ray(tris, bvh4, O[i], D[i], anyhit=True)
        if not afrag[i]:
            assert h == occ[i]
    assert np.array_equal(occ[~frag & ~afrag], hit[~frag & ~afrag])


def f32_deviation(name):
    """What plain f32 does: the reference in single precision against itself in float64, worst non-fragile pixel."""
    tris, sph, w, h, kw = pathref.case(name)
    ref = pathref.reference(name)
    r32 = pathref.render(tris, w, h, spheres=sph, dtype=np.float32, **kw)
    assert r32.img.dtype == np.float32
    return float(pathref.deviation(r32.img, ref.img)[~ref.fragile].max())


@pytest.mark.parametrize("name", ["soup300_frame3_accum2", "room", "cornell_spheres"])
def test_tol_is_the_measured_one(name):
    """pathref.TOL is the next power of ten at or above 4 x the worst f32-vs-f64 deviation of the reference itself over all cases
    (pathref.MEASURED); re-measured here on three of them so the constant cannot drift from its justification."""
    worst = f32_deviation(name)
    tol = pathref.TOL_SPHERES if name in pathref.SPHERE_CASES else pathref.TOL
    print("%s: f32 vs f64 worst non-fragile deviation %.3g (recorded %.3g), tol %g" % (name, worst, pathref.MEASURED[name], tol))
    assert 4 * worst <= tol
    assert abs(worst - pathref.MEASURED[name]) <= 0.25 * pathref.MEASURED[name]
    groups = {False: [v for k, v in pathref.MEASURED.items() if k not in pathref.SPHERE_CASES], True: [pathref.MEASURED[k] for k in pathref.SPHERE_CASES]}
    for spheres, want in ((False, pathref.TOL), (True, pathref.TOL_SPHERES)):
        assert want == 10.0 ** np.ceil(np.log10(4 * max(groups[spheres])))
