"""treeaudit.audit_points over the host twins: every triangle of every tree through closest_points_bvh4, radius_search_bvh4, nearest_k_bvh4 and
count_hits_bvh4, judged in float64 (tests/closestref.py, pathref's margins) against that triangle and the reported ones alone.  The sampled
tests of these queries (closest_cases, radius_cases, knn_cases) see a triangle only where a sampled point happens to be near it; here four
points sit 1e-4 above every triangle (the near pass) and one 16 * 2^-12 above every centroid (the far pass, where bound2's slack no longer
lets every nearby box in).  tests/test_gpu_point_audit.py runs the same cases through the kernels.

Scenes: the soups of the build tests, a sparse 120,000-triangle soup, the dragon-class and sponza-class stand-ins and the f16 grid, at accel
0, 1 and 2, built and refitted after `wave` and `deform`.  Left out, on purpose:
* the translated (+1,000) and x 27,000 scenes of test_tree_audit.EDGE_SCENES: they lie outside the domain for which DESIGN.md section 15
  proves bound2 sound (vertex coordinates in [-4, 4], point coordinates in [-32, 32]); test_edge_of_the_proven_domain goes to its edge;
* the DEGENERATE families: no distance can audit them (test_tree_audit.check_family says what each of them is);
* soup(120000, 6) at size 0.2 for closest and k-nearest: 1.87 % of its near-pass points are answered by another triangle; radius and counts run;
* `deform` of the sponza-class scene from the capped audit: 2.98 % of its near-pass points are answered by another triangle (the warp folds
  its walls into each other) and it holds slivers on which the f32 point-triangle arithmetic leaves the 16 units: test_deformed_sponza_slivers
  runs it through the judges that excuse nothing and pins what is known about the slivers.
A scene above 1 % is changed, never the cap.  `deform` lifts the size-0.2 soup of 30,000 to 1.01 % in the near pass, so that soup is refitted
to the warp of its own triangles at half their size (soup(n, seed, size) scales the triangles about fixed centres: 0.32 %).  NO_FAR_CLOSEST lists
the cases whose far pass has another triangle within 16 * 2^-12 of more than 1 % of the centroids (2.4 - 27 %): closest_points is not part of
their far pass -- it is neither called nor judged there -- while radius_search and nearest_k, which excuse nothing, are; wherever closest_points
is judged the cap is asserted.  The far pass of closest_points is carried by the small soups, by soup(30000, 5, size=0.02) -- a scene added for
this: the 30,000-triangle case of it -- by the dragon-class scene and by the f16 grid.  treeaudit.audit_points records every measured share."""
import numpy as np
import pytest

import closest_cases as clc
import closestref
import radius_cases as rc
import treeaudit as ta
from refit_cases import wave
from test_gpu_path_reference import deform

ACCELS = [0, 1, 2]
SOUPS = {1: 0, 2: 1, 3: 2, 4: 3, 5: 4, 64: 5, 65: 6, 777: 7, 30000: 5}
SCENES = ["soup%d" % n for n in sorted(SOUPS)] + ["sparse30000", "sparse120000", "dragon20000", "sponza12000", "f16_grid"]
MOVES = {"sponza12000": ("wave",)}                                                  # every other scene: wave and deform
NO_FAR_CLOSEST = {("soup30000", "deform"), ("soup30000", "built"), ("soup30000", "wave"), ("sparse30000", "deform"), ("sparse120000", "built"), ("sparse120000", "wave"),
               ("sparse120000", "deform"), ("dragon20000", "deform"), ("sponza12000", "built"), ("sponza12000", "wave")}


def scene(rt, name):
    if name.startswith("soup"):
        return ta.soup(int(name[4:]), SOUPS[int(name[4:])])
    if name.startswith("sparse"):
        return ta.soup(int(name[6:]), 5, size=0.02)
    if name == "f16_grid":
        return ta.f16_grid()
    return rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 20000) if name == "dragon20000" else rt.procedural_scene(rt.SCENE_SPONZA_CLASS, 12000)


def states(name, tris, moves=None):
    """[(what, triangles)]: built, then the refits of this scene"""
    moved = {"wave": wave(tris, 0.1, 3), "deform": deform(ta.soup(30000, SOUPS[30000], size=0.1) if name == "soup30000" else tris)}
    return [("built", tris)] + [(m, moved[m]) for m in (moves or MOVES.get(name, ("wave", "deform")))]


def built_and_refitted(ctx, name, tris, accel, kernels, moves=None):
    out = {}
    for what, now in states(name, tris, moves):
        if what == "built":
            ctx.set_triangles(tris); ctx.build_bvh(accel)
        else:
            ctx.update_triangles(now)
        out[what] = ta.audit_points(ctx, now, "%s accel %d %s" % (name, accel, what), kernels=kernels, far_closest=(name, what) not in NO_FAR_CLOSEST)
    return out


@pytest.fixture
def host(rt, orc):
    return ta.HostContext(rt, orc)


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name", SCENES)
def test_every_triangle_through_the_point_queries(rt, host, name, accel):
    built_and_refitted(host, name, scene(rt, name), accel, [False])


def test_the_dense_soup_through_radius_and_counts(host):
    """soup(120000, 6) at size 0.2, the scene of the aimed rays: 1.87 % of its points are answered by another triangle, so closest and
    k-nearest are not audited on it -- the radius and count judges exclude nothing, and hold."""
    tris = ta.soup(120000, 6)
    host.set_triangles(tris); host.build_bvh(0)
    rays = ta.aimed_rays(tris)
    for pts, rr in ((ta.near_points(rays, tris), rays), (ta.far_points(tris), None)):
        res = ta.point_queries(host, pts, rr, True, 1, stats=True)
        assert not any(res["drops"])
        ta.assert_point_judged(ta.judge_radius(tris, pts, res["search"][0], res["search"][1:], res["count"]), "soup 120000 size 0.2")
        if rr is not None:
            ta.assert_point_judged(ta.judge_counts(rr, res["hits"], tris), "soup 120000 size 0.2")


# ---- the judges against brute force ----------------------------------------------------------------------------------------------------
def test_judges_agree_with_float64_brute_force(rt, host):
    """On a subset small enough for closestref.nearest (every point against every triangle): a point the closest judge calls answered by
    another triangle has a float64 minimum below d_own - tol, every other auditable point has its own triangle within tol of the minimum;
    and a judge bites -- the own triangle struck from a list, a row or an answer is a lost triangle, a foreign one written in is a phantom."""
    tris = ta.soup(3000, 11)
    host.set_triangles(tris); host.build_bvh(0)
    rays = ta.aimed_rays(tris)
    for pts, k in ((ta.near_points(rays, tris), ta.K_NEAR), (ta.far_points(tris), ta.K_FAR)):
        res = ta.point_queries(host, pts, None, False, k)
        js = ta.judge_points(tris, pts, None, res, k)
        assert all(len(j.lost) == 0 and len(j.phantom) == 0 and len(j.malformed) == 0 for j in js.values())
        pick = np.random.default_rng(2).choice(pts.R, min(pts.R, 2000), replace=False)
        ref, _ = closestref.nearest(pts.P[pick], tris)
        other = js["closest"].excused[pick]
        assert np.array_equal(other, ref < pts.d_own[pick] - pts.tol)
        assert pts.auditable[pick].all() and np.all(ref <= pts.d_own[pick] + 1e-12)
        print("soup 3000 %s pass: %d of %d sampled points answered by another triangle, by brute force too" % (pts.what, int(other.sum()), len(pick)))
        # struck out and written in
        dist, prim, u, v = [a.copy() for a in res["closest"]]
        mine = np.flatnonzero(prim == pts.tri)[:7]
        prim[mine] = ta.MISS; dist[mine] = np.inf
        assert ta.judge_closest(tris, pts, (dist, prim, u, v)).lost.tolist() == mine.tolist()
        prim[mine] = (pts.tri[mine] + 1500) % 3000; dist[mine] = res["closest"][0][mine]
        j = ta.judge_closest(tris, pts, (dist, prim, u, v))
        assert j.phantom.tolist() == mine.tolist() and j.lost.tolist() == mine.tolist()
        off, (d, p, uu, vv) = np.asarray(res["search"][0]).astype(np.int64), res["search"][1:]
        drop = np.flatnonzero(p == np.repeat(pts.tri, np.diff(off)))[3]
        keep = np.arange(len(p)) != drop
        owner = int(np.searchsorted(off, drop, side="right") - 1)
        off2 = off.copy(); off2[owner + 1:] -= 1
        j = ta.judge_radius(tris, pts, off2, (d[keep], p[keep], uu[keep], vv[keep]), res["count"])
        assert j.lost.tolist() == [owner] and j.malformed.tolist() == [owner]       # the count no longer equals the list
        rows = [a.copy() for a in res["knn"]]
        c5, c6 = [int(np.argmax(rows[1][i] == pts.tri[i])) for i in (5, 6)]
        rows[1][5, c5], rows[1][6, c6] = ta.MISS, rows[1][40, 0]
        j = ta.judge_knn(tris, pts, rows, k)
        assert set(j.lost.tolist()) == {5, 6} and 5 in j.malformed and 6 in j.phantom
        with pytest.raises(AssertionError, match="lost triangles"):
            ta.assert_point_judged(j, "struck out")


# ---- the deformed sponza-class scene: slivers ------------------------------------------------------------------------------------------------
SLIVER = 64.0          # e^2 / 2A (longest edge squared over twice the area) from which a triangle counts as a sliver here


def aspect(tris):
    """e^2 / 2A per triangle, float64: the factor by which step 2 of the point-triangle arithmetic (f = e2 - (b / a) e1)
    cancels -- |f| is the triangle's height over e1, and each component of f carries a rounding error of a few 2^-24 e."""
    T = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    e = np.stack([T[:, 1] - T[:, 0], T[:, 2] - T[:, 0], T[:, 2] - T[:, 1]], 1)
    with np.errstate(all="ignore"):
        return (e ** 2).sum(-1).max(1) / np.linalg.norm(np.cross(e[:, 0], e[:, 1]), axis=1)


def check_deformed_sponza(rt, ctx, kernels):
    """The per-triangle audit found this scene: `deform` folds the sponza-class walls into triangles with edges of 0.54 over heights down to
    3e-4 (e^2 / 2A up to 1,843; 68 before the warp), and on 9 of the 66,682 listed near-pass entries dist and the (u, v) point are 16 to 59
    units of 2^-24 (max|p| + max|v|) from the float64 distance, against the 16 of closest_cases.TOL_K.  Not the walk: asserted here, every
    point's dist has the bits of the brute-force route, and the radius lists equal brute force's as sets.  It is the conditioning of step 2,
    which no change of the walk can mend and whose repair would change the bits of every answer.  So the scene is held to what excuses
    nothing -- no triangle missing from a radius list, a k-nearest row or behind a crossing count, no malformed list -- and the deviations
    are pinned to what is known: only on slivers (e^2 / 2A >= 64: below that every entry stays within the 16 units, as on every other scene
    of the audit), on at most 0.1 % of the entries, and by at most one unit per unit of e^2 / 2A -- the error grows with that factor;
    measured 0.243 of it, times four, rounded up to a power of two, as closest_cases derives TOL_K."""
    base = rt.procedural_scene(rt.SCENE_SPONZA_CLASS, 12000)
    assert aspect(base).max() < 70
    tris = deform(base)
    kap = aspect(tris)
    assert kap.max() > 1000 and (kap >= SLIVER).mean() > 0.2
    ctx.set_triangles(base); ctx.build_bvh(0)
    ctx.update_triangles(tris)
    rays = ta.aimed_rays(tris)
    d2_of = lambda p, prim: clc.product_d2(p, tris, prim)
    for pts, k, rr in ((ta.near_points(rays, tris), ta.K_NEAR, rays), (ta.far_points(tris), ta.K_FAR, None)):
        assert not any(ta.point_queries(ctx, pts, rr, True, k, stats=True)["drops"])
        rec = pts.records()
        unit = pts.tol / clc.TOL_K
        brute = ctx.closest_points(rec, brute_force=True)[:4]
        brute_r = ctx.radius_search(rec, brute_force=True)[:5]
        for simple in kernels:
            res = ta.point_queries(ctx, pts, rr, simple, k)
            clc.check_same_minimum(rec, tris, res["closest"], brute, d2_of)
            rc.assert_same_lists(res["search"], brute_r, ordered=False)
            js = ta.judge_points(tris, pts, rr, res, k)
            for q, j in js.items():
                print("deformed sponza simple %d %s %s" % (simple, q, j.summary()))
                assert len(j.lost) == 0 and len(j.malformed) == 0, (pts.what, simple, q, j.lost_tris[:10])
            if rr is not None:
                assert len(js["hits"].phantom) == 0
            # every listed entry, and the closest answer: deviation of dist and of the (u, v) point from the float64 distance of its triangle
            off = np.asarray(res["search"][0]).astype(np.int64)
            owner = np.repeat(np.arange(pts.R), np.diff(off))
            worst = 0.0
            for idx, (dist, prim, u, v) in ((owner, res["search"][1:]), (np.arange(pts.R), res["closest"])):
                prim = prim.astype(np.int64)
                assert np.all(prim < pts.n)
                d = pts.distance(idx, prim)
                dev = np.maximum(np.abs(dist.astype(np.float64) - d), np.abs(pts.uv_distance(idx, prim, u, v) - d)) / unit
                over = dev > clc.TOL_K
                assert np.all(kap[prim[over]] >= SLIVER), "an entry beyond the tolerance on a triangle that is no sliver"
                assert over.sum() <= 1e-3 * len(prim) and np.all(dev[over] <= kap[prim[over]])
                assert np.all(d <= pts.r_max[idx].astype(np.float64) + pts.tol * np.maximum(1.0, kap[prim] / clc.TOL_K))
                worst = max(worst, float(dev.max()))
                print("deformed sponza simple %d, %s pass: %d of %d entries beyond %g units, the largest deviation %.1f units, %.3f of its e^2 / 2A" % (
                    simple, pts.what, int(over.sum()), len(prim), clc.TOL_K, dev.max(), (dev / kap[prim]).max()))


def test_deformed_sponza_slivers(rt, host):
    check_deformed_sponza(rt, host, [False])


# ---- the edge of the domain DESIGN.md section 15 proves bound2 for ------------------------------------------------------------------------
def edge_points(tris):
    """-> [(name, (n, 4) PtPoint records)]: the aimed points of both passes with their radii; 4,000 points uniform in [-32, 32]^3 and 1,000
    with one coordinate exactly +-32, r_max = +inf."""
    rng = np.random.default_rng(32)
    inside = rng.uniform(-32, 32, (4000, 3)).astype(np.float32)
    face = rng.uniform(-32, 32, (1000, 3)).astype(np.float32)
    face[np.arange(1000), rng.integers(0, 3, 1000)] = np.where(rng.random(1000) < 0.5, -32, 32)
    wide = np.concatenate([inside, face])
    assert np.abs(wide).max() == 32 and (np.abs(wide) == 32).any(1).sum() >= 1000
    return [("near", ta.near_points(ta.aimed_rays(tris), tris).records()), ("far", ta.far_points(tris).records()),
            ("wide", np.concatenate([wide, np.full((5000, 1), np.inf, np.float32)], 1))]


def check_edge_of_domain(rt, ctx, kernels):
    """Vertices up to +-4 and points out to +-32, where the margin of the proof is smallest (5.7e-5 against 1.04e-4): twin and kernels against
    the brute-force route, which prunes nothing, bit for bit; and against float64."""
    base = (ta.soup(20000, 4) * np.float32(3.6)).astype(np.float32)
    assert 3.9 < np.abs(base).max() <= 4
    ctx.set_triangles(base); ctx.build_bvh(0)
    for what, tris in (("built", base), ("wave", wave(base, 0.04, 3))):
        assert np.abs(tris).max() <= 4
        if what == "wave":
            ctx.update_triangles(tris)
        bvh4 = ctx.read_bvh4()
        d2_of = lambda p, prim: clc.product_d2(p, tris, prim)
        sets = dict(edge_points(tris))
        for name, rec in sets.items():
            brute = ctx.closest_points(rec, brute_force=True)[:4]                   # the context's brute-force route: the kernel on a device
            twin = rt.closest_points_bvh4(tris, bvh4, rec, stats=True)
            assert twin[4]["stack_drops"] == 0
            clc.check_same_minimum(rec, tris, twin[:4], brute, d2_of)
            for simple in kernels:
                clc.check_same_minimum(rec, tris, ctx.closest_points(rec, simple=simple)[:4], brute, d2_of)
            print("edge of the domain, %s, %s points: %d points, the walk's dist equals brute force's in every bit" % (what, name, len(rec)))
        wide = sets["wide"]                                                         # the 5,000 points out to +-32
        sub = wide[np.random.default_rng(5).choice(len(wide), 2000, replace=False)]
        ref = closestref.nearest(sub[:, :3], tris)[0]
        for simple in kernels:
            clc.check_against_float64(sub, tris, ctx.closest_points(sub, simple=simple)[:4], ref)
        near8 = wide.copy()
        near8[:, 3] = 8
        rows16 = np.ascontiguousarray(wide)
        brute_r = ctx.radius_search(near8, brute_force=True)[:5]
        brute_k = ctx.nearest_k(rows16, 16, brute_force=True)[:4]
        tw = rt.radius_search_bvh4(tris, bvh4, near8, stats=True)
        assert tw[5]["stack_drops"] == 0 and int(tw[0][-1]) > 20000
        rc.assert_same_lists(tw[:5], brute_r, ordered=False)
        tk = rt.nearest_k_bvh4(tris, bvh4, rows16, 16, stats=True)
        assert tk[4]["stack_drops"] == 0
        assert clc.same_bits(tk[0], brute_k[0])
        for simple in kernels:
            rc.assert_same_lists(ctx.radius_search(near8, simple=simple)[:5], brute_r, ordered=False)
            assert clc.same_bits(ctx.nearest_k(rows16, 16, simple=simple)[0], brute_k[0])
        print("edge of the domain, %s: radius 8 lists %d entries, equal as sets; the 16 nearest of %d points equal in every bit of dist" % (what, int(tw[0][-1]), len(rows16)))


def test_edge_of_the_proven_domain(rt, host):
    check_edge_of_domain(rt, host, [False])
