"""tests/treeaudit.py on this side of the bus: the host twins of the build and the refit stand in for the device trees, and the oracle's
traversal (orc.trace_ray, one call per ray) for the ray-query kernels.  That keeps the helper honest where there is no GPU, and it audits
the oracle's traversal per triangle: every other CPU test compares the oracle with code that walks the same tree.

Every case prints its share of rays that are not auditable, of rays answered by an occluder and the number of flush exemptions; the shares
are held to pathref.FRAGILE_CAP by treeaudit.assert_judged.  Triangle counts stay small enough for the Python ray loop.

The detection tests damage a correct tree through its words only and hand it to the oracle (tests/test_gpu_tree_audit.py installs the same
trees with set_bvh4): as in test_damaged_tree, a damaged tree only loses hits."""
import numpy as np
import pytest

import pathref
import scenes
import treeaudit as ta
from refit_cases import halves, ord16, pack, unord16, wave
from test_accel_host import DEGENERATE, degenerate
from test_gpu_path_reference import deform

SEEDS = {1: 0, 2: 1, 3: 2, 4: 3, 5: 4, 64: 5, 65: 6, 777: 7, 2500: 8}


@pytest.fixture
def host(rt, orc):
    return ta.HostContext(rt, orc)


# ---- the helper against pathref itself -------------------------------------------------------------------------------------------------
def test_margins_are_pathrefs_and_occluders_are_brute_forces(host):
    """treeaudit.margins restates pathref._candidates for one pair; here against pathref.loosely_accepts on every aimed ray, and against
    pathref.query (every ray against every triangle) on a subset: where brute force is certain, its closest triangle is the ray's own or
    what judge calls an occluder, and the oracle's answers are judged as brute force judges them.  Up to 120,000 triangles this can be
    run on a CPU (1,500 rays of the 480,000 here); at full size the O(N) judge is the only possibility."""
    for n, seed, sub in ((3000, 11, 3000), (120000, 6, 1500)):
        tris = ta.soup(n, seed)
        rays = ta.aimed_rays(tris)
        own = ta.margins(tris, rays.O, rays.D, rays.tri, rays.t_max)
        pick = np.random.default_rng(1).choice(len(rays.tri), sub, replace=False)
        ok, t = pathref.loosely_accepts(tris, rays.O[pick], rays.D[pick], rays.tri[pick], rays.t_max[pick])
        assert np.array_equal(ok, own["loose"][pick]) and np.allclose(t, own["t"][pick], rtol=1e-12, atol=0)
        q = pathref.query(tris, rays.O[pick], rays.D[pick], rays.t_max[pick])
        aud = own["tight"][pick]
        sure = aud & ~q["fragile"]
        assert np.all(q["hit"][sure])
        other = sure & (q["prim"] != rays.tri[pick])
        assert np.all(q["t"][other] <= own["t"][pick][other] + pathref.D_T)
        print("soup %d: %d of %d sampled rays not auditable, %d fragile by brute force, %d answered by an occluder (%.3f %%)" % (
            n, int((~aud).sum()), sub, int((aud & q["fragile"]).sum()), int(other.sum()), 100 * other.mean()))
        assert (~aud).mean() + (aud & q["fragile"]).mean() + other.mean() <= pathref.FRAGILE_CAP
        if n > 3000:
            continue
        host.set_triangles(tris); host.build_bvh(0)
        sub_rays = ta.Rays()
        sub_rays.O, sub_rays.D, sub_rays.t_max, sub_rays.tri, sub_rays.n, sub_rays.own = rays.O[pick], rays.D[pick], rays.t_max[pick], rays.tri[pick], n, None
        j = ta.judge(tris, sub_rays, host.trace_rays(sub_rays.O, sub_rays.D, t_max=sub_rays.t_max))
        ta.assert_judged(j, "soup 3000 subset", capped=False)                  # a subset of the rays: the caps are asserted above, by brute force
        assert np.array_equal(j.occluder[sure], other[sure])                       # judge's occluders are brute force's


# ---- built trees ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted(SEEDS))
def test_reference_build(host, n):
    """orc.build_lbvh2 + collapse_lbvh2_to_bvh4 (accel 0)."""
    tris = ta.soup(n, SEEDS[n])
    host.set_triangles(tris); host.build_bvh(0)
    assert np.array_equal(host.b4, host.rt.collapse_lbvh2_to_bvh4(host.b2, n)[0])
    ta.audit_context(host, tris, "soup %d accel 0" % n, kernels=[False])


@pytest.mark.parametrize("scene,accel", [("soup2000", 1), ("soup2000", 2), ("dragon3000", 1), ("dragon3000", 2), ("sponza12000", 2)])
def test_area_collapse_and_ploc(rt, host, scene, accel):
    """collapse_bvh2_to_bvh4_accel at levels 1 and 2; level 2 over build_bvh2_ploc.  (The sponza-class scene has no fewer than 12,000 triangles.)"""
    tris = ta.soup(2000, 11) if scene == "soup2000" else rt.procedural_scene(0, 3000) if scene == "dragon3000" else rt.procedural_scene(1, 12000)
    host.set_triangles(tris); host.build_bvh(accel)
    ta.audit_context(host, tris, "%s accel %d" % (scene, accel), kernels=[False])


def test_bvh4_wide(rt, orc, host):
    """bvh2_to_bvh4_wide keeps the BVH2's ids and boxes: nodes no path reaches, no pre-order, boxes by the BVH2's rule -- held to topology
    and containment, and after an update to the BVH4's rules too."""
    tris = ta.soup(3000, 12)
    host.set_triangles(tris)
    host.set_bvh4(rt.bvh2_to_bvh4_wide(orc.build_lbvh2(tris)))
    r4, _ = ta.audit_context(host, tris, "BVH4_wide", built=False, exact=False, bvh2=False, kernels=[False])
    assert (r4.depth < 0).sum() > 100 and len(r4.stale) > 100                        # it is the tree this case means
    moved = wave(tris, 0.1, 2)
    host.update_triangles(moved)
    ta.audit_context(host, moved, "BVH4_wide refitted", built=False, bvh2=False, kernels=[False])


@pytest.mark.parametrize("accel", [0, 1, 2])
def test_refitted_trees(rt, host, accel):
    """refit_bvh4 / refit_bvh2 after the --animate wave, after the warp of test_gpu_path_reference.py, after eight updates, and after a
    cluster of triangles collapsed to a point and came back."""
    tris = rt.procedural_scene(0, 1500)
    host.set_triangles(tris); host.build_bvh(accel)
    built = host.b4.copy()
    for what, moved in (("wave", wave(tris, 0.1, 3)), ("deform", deform(tris))):
        host.update_triangles(moved)
        ta.audit_context(host, moved, "dragon 1500 accel %d %s" % (accel, what), kernels=[False])
    for k in range(8):
        moved = wave(tris, 0.04 * (k + 1), k)
        host.update_triangles(moved)
    ta.audit_context(host, moved, "dragon 1500 accel %d eight updates" % accel, kernels=[False])
    flat, pick = ta.collapse_cluster(tris, (0.1, 0.1, 0.1), 15)
    host.update_triangles(flat)
    r4, js = ta.audit_context(host, flat, "dragon 1500 accel %d collapsed cluster" % accel, kernels=[False])
    assert not js[False, False].auditable.reshape(-1, 4)[pick].any()                 # zero area: unhittable by the specification, classed so
    host.update_triangles(tris)
    assert np.array_equal(host.b4, built)
    ta.audit_context(host, tris, "dragon 1500 accel %d restored" % accel, kernels=[False])


# ---- geometry at the edges ------------------------------------------------------------------------------------------------------------
def check_family(ctx, kind, accel, kernels):
    """The DEGENERATE families were made for the build, not for this audit: their triangles are unhittable by the specification (tiny,
    and the area-less part of mixed_zero), copies of one another (identical), or so dense that another triangle lies within the ray's
    2e-4 (coplanar: 500 triangles of size 1 in one plane; signed_zero: a third of them in the plane x = 0, a third in y = 0; two_clusters:
    200 triangles in a cube of 2e-3).  No h can meet the caps there, so the shares are not capped: each family is classed instead, from the
    reference alone, and asserted to be what it is.  Containment, exact boxes, no lost triangle, no unexplained hit hold as everywhere."""
    tris = degenerate(kind)
    ctx.set_triangles(tris); ctx.build_bvh(accel)
    r4, js = ta.audit_context(ctx, tris, "%s accel %d" % (kind, accel), capped=False, kernels=kernels)
    rays = ta.aimed_rays(tris)
    below = np.abs(ta.margins(tris, rays.O, rays.D, rays.tri, rays.t_max)["det"]) < pathref.EPS_T + pathref.D_DET     # at or below the determinant threshold
    for (simple, any_hit), j in js.items():
        answered = j.occluder | j.fragile
        if kind == "tiny":                                                           # |e1 x e2| of about 1e-11, every box flushed to zero
            assert below.all() and not j.auditable.any() and len(r4.exempt) > 0
        elif kind == "identical":                                                    # 300 copies: whichever the walk meets first answers for all
            assert j.auditable.all() and not j.fragile.any() and j.occluder.mean() > 0.9
        elif kind == "mixed_zero":                                                   # half of the coordinates are +-0 or +-1e-9: many triangles have no area
            assert np.array_equal(~j.auditable, below) and 0.02 < below.mean() < 0.2
        elif not any_hit:                                                            # dense: most rays are answered by a nearer or coplanar triangle
            assert j.share_not_auditable <= pathref.FRAGILE_CAP and answered.mean() > 0.3
    return r4, js


@pytest.mark.parametrize("accel", [0, 2])
@pytest.mark.parametrize("kind", DEGENERATE)
def test_degenerate_families(host, kind, accel):
    check_family(host, kind, accel, [False])


def edge_scene(name):
    if name == "room":
        return scenes.room()
    if name == "cornell":
        return scenes.cornell()[0]
    if name == "f16_grid":
        return ta.f16_grid()
    if name == "plus1000":           # f16 steps of 0.5: loose boxes that must still contain.  It is |o| / e that conditions a pair, so the triangles
        return (ta.soup(2000, 9, 0.1) * np.float32(20) + np.float32(1000)).astype(np.float32)       # are of size 2, spread over [980, 1020]^3
    if name == "times27000":         # every coordinate below 30,000: f16 steps of 16
        return (ta.soup(2000, 9) * np.float32(27000)).astype(np.float32)
    raise KeyError(name)


EDGE_SCENES = ["room", "cornell", "f16_grid", "plus1000", "times27000"]


@pytest.mark.parametrize("name", EDGE_SCENES)
def test_axis_aligned_translated_and_scaled(host, name):
    tris = edge_scene(name)
    assert np.abs(tris).max() < 30000
    rays = ta.aimed_rays(tris)
    if name in ("room", "cornell", "f16_grid"):
        flat = name != "room"                                                      # the room's two panels are tilted
        axis_parallel = (rays.D == 0).sum(1) == 2
        assert axis_parallel.all() if flat else axis_parallel.mean() > 0.7
    for accel in (0, 2):
        host.set_triangles(tris); host.build_bvh(accel)
        ta.audit_context(host, tris, "%s accel %d" % (name, accel), kernels=[False], rays=rays)


# ---- detection: the audit must see a damaged tree, and see it where it is ---------------------------------------------------------------
def subtree_tris(r, words, node):
    rec = np.asarray(words[1:], np.uint32).reshape(-1, 8)
    out, stack = [], [int(node)]
    while stack:
        i = stack.pop()
        if rec[i, 7] & 0x80000000:
            out.append(int(rec[i, 7] & 0x7FFFFFFF))
        else:
            stack += [int(c) for c in rec[i, 3:7] if c != 0xFFFFFFFF]
    return np.array(sorted(out))


def shrink_case(tris, bvh4, rays, bounded, steps=16):
    """An internal node with 30..300 triangles below it whose upper x bound, taken `steps` f16 steps down, is missed by some aimed rays
    of those triangles and still met by others.  -> (damaged words, node, the triangles below it)."""
    r = ta.verify_bvh4(tris, bvh4)
    rec = bvh4[1:].reshape(-1, 8)
    aud = ta.margins(tris, rays.O, rays.D, rays.tri, rays.t_max)["tight"]
    for node in np.flatnonzero((rec[:, 7] & 0x80000000) == 0)[5:]:
        below = subtree_tris(r, bvh4, node)
        if not 30 <= len(below) <= 300:
            continue
        o = ord16(halves(rec[node, :3]))
        o[3] -= steps
        box = ta.decode(pack(unord16(o)))
        idx = (below[:, None] * 4 + np.arange(4)).reshape(-1)
        meets, misses = ta.segment_meets_box(rays, idx, box[:3], box[3:], bounded)
        if (misses & aud[idx]).sum() >= 2 and meets.sum() >= 2:
            bad = bvh4.copy()
            bad[1 + 8 * node: 4 + 8 * node] = pack(unord16(o))
            return bad, int(node), below
    raise AssertionError("no node to damage")


def point_passes(tris, rays):
    """[(points, k, the rays count_hits takes or None)] of treeaudit.audit_points"""
    return [(ta.near_points(rays, tris), ta.K_NEAR, rays), (ta.far_points(tris), ta.K_FAR, None)]


def judged_points(ctx, tris, passes, kernels):
    """Every pass through every kernel: yields (points, rays, simple, results, {query: judgement}); a damaged tree may lose triangles, but
    it reports nothing the reference cannot accept and no malformed list."""
    for pts, k, rr in passes:
        for simple in kernels:
            res = ta.point_queries(ctx, pts, rr, simple, k)
            js = ta.judge_points(tris, pts, rr, res, k)
            assert all(len(j.phantom) == 0 and len(j.malformed) == 0 for j in js.values())
            yield pts, rr, simple, res, js


def check_detection(ctx, tris, good, kernels):
    """Three damaged copies of the correct tree `good`, each installed with ctx.set_bvh4."""
    rays = ta.aimed_rays(tris)
    n = tris.size // 9
    # 1. one internal box shrunk: flagged as the one stale box (too tight), the triangles that leave it named with it, and the aimed rays
    #    lose exactly the triangles whose segment no longer meets the box -- a triangle below the node is found through every other box
    bounded = getattr(ctx, "prunes_at_t_max", True)
    bad, node, below = shrink_case(tris, good, rays, bounded)
    r = ta.verify_bvh4(tris, bad)
    assert r.stale.tolist() == [node] and not r.stale_loose[0] and not r.errors
    assert set(r.outside["node"].tolist()) == {node} and set(r.outside["tri"].tolist()) <= set(below.tolist())
    ctx.set_bvh4(bad)
    box = ta.decode(bad[1 + 8 * node: 4 + 8 * node])
    idx = (below[:, None] * 4 + np.arange(4)).reshape(-1)
    meets, misses = ta.segment_meets_box(rays, idx, box[:3], box[3:], bounded)
    for simple in kernels:
        for any_hit in (False, True):
            j = ta.judge(tris, rays, ctx.trace_rays(rays.O, rays.D, t_max=rays.t_max, any_hit=any_hit, simple=simple), any_hit)
            lost = set(j.lost.tolist())
            must = set(idx[misses & j.auditable[idx]].tolist())
            assert must and must <= lost and not lost & set(idx[meets].tolist()) and lost <= set(idx.tolist()), (simple, any_hit, len(must), len(lost))
            assert set(j.lost_tris.tolist()) <= set(r.outside["tri"].tolist())       # every loss is attributed
            with pytest.raises(AssertionError, match="lost triangles.*%d" % node):
                ta.assert_judged(j, "shrunk box", r)
    #    The point queries prune by bound2, restated in float64 with its slack: a point whose bound2 to the shrunk box
    #    exceeds r_max^2 cannot reach its triangle (radius: lost, no exception; closest and k-nearest: its own triangle is not reported; the
    #    judge excuses it only where a nearer triangle answers), one whose bound2 is below r_max^2 still finds it in its radius list.
    passes = point_passes(tris, rays)
    outside, seen = set(r.outside["tri"].tolist()), {}
    for pts, rr, simple, res, js in judged_points(ctx, tris, passes, kernels):
        pidx = idx if pts.what == "near" else below
        b2 = ta.bound2_f64(pts.P[pidx], box[:3], box[3:])
        r2 = pts.r_max[pidx].astype(np.float64) ** 2
        must = pidx[pts.auditable[pidx] & (b2 > r2 * (1 + 1e-3))]
        keep = set(pidx[b2 < r2 * (1 - 1e-3)].tolist())
        for j in js.values():
            assert set(j.lost_tris.tolist()) <= outside <= set(below.tolist()), (pts.what, simple, j.query)     # every lost triangle lies below the damaged node
        lost = set(js["radius"].lost.tolist())
        assert set(must.tolist()) <= lost and not lost & keep and lost <= set(pidx.tolist()), (pts.what, simple, len(must), len(lost))
        assert np.all(res["closest"][1][must] != pts.tri[must]) and not (res["knn"][1][must] == pts.tri[must, None]).any()
        assert set(must.tolist()) <= set(js["closest"].lost.tolist()) | set(np.flatnonzero(js["closest"].excused).tolist())
        if rr is not None:                                                            # count_hits prunes at t_max, on the host as on the device
            meets_c, misses_c = ta.segment_meets_box(rays, idx, box[:3], box[3:], True)
            lost_c = set(js["hits"].lost.tolist())
            assert set(idx[misses_c & js["hits"].auditable[idx]].tolist()) <= lost_c and not lost_c & set(idx[meets_c].tolist()) and lost_c <= set(idx.tolist())
        seen[pts.what] = (len(must), len(keep), len(lost))
        if lost:
            with pytest.raises(AssertionError, match="lost triangles.*%d" % node):
                ta.assert_point_judged(js["radius"], "shrunk box", r)
    print("shrunk box %d: points that must be lost / must be kept / lost by radius_search -- %s" % (node, seen))
    assert seen["near"][0] > 0 and seen["near"][1] > 0 and seen["near"][2] > 0     # without the damage nothing is lost: the audit sees this box
    # 2. two leaves' triangle indices swapped, boxes left: both leaves flagged, and only they
    rec = good[1:].reshape(-1, 8)
    leaves = np.flatnonzero(rec[:, 7] & 0x80000000)
    a, b = int(leaves[len(leaves) // 3]), int(leaves[2 * len(leaves) // 3])
    bad = good.copy()
    bad[8 * a + 8], bad[8 * b + 8] = good[8 * b + 8], good[8 * a + 8]
    r = ta.verify_bvh4(tris, bad)
    assert sorted(r.stale.tolist()) == sorted([a, b]) and not r.errors
    ta_, tb_ = int(good[8 * a + 8] & 0x7FFFFFFF), int(good[8 * b + 8] & 0x7FFFFFFF)
    assert set(r.outside["tri"].tolist()) == {ta_, tb_}
    ctx.set_bvh4(bad)
    j = ta.judge(tris, rays, ctx.trace_rays(rays.O, rays.D, t_max=rays.t_max, simple=kernels[0]))
    assert set(j.lost_tris.tolist()) == {ta_, tb_}
    #    Points: the walk meets each triangle in the other's leaf, so a point finds its own triangle only if that leaf's box lies within
    #    r_max (and the slack) of it.  Which of the two applies is computed from the boxes and printed: apart (as in the scenes of these
    #    tests, where the two leaves are a third of the tree apart), the radius lists must name both triangles and no other; within reach,
    #    the audit may name either, neither or both, and nothing but them.
    box_of = {ta_: ta.decode(good[1 + 8 * b: 4 + 8 * b]), tb_: ta.decode(good[1 + 8 * a: 4 + 8 * a])}           # the box each triangle now sits in
    for pts, rr, simple, res, js in judged_points(ctx, tris, passes, kernels):
        apart = True
        for t, bx in box_of.items():
            pi = np.flatnonzero(pts.tri == t)
            apart &= bool(np.all(pts.auditable[pi] & (ta.bound2_f64(pts.P[pi], bx[:3], bx[3:]) > pts.r_max[pi].astype(np.float64) ** 2 * (1 + 1e-3))))
        print("swapped leaves, %s pass, simple %d: %s" % (pts.what, simple, "the boxes are apart: both triangles must be named" if apart else
              "the boxes lie within r_max + s of each other's points: the audit need not name the triangles"))
        assert all(set(j.lost_tris.tolist()) <= {ta_, tb_} for j in js.values())
        if apart:
            assert set(js["radius"].lost_tris.tolist()) == {ta_, tb_}
            assert {ta_, tb_} <= set(js["closest"].lost_tris.tolist()) | set(pts.tri[js["closest"].excused].tolist())
    # 3. one box enlarged: no ray can see it, the no-loose-boxes check does
    bad = good.copy()
    o = ord16(halves(bad[1 + 8 * node: 4 + 8 * node]))
    o[4] += 3
    bad[1 + 8 * node: 4 + 8 * node] = pack(unord16(o))
    r = ta.verify_bvh4(tris, bad)
    assert r.stale.tolist() == [node] and r.stale_loose[0] and not r.errors and len(r.outside) == 0
    ctx.set_bvh4(bad)
    j = ta.judge(tris, rays, ctx.trace_rays(rays.O, rays.D, t_max=rays.t_max, simple=kernels[0]))
    assert len(j.lost) == 0
    for pts, rr, simple, res, js in judged_points(ctx, tris, passes, kernels):
        assert all(len(j.lost) == 0 for j in js.values())                             # invisible to the points as to the rays
    with pytest.raises(AssertionError, match="not the rule's"):
        ta.assert_tree(r, "enlarged box")


def test_damaged_trees_are_detected(rt, host):
    tris = rt.procedural_scene(0, 3000)
    host.set_triangles(tris); host.build_bvh(1)
    check_detection(host, tris, host.read_bvh4().copy(), [False])


def test_topology_damage_is_detected(rt, host):
    tris = ta.soup(500, 3)
    host.set_triangles(tris); host.build_bvh(0)
    good = host.read_bvh4()
    rec = good[1:].reshape(-1, 8)
    inner = np.flatnonzero((rec[:, 7] & 0x80000000) == 0)
    bad = good.copy(); bad[1 + 8 * inner[3] + 4] = 0xFFFFFFFF                           # a child dropped: its triangles sit in no leaf
    assert any("no reachable leaf" in e for e in ta.verify_bvh4(tris, bad).errors)
    bad = good.copy(); bad[1 + 8 * inner[3] + 4] = bad[1 + 8 * inner[3] + 3]            # a child named twice
    assert any("more than once" in e for e in ta.verify_bvh4(tris, bad).errors)
    bad = good.copy(); k = inner[3]; bad[1 + 8 * k + 3], bad[1 + 8 * k + 4] = good[1 + 8 * k + 4], good[1 + 8 * k + 3]
    assert any("pre-order" in e for e in ta.verify_bvh4(tris, bad).errors) and not ta.verify_bvh4(tris, bad, built=False).errors
    b2 = host.read_bvh2().copy()
    r2 = b2[1:].reshape(-1, 6)
    o = ord16(halves(r2[7, :3])); o[0] += 1
    r2[7, :3] = pack(unord16(o))                                                    # a BVH2 internal box that was not stepped outwards
    assert ta.verify_bvh2(tris, b2).stale.tolist() == [7]
