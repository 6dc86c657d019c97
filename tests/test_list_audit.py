"""treeaudit.audit_lists over the host twins: every triangle of every tree through list_hits_bvh4 (unsorted and sorted), the long counting
walk of count_hits_bvh4 and contains_bvh4, judged in float64 (pathref's margins) against that triangle and the listed ones alone.  The
sampled tests of these queries (tests/test_hitlist_host.py, tests/test_crossings_host.py) compare twin and kernel bit for bit on a few
thousand rays, which no triangle has to cross; here one ray per triangle (four below 1,000 triangles) runs through the whole scene and must
list its own triangle, whatever else it lists.  tests/test_gpu_list_audit.py runs the same cases through the kernels, and adds occlusion and
signed distance, which have no twin.

Scenes: those of tests/test_point_audit.py except the sparse soup of 120,000 (its 30,000-triangle case is here), at accel 0, 1 and 2, built
and refitted after `wave` and `deform`, with the substitutions that file documents (the size-0.2 soup of 30,000 is refitted to the warp of
its own triangles at half their size; the sponza-class scene is refitted by `wave` only).  The brute-force lists, which validate the judge
and do not depend on the tree, run once per scene here (accel 0, built: 9e8 pair tests per pass on the CPU); the GPU file runs them for
every tree.  treeaudit.audit_lists' docstring records every share these tests print."""
import numpy as np
import pytest

import pathref
import treeaudit as ta
from test_point_audit import ACCELS, SCENES, scene, states

LIST_SCENES = [s for s in SCENES if s != "sparse120000"]


@pytest.fixture
def host(rt, orc):
    return ta.HostContext(rt, orc)


def built_and_refitted(ctx, name, tris, accel, kernels, brute):
    out = {}
    for what, now in states(name, tris):
        if what == "built":
            ctx.set_triangles(tris); ctx.build_bvh(accel)
        else:
            ctx.update_triangles(now)
        out[what] = ta.audit_lists(ctx, now, "%s accel %d %s" % (name, accel, what), kernels=kernels, brute=brute and what == "built")
    return out


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name", LIST_SCENES)
def test_every_triangle_through_the_hit_lists(rt, host, name, accel):
    built_and_refitted(host, name, scene(rt, name), accel, [False], brute=accel == 0)


@pytest.mark.parametrize("accel", ACCELS)
def test_coincident_layers_are_ordered_by_triangle(host, accel):
    """Three doubled layers: every through ray lists pairs of entries with equal bits of t, which the sorted list must order by `prim` --
    the one place where the second half of the sort key decides (a key without it passes every other scene but the sponza-class one,
    where a single ray of 12,000 meets a tie)."""
    tris = ta.coincident_deck()
    host.set_triangles(tris); host.build_bvh(accel)
    j = ta.audit_lists(host, tris, "coincident deck accel %d" % accel, kernels=[False])["hits", False]
    off, t, prim = j.sorted[0], j.sorted[1], j.sorted[2]
    owner = np.repeat(np.arange(j.R), np.diff(off))
    tie = (owner[1:] == owner[:-1]) & (ta._bits(t)[1:] == ta._bits(t)[:-1])
    assert tie.sum() == 3 * j.R and np.all(prim[1:][tie] > prim[:-1][tie])         # six entries per ray, in three ties
    rays = ta.through_rays(tris)
    visit = host.list_hits(rays.O, rays.D)
    vo = np.repeat(np.arange(j.R), np.diff(np.asarray(visit[0]).astype(np.int64)))
    order = np.lexsort((np.arange(len(vo)), ta._bits(visit[1]), vo))                # a stable sort by t alone: what a key without `prim` gives
    vt = (vo[order][1:] == vo[order][:-1]) & (ta._bits(visit[1])[order][1:] == ta._bits(visit[1])[order][:-1])
    assert np.any(visit[2][order][1:][vt] < visit[2][order][:-1][vt])              # the walk visits some ties the other way round


# ---- the judges against brute force, and that they bite ---------------------------------------------------------------------------------
def strike(lists, e):
    """the lists without entry e"""
    off = np.asarray(lists[0]).astype(np.int64).copy()
    owner = int(np.searchsorted(off, e, side="right") - 1)
    off[owner + 1:] -= 1
    keep = np.arange(len(lists[2])) != e
    return (off,) + tuple(np.asarray(a)[keep] for a in lists[1:5]), owner


def test_judges_agree_with_float64_brute_force(rt, host):
    """On a 3,000-triangle subset, every ray against every triangle in float64 (pathref._candidates): every crossing the reference accepts
    for certain is in the list, and every listed entry is one it at least loosely accepts -- the judge, which looks at the listed pairs
    only, says the same.  And the judges bite: an own entry struck from a list is a lost triangle and a malformed list, a foreign triangle
    written in is a phantom, two sorted entries swapped are malformed, an `unoccluded` one above the bound is a lost triangle."""
    tris = ta.soup(3000, 11)
    n = tris.size // 9
    host.set_triangles(tris); host.build_bvh(0)
    rays = ta.through_rays(tris)
    lists = host.list_hits(rays.O, rays.D)
    srt = host.list_hits(rays.O, rays.D, sort=True)
    counts = host.count_hits(rays.O, rays.D)
    j = ta.judge_hits(tris, rays, lists, srt, counts)
    assert j.counts()[3:] == (0, 0, 0, 0, len(lists[2]), 0) and j.auditable.all()
    # every ray against every triangle
    off = np.asarray(lists[0]).astype(np.int64)
    owner = np.repeat(np.arange(len(rays.tri)), np.diff(off))
    listed = np.zeros((len(rays.tri), n), bool)
    listed[owner, lists[2]] = True
    sc = pathref.Scene(tris)
    certain = at_margin = 0
    for a in range(0, len(rays.tri), 250):
        c = pathref._candidates(sc, rays.O[a:a + 250].astype(np.float64), rays.D[a:a + 250].astype(np.float64), np.full(len(rays.O[a:a + 250]), pathref.INF_T))
        part = listed[a:a + 250]
        assert not (c["tight"] & ~part).any(), "a certain crossing of the reference is not listed"
        assert not (part & ~(c["loose"] | c["acc"])).any(), "a listed entry the reference does not even loosely accept"
        certain += int(c["tight"].sum()); at_margin += int((part & ~c["tight"]).sum())
    assert certain == len(j.certain[0]) and at_margin == len(lists[2]) - certain
    print("soup 3000: %d listed entries, %d certain crossings by brute force, all listed; %d entries at a margin; worst value deviation %.3f of its margin" % (len(lists[2]), certain, at_margin, j.worst))
    # struck out
    e = int(np.flatnonzero(lists[2] == rays.tri[owner])[5])
    cut, who = strike(lists, e)
    j = ta.judge_hits(tris, rays, cut, srt, counts)
    assert j.lost.tolist() == [who] and j.malformed.tolist() == [who] and len(j.phantom) == 0
    with pytest.raises(AssertionError, match="lost triangles"):
        ta.assert_point_judged(j, "struck out")
    # a foreign triangle written in, in both lists: a phantom, nothing else
    far = [a.copy() for a in lists]
    fs = [a.copy() for a in srt]
    foreign = (int(lists[2][e]) + 1500) % n
    assert not listed[who, foreign]
    far[2][e] = foreign
    se = int(np.asarray(srt[0]).astype(np.int64)[who] + np.flatnonzero(srt[2][int(srt[0][who]):int(srt[0][who + 1])] == lists[2][e])[0])
    fs[2][se] = foreign
    j = ta.judge_hits(tris, rays, far, fs, counts)
    assert j.phantom.tolist() == [who] and j.lost.tolist() == [who]
    # two sorted entries swapped
    long = int(np.argmax(np.diff(off)))
    a = int(srt[0][long])
    assert off[long + 1] - off[long] >= 2
    sw = [x.copy() for x in srt]
    for col in sw[1:5]:
        col[a], col[a + 1] = col[a + 1], col[a]
    j = ta.judge_hits(tris, rays, lists, sw, counts)
    assert j.malformed.tolist() == [long] and len(j.lost) == 0 and len(j.phantom) == 0
    # a sorted list that is no permutation: one u changed
    sw = [x.copy() for x in srt]
    sw[3][a] = np.float32(0.5) * sw[3][a] + np.float32(0.125)
    assert ta.judge_hits(tris, rays, lists, sw, counts).malformed.tolist() == [long]
    # a value beyond its margin
    bent = [x.copy() for x in lists]
    bent[3][e] += np.float32(0.01)
    j = ta.judge_hits(tris, rays, bent, srt, counts)
    assert j.values_off.tolist() == [who] and j.worst > 1
    # occlusion: exactly at the bound holds, one above is a lost triangle
    aim = rays.aimed
    floor = ta.occlusion_floor(tris, aim)
    unocc = (ta.OCC_SAMPLES - floor).astype(np.uint32)
    result = lambda u: ((u / np.float32(ta.OCC_SAMPLES)).astype(np.float32), u, np.full(len(u), ta.OCC_SAMPLES, np.uint32))
    j = ta.judge_occlusion(tris, aim, result(unocc))
    assert len(j.lost) == 0 and len(j.malformed) == 0 and 0.5 < j.share_sure < 0.9
    s = int(np.flatnonzero(floor > 0)[9])
    unocc[s] += 1
    j = ta.judge_occlusion(tris, aim, result(unocc))
    assert j.lost.tolist() == [s] and j.lost_tris.tolist() == [int(aim.tri[s])]
    vis, u, smp = result(unocc)
    vis[3] = np.nextafter(vis[3], np.float32(2))
    assert ta.judge_occlusion(tris, aim, (vis, u, smp)).malformed.tolist() == [3]
