"""Every triangle of every device tree through the hit lists, the long counting walk, occlusion, containment and signed distance
(treeaudit.audit_lists): list_hits unsorted and sorted, count_hits on the same long rays, occlusion over one surfel per aimed ray, contains
and signed_distance over the near-pass points -- persistent and simple kernels, and the brute-force kernel as the judge's own check --
judged in float64 against the own triangle and the listed ones alone, plus the compositions as equalities.  The scenes, the refits and the
substitutions are those of tests/test_list_audit.py; here the trees are the device's -- built at every level, refitted by update_triangles,
installed with set_bvh4 / set_bvh2 before and after an update.  After the kernels the host twin answers the same rays over the tree read
back from the device: its judgement must count the same in every category and its sorted lists must equal the device's bit for bit.

Measured on an MI355X, persistent, simple and brute-force kernels alike, and equal to the twin's figures in every case (they are in
treeaudit.audit_lists' docstring): no ray not auditable, nothing lost, unexplained or malformed, no push dropped; up to 676,057 entries per
call and lists of 57 (the 30,000-triangle soup after `wave`), whose walk stacks 31 of 64 entries; entries at a margin of the reference 0 -
0.73 %; the largest deviation of a listed t, u or v 0.148 of its pair's margin; occlusion: 61.0 - 78.1 % of the sample rays certainly cross
the own triangle, at most 0.367 % of the surfels (and of the triangles) have no such ray, no surfel below its bound; every composition
held.  The shrunk box loses 16 triangles, the 16 predicted, and keeps the 14 whose rays certainly meet it.

One context per test, plain sequential launches, one process.  No case above 30,000 triangles or 120,000 rays: the float64 judge is the cost."""
import numpy as np
import pytest

import treeaudit as ta
from refit_cases import halves, ord16, pack, unord16, wave
from test_list_audit import LIST_SCENES
from test_point_audit import ACCELS, MOVES, scene, states
from test_tree_audit import subtree_tris

pytestmark = pytest.mark.gpu

SMALL = [n for n in LIST_SCENES if n.startswith("soup") and int(n[4:]) < 1000]
LARGE = [n for n in LIST_SCENES if n not in SMALL]


def audit_device_and_twin(rt, ctx, tris, name):
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1)
    rays = ta.through_rays(tris)
    assert len(rays.tri) <= 120000
    dev = ta.audit_lists(ctx, tris, name, rays=rays)
    twin = ta.HostContext(rt, None)
    twin.set_triangles(tris)
    twin.set_bvh4(ctx.read_bvh4())
    counts = twin.count_hits(rays.O, rays.D)
    cap = int(counts.astype(np.int64).sum()) + 1
    host = ta.judge_hits(tris, rays, twin.list_hits(rays.O, rays.D, capacity=cap), twin.list_hits(rays.O, rays.D, sort=True, capacity=cap), counts)
    ta.assert_point_judged(host, name + " twin")
    for simple in ta.KERNELS:
        j = dev["hits", simple]
        assert j.counts() == host.counts(), (name, simple, j.counts(), host.counts())
        assert np.array_equal(j.sorted[0], host.sorted[0]) and np.array_equal(j.sorted[2], host.sorted[2]) \
            and all(np.array_equal(ta._bits(j.sorted[c]), ta._bits(host.sorted[c])) for c in (1, 3, 4)), (name, simple)
    return dev


def run_states(rt, ctx, name, tris, accel, only=None):
    for what, now in states(name, tris):
        if what == "built":
            ctx.set_triangles(tris); ctx.build_bvh(accel)
        else:
            ctx.update_triangles(now)
        if only is None or what == only:
            audit_device_and_twin(rt, ctx, now, "%s accel %d %s" % (name, accel, what))
        if what == only:
            break


@pytest.mark.parametrize("name", SMALL)
def test_small_soups_built_and_refitted(rt, gpu_ctx, name):
    """1 .. 777 triangles: a root that is a leaf, a single node, one block and several; four rays and surfels per triangle."""
    for accel in ACCELS:
        run_states(rt, gpu_ctx, name, scene(rt, name), accel)


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name, what", [(n, w) for n in LARGE for w in ["built"] + list(MOVES.get(n, ("wave", "deform")))])
def test_scenes_built_and_refitted(rt, gpu_ctx, name, what, accel):
    """One state per case (the refits applied in order up to it, the earlier ones not audited again): the dense soup lists 630,000 entries
    per call, which its float64 judgement and the twin's walks make the slowest case."""
    run_states(rt, gpu_ctx, name, scene(rt, name), accel, only=what)


def test_coincident_layers_are_ordered_by_triangle(rt, gpu_ctx):
    """treeaudit.coincident_deck: every through ray meets three ties of t, which only `prim` orders -- hit_sort_kernel's lane sort (lists
    of six entries), at every level, against the judge's order check and the twin's bits."""
    tris = ta.coincident_deck()
    for accel in ACCELS:
        gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh(accel)
        j = audit_device_and_twin(rt, gpu_ctx, tris, "coincident deck accel %d" % accel)["hits", False]
        off, t = j.sorted[0], j.sorted[1]
        owner = np.repeat(np.arange(j.R), np.diff(off))
        assert int(((owner[1:] == owner[:-1]) & (ta._bits(t)[1:] == ta._bits(t)[:-1])).sum()) == 3 * j.R


@pytest.mark.parametrize("how", ["set_bvh4", "set_bvh2", "set_bvh2_ploc"])
def test_installed_trees_before_and_after_an_update(rt, gpu_ctx, how):
    tris = rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 20000)
    n = tris.size // 9
    gpu_ctx.set_triangles(tris)
    gpu_ctx.build_bvh(0)
    lbvh2 = gpu_ctx.read_bvh2()
    gpu_ctx.set_triangles(tris)
    if how == "set_bvh4":
        gpu_ctx.set_bvh4(rt.collapse_bvh2_to_bvh4_accel(lbvh2, n, 1)[0])
    else:
        gpu_ctx.set_bvh2(rt.build_bvh2_ploc(tris) if how == "set_bvh2_ploc" else lbvh2)
    audit_device_and_twin(rt, gpu_ctx, tris, how)
    moved = wave(tris, 0.1, 2)
    gpu_ctx.update_triangles(moved)
    audit_device_and_twin(rt, gpu_ctx, moved, "%s after wave" % how)


def shrink_case(tris, bvh4, rays):
    """An internal node with 30..300 triangles below it and one of its six bounds, taken 16, 64 or 256 f16 steps inwards, so that the shrunk box
    is certainly missed by the through rays of some of those triangles and certainly met by others (a long ray along the normal leaves a
    box through a face only where the triangle lies close to it, so the aimed rays' 16 steps on the upper x bound do not always do).
    -> (damaged words, node, the rays of the triangles below it, the box)."""
    r = ta.verify_bvh4(tris, bvh4)
    rec = bvh4[1:].reshape(-1, 8)
    aud = ta.margins(tris, rays.O, rays.D, rays.tri, rays.t_max)["tight"]
    for node in np.flatnonzero((rec[:, 7] & 0x80000000) == 0)[5:]:
        below = subtree_tris(r, bvh4, node)
        if not 30 <= len(below) <= 300:
            continue
        idx = (below[:, None] * rays.k + np.arange(rays.k)).reshape(-1)
        for steps in (16, 64, 256):
            for face in range(6):
                o = ord16(halves(rec[node, :3]))
                o[face] += steps if face < 3 else -steps
                if o[face % 3] >= o[3 + face % 3]:
                    continue
                box = ta.decode(pack(unord16(o)))
                meets, misses = ta.segment_meets_box(rays, idx, box[:3], box[3:], bounded=False)
                if (misses & aud[idx]).sum() >= 2 and (meets & aud[idx]).sum() >= 2:
                    bad = bvh4.copy()
                    bad[1 + 8 * node: 4 + 8 * node] = pack(unord16(o))
                    return bad, int(node), idx, box
    raise AssertionError("no node to damage")


def test_a_shrunk_box_loses_exactly_the_rays_that_miss_it(rt, gpu_ctx):
    """The audit bites on the device: one internal box of a read-back tree shrunk, installed with set_bvh4.  The lists lose exactly the
    triangles whose through ray certainly misses the shrunk box and keep those whose ray certainly meets it; nothing they still list is
    a phantom or malformed.  Not a fault test: a damaged box only loses hits."""
    tris = rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 20000)
    gpu_ctx.set_triangles(tris)
    gpu_ctx.build_bvh(1)
    rays = ta.through_rays(tris)
    bad, node, idx, box = shrink_case(tris, gpu_ctx.read_bvh4().copy(), rays)
    r = ta.verify_bvh4(tris, bad)
    assert r.stale.tolist() == [node] and not r.stale_loose[0] and not r.errors
    gpu_ctx.set_bvh4(bad)
    meets, misses = ta.segment_meets_box(rays, idx, box[:3], box[3:], bounded=False)
    for simple in ta.KERNELS:
        counts = gpu_ctx.count_hits(rays.O, rays.D, simple=simple)
        j = ta.judge_hits(tris, rays, gpu_ctx.list_hits(rays.O, rays.D, simple=simple), gpu_ctx.list_hits(rays.O, rays.D, sort=True, simple=simple), counts)
        lost = set(j.lost.tolist())
        must = set(idx[misses & j.auditable[idx]].tolist())
        print("shrunk box %d simple %d: %d rays must lose their triangle, %d must keep it, %d lost" % (node, simple, len(must), int(meets.sum()), len(lost)))
        assert must and must <= lost and not lost & set(idx[meets].tolist()) and lost <= set(idx.tolist()), (simple, len(must), len(lost))
        assert len(j.phantom) == 0 and len(j.malformed) == 0 and len(j.values_off) == 0
        assert set(j.lost_tris.tolist()) <= set(r.outside["tri"].tolist())          # every loss is attributed to the damaged node
        with pytest.raises(AssertionError, match="lost triangles.*%d" % node):
            ta.assert_point_judged(j, "shrunk box", r)
