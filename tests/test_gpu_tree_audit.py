"""Every triangle of every device tree through tests/treeaudit.py: the words of read_bvh4() / read_bvh2() through the containment proof, and
four rays aimed at every triangle through trace_rays -- the persistent kernel and simple=True, closest hit and any hit -- judged by float64
Moeller-Trumbore against that triangle alone.  Built trees of every accel level, the same trees refitted by update_triangles, installed
trees before and after an update, and C2 (871,414 triangles, about 3.5 M rays) and C4 (262,144) at full size, where the O(N) judge is the
only reference there can be.  No oracle: nothing here uses the `orc` fixture, and the trees that are installed are made by the device build
and the host twins of the collapse.

The megakernel's own traversal (pt_megakernel_loop.inc) is not reached by caller rays and this audit does not claim it: it stays covered by
the sampled pathref renders (tests/test_gpu_path_reference.py) and by bit equality with the other kernels over the same arena, whose triangle
records, packed references and boxes the aimed rays do go through.

One context per test, plain sequential launches, one process."""
import numpy as np
import pytest

import treeaudit as ta
from refit_cases import wave
from test_accel_host import DEGENERATE, degenerate
from test_gpu_path_reference import deform
from test_tree_audit import EDGE_SCENES, check_detection, check_family, edge_scene

pytestmark = pytest.mark.gpu

ACCELS = [0, 1, 2]
SOUPS = {1: 0, 2: 1, 3: 2, 4: 3, 5: 4, 64: 5, 65: 6, 777: 7, 30000: 5, 120000: 6}      # the sizes of the build tests
SCENE_SEED = 20260109


def built_and_refitted(ctx, tris, name, amp=0.1, capped=True, moves=("wave", "deform")):
    """build_bvh at every level; each tree as built, then refitted in place after the --animate wave and after the warp of
    test_gpu_path_reference.py (which moves most triangles somewhere else)."""
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1)
    moved = {"wave": wave(tris, amp, 3), "deform": deform(tris)}
    rays = {k: ta.aimed_rays(v) for k, v in dict(moved, built=tris).items() if k == "built" or k in moves}
    for accel in ACCELS:
        ctx.set_triangles(tris)
        ctx.build_bvh(accel)
        ta.audit_context(ctx, tris, "%s accel %d built" % (name, accel), capped=capped, rays=rays["built"])
        for what in moves:
            ctx.update_triangles(moved[what])
            ta.audit_context(ctx, moved[what], "%s accel %d after %s" % (name, accel, what), capped=capped, rays=rays[what])


@pytest.mark.parametrize("n", sorted(SOUPS))
def test_soups_built_and_refitted(gpu_ctx, n):
    built_and_refitted(gpu_ctx, ta.soup(n, SOUPS[n]), "soup %d" % n)


@pytest.mark.parametrize("kind", DEGENERATE)
def test_degenerate_families(gpu_ctx, kind):
    """Classed, not skipped (test_tree_audit.check_family says what each family is and why no cap can apply); refitted, they are held to
    everything but the caps."""
    for accel in ACCELS:
        check_family(gpu_ctx, kind, accel, ta.KERNELS)
    built_and_refitted(gpu_ctx, degenerate(kind), kind, capped=False)


@pytest.mark.parametrize("name", EDGE_SCENES)
def test_axis_aligned_translated_and_scaled(gpu_ctx, name):
    """Exactly axis-parallel rays over boxes that are flat in one axis; coordinates of 1,000 and of 27,000, where an f16 step is 0.5 and 16."""
    tris = edge_scene(name)
    assert np.abs(tris).max() < 30000
    built_and_refitted(gpu_ctx, tris, name)
    assert np.abs(deform(tris)).max() < 30000 and np.abs(wave(tris, 0.1, 3)).max() < 30000


@pytest.mark.parametrize("accel", ACCELS)
def test_eight_updates_and_a_cluster_collapsed_and_back(rt, gpu_ctx, accel):
    tris = rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 20000)
    gpu_ctx.set_triangles(tris)
    gpu_ctx.build_bvh(accel)
    built = gpu_ctx.read_bvh4()
    for k in range(8):
        moved = wave(tris, 0.04 * (k + 1), k)
        gpu_ctx.update_triangles(moved)
    ta.audit_context(gpu_ctx, moved, "dragon 20000 accel %d after eight updates" % accel)
    flat, pick = ta.collapse_cluster(tris, (0.1, 0.1, 0.1), tris.size // 9 // 150)
    gpu_ctx.update_triangles(flat)
    r4, js = ta.audit_context(gpu_ctx, flat, "dragon 20000 accel %d, a cluster collapsed to a point" % accel)
    for j in js.values():
        assert not j.auditable.reshape(-1, 4)[pick].any()                            # zero area: unhittable by the specification, classed so
    gpu_ctx.update_triangles(tris)
    assert np.array_equal(gpu_ctx.read_bvh4(), built)
    ta.audit_context(gpu_ctx, tris, "dragon 20000 accel %d restored" % accel)


@pytest.mark.parametrize("how", ["set_bvh4", "set_bvh4_wide", "set_bvh2", "set_bvh2_ploc"])
def test_installed_trees_before_and_after_an_update(rt, gpu_ctx, how):
    """Installed trees are held to what DESIGN.md section 14 promises: a BVH4_wide promotion keeps the BVH2's ids and boxes (nodes no path
    reaches, no pre-order, boxes by another rule) until its first update, after which every reachable box follows the BVH4's rules."""
    tris = rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 20000)
    n = tris.size // 9
    gpu_ctx.set_triangles(tris)
    gpu_ctx.build_bvh(0)
    lbvh2 = gpu_ctx.read_bvh2()                                                     # the device's LBVH2, installed again below
    gpu_ctx.set_triangles(tris)
    kw = dict(built=True, bvh2=False)
    if how == "set_bvh4":
        gpu_ctx.set_bvh4(rt.collapse_bvh2_to_bvh4_accel(lbvh2, n, 1)[0])
    elif how == "set_bvh4_wide":
        gpu_ctx.set_bvh4(rt.bvh2_to_bvh4_wide(lbvh2))
        kw = dict(built=False, bvh2=False)
    else:
        gpu_ctx.set_bvh2(rt.build_bvh2_ploc(tris) if how == "set_bvh2_ploc" else lbvh2)
        kw = dict(built=True, bvh2=True)
    r4, _ = ta.audit_context(gpu_ctx, tris, how, exact=how != "set_bvh4_wide", **kw)
    if how == "set_bvh4_wide":
        assert (r4.depth < 0).sum() > n // 20 and len(r4.stale) > n // 20                  # it is the tree this case means
    for what, moved in (("wave", wave(tris, 0.1, 2)), ("deform", deform(tris))):
        gpu_ctx.update_triangles(moved)
        ta.audit_context(gpu_ctx, moved, "%s after %s" % (how, what), **kw)


def test_damaged_trees_are_detected(rt, gpu_ctx):
    """The audit bites on the device too: a shrunk box, two swapped leaves and an enlarged box, installed with set_bvh4.  Not a fault test:
    like test_damaged_tree, a damaged tree only loses hits."""
    tris = rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 20000)
    gpu_ctx.set_triangles(tris)
    gpu_ctx.build_bvh(1)
    check_detection(gpu_ctx, tris, gpu_ctx.read_bvh4().copy(), ta.KERNELS)


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("config", ["C2", "C4"])
def test_full_size(rt, gpu_ctx, config, accel):
    """C2 (dragon-class, 871,414 triangles) and C4 (sponza-class interior, 262,144), built and refitted once: every triangle, about 3.5 M and
    1 M rays per kernel and hit type.  Brute force is out of reach here; the judge is O(rays)."""
    tris = rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 871414, SCENE_SEED) if config == "C2" else rt.procedural_scene(rt.SCENE_SPONZA_CLASS, 262144, SCENE_SEED)
    gpu_ctx.set_triangles(tris)
    gpu_ctx.build_bvh(accel)
    ta.audit_context(gpu_ctx, tris, "%s accel %d built" % (config, accel))
    moved = wave(tris, 0.02, 4)
    gpu_ctx.update_triangles(moved)
    ta.audit_context(gpu_ctx, moved, "%s accel %d refitted" % (config, accel))
