"""Every triangle of every device tree through the point and crossing-count queries (treeaudit.audit_points): closest_points, radius_count,
radius_search, nearest_k and count_hits, persistent and simple kernels, judged in float64 against that triangle and the reported ones alone.
The scenes, the refits and what is left out are those of tests/test_point_audit.py, which says why; here the trees are the device's --
built at every level, refitted by update_triangles, installed with set_bvh4 / set_bvh2 before and after an update.  After the kernels the
host twins answer the same points over the tree read back from the device: their judgements must show the same counts in every category.

One context per test, plain sequential launches, one process.  Nothing at full C2 or C4 size: the float64 judge is the cost."""
import numpy as np
import pytest

import treeaudit as ta
from refit_cases import wave
from test_gpu_path_reference import deform
from test_point_audit import ACCELS, NO_FAR_CLOSEST, SCENES, check_deformed_sponza, check_edge_of_domain, scene, states

pytestmark = pytest.mark.gpu

SMALL = [n for n in SCENES if n.startswith("soup") and int(n[4:]) < 1000]
LARGE = [n for n in SCENES if n not in SMALL and n != "sparse120000"]


def audit_device_and_twin(rt, ctx, tris, name, far_closest=True):
    """audit_points through both kernels of the device context, then through the host twins over the words the device holds: the bits are the
    same, so every judgement must count the same points in every category."""
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1)
    rays = ta.aimed_rays(tris)
    passes = [ta.near_points(rays, tris), ta.far_points(tris)]
    dev = ta.audit_points(ctx, tris, name, rays=rays, far_closest=far_closest, passes=passes)
    twin = ta.HostContext(rt, None)
    twin.set_triangles(tris)
    twin.set_bvh4(ctx.read_bvh4())
    host = ta.audit_points(twin, tris, name + " twin", rays=rays, kernels=[False], far_closest=far_closest, passes=passes)
    for (what, simple), js in dev.items():
        for q, j in js.items():
            assert j.counts() == host[what, False][q].counts(), (name, what, simple, q, j.counts(), host[what, False][q].counts())
    return dev


def run_states(rt, ctx, name, tris, accel, only=None):
    for what, now in states(name, tris):
        if what == "built":
            ctx.set_triangles(tris); ctx.build_bvh(accel)
        else:
            ctx.update_triangles(now)
        if only is None or what == only:
            audit_device_and_twin(rt, ctx, now, "%s accel %d %s" % (name, accel, what), (name, what) not in NO_FAR_CLOSEST)
        if what == only:
            break


@pytest.mark.parametrize("name", SMALL)
def test_small_soups_built_and_refitted(rt, gpu_ctx, name):
    """1 .. 777 triangles: a root that is a leaf, a single node, one block and several."""
    for accel in ACCELS:
        run_states(rt, gpu_ctx, name, scene(rt, name), accel)


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name", LARGE)
def test_scenes_built_and_refitted(rt, gpu_ctx, name, accel):
    run_states(rt, gpu_ctx, name, scene(rt, name), accel)


@pytest.mark.parametrize("what", ["built", "wave"])
@pytest.mark.parametrize("accel", [0, 2])
def test_sparse_soup_of_120000(rt, gpu_ctx, accel, what):
    """480,000 + 120,000 points per query and kernel."""
    run_states(rt, gpu_ctx, "sparse120000", scene(rt, "sparse120000"), accel, only=what)


def test_the_dense_soup_through_radius_and_counts(gpu_ctx):
    """soup(120000, 6) at size 0.2: not a scene for closest and k-nearest (tests/test_point_audit.py); radius and counts exclude nothing."""
    tris = ta.soup(120000, 6)
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh(0)
    rays = ta.aimed_rays(tris)
    for pts, rr in ((ta.near_points(rays, tris), rays), (ta.far_points(tris), None)):
        rec = pts.records()
        gpu_ctx.radius_count(rec, stats=True)
        assert gpu_ctx.stats()["stack_drops"] == 0
        for simple in ta.KERNELS:
            found = gpu_ctx.radius_search(rec, simple=simple)
            j = ta.judge_radius(tris, pts, found[0], found[1:], gpu_ctx.radius_count(rec, simple=simple))
            ta.assert_point_judged(j, "soup 120000 size 0.2 simple %d" % simple)
            if rr is not None:
                ta.assert_point_judged(ta.judge_counts(rr, gpu_ctx.count_hits(rr.O, rr.D, t_max=rr.t_max, simple=simple), tris), "soup 120000 size 0.2 simple %d" % simple)
    gpu_ctx.count_hits(rays.O, rays.D, t_max=rays.t_max, stats=True)
    assert gpu_ctx.stats()["stack_drops"] == 0


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
    moved = deform(tris)
    gpu_ctx.update_triangles(moved)
    audit_device_and_twin(rt, gpu_ctx, moved, "%s after deform" % how, far_closest=False)     # dragon-class after deform: 3.6 % (test_point_audit.NO_FAR_CLOSEST)


def test_edge_of_the_proven_domain(rt, gpu_ctx):
    """Vertices up to +-4, points out to +-32: both kernels and the twin against the brute-force kernel, bit for bit."""
    check_edge_of_domain(rt, gpu_ctx, ta.KERNELS)


def test_deformed_sponza_slivers(rt, gpu_ctx):
    """The scene the audit found (test_point_audit.check_deformed_sponza): nothing lost, the walk's bits are brute force's, and the deviations
    from float64 stay on the slivers and within what their aspect explains -- through both kernels and the brute-force kernel."""
    check_deformed_sponza(rt, gpu_ctx, ta.KERNELS)
