"""The surface of the two bindings above the C ABI, which the shared query routes must leave as it was: the signatures and names of the Python
package, its numpy front end (every form of a record batch gives the words of the pack_* records and leaves the caller's array alone), and the
names the N-API addon exports.  No GPU: the numpy front end is exercised through the host twins with brute_force=True."""
import inspect
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import crossing_cases as cc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "raytracer-public_amd", "napi", "mi355pt.node")

CONTEXT_SIGNATURES = {
    "trace_rays": "(self, origins, directions=None, t_max=None, any_hit=False, stats=False, simple=False)",
    "trace_rays_device": "(self, rays_ptr, n, hits_ptr, flags=0)",
    "closest_points": "(self, points, r_max=None, stats=False, simple=False, brute_force=False)",
    "closest_points_device": "(self, ptr, n, out_ptr, flags=0)",
    "sweep_spheres": "(self, origins, directions=None, radius=None, t_max=None, stats=False, simple=False, brute_force=False)",
    "sweep_spheres_device": "(self, ptr, n, out_ptr, flags=0)",
    "occlusion": "(self, surfels, samples, seed=0, bias=0.0001, index_base=0, stats=False, simple=False)",
    "occlusion_device": "(self, surfels_ptr, n, params, out_ptr)",
    "occlusion_rays": "(self, surfels, samples, seed=0, bias=0.0001, index_base=0)",
    "occlusion_rays_device": "(self, surfels_ptr, n, params, rays_ptr)",
    "hit_surfels": "(self, rays, hits, r_max=inf)",
    "hit_surfels_device": "(self, rays_ptr, hits_ptr, n, r_max, surfels_ptr)",
    "count_hits": "(self, origins, directions=None, t_max=None, stats=False, simple=False, brute_force=False)",
    "count_hits_device": "(self, rays_ptr, n, counts_ptr, flags=0)",
    "contains": "(self, points, samples=3, seed=0, index_base=0, stats=False, simple=False)",
    "contains_device": "(self, points_ptr, n, params, out_ptr)",
    "signed_distance": "(self, points, r_max=None, samples=3, seed=0, index_base=0, simple=False)",
    "signed_distance_device": "(self, points_ptr, n, params, out_ptr)",
    "radius_count": "(self, points, r_max=None, stats=False, simple=False, brute_force=False)",
    "radius_count_device": "(self, points_ptr, n, counts_ptr, flags=0)",
    "radius_search": "(self, points, r_max=None, capacity=None, stats=False, simple=False, brute_force=False)",
    "radius_search_device": "(self, points_ptr, n, offsets_ptr, entries_ptr, capacity, flags=0)",
    "box_count": "(self, lo, hi=None, stats=False, simple=False, brute_force=False)",
    "box_count_device": "(self, boxes_ptr, n, counts_ptr, flags=0)",
    "box_search": "(self, lo, hi=None, capacity=None, stats=False, simple=False, brute_force=False)",
    "box_search_device": "(self, boxes_ptr, n, offsets_ptr, entries_ptr, capacity, flags=0)",
    "list_hits": "(self, origins, directions=None, t_max=None, capacity=None, sort=False, stats=False, simple=False, brute_force=False)",
    "list_hits_device": "(self, rays_ptr, n, offsets_ptr, hits_ptr, capacity, flags=0)",
    "nearest_k": "(self, points, k, r_max=None, stats=False, simple=False, brute_force=False)",
    "nearest_k_device": "(self, ptr, n, k, out_ptr, flags=0)",
}
MODULE_SIGNATURES = {
    "closest_points_bvh4": "(tris, bvh4, points, r_max=None, stats=False, simple=False, brute_force=False)",
    "sweep_spheres_bvh4": "(tris, bvh4, origins, directions=None, radius=None, t_max=None, stats=False, simple=False, brute_force=False)",
    "count_hits_bvh4": "(tris, bvh4, origins, directions=None, t_max=None, stats=False, simple=False, brute_force=False)",
    "radius_search_bvh4": "(tris, bvh4, points, r_max=None, capacity=None, stats=False, simple=False, brute_force=False)",
    "box_search_bvh4": "(tris, bvh4, lo, hi=None, capacity=None, stats=False, simple=False, brute_force=False)",
    "list_hits_bvh4": "(tris, bvh4, origins, directions=None, t_max=None, capacity=None, sort=False, stats=False, simple=False, brute_force=False)",
    "nearest_k_bvh4": "(tris, bvh4, points, k, r_max=None, stats=False, simple=False, brute_force=False)",
    "contains_bvh4": "(tris, bvh4, points, samples=3, seed=0, index_base=0, stats=False, simple=False)",
    "pack_rays": "(origins, directions, t_max=None)",
    "pack_points": "(points, r_max=None)",
    "pack_sweeps": "(origins, directions, radius, t_max=None)",
    "pack_boxes": "(lo, hi)",
    "pack_surfels": "(points, normals, r_max=None)",
}
PUBLIC_NAMES = """Context EXPORTS EXPOSE_GATES Group LIB_PATH PLAN_FIELDS PRIM_NONE PT_ACCEL_AREA_COLLAPSE PT_ACCEL_PLOC PT_ACCEL_REFERENCE
PT_BOX_BRUTE_FORCE PT_BOX_SIMPLE_KERNEL PT_BOX_STATS PT_CLOSEST_BRUTE_FORCE PT_CLOSEST_SIMPLE_KERNEL PT_CLOSEST_STATS PT_CONTAIN_SIMPLE_KERNEL
PT_CONTAIN_STATS PT_COUNT_BRUTE_FORCE PT_COUNT_SIMPLE_KERNEL PT_COUNT_STATS PT_FLAG_BRUTE_FORCE PT_FLAG_COMPACT PT_FLAG_SIMPLE_KERNEL PT_FLAG_STATS
PT_GROUP_TRANSPORT_COPY PT_GROUP_TRANSPORT_RCCL PT_HITS_BRUTE_FORCE PT_HITS_SIMPLE_KERNEL PT_HITS_SORTED PT_HITS_STATS PT_MODE_PATH
PT_MODE_REFERENCE PT_MODE_REFERENCE_PACKET PT_NEAREST_BRUTE_FORCE PT_NEAREST_MAX_K PT_NEAREST_SIMPLE_KERNEL PT_NEAREST_STATS
PT_OCCLUSION_SIMPLE_KERNEL PT_OCCLUSION_STATS PT_RADIUS_BRUTE_FORCE PT_RADIUS_SIMPLE_KERNEL PT_RADIUS_STATS PT_SWEEP_BRUTE_FORCE
PT_SWEEP_SIMPLE_KERNEL PT_SWEEP_STATS PT_TRACE_ANY_HIT PT_TRACE_SIMPLE_KERNEL PT_TRACE_STATS PathTracer PtAccumInfo PtBox PtClosest PtContainParams
PtContainment PtError PtHit PtOcclusion PtOcclusionParams PtOverlap PtPoint PtRay PtRenderParams PtStats PtSurfel PtSweep SCENE_DRAGON_CLASS
SCENE_SPONZA_CLASS _TORCH_FIRST _aligned_zeros lib occlusion_rays_host exposure_flags_host focal_aspect""".split()
ADDON_EXPORTS = [
    "boxCount", "boxSearch", "buildBVH", "bvh4Wide", "bvhCost", "cameraRay", "closestPoints", "collapse", "computeBVH2Sizing", "computeBVH4Sizing",
    "contains", "countHits", "create", "destroy", "flush", "getStats", "groupBoxCount", "groupBoxSearch", "groupBuildBVH", "groupBvhCost",
    "groupClosestPoints", "groupContains", "groupCountHits", "groupCreate", "groupDestroy", "groupFlush", "groupHitSurfels", "groupListHits",
    "groupNearestK", "groupOcclusion", "groupRadiusCount", "groupRadiusSearch", "groupReadBVH2", "groupReadRGBA8", "groupReadRadiance",
    "groupReadTonemapped", "groupRender", "groupSetBVH2", "groupSetBVH4", "groupSetBatch", "groupSetTriangles", "groupSignedDistance", "groupSize",
    "groupSweepSpheres", "groupSynchronize", "groupTraceRays", "groupUpdateTriangles", "hitSurfels", "lastRenderMs", "listHits", "mortonSort",
    "nearestK", "occlusion", "proceduralScene", "radiusCount", "radiusSearch", "readAccumulation", "readBVH2", "readBVH4", "readRGBA8", "readRadiance",
    "readTonemapped", "readU32File", "render", "restoreAccumulation", "sceneInfo", "setBVH2", "setBVH4", "setBatch", "setSpheres", "setTriangles",
    "signedDistance", "sweepSpheres", "synchronize", "traceRays", "updateTriangles", "version", "writeU32File"]
N = 16


def test_signatures_and_docstrings_are_the_published_ones(rt):
    for name, want in CONTEXT_SIGNATURES.items():
        f = getattr(rt.Context, name)
        assert inspect.isfunction(f) and str(inspect.signature(f)) == want, name
        assert f.__doc__ and f.__doc__.strip(), name
    for name, want in MODULE_SIGNATURES.items():
        f = getattr(rt, name)
        assert inspect.isfunction(f) and str(inspect.signature(f)) == want, name
        assert f.__doc__ and f.__doc__.strip(), name


def test_public_names_are_attributes_of_the_package(rt):
    missing = [n for n in PUBLIC_NAMES + list(MODULE_SIGNATURES) if not hasattr(rt, n)]
    assert not missing, missing
    assert "pt_sweep_spheres_host" in rt.EXPORTS and rt.lib.pt_version().decode()


def words(res):
    """the results of a twin as a list of integer arrays (float32 columns as their bits)"""
    return [a.view(np.uint32) if a.dtype == np.float32 else a for a in (res if isinstance(res, tuple) else (res,))]


def same(got, want):
    got, want = words(got), words(want)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)


@pytest.fixture(scope="module")
def batch(rt):
    """16 records of every kind about the tetrahedron: what the split-column calls take, and the pack_* records of the same"""
    rng = np.random.default_rng(11)
    org = rng.uniform(-1.6, 1.6, (N, 3)).astype(np.float32)
    direction = (rng.uniform(-0.4, 0.4, (N, 3)) - org).astype(np.float32)            # roughly at the tetrahedron
    t_max = rng.uniform(0.5, 3.0, N).astype(np.float32); t_max[::5] = np.inf
    r_max = rng.uniform(0.2, 2.5, N).astype(np.float32)
    radius = rng.uniform(0.0, 0.4, N).astype(np.float32)
    lo = rng.uniform(-1.2, 0.5, (N, 3)).astype(np.float32)
    hi = (lo + rng.uniform(0.1, 1.5, (N, 3))).astype(np.float32)
    tris = cc.geometry(rt, "tetra")
    return {
        # kind: (the twin on the tetrahedron, split arguments, split keywords, packed records, {override keyword: (column, value)}, packer)
        "rays": (lambda *a, **k: rt.list_hits_bvh4(tris, None, *a, brute_force=True, **k), (org, direction), {"t_max": t_max},
                 rt.pack_rays(org, direction, t_max), {"t_max": (3, 1.75)}, lambda a: rt._ray_records(a, None, None)),
        "points": (lambda *a, **k: rt.closest_points_bvh4(tris, None, *a, brute_force=True, **k), (org,), {"r_max": r_max},
                   rt.pack_points(org, r_max), {"r_max": (3, 0.9)}, lambda a: rt._point_records(a, None)),
        "sweeps": (lambda *a, **k: rt.sweep_spheres_bvh4(tris, None, *a, brute_force=True, **k), (org, direction), {"radius": radius, "t_max": t_max},
                   rt.pack_sweeps(org, direction, radius, t_max), {"t_max": (3, 1.75), "radius": (7, 0.25)}, lambda a: rt._sweep_records(a, None, None, None)),
        "boxes": (lambda *a, **k: rt.box_search_bvh4(tris, None, *a, brute_force=True, **k), (lo, hi), {},
                  rt.pack_boxes(lo, hi), {}, lambda a: rt._box_records(a, None)),
    }


def packed_forms(rt, rec):
    """the same records as the caller may hold them: (name, array, whether the C side can read it in place)"""
    aligned = rt._aligned_zeros(rec.shape, np.float32); aligned[...] = rec
    shifted = rt._aligned_zeros((rec.size + 4,), np.float32)[1: 1 + rec.size].reshape(rec.shape); shifted[...] = rec
    wide = rt._aligned_zeros((2 * rec.shape[0], rec.shape[1]), np.float32); wide[::2] = rec; wide[1::2] = 7.0
    assert aligned.ctypes.data % 16 == 0 and shifted.ctypes.data % 16 == 4 and not wide[::2].flags.c_contiguous
    return [("aligned", aligned, True), ("misaligned", shifted, False), ("every second row", wide[::2], False), ("float64", rec.astype(np.float64), False)]


@pytest.mark.parametrize("kind", ["rays", "points", "sweeps", "boxes"])
def test_every_form_of_a_batch_gives_the_words_of_the_packed_records(rt, batch, kind):
    twin, split, split_kw, rec, overrides, _ = batch[kind]
    want = twin(rec)
    assert any(a.dtype == np.uint32 and (a != cc.MISS).sum() >= N // 4 for a in want)   # the batch does meet the mesh (prim is the uint32 column)
    before = [a.copy() for a in split]
    same(twin(*split, **split_kw), want)
    assert all(np.array_equal(a, b) for a, b in zip(split, before))
    for name, arr, _ in packed_forms(rt, rec):
        kept = arr.copy()
        same(twin(arr), want)
        assert arr.tobytes() == kept.tobytes(), name                                  # the caller's array holds its original bits
        for key, (column, value) in overrides.items():
            changed = rec.copy(); changed[:, column] = value
            same(twin(arr, **{key: value}), twin(changed))
            assert arr.tobytes() == kept.tobytes(), (name, key)


@pytest.mark.parametrize("kind", ["rays", "points", "sweeps", "boxes"])
def test_aligned_records_pass_through_without_a_copy(rt, batch, kind):
    _, _, _, rec, _, packer = batch[kind]
    for name, arr, in_place in packed_forms(rt, rec):
        out = packer(arr)
        assert np.shares_memory(out, arr) == in_place, name
        assert out.ctypes.data % 16 == 0 and out.flags.c_contiguous and out.dtype == np.float32 and np.array_equal(out, rec), name
    if rec.shape[1] == 8:
        arr = packed_forms(rt, rec)[0][1]
        assert np.shares_memory(rt._records8(arr, "records"), arr)


def test_an_override_works_on_a_copy(rt, batch):
    rays, points = packed_forms(rt, batch["rays"][3])[0][1], packed_forms(rt, batch["points"][3])[0][1]
    for out, arr in ((rt._ray_records(rays, None, 2.0), rays), (rt._point_records(points, 2.0), points),
                     (rt._sweep_records(rays, None, 0.5, None), rays), (rt._sweep_records(rays, None, None, 2.0), rays)):
        assert not np.shares_memory(out, arr)


@pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the built addon is missing")
def test_addon_exports_the_published_names():
    out = subprocess.check_output([NODE, "-e", "console.log(JSON.stringify(Object.keys(require(%s)).sort()))" % json.dumps(ADDON)], text=True, timeout=60)
    assert json.loads(out) == ADDON_EXPORTS
