#!/usr/bin/env python3
"""Pins of the host twins' output (no GPU): per case the sha256 of the output bytes and the five counters, written to
tests/golden/twin_pins.json.  Run it on the commit whose output is to be held -- before a change to pt_host.cpp or to a header the twins
compile that is meant to leave every bit as it was -- and tests/test_twin_pins.py then holds every later commit to the file, with the
cases this module builds.

Twins: count_hits, contains, list_hits (unsorted, sorted, and sorted with a capacity below the total), occlusion_rays_host,
closest_points, radius_search, box_search, sweep_spheres and nearest_k: every user of pt_host.cpp's walk.
Trees: the comb (tests/scenes.py: the walks run into the 64-entry cap; asserted here: drops > 0, max stack 64), the spoiled tree
(out-of-range leaves and degenerate slots), the tetrahedron and soup1k at build level 0; per geometry also the brute-force route.
Items: N per case from the recipes of the case modules under tests/, the first few replaced by items that are not walked (a NaN in the
origin or the direction, t_max <= 0, r_max <= 0, an inverted box).  The counters are sums and maxima over the twins' workers, so they do
not depend on the thread count.

Build twins (the arithmetic of pt_bounds.h): morton_sort, the collapse at build levels 0 and 1, build_bvh2_ploc, bvh2_to_bvh4_wide,
refit_bvh4, refit_bvh2 and bvh4_cost over the tetrahedron, soup1k and a hostile soup (hostile_geometry: signed zeros, f16 subnormals,
coordinates beyond +-65504, an infinite and a NaN vertex, exact area ties); the LBVH2 they start from is the oracle's.

    python tools/twin_pins.py [--out tests/golden/twin_pins.json]
"""
import argparse
import hashlib
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import box_cases  # noqa: E402
import crossing_cases as cc  # noqa: E402
import knn_cases  # noqa: E402
import radius_cases  # noqa: E402
import sweep_cases  # noqa: E402

PINS = os.path.join(ROOT, "tests", "golden", "twin_pins.json")
N = 512
K = 5
SAMPLES = 3
COUNTERS = ("rays_closest", "nodes_examined", "tris_tested", "stack_drops", "max_stack")
TREES = ("comb", "spoiled", "tetra", "soup1k")


def tree_of(rt, orc, name, tris):
    if name == "comb":
        return cc.comb_tree()
    if name == "spoiled":
        return cc.spoiled_tree(rt, orc, tris)
    return cc.host_trees(rt, orc, tris, 0)[1]


def items_of(rt, name, tris):
    """The item sets of one geometry: rays, points (r_max drawn, and +inf), boxes, sweeps; in each the first few are not walked."""
    nan = np.float32(np.nan)
    rays = cc.ray_set(rt, tris, N, 11)
    points = radius_cases.point_records(rt, tris, n=N)
    far = knn_cases.point_records(rt, tris, "inf", n=N)
    if name == "comb":                                   # the items that run the walks into the cap
        rays[N // 2:] = cc.comb_rays(rt, N - N // 2, 3)
        far[N // 2:] = knn_cases.comb_points(rt, N - N // 2)
    rays[0, 0] = nan; rays[1, 5] = nan; rays[2, 3] = 0.0; rays[3, 3] = -1.0
    for p in (points, far):
        p[0, 1] = nan; p[1, 3] = 0.0; p[2, 3] = -1.0
    boxes = box_cases.box_records(rt, tris, n=N)
    boxes[0, 2] = nan; boxes[1, 0], boxes[1, 4] = boxes[1, 4] + 1.0, boxes[1, 0]
    sweeps = sweep_cases.sweep_set(rt, tris, N, 5)
    sweeps[0, 1] = nan; sweeps[1, 4] = nan; sweeps[2, 3] = 0.0; sweeps[3, 7] = -1.0; sweeps[4, 4:7] = 0.0
    return dict(rays=rays, points=points, far=far, boxes=boxes, sweeps=sweeps)


def surfels(rt):
    rng = np.random.default_rng(29)
    p = rng.uniform(-1, 1, (N, 3)).astype(np.float32)
    n = rng.normal(size=(N, 3)); n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    n[5] = (0, 0, 1); n[6] = (0, 0, -1); n[7] = (1, 0, 0)
    sf = rt.pack_surfels(p, n, rng.uniform(0.1, 2.0, N).astype(np.float32))
    sf[0, 0] = np.nan; sf[1, 6] = np.nan; sf[2, 3] = 0.0; sf[3, 3] = -2.0; sf[4, 3] = np.nan
    return sf


def route_cases(rt, label, tris, b4, it):
    """The cases of one geometry over one route: the tree b4, or brute force (b4 None)."""
    kw = dict(stats=True, brute_force=b4 is None)

    def short_lists():
        total = int(rt.list_hits_bvh4(tris, b4, it["rays"], brute_force=b4 is None)[0][-1])
        assert total >= 2, (label, total)
        return rt.list_hits_bvh4(tris, b4, it["rays"], sort=True, capacity=total // 2, **kw)
    out = [("count_hits", lambda: rt.count_hits_bvh4(tris, b4, it["rays"], **kw)),
           ("list_hits", lambda: rt.list_hits_bvh4(tris, b4, it["rays"], **kw)),
           ("list_hits_sorted", lambda: rt.list_hits_bvh4(tris, b4, it["rays"], sort=True, **kw)),
           ("list_hits_sorted_short", short_lists),
           ("closest_points", lambda: rt.closest_points_bvh4(tris, b4, it["far"], **kw)),
           ("radius_search", lambda: rt.radius_search_bvh4(tris, b4, it["points"], **kw)),
           ("box_search", lambda: rt.box_search_bvh4(tris, b4, it["boxes"], **kw)),
           ("sweep_spheres", lambda: rt.sweep_spheres_bvh4(tris, b4, it["sweeps"], **kw)),
           ("nearest_k", lambda: rt.nearest_k_bvh4(tris, b4, it["far"], K, **kw))]
    if b4 is not None:                                   # (pt_contains_bvh4 has no brute-force route)
        out.append(("contains", lambda: rt.contains_bvh4(tris, b4, it["points"], samples=SAMPLES, seed=5, index_base=4294967000, stats=True)))
    return [("%s/%s" % (label, twin), run) for twin, run in out]


def cases(rt, orc):
    """[(name, run)]: run() returns the twin's results with the counters dict in last place (None where the twin has none)."""
    out = [("occlusion_rays", lambda: (rt.occlusion_rays_host(surfels(rt), SAMPLES, seed=7, bias=1e-3, index_base=4294967000), None))]
    for name in TREES:
        tris = cc.geometry(rt, name)
        it = items_of(rt, name, tris)
        out += route_cases(rt, name + "/walk", tris, tree_of(rt, orc, name, tris), it)
        out += route_cases(rt, name + "/brute", tris, None, it)
    return out + build_cases(rt, orc)


BUILD_GEOMETRIES = ("tetra", "soup1k", "hostile")
HOSTILE_N, HOSTILE_SEED = 300, 41


def hostile_geometry(n=HOSTILE_N, seed=HOSTILE_SEED):
    """A soup of n triangles with what the scenes are thin in, each in a known triangle: 0: +0 and -0 coordinates; 1: magnitudes of about
    1e-6, f16 subnormals; 2: a coordinate above 65504; 3: one below -65504; 4: an infinite vertex; 5: a NaN vertex; 6..9 and 10..13: two
    groups of four equal triangles at offsets that are powers of two, so that the union of 6 and 7 has exactly the area of the union of 8 and 9
    (and 10, 11 that of 12, 13): ties in PLOC's key and in the area-guided collapse."""
    t = cc.random_soup(n, seed).reshape(n, 3, 3)
    t[0] = [[0.0, -0.0, 0.25], [-0.0, 0.0, 0.25], [0.0, 0.25, -0.0]]
    t[1] = [[1e-6, -2e-6, 3e-6], [-1e-6, 2e-6, -3e-6], [5e-7, 6e-8, -6e-8]]
    t[2, 0, 0] = 70000.0
    t[3, 1, 1] = -70000.0
    t[4, 2, 2] = np.inf
    t[5, 0, 1] = np.nan
    shape = np.array([[0.0, 0.0, 0.0], [0.125, 0.0, 0.0625], [0.0, 0.125, 0.03125]], np.float32)
    for first, origin in ((6, (2.0, 2.0, 2.0)), (10, (-4.0, 2.0, -2.0))):
        for k, off in enumerate(((0.0, 0.0, 0.0), (0.25, 0.0, 0.0), (0.0, 0.0, 1.0), (0.25, 0.0, 1.0))):
            t[first + k] = shape + np.array(origin, np.float32) + np.array(off, np.float32)
    return t.reshape(-1)


def build_cases(rt, orc):
    """The build and refit twins over BUILD_GEOMETRIES; the refits take each triangle's successor as its new vertices (no arithmetic, so
    the hostile values stay what they are)."""
    out = []
    for name in BUILD_GEOMETRIES:
        tris = hostile_geometry() if name == "hostile" else cc.geometry(rt, name)
        n = tris.size // 9
        moved = np.roll(tris.reshape(n, 9), -1, axis=0).reshape(-1)
        b2 = orc.build_lbvh2(tris)
        b4 = rt.collapse_bvh2_to_bvh4_accel(b2, n, 0)[0]
        twins = [("morton_sort", lambda tris=tris: rt.morton_sort(tris)),
                 ("collapse_accel0", lambda b2=b2, n=n: rt.collapse_bvh2_to_bvh4_accel(b2, n, 0)),
                 ("collapse_accel1", lambda b2=b2, n=n: rt.collapse_bvh2_to_bvh4_accel(b2, n, 1)),
                 ("build_bvh2_ploc", lambda tris=tris: (rt.build_bvh2_ploc(tris),)),
                 ("bvh2_to_bvh4_wide", lambda b2=b2: (rt.bvh2_to_bvh4_wide(b2),)),
                 ("refit_bvh4", lambda moved=moved, b4=b4: (rt.refit_bvh4(moved, b4),)),
                 ("refit_bvh2", lambda moved=moved, b2=b2: (rt.refit_bvh2(moved, b2),)),
                 ("bvh4_cost", lambda b4=b4: (np.float64(rt.bvh4_cost(b4)),))]
        out += [("build/%s/%s" % (name, twin), lambda run=run: tuple(np.asarray(a) for a in run()) + (None,)) for twin, run in twins]
    return out


def pin_of(result):
    *arrays, st = result
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return dict(sha256=h.hexdigest(), counters=None if st is None else [int(st[k]) for k in COUNTERS])


def pins(rt, orc):
    got = {name: pin_of(run()) for name, run in cases(rt, orc)}
    for twin in ("count_hits", "list_hits", "closest_points", "nearest_k"):        # the comb reaches the cap in the ray walk and the point walk
        c = got["comb/walk/" + twin]["counters"]
        assert c[3] > 0 and c[4] == 64, (twin, c)
    return got


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=PINS)
    args = ap.parse_args()
    import orc as orc_mod
    got = pins(importlib.import_module("raytracer-public_amd"), orc_mod.load())
    with open(args.out, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s" % (len(got), args.out))


if __name__ == "__main__":
    main()
