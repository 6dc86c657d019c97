"""The host twins against their pinned output (no GPU): tests/golden/twin_pins.json holds, per case of tools/twin_pins.py, the sha256 of
the twin's output bytes and its five counters as the commit that wrote the file computed them.  A change to pt_host.cpp or to a header
the twins compile (pt_bounds.h, pt_raymath.h, pt_closest.h, pt_overlap.h, pt_sweep.h) that is meant to move no bit passes this as it stands; one that
is meant to move some regenerates the file with the tool and says so."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import twin_pins  # noqa: E402


@pytest.fixture(scope="module")
def pinned():
    with open(twin_pins.PINS) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def computed(rt, orc):
    return twin_pins.pins(rt, orc)


def test_the_cases_are_the_pinned_cases(pinned, computed):
    assert sorted(computed) == sorted(pinned)
    twins = {name.rsplit("/", 1)[-1] for name in pinned}
    assert twins >= {"count_hits", "contains", "list_hits", "list_hits_sorted", "list_hits_sorted_short", "occlusion_rays", "closest_points",
                     "radius_search", "box_search", "sweep_spheres", "nearest_k",
                     "morton_sort", "collapse_accel0", "collapse_accel1", "build_bvh2_ploc", "bvh2_to_bvh4_wide", "refit_bvh4", "refit_bvh2",
                     "bvh4_cost"}
    for tree in twin_pins.TREES:
        assert {tree + "/walk/count_hits", tree + "/brute/count_hits"} <= set(pinned)
    for geometry in twin_pins.BUILD_GEOMETRIES:
        assert {"build/%s/morton_sort" % geometry, "build/%s/refit_bvh2" % geometry} <= set(pinned)


def test_every_twin_computes_its_pinned_bytes_and_counters(pinned, computed):
    differing = [name for name in sorted(pinned) if computed[name] != pinned[name]]
    for name in differing:
        print("%s: pinned %s, computed %s" % (name, pinned[name], computed[name]))
    assert not differing
