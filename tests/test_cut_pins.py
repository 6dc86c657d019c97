"""The host twin of the plane-cut query against its pinned output (no GPU): tests/golden/cut_pins.json holds, per case, the sha256 of
pt_cut_search_bvh4's output bytes (offsets, prim, code, t0, t1) and its five counters as the commit that wrote the file computed them.
The trees and the routes are those of tools/twin_pins.py -- the comb, the spoiled tree, the tetrahedron and soup1k at build level 0, each
walked and by brute force -- with 512 planes of cut_cases.plane_records, the first few replaced by records that are not walked and, on the
comb, the second half by planes that hold the z direction with the whole-scene window.  A change to pt_host.cpp, pt_cut.h or a header it
compiles that is meant to move no bit passes this as it stands; one that is meant to move some regenerates the file and says so:

    python tests/test_cut_pins.py [--out tests/golden/cut_pins.json]
"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import cut_cases as ctc  # noqa: E402
import twin_pins  # noqa: E402
from twin_pins import cc  # noqa: E402

PINS = os.path.join(ROOT, "tests", "golden", "cut_pins.json")


def planes_of(rt, name, tris):
    rec = ctc.plane_records(rt, tris, n=twin_pins.N - 32, beside=32)
    if name == "comb":                                    # the item that stacks most: it cuts every triangle, so every leaf passes
        rec[twin_pins.N // 2:] = ctc.vertical_planes(rt, tris, twin_pins.N - twin_pins.N // 2)
    rec[0, 1] = np.nan; rec[1, 3] = np.inf; rec[2, 10] = -np.inf
    rec[3, 0:3] = 0.0                                      # n = 0
    rec[4, 4] = rec[4, 8] + np.float32(1.0)                # lo > hi
    return rec


def pins(rt, orc):
    got = {}
    for name in twin_pins.TREES:
        tris = cc.geometry(rt, name)
        rec = planes_of(rt, name, tris)
        for route, b4 in (("walk", twin_pins.tree_of(rt, orc, name, tris)), ("brute", None)):
            got["%s/%s/cut_search" % (name, route)] = twin_pins.pin_of(rt.cut_search_bvh4(tris, b4, rec, stats=True, brute_force=b4 is None))
    return got


@pytest.fixture(scope="module")
def pinned():
    with open(PINS) as f:
        return json.load(f)


def test_the_twin_computes_its_pinned_bytes_and_counters(rt, orc, pinned):
    computed = pins(rt, orc)
    assert sorted(computed) == sorted(pinned) and len(pinned) == 2 * len(twin_pins.TREES)
    differing = [name for name in sorted(pinned) if computed[name] != pinned[name]]
    for name in differing:
        print("%s: pinned %s, computed %s" % (name, pinned[name], computed[name]))
    assert not differing
    for name, pin in pinned.items():                      # every case lists something, and counts its 512 planes
        assert pin["counters"][0] == twin_pins.N and pin["counters"][2] > 0, (name, pin)


if __name__ == "__main__":
    import argparse
    import importlib
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=PINS)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import orc as orc_mod
    got = pins(importlib.import_module("raytracer-public_amd"), orc_mod.load())
    with open(args.out, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s" % (len(got), args.out))
