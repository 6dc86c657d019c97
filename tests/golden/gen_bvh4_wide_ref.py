#!/usr/bin/env python3
"""Records what the reference's BVH2 -> BVH4_wide converter (its tests/test.cpp, compiled by `make -C oracle ref` into
oracle/_ref/bvh4_wide_ref) writes for the oracle's LBVH2 of the seeded triangle soups of
tests/test_oracle_golden.py::test_bvh4_wide_matches_reference_binary, so that the test runs without that binary.

usage: python3 tests/golden/gen_bvh4_wide_ref.py      (after `make -C oracle all ref`)
-> tests/golden/bvh4_wide_ref_golden.npz: bvh2_<n> (the input, BVH2.bin words) and wide_<n> (BVH4_wide.bin words), uint32
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import orc as orc_mod  # noqa: E402

SIZES = [1, 2, 4, 37, 1000]
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "bvh4_wide_ref")


def main():
    orc = orc_mod.load()
    out = {}
    for n in SIZES:
        rng = np.random.default_rng(n)
        tris = (rng.random((n, 9), dtype=np.float32) * 2 - 1).astype(np.float32)
        bvh2 = orc.build_lbvh2(tris)
        with tempfile.TemporaryDirectory() as d:
            a, b = os.path.join(d, "BVH2.bin"), os.path.join(d, "BVH4_wide.bin")
            bvh2.tofile(a)
            subprocess.check_call([REF_BIN, a, b], stdout=subprocess.DEVNULL)
            out["bvh2_%d" % n] = np.asarray(bvh2, np.uint32)
            out["wide_%d" % n] = np.fromfile(b, dtype=np.uint32)
    np.savez_compressed(os.path.join(HERE, "bvh4_wide_ref_golden.npz"), **out)


if __name__ == "__main__":
    main()
