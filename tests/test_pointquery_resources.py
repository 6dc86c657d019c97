"""What the compiler made of the closest-point kernels (pt_pointquery.hip), pinned -- compile-only, like test_rayquery_resources.py."""
import os
import re

import pytest

from kres import CSRC, HIPCC, resources

WAVES_PER_SIMD = 6          # pt_kernels.h PT_PQ_WAVES_PER_SIMD: what the launch grid of closest_points_kernel assumes


@pytest.mark.skipif(HIPCC is None, reason="hipcc is missing")
def test_pointquery_kernels_registers_scratch_and_occupancy():
    seen = resources("resource-usage-pointquery")
    persistent = {k: v for k, v in seen.items() if k.startswith("_ZN3ptk21closest_points_kernel")}
    simple = {k: v for k, v in seen.items() if k.startswith("_ZN3ptk28closest_points_simple_kernel")}
    brute = {k: v for k, v in seen.items() if k.startswith("_ZN3ptk27closest_points_brute_kernel")}
    assert len(persistent) == 1 and len(simple) == 2 and len(brute) == 2 and len(seen) == 5, sorted(seen)
    with open(os.path.join(CSRC, "pt_kernels.h")) as f:
        assert re.search(r"#define PT_PQ_WAVES_PER_SIMD %d\b" % WAVES_PER_SIMD, f.read())
    for f in persistent.values():
        # the hot path, pinned as DESIGN.md section 15 states it: 60 VGPRs, no scratch, no spills, the 12-entry LDS stack of one wavefront
        # (6 KB: 26 wavefronts per CU fit in 160 KB, six per SIMD)
        assert f["VGPRs"] == 60 and f["AGPRs"] == 0, f
        assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, f
        assert f["LDS Size [bytes/block]"] == 12 * 64 * 8, f
        assert f["Occupancy [waves/SIMD]"] >= WAVES_PER_SIMD, f
    for f in simple.values():
        # the A/B and counting kernel: the 64-entry private stack (512 B per lane, plus the frame's alignment) is its only scratch use
        assert f["VGPRs"] <= 64 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, f
        assert 512 <= f["ScratchSize [bytes/lane]"] <= 544, f
        assert f["Occupancy [waves/SIMD]"] == 8, f
    for f in brute.values():
        # 256 triangle records of three 16-byte pieces per workgroup in LDS
        assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, f
        assert f["LDS Size [bytes/block]"] == 256 * 3 * 16 and f["Occupancy [waves/SIMD]"] == 8, f

