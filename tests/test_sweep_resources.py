"""What the compiler made of the sphere-cast kernels (pt_sweep.hip), pinned -- compile-only, like test_box_resources.py.  sweep_kernel is the
persistent walk that the other batched queries are too (pt_walk.h), instantiated in its own translation unit with SweepWalk, a Q derived
from pt_rays.h::RayState; the simple kernel is pt_points.h::key_traverse, the brute-force kernel pt_walk.h::brute_records."""

import re

import pytest

from kres import CSRC, HIPCC, resources


def knob(name):
    with open(CSRC + "/pt_kernels.h") as f:
        return int(re.search(r"#define %s (\d+)" % name, f.read()).group(1))


@pytest.mark.skipif(HIPCC is None, reason="hipcc is missing")
def test_sweep_kernels_registers_scratch_and_occupancy():
    seen = resources("resource-usage-sweep")
    own = {k: v for k, v in seen.items() if k.startswith("_ZN3ptk")}
    walk = {k: v for k, v in own.items() if k.startswith("_ZN3ptk12sweep_kernelE")}
    simple = {k: v for k, v in own.items() if k.startswith("_ZN3ptk19sweep_simple_kernelILb")}
    brute = {k: v for k, v in own.items() if k.startswith("_ZN3ptk18sweep_brute_kernelILb")}
    # one persistent kernel; with and without the counters of the other two
    assert len(walk) == 1 and len(simple) == 2 and len(brute) == 2 and len(own) == 5, sorted(own)
    f = next(iter(walk.values()))
    # required: no scratch, no spills, no AGPRs, at least the waves per SIMD the launch grid assumes (PT_SW_WAVES_PER_SIMD), the LDS stack
    # of one wavefront (PT_SW_SHORT_STACK x 64 lanes x 8 bytes).  Recorded as compiled: 80 VGPRs, the most at which the register file
    # holds 6 waves per SIMD (512 / 80).  The lane holds RayState's fifteen values, the radius, the two shifted origins per axis and two
    # words of the result; the leaf arithmetic (the own box, the closest point, seven contact candidates) peaks above that.  Left alone
    # the allocator takes 84; the kernel asks for PT_SW_WAVES_PER_SIMD waves (amdgpu_waves_per_eu) and gets them without scratch.
    assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, f
    assert f["AGPRs"] == 0, f
    assert f["Occupancy [waves/SIMD]"] >= knob("PT_SW_WAVES_PER_SIMD"), f
    assert f["LDS Size [bytes/block]"] == knob("PT_SW_SHORT_STACK") * 64 * 8, f
    assert f["VGPRs"] == 80, f
    for f in simple.values():
        # the 64-entry private stack (512 B per lane) is the only scratch use, as in closest_points_simple_kernel
        assert f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0 and f["AGPRs"] == 0, f
        assert 512 <= f["ScratchSize [bytes/lane]"] <= 544, f
    for f in brute.values():
        # 256 records of three 16-byte pieces in LDS
        assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0 and f["AGPRs"] == 0, f
        assert f["LDS Size [bytes/block]"] == 256 * 3 * 16, f
