"""What the compiler made of the ambient-occlusion kernels (pt_occlusion.hip), pinned -- compile-only, like test_rayquery_resources.py.
occlusion_kernel is the persistent walk that trace_rays_kernel<true> and closest_points_kernel are too (pt_walk.h), instantiated in its own
translation unit; the kernels of pt_rayquery.hip and the megakernel keep their own lines (test_rayquery_resources.py,
test_kernel_resources.py), and this file adds no kernel to theirs."""

import pytest

from kres import HIPCC, resources


@pytest.mark.skipif(HIPCC is None, reason="hipcc is missing")
def test_occlusion_kernels_registers_scratch_and_occupancy():
    seen = resources("resource-usage-occlusion")
    persistent = {k: v for k, v in seen.items() if k.startswith("_ZN3ptk16occlusion_kernelE")}
    simple = {k: v for k, v in seen.items() if k.startswith("_ZN3ptk23occlusion_simple_kernel")}
    small = {k: v for k, v in seen.items() if k.startswith(("_ZN3ptk23occlusion_finish_kernel", "_ZN3ptk21occlusion_rays_kernel", "_ZN3ptk18hit_surfels_kernel"))}
    assert len(persistent) == 1 and len(simple) == 2 and len(small) == 3 and len(seen) == 6, sorted(seen)
    for f in persistent.values():
        # required: no scratch, no spills, at least the 6 waves per SIMD the launch grid assumes (PT_OC_WAVES_PER_SIMD), the 12-entry LDS
        # stack of one wavefront.  Recorded as compiled: 70 VGPRs (the line of trace_rays_kernel: building the ray from the surfel costs no
        # register the walk needs), which the register file turns into 7 waves per SIMD.
        assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, f
        assert f["Occupancy [waves/SIMD]"] >= 6, f
        assert f["LDS Size [bytes/block]"] == 12 * 64 * 8, f
        assert f["VGPRs"] == 70 and f["AGPRs"] == 0, f
        assert f["Occupancy [waves/SIMD]"] == 7, f
    for f in simple.values():
        # traverse()'s 64-entry private stack (512 B per lane) is its only scratch use, as in trace_rays_simple_kernel
        assert f["VGPRs"] <= 64 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, f
        assert 512 <= f["ScratchSize [bytes/lane]"] <= 544, f
        assert f["Occupancy [waves/SIMD]"] == 8, f
    for f in small.values():
        assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0 and f["Occupancy [waves/SIMD]"] == 8, f
