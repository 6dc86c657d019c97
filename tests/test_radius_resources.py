"""What the compiler made of the radius-query kernels (pt_radius.hip), pinned -- compile-only, like test_crossings_resources.py.
radius_kernel<FILL> is the persistent walk that the ray, point, occlusion and crossing queries are too (pt_walk.h), instantiated in its own
translation unit with its own Q (RadiusWalk); the simple and the brute-force kernel are instantiated from pt_region.h, the frame they
share with the box query (test_box_resources.py); pt_radius.hip holds the sphere policy, the __global__ wrappers, whose names and
variants are counted here, and the scan.
The translation unit also holds the scan's library kernels (hipcub::DeviceScan), whose number depends on the ROCm release: only the
project's own kernels are counted."""

import pytest

from kres import HIPCC, resources


@pytest.mark.skipif(HIPCC is None, reason="hipcc is missing")
def test_radius_kernels_registers_scratch_and_occupancy():
    seen = resources("resource-usage-radius")
    own = {k: v for k, v in seen.items() if k.startswith("_ZN3ptk")}
    walk = {k: v for k, v in own.items() if k.startswith("_ZN3ptk13radius_kernelILb")}
    simple = {k: v for k, v in own.items() if k.startswith("_ZN3ptk20radius_simple_kernelILb")}
    brute = {k: v for k, v in own.items() if k.startswith("_ZN3ptk19radius_brute_kernelILb")}
    # count and fill of the persistent kernel; count, count + stats and fill of the other two
    assert len(walk) == 2 and len(simple) == 3 and len(brute) == 3 and len(own) == 8, sorted(own)
    count = next(v for k, v in walk.items() if k.startswith("_ZN3ptk13radius_kernelILb0E"))
    fill = next(v for k, v in walk.items() if k.startswith("_ZN3ptk13radius_kernelILb1E"))
    for f, vgprs in ((count, 55), (fill, 57)):
        # required: no scratch, no spills, no AGPRs, at least the 6 waves per SIMD the launch grid assumes (PT_RD_WAVES_PER_SIMD), the
        # 12-entry LDS stack of one wavefront (PT_RD_SHORT_STACK x 64 lanes x 8 bytes).  Recorded as compiled: 55 VGPRs for the count walk
        # (closest_points_kernel's 60 less the best triangle and the moving best2), 57 for the fill walk (the 64-bit base and u, v of the
        # entry).  Both are below the 64 VGPRs at which the register file still holds 8 waves per SIMD; the 7 the compiler reports come from
        # the LDS stack: 6,144 B per one-wavefront workgroup, 26 workgroups in a CU's 160 KB, 6.5 per SIMD (PT_RD_SHORT_STACK sets it).
        assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, f
        assert f["AGPRs"] == 0, f
        assert f["Occupancy [waves/SIMD]"] >= 6, f
        assert f["LDS Size [bytes/block]"] == 12 * 64 * 8, f
        assert f["VGPRs"] == vgprs, f
    for f in simple.values():
        # the 64-entry private stack (512 B per lane) is the only scratch use, as in closest_points_simple_kernel
        assert f["VGPRs"] <= 64 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0 and f["AGPRs"] == 0, f
        assert 512 <= f["ScratchSize [bytes/lane]"] <= 544, f
        assert f["Occupancy [waves/SIMD]"] == 8, f
    for f in brute.values():
        # 256 records of three 16-byte pieces in LDS
        assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0 and f["AGPRs"] == 0, f
        assert f["LDS Size [bytes/block]"] == 256 * 3 * 16, f
