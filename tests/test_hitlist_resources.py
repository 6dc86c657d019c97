"""What the compiler made of the hit-list kernels (pt_hitlist.hip), pinned -- compile-only, like test_radius_resources.py.
hit_fill_kernel is the persistent walk that the ray, point, occlusion, crossing and radius queries are too (pt_walk.h), instantiated in
its own translation unit; the count walk and the scan are launched from pt_crossings.hip and pt_radius.hip, which this file leaves as
they are (their resource tests)."""

import pytest

from kres import HIPCC, resources


@pytest.mark.skipif(HIPCC is None, reason="hipcc is missing")
def test_hitlist_kernels_registers_scratch_and_occupancy():
    seen = resources("resource-usage-hitlist")
    own = {k: v for k, v in seen.items() if k.startswith("_ZN3ptk")}
    walk = next(v for k, v in own.items() if k.startswith("_ZN3ptk15hit_fill_kernelE"))
    simple = next(v for k, v in own.items() if k.startswith("_ZN3ptk22hit_fill_simple_kernelE"))
    brute = next(v for k, v in own.items() if k.startswith("_ZN3ptk21hit_fill_brute_kernelE"))
    sort = next(v for k, v in own.items() if k.startswith("_ZN3ptk15hit_sort_kernelE"))
    # the fill walk of each of the three counting kernels, and the sort
    assert len(own) == 4 and len(seen) == 4, sorted(seen)
    for f in (walk, sort):
        assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, f
        assert f["AGPRs"] == 0, f
    # required of the persistent kernel: at least the 6 waves per SIMD the launch grid assumes (PT_HL_WAVES_PER_SIMD) and the 12-entry LDS
    # stack of one wavefront (PT_HL_SHORT_STACK x 64 lanes x 8 bytes).  Recorded as compiled: 67 VGPRs -- count_hits_kernel's walk with the
    # 64-bit base, the capacity, the entry pointer and u, v of the entry; 7 waves per SIMD by the registers, 6.5 by the LDS.
    assert walk["Occupancy [waves/SIMD]"] >= 6, walk
    assert walk["LDS Size [bytes/block]"] == 12 * 64 * 8, walk
    assert walk["VGPRs"] == 67, walk
    # the sort: a one-wavefront workgroup with PT_HL_LDS_MAX = 512 entries of 16 bytes in LDS, 20 workgroups in a CU's 160 KB: 5 waves per
    # SIMD.  Its grid is one workgroup per 64 lists and assumes no residency.  Recorded as compiled: 27 VGPRs.
    assert sort["LDS Size [bytes/block]"] == 512 * 16, sort
    assert sort["Occupancy [waves/SIMD]"] >= 5, sort
    assert sort["VGPRs"] == 27, sort
    # the 64-entry private stack (512 B per lane) is the only scratch use, as in count_hits_simple_kernel
    assert simple["VGPRs"] <= 64 and simple["VGPRs Spill"] == 0 and simple["SGPRs Spill"] == 0 and simple["AGPRs"] == 0, simple
    assert 512 <= simple["ScratchSize [bytes/lane]"] <= 544, simple
    assert simple["Occupancy [waves/SIMD]"] == 8, simple
    # 256 records of three 16-byte pieces in LDS
    assert brute["ScratchSize [bytes/lane]"] == 0 and brute["VGPRs Spill"] == 0 and brute["SGPRs Spill"] == 0 and brute["AGPRs"] == 0, brute
    assert brute["LDS Size [bytes/block]"] == 256 * 3 * 16, brute
