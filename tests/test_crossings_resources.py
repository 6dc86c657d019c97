"""What the compiler made of the crossing-count and containment kernels (pt_crossings.hip), pinned -- compile-only, like
test_occlusion_resources.py.  count_hits_kernel and contains_kernel are the persistent walk that the ray, point and occlusion queries are
too (pt_walk.h), instantiated in their own translation unit; the kernels of the other files keep their own lines (their resource tests),
and this file adds no kernel to theirs."""

import pytest

from kres import HIPCC, resources


@pytest.mark.skipif(HIPCC is None, reason="hipcc is missing")
def test_crossing_kernels_registers_scratch_and_occupancy():
    seen = resources("resource-usage-crossings")
    count = {k: v for k, v in seen.items() if k.startswith("_ZN3ptk17count_hits_kernelE")}
    contains = {k: v for k, v in seen.items() if k.startswith("_ZN3ptk15contains_kernelE")}
    simple = {k: v for k, v in seen.items() if k.startswith(("_ZN3ptk24count_hits_simple_kernel", "_ZN3ptk22contains_simple_kernel"))}
    brute = {k: v for k, v in seen.items() if k.startswith("_ZN3ptk23count_hits_brute_kernel")}
    small = {k: v for k, v in seen.items() if k.startswith(("_ZN3ptk22contains_finish_kernel", "_ZN3ptk17apply_sign_kernel"))}
    assert len(count) == 1 and len(contains) == 1 and len(simple) == 4 and len(brute) == 2 and len(small) == 2 and len(seen) == 10, sorted(seen)
    for f, vgprs in ((list(count.values())[0], 66), (list(contains.values())[0], 71)):
        # required: no scratch, no spills, at least the 6 waves per SIMD the launch grid assumes (PT_CR_WAVES_PER_SIMD), the 12-entry LDS
        # stack of one wavefront (PT_CR_SHORT_STACK x 64 lanes x 8 bytes).  Recorded as compiled: 66 VGPRs for the ray records (a counter in
        # place of trace_rays_kernel's hit triangle and hit distance), 71 for the points (the sample-ray parameters live across the walk),
        # which the register file turns into 7 waves per SIMD.
        assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, f
        assert f["Occupancy [waves/SIMD]"] >= 6, f
        assert f["LDS Size [bytes/block]"] == 12 * 64 * 8, f
        assert f["VGPRs"] == vgprs and f["AGPRs"] == 0, f
        assert f["Occupancy [waves/SIMD]"] == 7, f
    for f in simple.values():
        # the 64-entry private stack (512 B per lane) is the only scratch use, as in trace_rays_simple_kernel
        assert f["VGPRs"] <= 64 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, f
        assert 512 <= f["ScratchSize [bytes/lane]"] <= 544, f
        assert f["Occupancy [waves/SIMD]"] == 8, f
    for f in brute.values():
        # 256 records of three 16-byte pieces in LDS
        assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0 and f["Occupancy [waves/SIMD]"] == 8, f
        assert f["LDS Size [bytes/block]"] == 256 * 3 * 16, f
    for f in small.values():
        assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0 and f["Occupancy [waves/SIMD]"] == 8, f
