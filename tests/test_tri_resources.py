"""What the compiler made of the triangle-overlap kernels (pt_tritri.hip), pinned -- compile-only, like test_box_resources.py.
tri_kernel<FILL> is the persistent walk that the other batched queries are too (pt_walk.h), instantiated in its own translation unit.  Its Q
(TriWalk) is in pt_tritri.hip; the bodies of the simple and the brute-force kernel and the dispatch are pt_region.h's.  The scan between the
two walks is pt_radius.hip's, so this translation unit holds the project's own kernels only."""

import re

import pytest

from kres import CSRC, HIPCC, resources


def knob(name):
    with open(CSRC + "/pt_kernels.h") as f:
        return int(re.search(r"#define %s (\d+)" % name, f.read()).group(1))


@pytest.mark.skipif(HIPCC is None, reason="hipcc is missing")
def test_tri_kernels_registers_scratch_and_occupancy():
    seen = resources("resource-usage-tri")
    own = {k: v for k, v in seen.items() if k.startswith("_ZN3ptk")}
    walk = {k: v for k, v in own.items() if k.startswith("_ZN3ptk10tri_kernelILb")}
    simple = {k: v for k, v in own.items() if k.startswith("_ZN3ptk17tri_simple_kernelILb")}
    brute = {k: v for k, v in own.items() if k.startswith("_ZN3ptk16tri_brute_kernelILb")}
    # count and fill of the persistent kernel; count, count + stats and fill of the other two
    assert len(walk) == 2 and len(simple) == 3 and len(brute) == 3 and len(own) == 8, sorted(own)
    count = next(v for k, v in walk.items() if k.startswith("_ZN3ptk10tri_kernelILb0E"))
    fill = next(v for k, v in walk.items() if k.startswith("_ZN3ptk10tri_kernelILb1E"))
    for f, vgprs in ((count, 66), (fill, 69)):
        # required: no scratch, no spills, no AGPRs, at least the waves per SIMD the launch grid assumes (PT_TT_WAVES_PER_SIMD), the LDS
        # stack of one wavefront (PT_TT_SHORT_STACK x 64 lanes x 8 bytes).  Recorded as compiled: 66 VGPRs for the count walk, 69 for the
        # fill walk, with the box's twelve values and the caller's nine coordinates held per lane for the whole walk.  The form that reads
        # the 48-byte record again at a leaf compiled to 68 and 81 and was not kept.
        assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, f
        assert f["AGPRs"] == 0, f
        assert f["Occupancy [waves/SIMD]"] >= knob("PT_TT_WAVES_PER_SIMD"), f
        assert f["LDS Size [bytes/block]"] == knob("PT_TT_SHORT_STACK") * 64 * 8, f
        assert f["VGPRs"] == vgprs, f
    # the LDS stacks of the grid's waves fit a CU: 4 SIMDs x PT_TT_WAVES_PER_SIMD x the stack of one wavefront within 160 KiB
    assert 4 * knob("PT_TT_WAVES_PER_SIMD") * knob("PT_TT_SHORT_STACK") * 64 * 8 <= 160 * 1024
    for f in simple.values():
        # the 64-entry private stack (512 B per lane) is the only scratch use, as in box_simple_kernel
        assert f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0 and f["AGPRs"] == 0, f
        assert 512 <= f["ScratchSize [bytes/lane]"] <= 544, f
    for f in brute.values():
        # 256 records of three 16-byte pieces in LDS
        assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0 and f["AGPRs"] == 0, f
        assert f["LDS Size [bytes/block]"] == 256 * 3 * 16, f
