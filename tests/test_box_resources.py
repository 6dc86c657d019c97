"""What the compiler made of the box-overlap kernels (pt_overlap.hip), pinned -- compile-only, like test_radius_resources.py.
box_kernel<FILL> is the persistent walk that the other batched queries are too (pt_walk.h), instantiated in its own translation unit.  Its Q
(BoxWalk) is in pt_overlap.hip; the bodies of the simple and the brute-force kernel and the dispatch are pt_region.h's, the frame
radius_simple_kernel and radius_brute_kernel are instantiated from as well (test_radius_resources.py); pt_overlap.hip holds the box
policy and the __global__ wrappers, whose names and variants are counted here.  The scan between the two walks is pt_radius.hip's, so this translation unit holds the project's own kernels only."""

import re

import pytest

from kres import CSRC, HIPCC, resources


def knob(name):
    with open(CSRC + "/pt_kernels.h") as f:
        return int(re.search(r"#define %s (\d+)" % name, f.read()).group(1))


@pytest.mark.skipif(HIPCC is None, reason="hipcc is missing")
def test_box_kernels_registers_scratch_and_occupancy():
    seen = resources("resource-usage-box")
    own = {k: v for k, v in seen.items() if k.startswith("_ZN3ptk")}
    walk = {k: v for k, v in own.items() if k.startswith("_ZN3ptk10box_kernelILb")}
    simple = {k: v for k, v in own.items() if k.startswith("_ZN3ptk17box_simple_kernelILb")}
    brute = {k: v for k, v in own.items() if k.startswith("_ZN3ptk16box_brute_kernelILb")}
    # count and fill of the persistent kernel; count, count + stats and fill of the other two
    assert len(walk) == 2 and len(simple) == 3 and len(brute) == 3 and len(own) == 8, sorted(own)
    count = next(v for k, v in walk.items() if k.startswith("_ZN3ptk10box_kernelILb0E"))
    fill = next(v for k, v in walk.items() if k.startswith("_ZN3ptk10box_kernelILb1E"))
    for f, vgprs in ((count, 78), (fill, 79)):
        # required: no scratch, no spills, no AGPRs, at least the waves per SIMD the launch grid assumes (PT_BX_WAVES_PER_SIMD), the LDS
        # stack of one wavefront (PT_BX_SHORT_STACK x 64 lanes x 8 bytes).  Recorded as compiled: 78 VGPRs for the count walk, 79 for the
        # fill walk (the 64-bit base).  The box holds twelve values per lane for the whole walk (the corners, and the corners moved out by
        # the slack) where a radius query holds ten, and the leaf test has the three vertices, the centre-relative vertices and the
        # half-extent live at once: 23 registers above radius_kernel's 55.  80 VGPRs is the most at which the register file holds 6 waves
        # per SIMD (512 / 80), which is what PT_BX_WAVES_PER_SIMD = 6 asks for.
        assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, f
        assert f["AGPRs"] == 0, f
        assert f["Occupancy [waves/SIMD]"] >= knob("PT_BX_WAVES_PER_SIMD"), f
        assert f["LDS Size [bytes/block]"] == knob("PT_BX_SHORT_STACK") * 64 * 8, f
        assert f["VGPRs"] == vgprs, f
    for f in simple.values():
        # the 64-entry private stack (512 B per lane) is the only scratch use, as in radius_simple_kernel
        assert f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0 and f["AGPRs"] == 0, f
        assert 512 <= f["ScratchSize [bytes/lane]"] <= 544, f
    for f in brute.values():
        # 256 records of three 16-byte pieces in LDS
        assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0 and f["AGPRs"] == 0, f
        assert f["LDS Size [bytes/block]"] == 256 * 3 * 16, f
