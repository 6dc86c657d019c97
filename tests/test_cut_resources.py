"""What the compiler made of the plane-cut kernels (pt_cut.hip), pinned -- compile-only, like test_tri_resources.py.  cut_kernel<FILL> is
the persistent walk that the other batched queries are too (pt_walk.h), instantiated in its own translation unit.  Its Q (CutWalk) is in
pt_cut.hip; the bodies of the simple and the brute-force kernel and the dispatch are pt_region.h's.  The scan between the two walks is
pt_radius.hip's, so this translation unit holds the project's own kernels only."""

import re

import pytest

from kres import CSRC, HIPCC, resources


def knob(name):
    with open(CSRC + "/pt_kernels.h") as f:
        return int(re.search(r"#define %s (\d+)" % name, f.read()).group(1))


@pytest.mark.skipif(HIPCC is None, reason="hipcc is missing")
def test_cut_kernels_registers_scratch_and_occupancy():
    seen = resources("resource-usage-cut")
    own = {k: v for k, v in seen.items() if k.startswith("_ZN3ptk")}
    walk = {k: v for k, v in own.items() if k.startswith("_ZN3ptk10cut_kernelILb")}
    simple = {k: v for k, v in own.items() if k.startswith("_ZN3ptk17cut_simple_kernelILb")}
    brute = {k: v for k, v in own.items() if k.startswith("_ZN3ptk16cut_brute_kernelILb")}
    # count and fill of the persistent kernel; count, count + stats and fill of the other two
    assert len(walk) == 2 and len(simple) == 3 and len(brute) == 3 and len(own) == 8, sorted(own)
    count = next(v for k, v in walk.items() if k.startswith("_ZN3ptk10cut_kernelILb0E"))
    fill = next(v for k, v in walk.items() if k.startswith("_ZN3ptk10cut_kernelILb1E"))
    stack_bytes = knob("PT_CT_SHORT_STACK") * 64 * 8
    for f, vgprs in ((count, 61), (fill, 62)):
        # required: no scratch, no spills, no AGPRs, the LDS stack of one wavefront (PT_CT_SHORT_STACK x 64 lanes x 8 bytes), and a launch
        # grid that assumes no more waves per SIMD than registers and LDS both allow.  Recorded as compiled: 61 VGPRs for the count walk,
        # 62 for the fill walk (7 waves per SIMD by registers), with the window's twelve values, n and d held per lane and the corner
        # selectors derived from the sign of n_k at each node.  The form that holds the three selectors compiled to 62 and 63 (DESIGN.md
        # section 24) and was not kept.
        assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, f
        assert f["AGPRs"] == 0, f
        assert f["LDS Size [bytes/block]"] == stack_bytes, f
        by_lds = (160 * 1024) // (4 * stack_bytes)
        assert knob("PT_CT_WAVES_PER_SIMD") <= min(f["Occupancy [waves/SIMD]"], by_lds), (f, by_lds)
        assert f["VGPRs"] == vgprs and f["Occupancy [waves/SIMD]"] == 7, f
    # the knob is the minimum of the two ceilings: 7 by registers, 6 by the LDS stacks of a CU's four SIMDs within 160 KiB
    assert knob("PT_CT_WAVES_PER_SIMD") == min(count["Occupancy [waves/SIMD]"], fill["Occupancy [waves/SIMD]"], (160 * 1024) // (4 * stack_bytes)) == 6
    assert knob("PT_CT_FILL") == knob("PT_BX_FILL")                       # taken over from the box query
    for f in simple.values():
        # the 64-entry private stack (512 B per lane) is the only scratch use, as in box_simple_kernel
        assert f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0 and f["AGPRs"] == 0, f
        assert 512 <= f["ScratchSize [bytes/lane]"] <= 544, f
    for f in brute.values():
        # 256 records of three 16-byte pieces in LDS
        assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0 and f["AGPRs"] == 0, f
        assert f["LDS Size [bytes/block]"] == 256 * 3 * 16, f
