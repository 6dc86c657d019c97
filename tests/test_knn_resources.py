"""What the compiler made of the k-nearest kernels (pt_knn.hip), pinned -- compile-only, like test_radius_resources.py.
nearest_k_kernel<KCAP> is the persistent walk that the ray, point, occlusion, crossing and radius queries are too (pt_walk.h), instantiated
in its own translation unit with its own Q (NearestWalk).  The simple kernel walks pt_points.h::key_traverse and the brute-force kernel
streams pt_walk.h::brute_records, the functions the closest-point, radius and box kernels use; the figures of those two kernels are
recorded as compiled on the shared functions (the brute-force kernel with counters went from 37 to 36 VGPRs when its LDS loop became
the shared one, profiles/point_share_isa.txt)."""
import pytest

from kres import HIPCC, resources

SHORT_STACK = 12        # PT_NK_SHORT_STACK
# KCAP -> (VGPRs as compiled, waves per SIMD the launch grid assumes: PT_NK_WAVES_PER_SIMD_<KCAP>)
TIERS = {4: (62, 5), 16: (63, 2), 64: (63, 1)}


@pytest.mark.skipif(HIPCC is None, reason="hipcc is missing")
def test_knn_kernels_registers_scratch_lds_and_occupancy():
    seen = resources("resource-usage-knn")
    own = {k: v for k, v in seen.items() if k.startswith("_ZN3ptk")}
    walk = {k: v for k, v in own.items() if k.startswith("_ZN3ptk16nearest_k_kernelILi")}
    simple = {k: v for k, v in own.items() if k.startswith("_ZN3ptk23nearest_k_simple_kernelILb")}
    brute = {k: v for k, v in own.items() if k.startswith("_ZN3ptk22nearest_k_brute_kernelILb")}
    assert len(walk) == 3 and len(simple) == 2 and len(brute) == 2 and len(own) == 7, sorted(own)
    for kcap, (vgprs, waves) in TIERS.items():
        f = next(v for k, v in walk.items() if k.startswith("_ZN3ptk16nearest_k_kernelILi%dEE" % kcap))
        # required: no scratch, no spills, no AGPRs; the LDS of a one-wavefront workgroup is the 12-entry stack plus the KCAP-row list,
        # 8 bytes x 64 lanes each: 6,144 + 512 * KCAP.  That LDS, not the registers (below 64 VGPRs: 8 waves per SIMD), bounds the
        # occupancy: floor(163,840 / LDS) workgroups per CU, a quarter of them per SIMD.  The grid assumes the floor of that quotient; the
        # compiler's own figure rounds it up for KCAP = 16 (11 workgroups per CU: 3), so it is at least the grid's.
        lds = 8 * 64 * (SHORT_STACK + kcap)
        assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, (kcap, f)
        assert f["AGPRs"] == 0, (kcap, f)
        assert f["LDS Size [bytes/block]"] == lds == 6144 + 512 * kcap, (kcap, f)
        assert waves == min(6, (163840 // lds) // 4) and f["Occupancy [waves/SIMD]"] >= waves, (kcap, f)
        assert f["VGPRs"] == vgprs, (kcap, f)
    for stats, vgprs in ((0, 48), (1, 52)):
        f = next(v for k, v in simple.items() if k.startswith("_ZN3ptk23nearest_k_simple_kernelILb%dEE" % stats))
        # the 64-entry private stack and the 64-pair private list (512 B per lane each, 16 B of alignment) are the only scratch use; no LDS
        assert f["VGPRs"] == vgprs and f["AGPRs"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, (stats, f)
        assert f["ScratchSize [bytes/lane]"] == 1040, (stats, f)
        assert f["LDS Size [bytes/block]"] == 0, (stats, f)
        assert f["Occupancy [waves/SIMD]"] == 8, (stats, f)
    for stats, vgprs in ((0, 36), (1, 36)):
        f = next(v for k, v in brute.items() if k.startswith("_ZN3ptk22nearest_k_brute_kernelILb%dEE" % stats))
        # 256 records of three 16-byte pieces in LDS; the private list (512 B per lane, 16 B of alignment) is the only scratch use
        assert f["VGPRs"] == vgprs and f["AGPRs"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, (stats, f)
        assert f["ScratchSize [bytes/lane]"] == 528, (stats, f)
        assert f["LDS Size [bytes/block]"] == 256 * 3 * 16, (stats, f)
        assert f["Occupancy [waves/SIMD]"] == 8, (stats, f)
