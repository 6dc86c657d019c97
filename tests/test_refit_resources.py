"""What the compiler made of the refit kernels (pt_refit.hip), pinned -- compile-only, like test_rayquery_resources.py -- next to the
sizes of the records those kernels rewrite; and the megakernel's and the ray-query kernel's resource lines, which a new translation
unit must not move."""
import os
import shutil
import subprocess

import pytest

from kres import CSRC, HIPCC, resources

KERNELS = ("refit_prepare4_kernel", "refit4_kernel", "refit_wide_kernel", "refit_prepare2_kernel", "refit2_kernel", "bvh_cost_kernel")


@pytest.mark.skipif(HIPCC is None, reason="hipcc is missing")
def test_refit_kernels_have_no_scratch_and_no_spills():
    seen = resources("resource-usage-refit")
    assert len(seen) == len(KERNELS), sorted(seen)
    for name in KERNELS:
        hit = [v for k, v in seen.items() if name in k]
        assert len(hit) == 1, (name, sorted(seen))
        f = hit[0]
        assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, (name, f)
        # streaming kernels with dependent loads: nothing may cost them wavefronts (8 per SIMD needs at most 64 VGPRs)
        assert f["VGPRs"] <= 64 and f["AGPRs"] == 0 and f["Occupancy [waves/SIMD]"] == 8, (name, f)
    cost = [v for k, v in seen.items() if "bvh_cost_kernel" in k][0]
    assert cost["LDS Size [bytes/block]"] == 4 * 8                          # one f64 partial sum per wavefront of the block


@pytest.mark.skipif(HIPCC is None, reason="hipcc is missing")
def test_megakernel_and_rayquery_resource_lines_are_unchanged():
    seen = resources("resource-usage")
    for bounded in (0, 1):
        f = seen["_ZN3ptk18trace_paths_kernelILi0ELb%dEEEvNS_10RenderArgsE" % bounded]
        assert (f["VGPRs"], f["AGPRs"], f["ScratchSize [bytes/lane]"], f["Occupancy [waves/SIMD]"], f["VGPRs Spill"], f["LDS Size [bytes/block]"]) == \
            (80, 0, 0, 6, 0, 6144), f
    rq = {k: v for k, v in resources("resource-usage-rayquery").items() if k.startswith("_ZN3ptk17trace_rays_kernel")}
    assert len(rq) == 2
    for f in rq.values():
        assert (f["VGPRs"], f["AGPRs"], f["ScratchSize [bytes/lane]"], f["VGPRs Spill"], f["LDS Size [bytes/block]"]) == (70, 0, 0, 0, 12 * 64 * 8), f


@pytest.mark.skipif(HIPCC is None, reason="hipcc is missing")
def test_records_the_refit_rewrites_are_64_bytes(tmp_path):
    """The refit writes whole triangle records and whole wide nodes with four 16-byte stores each."""
    src = tmp_path / "layout.cpp"
    src.write_text('#include "pt_host.h"\nstatic_assert(sizeof(pt::WideNode) == 64 && sizeof(pt::WideNode::Child) == 16, "wide node");\n'
                   'static_assert(sizeof(pt::TriRecord) == 64, "triangle record");\nint main() { return 0; }\n')
    cxx = shutil.which("c++") or shutil.which("g++") or os.path.join(os.path.dirname(HIPCC), "..", "llvm", "bin", "clang++")
    subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I" + CSRC, str(src)], check=True, capture_output=True, timeout=120)
