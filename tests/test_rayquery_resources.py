"""What the compiler made of the ray-query kernels (pt_rayquery.hip), pinned -- compile-only, like test_kernel_resources.py -- and the
C layout of the PtRay / PtHit records those kernels read and write as 16-byte pieces."""
import os
import shutil
import subprocess

import pytest

from kres import HIPCC, ROOT, resources


@pytest.mark.skipif(HIPCC is None, reason="hipcc is missing")
def test_rayquery_kernels_registers_scratch_and_occupancy():
    seen = resources("resource-usage-rayquery")
    persistent = {k: v for k, v in seen.items() if k.startswith("_ZN3ptk17trace_rays_kernel")}
    simple = {k: v for k, v in seen.items() if k.startswith("_ZN3ptk24trace_rays_simple_kernel")}
    camera = {k: v for k, v in seen.items() if k.startswith("_ZN3ptk18camera_rays_kernel")}
    assert len(persistent) == 2 and len(simple) == 4 and len(camera) == 1, sorted(seen)
    for f in persistent.values():
        # the hot path: 70 VGPRs, no scratch, the 12-entry LDS stack of one wavefront; the launch grid assumes 6 waves per SIMD (PT_RQ_WAVES_PER_SIMD)
        assert f["VGPRs"] == 70 and f["AGPRs"] == 0, f
        assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, f
        assert f["LDS Size [bytes/block]"] == 12 * 64 * 8, f
        assert f["Occupancy [waves/SIMD]"] >= 6, f
    for f in simple.values():
        # the A/B and counting kernel keeps traverse()'s 64-entry private stack (512 B per lane), as render_rays_kernel does: that is its
        # only scratch use; no register spills
        assert f["VGPRs"] <= 64 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, f
        assert 512 <= f["ScratchSize [bytes/lane]"] <= 544, f
        assert f["Occupancy [waves/SIMD]"] == 8, f
    for f in camera.values():
        assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["Occupancy [waves/SIMD]"] == 8, f


@pytest.mark.skipif(HIPCC is None, reason="hipcc is missing")
def test_megakernel_resource_line_is_unchanged():
    """pt_device.h now also holds the simple kernels' traversal: the megakernel's production variants keep their exact resource line."""
    seen = resources("resource-usage")
    for bounded in (0, 1):
        f = seen["_ZN3ptk18trace_paths_kernelILi0ELb%dEEEvNS_10RenderArgsE" % bounded]
        assert (f["VGPRs"], f["AGPRs"], f["ScratchSize [bytes/lane]"], f["Occupancy [waves/SIMD]"], f["VGPRs Spill"], f["LDS Size [bytes/block]"]) == \
            (80, 0, 0, 6, 0, 6144), f


@pytest.mark.skipif(HIPCC is None, reason="hipcc is missing")
def test_header_records_are_32_and_16_bytes(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stddef.h>\n#include "mi355pt.h"\n'
        "_Static_assert(sizeof(PtRay) == 32, \"PtRay\");\n"
        "_Static_assert(offsetof(PtRay, t_max) == 12 && offsetof(PtRay, dir) == 16 && offsetof(PtRay, reserved) == 28, \"PtRay fields\");\n"
        "_Static_assert(sizeof(PtHit) == 16, \"PtHit\");\n"
        "_Static_assert(offsetof(PtHit, prim) == 4 && offsetof(PtHit, u) == 8 && offsetof(PtHit, v) == 12, \"PtHit fields\");\n"
        "_Static_assert(PT_TRACE_ANY_HIT == 1 && PT_TRACE_STATS == 2 && PT_TRACE_SIMPLE_KERNEL == 4, \"flags\");\n")
    cc = shutil.which("cc") or shutil.which("gcc") or os.path.join(os.path.dirname(HIPCC), "..", "llvm", "bin", "clang")
    subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], check=True, capture_output=True, timeout=120)


def test_python_records_match_the_header(rt):
    import ctypes as C
    assert C.sizeof(rt.PtRay) == 32 and C.sizeof(rt.PtHit) == 16
    assert rt.PtRay.t_max.offset == 12 and rt.PtRay.dir.offset == 16 and rt.PtHit.u.offset == 8
    assert (rt.PT_TRACE_ANY_HIT, rt.PT_TRACE_STATS, rt.PT_TRACE_SIMPLE_KERNEL) == (1, 2, 4)
