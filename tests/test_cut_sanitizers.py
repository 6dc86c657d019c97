"""The host twin of the plane-cut queries (pt_host.cpp::cut_search) under AddressSanitizer + UBSan: a stand-alone program, CPU only, the
way tests/test_tri_sanitizers.py builds its own.  Nothing is loaded into Python."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_cut_twin_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "cut_sanitize")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(HERE, "native", "cut_sanitize.cpp"), os.path.join(ROOT, "raytracer-public_amd", "csrc", "pt_host.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    out = subprocess.check_output([exe], text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert "cut_sanitize ok" in out, out
