"""The host twin of the sphere-cast queries (pt_host.cpp::sweep_spheres) under AddressSanitizer + UBSan: a stand-alone program, CPU only, the
way tests/test_box_sanitizers.py builds its own."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_sweep_twin_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sweep_sanitize")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(HERE, "native", "sweep_sanitize.cpp"), os.path.join(ROOT, "raytracer-public_amd", "csrc", "pt_host.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    out = subprocess.check_output([exe], text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert "sweep_sanitize ok" in out, out
