"""The resource lines of a translation unit's kernels, as the compiler reports them (-Rpass-analysis=kernel-resource-usage through the
csrc Makefile's resource-usage* targets): shared by the test_*_resources.py files.  Compile-only, no GPU."""
import os
import re
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "raytracer-public_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
FIELDS = r"(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\])"


def resources(target):
    """{mangled kernel name: {field: value}} of `make <target>`"""
    out = subprocess.run(["make", "-s", "-C", CSRC, target], capture_output=True, text=True, timeout=900)
    text = out.stdout + out.stderr
    seen = {}
    for b in re.split(r"remark: Function Name: ", text)[1:]:
        seen[b.split()[0]] = {k: int(v) for k, v in re.findall(r"remark:\s+" + FIELDS + r": (\d+)", b)}
    return seen
