"""The wide exact-L2 kernel (d up to 2^24, int64 row norms) keeps its K loop free of scratch traffic: gl_l2knn.hip cross-compiled to
gfx950 assembly here, no GPU needed.  Its 64 int64 totals sit next to the 64 int32 accumulators of the 128 x 128 tile; one spilled
total would put a scratch reload and a vmcnt(0) wait into every K slice."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from check_loop_spills import loop_spills  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="needs hipcc")
def test_wide_l2_kernel_has_no_spills_in_its_k_loop(tmp_path):
    out = str(tmp_path / "gl_l2knn.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--cuda-device-only", "-S",
           os.path.join(ROOT, "gan-leaks_amd", "csrc", "gl_l2knn.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    asm = open(out).read()
    assert loop_spills(asm, "l2_knn_i8_wide_kernel") == 0
    # the existing 128-tile instantiations are still there and still clean
    assert loop_spills(asm, "l2_knn_i8_kernelILb1E") == 0
    assert loop_spills(asm, "l2_knn_i8_kernelILb0E") == 0
