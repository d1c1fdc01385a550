"""No scratch in the staged-once form of gather_conv_h3 (the 128 x 128 tile of 8 rows of a 16 x 16 image, each input chunk staged once,
XONCE): cross-compiled to gfx950 assembly here, no GPU needed (tools/check_loop_spills.py).  It is a fused-tail form, which multiplies again
in its epilogue, so "between the first and the last MFMA" spans more than its K loop: the check asks for no scratch in all of that."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["gather_conv_h3_kernelILi2ELi2ELi4ELi4ELb1ELb0ELb0ELb1E",      # XONCE
           "gather_conv_h3_kernelILi2ELi2ELi4ELi4ELb1ELb0ELb0ELb0E"]      # its fall-back for other geometries


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
def test_no_spills_inside_the_k_loop_of_the_staged_once_tile():
    arg = ",".join("gl_conv_h3.hip:" + k for k in KERNELS)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_loop_spills.py"), "--kernels", arg], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("0 scratch instructions inside the K loop") == len(KERNELS), r.stdout
