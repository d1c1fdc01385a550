"""No scratch and at most 256 registers in the 256 x 256 tiles of gather_conv_h3 that store their split output 16 bytes per lane (EPI16:
a v_permlane16_swap per dword, csrc/gl_conv_h3_epi.h): cross-compiled to gfx950 assembly here, no GPU needed (tools/check_loop_spills.py).
The epilogue of this tile has spilled before without a line of its K loop changing, and did again while the 16-byte form was written (the
chain of ORs behind the saturation flag kept every converted value alive: 124 bytes of scratch), so the whole kernel's scratch is asserted
to be zero here, not only the K loop's.  The tuning build's arms (the 8-byte stores, the stamped instantiations) are held to the same."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#                                        WC    WP    TC    TP   tail  UP    T4  XONCE EPI16 STAMP
TILE = "gather_conv_h3_kernelILi2ELi4ELi8ELi4ELb0ELb0E"
SHIPPED = [TILE + "Lb0ELb0ELb1ELb0E", TILE + "Lb1ELb0ELb1ELb0E"]                       # raster, T4
TUNING = [TILE + t4 + "Lb0E" + epi + stamp for t4 in ("Lb0E", "Lb1E") for epi in ("Lb0E", "Lb1E") for stamp in ("Lb0E", "Lb1E")]
needs_hipcc = pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")


def check(kernels, *flags):
    arg = ",".join("gl_conv_h3.hip:" + k for k in kernels)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_loop_spills.py"), "--registers", "--kernels", arg] + list(flags),
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("0 scratch instructions inside the K loop") == len(kernels), r.stdout
    regs = re.findall(r"(\d+) VGPRs, (\d+) bytes of scratch in the whole kernel", r.stdout)
    assert len(regs) == len(kernels), r.stdout
    for vgprs, scratch in regs:
        assert int(vgprs) <= 256 and int(scratch) == 0, r.stdout


@needs_hipcc
def test_shipped_16_byte_store_tiles_have_no_scratch_and_fit_256_registers():
    check(SHIPPED)


@needs_hipcc
def test_tuning_arms_and_stamped_tiles_have_no_scratch_and_fit_256_registers():
    check(TUNING, "--tuning")
