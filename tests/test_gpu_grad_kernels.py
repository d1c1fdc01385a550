"""GPU: the element-wise and per-position kernels of the white-box backward passes, one launch at a time, against exact host restatements and the
float64 formulas.

    csrc/gl_dcgan_grad.hip   tanh_grad_kernel<L2>, patch_rgb_kernel, relu_bn_grad_kernel<PLANAR>
    csrc/gl_pggan_grad.hip   pg_out_grad_kernel<L2>, pg_rgb_grad_kernel, pg_pn_grad_kernel, pg_leaky_grad_kernel, pg_rowpn_grad_kernel
    csrc/gl_lpips_grad.hip   lg_conv1_kernel<T>, lg_maxpool_kernel, lg_ref_kernel<J>, lg_act_grad_kernel<J>, lg_conv1_grad_kernel, lg_loss_kernel

gl_tune_grad_op (tuning build, csrc/gl_tune.hip) launches one kernel through the launcher the production pass calls -- the grid, its cap and the
template instance are the production ones -- on host arrays from tests/grad_kernels_common.py: every input between poison guards, every output
pre-filled with a sentinel between sentinel guards.  One child process with $GANLEAKS_LIB pointing at the tuning library does all launches and
compares; the tests below only read its result.  Every case runs with n = 3 (images 0 and 2 equal: equal bits) and once more with image 0 alone
(same bits again); image 1 differs; the guards are intact; nothing is left at the sentinel except what the kernel is documented not to write (the
stretches of the longer reference and part rows around a tap's values); everything is finite.

Exact cases (preconditions asserted in tests/test_grad_kernels_cpu.py) are compared value for value with the float32 restatement: the max-pool tie
rule over all 81 patterns of a 2 x 2 cell for every J, the ReLU mask at +0 and -0, the lane-to-channel map and the chunked output, the mirrored taps
and borders of conv1_1's data gradient, the patch gather's borders and zero columns, the phase-planar and K-chunked destinations, toRGB backwards
plain and pooled, the LeakyReLU slope at and below zero.

Real-valued cases: |g - g64|_2 / |g64|_2 per image and per position (the norms over the channels of one position) against the float64 formula; the
bound is SLACK = 4 times the largest such value of the float32 host restatement on the same inputs; where the float64 reference of a position is all
zero (an all-zero tap position behind the ReLU mask) the device has to give exactly zero, and where the formula cancels beyond float32 in the host
restatement itself (grad_kernels_common.position_errors: the one-hot tap position with nothing arriving from above) the device's absolute error
is held against the restatement's at that position.  The losses are compared with the float64 sum rounded to
float32, within 1 ulp.  The measured ratios are printed by the test and recorded in DESIGN.md section 5.
"""
import json
import os
import subprocess
import sys

import pytest

import gpu_common  # noqa: F401
import grad_kernels_common as gk

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, os, sys, time
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import grad_kernels_common as gk
import ganleaks_amd as gl
from ganleaks_amd import _lib
assert _lib.LIB_PATH.endswith("libganleaks_hip_tuning.so")
ctx = gl.Context.get()
out = {}
t_start = time.perf_counter()
for c in gk.ALL_CASES:
    d = c.make()
    try:
        dev3, rest3, g3 = gk.run_case(ctx.lib, ctx.handle, c, d, [0, 1, 2])
        dev1, rest1, g1 = gk.run_case(ctx.lib, ctx.handle, c, d, [0])
    except Exception as e:                                 # a refused or failed launch: nothing more runs on the GPU
        out[c.name] = {"error": str(e)}
        print("RESULT " + json.dumps(out))
        raise
    out[c.name] = gk.evaluate(c, d, dev3, rest3 + rest1, dev1, g3 and g1)
out["seconds"] = time.perf_counter() - t_start
print("RESULT " + json.dumps(out))
'''


@pytest.fixture(scope="module")
def result():
    tuning = os.path.join(ROOT, "gan-leaks_amd", "libganleaks_hip_tuning.so")
    if not os.path.exists(tuning):
        subprocess.run(["make", "-C", os.path.join(ROOT, "gan-leaks_amd", "csrc"), "-j8", "tuning"], check=True)
    env = dict(os.environ, GANLEAKS_LIB=tuning)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("RESULT ")]
    assert r.returncode == 0 and lines, (lines[-1][:2000] if lines else "") + r.stderr.decode()[-3000:]
    out = json.loads(lines[-1][7:])
    print("child: %.1f s" % out["seconds"])
    return out


@pytest.mark.parametrize("c", gk.EXACT_CASES, ids=repr)
def test_exact_case_is_bit_exact(c, result):
    r = result[c.name]
    assert gk.verdict(c, r) == [], r


@pytest.mark.parametrize("c", gk.REAL_CASES, ids=repr)
def test_real_valued_error_within_the_float32_bound(c, result):
    r = result[c.name]
    assert "error" not in r, r
    for k in r["err_dev"]:
        a, dev = max(r["err_f32"][k]), max(r["err_dev"][k])
        print("%s %s: image: float32 host %.3e  device %.3e  ratio %.2f   worst position: float32 host %.3e  device %.3e  ratio %.2f   cancelling "
              "positions: %d, absolute error / float32 host's %.2f"
              % (c.name, k, a, dev, dev / a if a else 0.0, r["pos_f32"][k], r["pos_dev"][k], r["pos_dev"][k] / r["pos_f32"][k] if r["pos_f32"][k] else 0.0,
                 r["ill"][k], r["ill_ratio"][k]))
    for k, v in r["ulp"].items():
        print("%s %s: %d ulp from the float64 sum rounded to float32" % (c.name, k, v))
    assert gk.verdict(c, r) == [], r
