"""GPU: attention_core_kernel<C, SPLIT> (csrc/gl_dcgan.hip) alone, one launch at a time, against closed forms and a float64 softmax attention.

gl_tune_attention (tuning build, csrc/gl_tune.hip) runs ONE launch of launch_attention_core<64 | 128> on host arrays from
tests/attention_common.py -- qkv and x between poison guards, y pre-filled with a sentinel between sentinel guards -- and returns the raw y bytes,
the guards and the change of the split-store saturation counter.  One child process with $GANLEAKS_LIB pointing at the tuning library does all
launches and compares; the tests below only read its result.  Every case runs for C in {64, 128} x {fp32, split} with n = 3 (images 0 and 2
equal: their outputs must be equal bit for bit) and once more with image 0 alone (same bytes again).

Exact cases (preconditions asserted in tests/test_attention_cpu.py), whole y compared with np.array_equal:
    uniform / uniform_lo   q = 0: every weight exp(0) = 1, sum 256, y = gamma / 256 sum_j v_j + x (uniform_lo: stored x with a non-zero lo half)
    onehot                 k_j = 8 code(j), q_i = 8 code(pi(i)): energies up to 512, runner-up 128 lower -> y = gamma v_pi(i) + x; pins the pairing of
                           every i with every j and v row and needs the max subtraction
    twohot_b2 / _b5        two maxima (partner in the other lane half / in another 32-row block): y = gamma / 2 (v_a + v_a') + x; pins both shuffles
    clamp_at / clamp_over  split only: largest |16 y| exactly 65504 (exact, not counted) / 65520 (clamped to +-65504 at exactly those elements, counted)

Real-valued cases (Gaussian q, k, v; energies of standard deviation 0.9 / 12 / 1500; x = 0 or Gaussian; gamma = 0.7), row metric
|y - y64|_2 / |y64|_2 per image against float64, with two reference-side quantities: (a) 4 x the largest error of a float32 torch CPU
evaluation of the same formula (the gate), (b) the allowance for the hardware exponential of attention_common.exp_allowance (reported).
Measured on an MI355X (largest of the three images; device / a is what the assertion gates at 4):
                               (a) float32 CPU   (b) exp allowance   device     device / a
    real_mild_x0     c64  f32      2.375e-07         2.651e-06      3.348e-07      1.41        split 3.377e-07  1.42
    real_mild        c64  f32      2.981e-08         1.744e-07      3.355e-08      1.13        split 5.511e-08  1.85
    real_peaked_x0   c64  f32      4.226e-07         1.124e-07      4.356e-07      1.03        split 4.376e-07  1.04
    real_peaked      c64  f32      2.411e-07         5.486e-08      2.460e-07      1.02        split 2.498e-07  1.04
    real_extreme_x0  c64  f32      5.842e-06         8.069e-09      5.843e-06      1.00        split 5.842e-06  1.00
    real_extreme     c64  f32      6.298e-06         5.825e-09      6.298e-06      1.00        split 6.298e-06  1.00
    real_mild_x0     c128 f32      2.495e-07         2.785e-06      3.355e-07      1.34        split 3.378e-07  1.35
    real_mild        c128 f32      3.080e-08         1.847e-07      3.497e-08      1.14        split 5.616e-08  1.82
    real_peaked_x0   c128 f32      5.285e-07         9.831e-08      5.333e-07      1.01        split 5.353e-07  1.01
    real_peaked      c128 f32      3.255e-07         4.920e-08      3.275e-07      1.02        split 3.302e-07  1.02
    real_extreme_x0  c128 f32      8.172e-06         8.107e-09      8.174e-06      1.00        split 8.174e-06  1.00
    real_extreme     c128 f32      7.136e-06         5.733e-09      7.136e-06      1.00        split 7.136e-06  1.00
The device stays within (a) alone everywhere (at most 1.85 x the float32 CPU error, where the split store's ~22 bits show next to a small
reference error), so (b) is NOT part of the assertion: the gate is device <= 4 a; (b) is still computed and printed.  With energies in the
thousands the error is that of the float32 energies, which every float32 evaluation has (device / a = 1.00).
Every exact case passes by equality; with the v row of the second GEMM read at j ^ 4 (tried on a scratch copy of the kernel, not committed)
onehot, twohot_b5 and both clamp cases fail at 93 - 96 % of their elements (twohot_b2 is symmetric under that swap by construction).
The whole child takes ~1.2 s.
"""
import json
import os
import subprocess
import sys

import pytest

import gpu_common  # noqa: F401
import attention_common as ac

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import attention_common as ac
import ganleaks_amd as gl
from ganleaks_amd import _lib
assert _lib.LIB_PATH.endswith("libganleaks_hip_tuning.so")
ctx = gl.Context.get()
torch.set_num_threads(min(16, torch.get_num_threads()))
out = {}
t_start = time.perf_counter()
sent = bytes([ac.SENTINEL]) * ac.GUARD
for c in ac.ALL_CASES:
    d = ac.make_inputs(c)
    try:
        r3 = ac.run_attention(ctx.lib, ctx.handle, c, d, [0, 1, 2])
        r1 = ac.run_attention(ctx.lib, ctx.handle, c, d, [0])
    except Exception as e:                                 # a refused or failed launch: nothing more runs on the GPU
        out[c.name] = {"error": str(e)}
        print("RESULT " + json.dumps(out))
        raise
    img = ac.T * c.C * 4
    dev = ac.decode_y(c, r3["y"], 3)
    res = {"guards_ok": all(g == sent for g in r3["guards"] + r1["guards"]), "finite": bool(np.isfinite(dev).all()),
           "img0_eq_img2": r3["y"][:img] == r3["y"][2 * img:], "img0_ne_img1": r3["y"][:img] != r3["y"][img:2 * img], "n1_eq_img0": r1["y"] == r3["y"][:img],
           "sat_delta": r3["sat_delta"], "sat_delta_n1": r1["sat_delta"]}
    if c.exact:
        want = ac.expected_exact(c, d)
        bad = np.argwhere(dev != want)
        over = np.abs(ac.closed_form(c, d)) * ac.ACT_SCALE > ac.F16_MAX
        res.update(nbad=int(len(bad)), first_bad=[list(map(int, b)) for b in bad[:4]], maxdiff=float(np.nanmax(np.abs(dev - want))),
                   absmax16=float(np.abs(ac.closed_form(c, d)).max() * ac.ACT_SCALE), nclamped=int(over.sum()),
                   clamped_ok=bool(np.array_equal(np.abs(dev[over]) * ac.ACT_SCALE, np.full(int(over.sum()), ac.F16_MAX))))
    else:
        ref = ac.reference64(c, d)
        res.update(err_dev=ac.row_errors(dev, ref[0]).tolist(), err_f32=ac.row_errors(ac.reference32(c, d), ref[0]).tolist(),
                   allowance=ac.exp_allowance(c, d, ref).tolist())
    out[c.name] = res
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
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    line = [l for l in r.stdout.decode().splitlines() if l.startswith("RESULT ")][-1]
    out = json.loads(line[7:])
    print("child: %.1f s" % out["seconds"])
    return out


def common_checks(c, r):
    assert "error" not in r, r
    assert r["guards_ok"] and r["finite"], r
    assert r["img0_eq_img2"] and r["n1_eq_img0"] and r["img0_ne_img1"], r


@pytest.mark.parametrize("c", [c for c in ac.EXACT_CASES if c.kind != "clamp_over"], ids=repr)
def test_exact_case_is_bit_exact(c, result):
    r = result[c.name]
    common_checks(c, r)
    assert r["nbad"] == 0, r
    assert r["sat_delta"] == 0 and r["sat_delta_n1"] == 0, r
    if c.kind == "clamp_at":
        assert r["absmax16"] == 65504.0 and r["nclamped"] == 0, r


@pytest.mark.parametrize("c", [c for c in ac.EXACT_CASES if c.kind == "clamp_over"], ids=repr)
def test_split_store_above_the_fp16_limit_is_clamped_and_counted(c, result):
    r = result[c.name]
    common_checks(c, r)
    assert r["absmax16"] == 65520.0 and r["nclamped"] == 6, r       # + and - in each of the three images
    assert r["nbad"] == 0 and r["clamped_ok"], r                    # +-65504 at exactly those elements, everything else exact
    assert r["sat_delta"] > 0 and r["sat_delta_n1"] > 0, r


@pytest.mark.parametrize("c", ac.REAL_CASES, ids=repr)
def test_real_valued_error_within_4x_of_float32(c, result):
    r = result[c.name]
    common_checks(c, r)
    a, b, dev = max(r["err_f32"]), max(r["allowance"]), max(r["err_dev"])
    print("%s: (a) float32 CPU %.3e  (b) exponential allowance %.3e  device %.3e  device / a %.2f  device / (4 a + b) %.2f"
          % (c.name, a, b, dev, dev / a, dev / (ac.SLACK * a + b)))
    assert dev <= ac.SLACK * a, r                                    # within (a) alone on an MI355X (docstring), so (b) is not added
    assert r["sat_delta"] == 0, r
