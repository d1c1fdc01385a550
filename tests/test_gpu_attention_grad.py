"""GPU: the attention backward (csrc/gl_attention_grad.hip) alone, one launch sequence at a time, against closed forms and the float64 formulas.

gl_tune_attention_grad (tuning build, csrc/gl_tune.hip) runs the row kernel and the column kernel once on host arrays from
tests/attention_grad_common.py -- qkv and dY between poison guards, dqkv and the statistics pre-filled with a sentinel between sentinel guards -- and
returns both outputs and the guards.  One child process with $GANLEAKS_LIB pointing at the tuning library does all launches and compares; the tests
below only read its result.  Every case runs for C in {64, 128} with n = 3 (images 0 and 2 equal: their rows must be equal bit for bit) and once more
with image 0 alone (same bits again).

Exact cases (preconditions asserted in tests/test_attention_grad_cpu.py), compared with np.array_equal:
    uniform   q = k = 0, small-integer dY and v, gamma = 1/2: every weight exp(0) = 1, l = 256: dv_j = gamma / 256 sum_i dY_i, dq = dk = 0 (dE is NOT zero
              here: the zeros come from k = 0 and q = 0 in the last products)
    onehot    k_j = 8 code(j), q_i = 8 code(pi(i)), gamma = 2: P is the permutation matrix, dv_pi(i) = gamma dY_i, D_i = dP_i,pi(i) exactly, so dE = 0 and
              dq = dk = 0; pins the pairing of every i with every j in both kernels and the row statistics handed from the first to the second
    gamma0    real-valued inputs, gamma = 0: all of dqkv is zero
and in every case the zero columns behind dv are zero, the guards are intact and nothing is left at the sentinel.

Real-valued cases (Gaussian q, k, v, dY; energies of standard deviation 0.9 / 12; gamma = 0.7), row metric |g - g64|_2 / |g64|_2 per image and per part
(dq, dk, dv) against the float64 formulas.  The bound comes from the reference side only: (a) the largest error of a float32 torch autograd evaluation
of the same graph on the same inputs times SLACK = 4, plus (b) the allowance for the hardware exponential of attention_grad_common.exp_allowance.
Every image is counted.  Two more gates: the device also stays within 4 a alone (it does on an MI355X, at most 1.44 a; in the mild cases b is 25 times
a and would hide a small defect), and the same metric taken position by position -- the norms over the channels of one query or key position, the
largest of all 768 positions -- stays within 4 x the float32 evaluation's largest position plus the allowance's (for dq at the peaked temperature that
gate says little: an almost one-hot query row has a dq row of almost no norm and a relative error of order 1 in any float32 evaluation).  The measured figures are printed by
the test and recorded in DESIGN.md section 5.
"""
import json
import os
import subprocess
import sys

import pytest

import gpu_common  # noqa: F401
import attention_grad_common as ag

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import attention_grad_common as ag
import ganleaks_amd as gl
from ganleaks_amd import _lib
assert _lib.LIB_PATH.endswith("libganleaks_hip_tuning.so")
ctx = gl.Context.get()
torch.set_num_threads(min(16, torch.get_num_threads()))
out = {}
t_start = time.perf_counter()
sent = bytes([ag.SENTINEL]) * ag.GUARD
sent_f32 = np.frombuffer(bytes([ag.SENTINEL]) * 4, np.float32)[0]
for c in ag.ALL_CASES:
    d = ag.make_inputs(c)
    try:
        r3 = ag.run_attention_grad(ctx.lib, ctx.handle, c, d, [0, 1, 2])
        r1 = ag.run_attention_grad(ctx.lib, ctx.handle, c, d, [0])
    except Exception as e:                                 # a refused or failed launch: nothing more runs on the GPU
        out[c.name] = {"error": str(e)}
        print("RESULT " + json.dumps(out))
        raise
    bits3, bits1 = r3["dqkv"].view(np.uint32), r1["dqkv"].view(np.uint32)
    s3, s1 = r3["stats"].view(np.uint32), r1["stats"].view(np.uint32)
    dev = ag.split(c, r3["dqkv"])
    res = {"guards_ok": all(g == sent for g in r3["guards"] + r1["guards"]),
           "finite": bool(np.isfinite(r3["dqkv"]).all() and np.isfinite(r3["stats"]).all()),
           "written": bool((bits3 != sent_f32.view(np.uint32)).all() and (s3 != sent_f32.view(np.uint32)).all()),
           "pad_zero": bool((dev["pad"] == 0).all()),
           "img0_eq_img2": bool(np.array_equal(bits3[0], bits3[2]) and np.array_equal(s3[0], s3[2])),
           "img0_ne_img1": bool(not np.array_equal(bits3[0], bits3[1])) or c.kind == "gamma0",
           "n1_eq_img0": bool(np.array_equal(bits1[0], bits3[0]) and np.array_equal(s1[0], s3[0]))}
    if c.exact:
        want = ag.closed_form(c, d)
        res["nbad"] = {n: int((dev[n].astype(np.float64) != want[n]).sum()) for n in ag.PARTS}
        res["maxdiff"] = {n: float(np.abs(dev[n] - want[n]).max()) for n in ag.PARTS}
    else:
        f = ag.backward64(c, d, full=True)
        g32 = ag.autograd(c, d, torch.float32)
        res["err_dev"] = {n: ag.row_errors(dev[n], f[n]).tolist() for n in ag.PARTS}
        res["err_f32"] = {n: ag.row_errors(g32[n], f[n]).tolist() for n in ag.PARTS}
        res["allowance"] = {n: v.tolist() for n, v in ag.exp_allowance(c, d, f).items()}
        res["pos_dev"] = {n: ag.position_error(dev[n], f[n]) for n in ag.PARTS}
        res["pos_f32"] = {n: ag.position_error(g32[n], f[n]) for n in ag.PARTS}
        res["pos_allow"] = ag.exp_allowance(c, d, f, per_position=True)
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
    assert r["guards_ok"] and r["finite"] and r["written"] and r["pad_zero"], r
    assert r["img0_eq_img2"] and r["n1_eq_img0"] and r["img0_ne_img1"], r


@pytest.mark.parametrize("c", ag.EXACT_CASES, ids=repr)
def test_exact_case_is_bit_exact(c, result):
    r = result[c.name]
    common_checks(c, r)
    assert r["nbad"] == {"dq": 0, "dk": 0, "dv": 0}, r


@pytest.mark.parametrize("c", ag.REAL_CASES, ids=repr)
def test_real_valued_error_within_the_float32_bound(c, result):
    r = result[c.name]
    common_checks(c, r)
    for n in ag.PARTS:
        a, b, dev = max(r["err_f32"][n]), max(r["allowance"][n]), max(r["err_dev"][n])
        print("%s %s: (a) float32 CPU %.3e  (b) exponential allowance %.3e  device %.3e  device / a %.2f  device / (4 a + b) %.2f"
              % (c.name, n, a, b, dev, dev / a, dev / (ag.SLACK * a + b)))
        print("    worst position: float32 CPU %.3e  allowance %.3e  device %.3e  device / float32 %.2f"
              % (r["pos_f32"][n], r["pos_allow"][n], r["pos_dev"][n], r["pos_dev"][n] / r["pos_f32"][n]))
    for n in ag.PARTS:
        a, b = max(r["err_f32"][n]), max(r["allowance"][n])
        assert all(e <= ag.SLACK * a + b for e in r["err_dev"][n]), (n, r)
        # on an MI355X the device stays within (a) alone (at most 1.44 a), and in the mild cases (b) is 25 times (a): the
        # allowance is not needed, so it is not relied on -- as tests/test_gpu_attention.py gates the forward
        assert all(e <= ag.SLACK * a for e in r["err_dev"][n]), (n, r)
        # and position by position: no query or key position may hide a defect behind the norm of its image
        assert r["pos_dev"][n] <= ag.SLACK * r["pos_f32"][n] + r["pos_allow"][n], (n, r["pos_dev"][n], r["pos_f32"][n], r["pos_allow"][n])
