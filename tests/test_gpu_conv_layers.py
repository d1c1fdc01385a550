"""GPU: every convolution kernel form against a float64 convolution over the WHOLE output tensor, one layer at a time.

gl_tune_conv_layer (tuning build, csrc/gl_tune.hip) runs ONE launch of gl_launch_gather_conv / gl_launch_gather_conv_h3 on a problem from
tests/conv_layer_common.py and returns the raw output bytes, the guards around input and output, the change of the saturation counter and the
id of the instantiation that ran.  One child process with $GANLEAKS_LIB pointing at the tuning library does all launches and compares; the
tests below only read its result.

Structural cases (integer activations in {1, 2, 3}, weights in {-2, -1, 1, 2}, power-of-two scale, integer shift / residual): every partial
sum is exact in any order (preconditions asserted in tests/test_conv_layers_cpu.py), so the device must equal the float64 reference bit for
bit -- a wrong tap mask, a missing zero fill (the input guards hold 64, not 0), a wrong `c % cmod`, a store outside the tensor (sentinel guards,
and the output itself is pre-filled with the sentinel) or a misplaced half of the split layout all show as a plain mismatch.  Every case also
asserts the form id it was written for, so a moved dispatch threshold cannot put it onto another kernel unnoticed.

Split arithmetic cases: one operand carries a low half (1 + b 2^-12), so a dropped or misrouted hi*lo product shows at 2^-12 per product.
Real-valued cases: error against float64 relative to a float32 CPU conv2d's on the same inputs, gated at 4x (tests/test_gpu_wb.py's margin).
Measured on an MI355X (kernel error / float32 CPU error, both the largest absolute difference from float64):
    real_t0_c3_cin64    1.72e-06 / 2.36e-06 = 0.73      real_t2_ct_n253     1.91e-06 / 2.18e-06 = 0.87
    real_halo2_cin64    4.30e-06 / 4.17e-06 = 1.03      real_halo1_cin32    2.86e-06 / 3.25e-06 = 0.88
    real_tail_xonce     7.14e-07 / 9.75e-07 = 0.73      real_tail_cols64    9.16e-07 / 1.13e-06 = 0.81
    real_f32w_c3_cin64  2.21e-06 / 2.45e-06 = 0.90      real_f32n_c3_cin64  2.57e-06 / 2.33e-06 = 1.11
The split arithmetic cases came out exact (largest difference 0.0), so the derived bound the child also reports was not needed.
The whole child takes ~17 s, most of it the float64 references.
"""
import json
import os
import subprocess
import sys

import pytest

import gpu_common  # noqa: F401
import conv_layer_common as cl

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import conv_layer_common as cl
import ganleaks_amd as gl
from ganleaks_amd import _lib
assert _lib.LIB_PATH.endswith("libganleaks_hip_tuning.so")
ctx = gl.Context.get()
torch.set_num_threads(min(16, torch.get_num_threads()))
out, cache = {}, {}
t_start = time.perf_counter()
for c in sorted(cl.ALL_CASES, key=lambda c: c.key):        # cases a tuning switch apart share inputs and reference
    if c.key not in cache:
        cache.clear()
        d = cl.make_inputs(c)
        cache[c.key] = (d, cl.reference(c, d))
    d, ref = cache[c.key]
    try:
        r = cl.run_layer(ctx.lib, ctx.handle, c, d)
    except Exception as e:                                 # a refused or failed launch: nothing more runs on the GPU
        out[c.name] = {"error": str(e)}
        print("RESULT " + json.dumps(out))
        raise
    dev = cl.decode_output(c, r["out"])
    diff = np.abs(dev - ref)
    bad = np.argwhere(dev != ref)
    guard = cl.expected_in_guard(c)
    sent = bytes([cl.SENTINEL]) * cl.OUT_GUARD
    res = {"form": r["form"], "sat_delta": r["sat_delta"], "in_guards_ok": r["in_guards"][0] == guard and r["in_guards"][1] == guard,
           "out_guards_ok": r["out_guards"][0] == sent and r["out_guards"][1] == sent, "finite": bool(np.isfinite(dev).all()),
           "nbad": int(len(bad)), "n": int(dev.size), "maxdiff": float(np.nanmax(diff)), "first_bad": [list(map(int, b)) for b in bad[:4]],
           "ref_absmax": float(np.abs(ref).max())}
    if c.inputs in ("arith_w", "arith_x"):
        # the derived bound, should exact equality not hold: 2^-23 of the largest partial-sum magnitude of each output (<= its sum of |products|)
        psum = cl.accumulate(c, np.abs(d["x"]), np.abs(d["w"])).numpy()
        res["bound_excess"] = float((diff - psum * 2.0 ** -23).max())
        res["maxdiff_over_bound"] = float((diff / (psum * 2.0 ** -23)).max())
    if c.inputs == "real":
        e32 = float(np.abs(cl.reference(c, d, dtype=torch.float32).astype(np.float64) - ref).max())
        res["err_kernel"], res["err_f32"], res["ratio"] = res["maxdiff"], e32, res["maxdiff"] / e32
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
    for k in ("GL_H3_XONCE", "GL_H3_T4", "GL_H3_HALO", "GL_H3_TILE128", "GL_HALO_RING", "GL_HALO_DIAG"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    line = [l for l in r.stdout.decode().splitlines() if l.startswith("RESULT ")][-1]
    out = json.loads(line[7:])
    print(json.dumps(out, indent=1))
    return out


def common_checks(c, r):
    assert r["form"] == c.form, "case written for form 0x%x ran as 0x%x" % (c.form, r["form"])
    assert r["in_guards_ok"] and r["out_guards_ok"], r
    assert r["finite"], r


@pytest.mark.parametrize("c", cl.STRUCT_CASES, ids=repr)
def test_structural_case_is_bit_exact(c, result):
    r = result[c.name]
    common_checks(c, r)
    assert r["nbad"] == 0, r
    assert r["sat_delta"] == 0, r


@pytest.mark.parametrize("c", cl.ARITH_CASES, ids=repr)
def test_split_arithmetic_is_exact(c, result):
    """every partial sum fits 24 bits (K <= 576; asserted on the CPU), so hi*hi + hi*lo + lo*hi must give the float64 sum exactly"""
    r = result[c.name]
    common_checks(c, r)
    print(c.name, "maxdiff", r["maxdiff"], "maxdiff / (2^-23 partial sum)", r["maxdiff_over_bound"])
    assert r["nbad"] == 0, r
    assert r["sat_delta"] == 0, r


@pytest.mark.parametrize("c", [c for c in cl.ACT_CASES if c.sat is None], ids=repr)
def test_activation_codes(c, result):
    """1 and 2 exact (2 against float32(float32(0.2) * v)); 3 and 4 (fp32 kernel only) within the golden tolerance 2e-5 of float64"""
    r = result[c.name]
    common_checks(c, r)
    print(c.name, "maxdiff", r["maxdiff"])
    if c.atol is None:
        assert r["nbad"] == 0, r
    else:
        assert r["maxdiff"] < c.atol, r
    assert r["sat_delta"] == 0, r


def test_split_store_just_below_the_fp16_limit_is_exact_and_not_counted(result):
    c = cl.BY_NAME["sat_below"]
    r = result[c.name]
    common_checks(c, r)
    assert r["ref_absmax"] * cl.ACT_SCALE == 65488.0
    assert r["nbad"] == 0 and r["sat_delta"] == 0, r


def test_split_store_just_above_the_fp16_limit_is_counted(result):
    c = cl.BY_NAME["sat_above"]
    r = result[c.name]
    common_checks(c, r)
    assert r["ref_absmax"] * cl.ACT_SCALE == 65520.0
    assert r["sat_delta"] > 0, r
    assert r["nbad"] == 1 and r["maxdiff"] == (65520.0 - 65504.0) / cl.ACT_SCALE, r       # the one clamped value, nothing else


@pytest.mark.parametrize("c", cl.REAL_CASES, ids=repr)
def test_real_valued_error_within_4x_of_float32(c, result):
    r = result[c.name]
    common_checks(c, r)
    print("%s: kernel %.3e  float32 CPU %.3e  ratio %.2f" % (c.name, r["err_kernel"], r["err_f32"], r["ratio"]))
    assert r["ratio"] < cl.RATIO_GATE, r
    assert r["sat_delta"] == 0, r
