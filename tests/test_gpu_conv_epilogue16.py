"""GPU: the 256 x 256 tile of gather_conv_h3 with its split output stored 16 bytes per lane after a lane swap (GL_H3_EPI16=1; shipped)
against the 8-byte stores (0), byte for byte.  The switch changes neither a value nor an address, so every output byte must be the same, the
sentinel guards around the output must survive (a ragged tile's absent positions stay silent after the lane swap) and, the inputs being the
structural ones of conv_layer_common, the output must also equal the float64 convolution exactly.  The switch exists only in the tuning build
(libganleaks_hip_tuning.so), loaded in ONE child process through $GANLEAKS_LIB; GL_H3_TILE256=1 puts these small layers onto the 256 x 256 tile,
which otherwise wants 256 workgroups.  A launch counter of the tuning build proves which form an arm took.

Layers (one launch each, gl_tune_conv_layer), every one in both arms:
  a  4 x 4 grid, ConvTranspose phases, Cin 64, 256 columns, 32 images: two full 256-position tiles in the fragment-per-position order (T4)
  b  8 x 8 grid, ConvTranspose phases, Cin 32, 512 columns, 5 images: 320 positions, the second position tile holds 64
  c  1 x 1 grid, one tap, Cin 128, 512 columns, 300 positions (the generator's first layer; c % cmod wraps): ragged as well
  d  an upsampled 8 x 8 layer (UP keeps the 8-byte stores in both arms) and a 9-tap layer on the 4 x 4 grid (T4 with skipped fragments)
and one DCGAN-64 forward of 48 images, float and 8-bit output, whose first three layers then run on this tile.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_common  # noqa: F401
import conv_layer_common as cl

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL = 2e-5                                    # tests/test_gpu_dcgan.py: the golden file's tolerance
ARMS = [0, 1]                                  # GL_H3_EPI16; the first is the baseline
H3, UP, T4 = cl.H3, cl.UP, cl.T4

# name -> (case, takes the 16-byte form when asked)
LAYERS = {
    "a_t4_ct": (cl.Case("e16_a_t4_ct", "h3", "ct", 32, 4, 4, 64, 256, H3 | 2 | T4, out="split", act=1), True),
    "b_8x8_ct_ragged": (cl.Case("e16_b_8x8_ct", "h3", "ct", 5, 8, 8, 32, 512, H3 | 2, out="split"), True),
    "c_1x1_ragged": (cl.Case("e16_c_1x1", "h3", "one", 300, 1, 1, 128, 512, H3 | 2, out="split", cmod=32, act=1), True),
    "d_up_8x8": (cl.Case("e16_d_up", "h3", "ct", 5, 8, 8, 32, 256, H3 | 2 | UP, out="split", up=1), False),
    "d_t4_9taps": (cl.Case("e16_d_c3", "h3", "c3", 32, 4, 4, 32, 256, H3 | 2 | T4, out="split"), True),
}

CHILD = r'''
import ctypes, json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import conv_layer_common as cl
import test_gpu_conv_epilogue16 as me
import ganleaks_amd as gl
from ganleaks_amd import _lib
assert _lib.LIB_PATH.endswith("libganleaks_hip_tuning.so")
from ganleaks_amd.gan_models.dcgan.model_torch import Generator
ctx = gl.Context.get()
ctx.lib.gl_tune_h3_epi16_launches.restype = ctypes.c_longlong
counts = ctx.lib.gl_tune_h3_epi16_launches             # tuning build: launches of the 16-byte store form so far
os.environ["GL_H3_TILE256"] = "1"

def arm(e):
    os.environ["GL_H3_EPI16"] = str(e)

out = {"layers": {}, "dcgan": {}}
for name, (c, _) in me.LAYERS.items():
    d = cl.make_inputs(c)
    ref = cl.reference(c, d)
    problems = cl.exactness_problems(c, d, ref)
    guard, sent = cl.expected_in_guard(c), bytes([cl.SENTINEL]) * cl.OUT_GUARD
    res = {"problems": problems, "arms": []}
    base = None
    for e in me.ARMS:
        arm(e)
        c0 = counts()
        r = cl.run_layer(ctx.lib, ctx.handle, c, d)
        c1 = counts()
        base = r["out"] if base is None else base
        dev = cl.decode_output(c, r["out"])
        res["arms"].append({"form": r["form"], "launches": c1 - c0, "bytes_equal": r["out"] == base,
                            "nbad_vs_float64": int((dev != ref).sum()), "sat_delta": r["sat_delta"], "nonzero": bool(np.abs(dev).max() > 0),
                            "guards_ok": bool(r["in_guards"][0] == guard and r["in_guards"][1] == guard and r["out_guards"][0] == sent
                                              and r["out_guards"][1] == sent)})
    out["layers"][name] = res

golden = np.load(os.path.join(%(root)r, "tests", "golden", "dcgan_gen.npz"))
sd = gl.synth.dcgan_state_dict(int(golden["weight_seed"]))
zg = gl.synth.latent(int(golden["z_seed"]), int(golden["n"]))
idx = np.arange(48) %% len(zg)                  # image i is the golden file's image i mod 8
base = None
for e in me.ARMS:
    arm(e)
    g = Generator(100, 3, 64, ctx)
    g.load_state_dict(sd)
    c0 = counts()
    f32, u8 = g.forward_device(zg[idx], True, True)
    f32, u8 = f32.numpy().copy(), u8.numpy().copy()
    c1 = counts()
    base = (f32, u8) if base is None else base
    out["dcgan"][str(e)] = {"launches": c1 - c0, "f32_equal": bool(np.array_equal(f32, base[0])),
                            "u8_equal": bool(np.array_equal(u8, base[1])), "golden_err": float(np.abs(f32 - golden["out"][idx]).max())}
print("RESULT " + json.dumps(out))
'''


@pytest.fixture(scope="module")
def result():
    tuning = os.path.join(ROOT, "gan-leaks_amd", "libganleaks_hip_tuning.so")
    if not os.path.exists(tuning):
        subprocess.run(["make", "-C", os.path.join(ROOT, "gan-leaks_amd", "csrc"), "-j8", "tuning"], check=True)
    env = dict(os.environ, GANLEAKS_LIB=tuning)
    for k in ("GL_H3_EPI16", "GL_H3_TILE256", "GL_H3_T4", "GL_H3_XONCE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    line = [l for l in r.stdout.decode().splitlines() if l.startswith("RESULT ")][-1]
    out = json.loads(line[7:])
    print(json.dumps(out, indent=1))
    return out


@pytest.mark.parametrize("name", list(LAYERS))
def test_layer_bytes_identical_in_every_arm(name, result):
    c, _ = LAYERS[name]
    r = result["layers"][name]
    assert r["problems"] == [], r["problems"]          # the exact comparison with float64 is sound for these inputs
    for a in r["arms"]:
        assert a["form"] == c.form, "case written for form 0x%x ran as 0x%x" % (c.form, a["form"])
        assert a["bytes_equal"] and a["guards_ok"] and a["nonzero"], a
        assert a["nbad_vs_float64"] == 0 and a["sat_delta"] == 0, a


@pytest.mark.parametrize("name", list(LAYERS))
def test_the_switch_selects_the_form(name, result):
    """one launch per arm: the 16-byte store form exactly when asked for, and never on an upsampled layer"""
    _, epi16 = LAYERS[name]
    for e, a in zip(ARMS, result["layers"][name]["arms"]):
        assert a["launches"] == int(epi16 and e), (e, a)


@pytest.mark.parametrize("arm", ARMS, ids=lambda a: "epi16_%d" % a)
def test_dcgan_forward_identical_and_within_golden_tolerance(arm, result):
    """48 images, float and 8-bit output; the three hidden layers in front of the fused-tail one run on the 256 x 256 tile"""
    r = result["dcgan"][str(arm)]
    assert r["launches"] == 3 * arm, r
    assert r["f32_equal"] and r["u8_equal"], r
    assert r["golden_err"] < ATOL, r
