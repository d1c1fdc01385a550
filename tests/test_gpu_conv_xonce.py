"""GPU: gather_conv_h3 with each input chunk staged ONCE per tile and the taps read as shifted rows of a padded LDS image (GL_H3_XONCE=1;
shipped) against the form that stages every tap's shifted rows again (GL_H3_XONCE=0), bit for bit.  Only the address an MFMA operand is
read from differs, so every output bit must be the same; the generator must also still agree with tests/golden/dcgan_gen.npz at that
file's tolerance (2e-5, tests/test_gpu_dcgan.py).  The switch exists only in the tuning build (libganleaks_hip_tuning.so), loaded in ONE
child process through $GANLEAKS_LIB; all tests below read that child's result.

The staged-once form is the 128 x 128 tile of DCGAN's last hidden layer (16 x 16 -> 32 x 32 with the RGB layer in its epilogue): a tile is 8
rows of one image, so every image has a first band (zero guard row above, the other band's first row as halo below) and a second one (the
reverse), whatever the number of images: 1, 3, 5, 17 and 33 images, the last also in passes of 16.  A launch counter of the tuning build
proves that arm 1 ran the staged-once instantiation and arm 0 did not.  The first and last rows and columns
of the 64 x 64 output are compared on their own: a wrong guard row or zero column shows there, a wrong halo row in rows 31 / 32.  VGG16
feature rows (3 and 17 images at 64 x 64; conv5_x is the 9-tap layer on a 4 x 4 grid) pin that the switch leaves every other layer alone.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_common  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL = 2e-5                                    # tests/test_gpu_dcgan.py: the golden file's tolerance
DCGAN_N = [1, 3, 5, 17, 33]
VGG_N = [3, 17]

CHILD = r'''
import json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
import ganleaks_amd as gl
from ganleaks_amd import _lib
assert _lib.LIB_PATH.endswith("libganleaks_hip_tuning.so")
from ganleaks_amd.gan_models.dcgan.model_torch import Generator
from ganleaks_amd.lpips import LpipsModel
ctx = gl.Context.get()
golden = np.load(os.path.join(%(root)r, "tests", "golden", "dcgan_gen.npz"))
sd = gl.synth.dcgan_state_dict(int(golden["weight_seed"]))
zg = gl.synth.latent(int(golden["z_seed"]), int(golden["n"]))
gout = golden["out"]
out = {"dcgan": {}, "vgg": {}, "border": {}, "chunk": {}, "launches": {}}

import ctypes
ctx.lib.gl_tune_h3_xonce_launches.restype = ctypes.c_longlong
launches = ctx.lib.gl_tune_h3_xonce_launches       # tuning build: launches of the staged-once form so far

def gen(n, xonce, chunk=None):
    os.environ["GL_H3_XONCE"] = str(xonce)
    g = Generator(100, 3, 64, ctx)
    g.load_state_dict(sd)
    if chunk:
        g.set_chunk(chunk)
    z = zg[np.arange(n) %% len(zg)]              # image i is the golden file's image i mod 8
    f32, u8 = g.forward_device(z, True, True)
    return f32.numpy().copy(), u8.numpy().copy()

for n in %(dcgan_n)r:
    c0 = launches()
    f1, u1 = gen(n, 1)
    c1 = launches()
    f0, u0 = gen(n, 0)
    c2 = launches()
    idx = np.arange(n) %% len(zg)
    out["launches"][str(n)] = [c1 - c0, c2 - c1]     # arm 1: one staged-once launch per pass; arm 0: none
    out["dcgan"][str(n)] = {"f32_equal": bool(np.array_equal(f1, f0)), "u8_equal": bool(np.array_equal(u1, u0)),
                            "golden_err": float(np.abs(f1 - gout[idx]).max()), "golden_err_0": float(np.abs(f0 - gout[idx]).max())}
    # first and last row and column of every image, and the two rows either side of the band boundary (output rows 31, 32)
    b = lambda a: np.concatenate([a[:, :, [0, 31, 32, -1], :].reshape(len(a), -1), a[:, :, :, [0, -1]].reshape(len(a), -1)], axis=1)
    out["border"][str(n)] = {"equal": bool(np.array_equal(b(f1), b(f0))), "nonzero": bool(np.all(np.abs(b(f1)).reshape(n, -1).max(axis=1) > 1e-3))}
    if n == 33:
        fc, uc = gen(n, 1, chunk=16)              # passes of 16 images (128 x 128 tiles) against one pass
        out["chunk"][str(n)] = {"f32_equal": bool(np.array_equal(fc, f1)), "u8_equal": bool(np.array_equal(uc, u1))}

lin = np.load(os.path.join(%(root)r, "tests", "golden", "lpips_lin_v0.1.npz"))
m = LpipsModel(ctx).load_state_dicts(gl.synth.vgg16_state_dict(7), {"lin%%d" %% i: lin["lin%%d" %% i] for i in range(5)})
rng = np.random.default_rng(5)
for n in %(vgg_n)r:
    imgs = rng.integers(0, 256, size=(n, 3, 64, 64), dtype=np.uint8)
    res = {}
    for v in (1, 0):
        os.environ["GL_H3_XONCE"] = str(v)
        fb = m.features(imgs, role="bank")
        res[v] = (fb.rows_numpy().copy(), fb.norms.numpy().copy())
    out["vgg"][str(n)] = {"rows_equal": bool(np.array_equal(res[1][0], res[0][0])), "norms_equal": bool(np.array_equal(res[1][1], res[0][1])),
                          "finite_nonzero": bool(np.isfinite(res[1][0]).all() and np.abs(res[1][0]).max() > 0)}
print("RESULT " + json.dumps(out))
'''


@pytest.fixture(scope="module")
def result():
    tuning = os.path.join(ROOT, "gan-leaks_amd", "libganleaks_hip_tuning.so")
    if not os.path.exists(tuning):
        subprocess.run(["make", "-C", os.path.join(ROOT, "gan-leaks_amd", "csrc"), "-j8", "tuning"], check=True)
    env = dict(os.environ, GANLEAKS_LIB=tuning)
    env.pop("GL_H3_XONCE", None)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "dcgan_n": DCGAN_N, "vgg_n": VGG_N}], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    line = [l for l in r.stdout.decode().splitlines() if l.startswith("RESULT ")][-1]
    out = json.loads(line[7:])
    print(json.dumps(out, indent=1))
    return out


@pytest.mark.parametrize("n", DCGAN_N)
def test_dcgan_outputs_identical_and_within_golden_tolerance(n, result):
    r = result["dcgan"][str(n)]
    assert r["f32_equal"] and r["u8_equal"], r
    assert r["golden_err"] < ATOL and r["golden_err_0"] < ATOL, r


@pytest.mark.parametrize("n", DCGAN_N)
def test_the_switch_selects_the_staged_once_form(n, result):
    """one pass = one launch of the last hidden layer: GL_H3_XONCE=1 must take the staged-once instantiation, 0 must not"""
    assert result["launches"][str(n)] == [1, 0], result["launches"]


@pytest.mark.parametrize("n", DCGAN_N)
def test_border_rows_and_columns_identical(n, result):
    r = result["border"][str(n)]
    assert r["nonzero"] and r["equal"], r


@pytest.mark.parametrize("n", VGG_N)
def test_vgg16_feature_rows_identical(n, result):
    r = result["vgg"][str(n)]
    assert r["finite_nonzero"] and r["rows_equal"] and r["norms_equal"], r


@pytest.mark.parametrize("n", [33])
def test_pass_size_invariance(n, result):
    r = result["chunk"][str(n)]
    assert r["f32_equal"] and r["u8_equal"], r
