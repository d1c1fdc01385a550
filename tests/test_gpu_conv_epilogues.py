"""GPU: the fused PixelNorm, toRGB and LPIPS tap (+ 2 x 2 max-pool) epilogues of csrc/gl_conv_h3_epi.h, and the stand-alone kernels that do the
same work on stored activations, one launch at a time against float64 references and an exact host oracle.

gl_tune_conv_layer (tuning build, csrc/gl_tune.hip) runs ONE convolution launch with a fused epilogue (fuse 1 PixelNorm, 2 PixelNorm + toRGB,
3 tap) on a problem from the second half of tests/conv_layer_common.py; rgb_out, the V rows and the pooled tensor each sit in an allocation of
their own, pre-filled with the sentinel byte between 4 KiB sentinel guards, and come back as raw bytes.  gl_tune_split_post runs ONE launch of
pixelnorm_split_kernel, lpips_tap_split_kernel or lpips_tap_pool_split_kernel on host bytes of a split activation.  One child process on the
tuning library does all launches and compares; the tests below only read its result.  If a launch fails, the child stops there.

Exact cases (structural inputs, Cin = 32, act 0 / 1): the sum of squares of a position is exact in any order (preconditions asserted in
tests/test_conv_epilogues_cpu.py) and every later step is ONE correctly rounded float32 operation (/, sqrt, +, *), which numpy's float32
repeats on the host, so the device halves must EQUAL the oracle's, bit for bit: a tile that is absent but not counted as 0, the wrong pool
partner, a misplaced V row, chunk or K-block all show as plain mismatches; so does a store outside the written range (the rest of every buffer
must still hold the sentinel; for fuse 2 and 3 `out` too).
Bounded cases (toRGB, act 2, the clamped pair, real-valued stand-alone inputs): elementwise against float64 under the derived bounds of
tests/conv_layer_common.py; the largest error / bound is printed per case.
Fused == unfused: for every fused PixelNorm / tap case with 64 or 128 channels the same convolution without the epilogue, fed to
gl_tune_split_post, must give the same bytes (activation, whole V buffer, pool) -- also where the sums are NOT exact (act 2, the clamped pair),
which pins the canonical summation order both sides promise.  GL_PIXNORM_FUSE=0 and GL_TAP_FUSE=0 must not change a bit of a whole PGGAN /
VGG16 + LPIPS run either; GL_RGB_FUSE=0 (another arithmetic) stays within the generator's tolerance.

The defect these tests found: the square root of the sum of squares was __fsqrt_rn, which hipcc lowers to a bare v_sqrt_f32 (1 ulp).  68 of
the 84 exact cases failed: up to 21 % of the positions of a case had taken a float32 neighbour of the rounded root (39 664 of 262 656 in
pn_halo2_cols128, 21 of 216 in pn_t0_cols128), which moved 2 - 7 % of the low halves (1981 of 55 296 halves in pn_t0_cols128) and about one fp16
row value in 10^5.  All five sites now call gl_sqrt_rn (csrc/gl_conv.h), the IEEE operation; every exact case equals the oracle.

Measured on an MI355X, largest device error / bound over the cases of a kind (the exact cases equal the oracle, whose own figures
tests/test_conv_epilogues_cpu.py prints):
    fused PixelNorm   exact cases 0.38 - 0.46    act 2 0.55 - 0.58    clamped pair 0.45 - 0.47
    fused toRGB       0.05 - 0.10
    fused tap         split rows 0.50 - 0.64     fp16 rows 0.985 - 0.999 (the bound is the fp16 rounding itself)
    stand-alone       PixelNorm 0.33 - 0.42 (exact inputs), 0.42 - 0.48 (real);  tap split rows 0.52 - 0.62, 0.53 - 0.66;  fp16 rows 0.986 - 0.997, 0.966 - 0.996
    GL_RGB_FUSE=0 against the fused toRGB: 1.1e-6 on images in (-1, 1)
The whole child (67 fused, 5 refused and 60 stand-alone launches, 47 unfused chains, two small networks for the switches) takes 18 - 20 s, most of
it the float64 references and decoding the halo shape's V buffers on the host.
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
import itertools, json, os, sys, time
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
out = {}
t_start = time.perf_counter()
SENT = bytes([cl.SENTINEL]) * cl.OUT_GUARD
bits = lambda a: np.ascontiguousarray(a).view(np.uint16)
nbad = lambda a, b: int((bits(a) != bits(b)).sum())
guards_ok = lambda pairs: all(lo == SENT and hi == SENT for lo, hi in pairs)
untouched = lambda buf: bool((np.frombuffer(buf, np.uint8) == cl.SENTINEL).all())
ratio = lambda dev, want, bound: float(np.nanmax(np.abs(dev - want) / bound))


def launch(name, f, *a, **kw):
    try:
        return f(*a, **kw)
    except Exception as e:                                 # a failed launch: nothing more runs on the GPU
        out[name] = {"error": str(e)}
        print("RESULT " + json.dumps(out))
        raise


def against_oracle(res, kind, dev, make_oracle):
    """dev: the device's float16 arrays [positions][C] (hi, or hi and lo); make_oracle() -> the oracle's (hi, lo).  nbad: halves that differ"""
    o = memo(kind, make_oracle)
    res["nbad"] = int(sum((bits(a) != bits(b)).sum() for a, b in zip(dev, o)))


def check_tap(c, res, V, pool, stored32, ref_true, coef, exact):
    """V buffer and pooled tensor of a tap launch (fused or stand-alone) against the float64 reference and the oracle"""
    ldv, vb = cl.v_geometry(c)
    K = c.Ho * c.Wo * c.cols
    hi, lo, res["v_rest_sentinel"] = cl.decode_vrows(V, c.tap_fmt, ldv, c.tap_row0, c.n, c.tap_off, K)
    hi, lo = hi.reshape(-1, c.cols), (None if lo is None else lo.reshape(-1, c.cols))
    want = memo("tap_ref", lambda: cl.ref_tap(ref_true, coef).reshape(-1, c.cols))
    if c.tap_fmt == 0:
        dev = cl.halves_value(hi, lo)
        res["ratio"] = ratio(dev, want, cl.bound_split(want))
    else:
        dev = hi.astype(np.float64)
        res["ratio"] = ratio(dev, want, cl.bound_f16(want))
    res["finite"] = bool(np.isfinite(dev).all())
    if exact:
        against_oracle(res, "tap_oracle", [hi, lo] if c.tap_fmt == 0 else [hi], lambda: cl.oracle_tap(stored32, coef))
    if c.tap_pool:
        ph, pl = cl.split_halves(pool.tobytes(), c.n * (c.Ho // 2) * (c.Wo // 2), c.cols)
        oph, opl = memo("pool_oracle", lambda: cl.oracle_pool(stored32.reshape(c.n, c.Ho, c.Wo, c.cols)))
        res["nbad_pool"] = nbad(ph, oph) + nbad(pl, opl)         # the pool of stored values is exact whatever the inputs


# --------------------------------------------------------------- the three switches, before anything moves the saturation counter
# GL_PIXNORM_FUSE, GL_RGB_FUSE (gl_pggan.hip pg_conv) and GL_TAP_FUSE (gl_conv_h3_tap_fusable) choose between a fused epilogue and the
# stand-alone kernel inside whole networks: the stored activations, and with them the images and the feature rows, must not change by a bit
def switched_off(names, f):
    for k in names:
        os.environ[k] = "0"
    try:
        return f()
    finally:
        for k in names:
            os.environ.pop(k, None)

from ganleaks_amd.gan_models.pggan.model_torch import Generator
from ganleaks_amd.lpips import LpipsModel
gen = Generator(128, 128, 3)
gen.load_state_dict(gl.synth.pggan_state_dict(77, 128, 128))
gen.set_precision(1)
z = gl.synth.latent(9, 6, 128)
pg = lambda: gen.forward_device(z, 4, 1.0, True, False)[0].numpy().copy()
img = pg()
sw = {"pggan_finite": bool(np.isfinite(img).all()) and img.shape == (6, 3, 64, 64)}
rgb_off = switched_off(["GL_RGB_FUSE"], pg)              # toRGB as a split-fp16 convolution of its own: other arithmetic, not the same bits
sw["GL_RGB_FUSE_maxdiff"] = float(np.abs(rgb_off - img).max())
sw["GL_PIXNORM_FUSE"] = bool(np.array_equal(switched_off(["GL_RGB_FUSE", "GL_PIXNORM_FUSE"], pg), rgb_off))   # the fused toRGB needs the fused PixelNorm
lin = np.load(os.path.join(%(root)r, "tests", "golden", "lpips_lin_v0.1.npz"))
model = LpipsModel().load_state_dicts(gl.synth.vgg16_state_dict(7), {"lin%%d" %% i: lin["lin%%d" %% i] for i in range(5)})
x = np.random.default_rng(11).integers(0, 256, size=(6, 3, 32, 32), dtype=np.uint8)
sw["GL_TAP_FUSE"] = True
for role in (None, "bank"):
    feat = lambda: model.features(x, role=role).rows_numpy().copy()
    rows = feat()
    sw["GL_TAP_FUSE"] = sw["GL_TAP_FUSE"] and bool(np.isfinite(rows.astype(np.float32)).all()) and bool(np.array_equal(switched_off(["GL_TAP_FUSE"], feat), rows))
sw["saturations"] = int(ctx.h3_saturations())
out["switches"] = sw

# ---------------------------------------------------------------------------------------------- the fused epilogues
for key, group in itertools.groupby(sorted(cl.EPI_CASES, key=lambda c: c.key), key=lambda c: c.key):
    group = list(group)
    c0 = group[0]
    d = cl.make_epi_inputs(c0)
    ref = cl.ref_clamped(c0, cl.reference(c0, d))              # what pass 1 keeps: clamped to the fp16 range of the stored value
    stored32 = (ref * cl.ACT_SCALE).reshape(-1, c0.cols).astype(np.float32)
    cache = {}
    memo = lambda k, f: cache[k] if k in cache else cache.setdefault(k, f())
    unfused = None
    for c in group:
        r = launch(c.name, cl.run_layer, ctx.lib, ctx.handle, c, d)
        guard = cl.expected_in_guard(c)
        res = {"form": r["form"], "sat_delta": r["sat_delta"], "in_guards_ok": r["in_guards"][0] == guard and r["in_guards"][1] == guard,
               "out_guards_ok": guards_ok([r["out_guards"]]) and guards_ok(r["aux_guards"])}
        if c.fuse == 1:
            hi, lo = cl.split_halves(r["out"], c.opos, c.cols)
            dev = cl.halves_value(hi, lo)
            want = memo("pn_ref", lambda: cl.ref_pixelnorm(ref).reshape(-1, c.cols) * cl.ACT_SCALE)
            res["finite"] = bool(np.isfinite(dev).all())
            res["ratio"] = ratio(dev, want, cl.bound_split(want))
            if cl.epi_exact(c):
                against_oracle(res, "pn_oracle", [hi, lo], lambda: cl.oracle_pixelnorm(stored32))
        else:
            res["out_untouched"] = untouched(r["out"])          # "`out` is NOT written"
        if c.fuse == 2:
            rgb = cl.decode_rgb(r["rgb"].tobytes(), c.opos)
            want, S = cl.ref_rgb(memo("pn_true", lambda: cl.ref_pixelnorm(ref)), d["rgb_w"][:c.rgb_n], d["rgb_b"][:c.rgb_n])
            res["finite"] = bool(np.isfinite(rgb).all())
            res["ratio"] = ratio(rgb[:, :c.rgb_n].astype(np.float64), want, cl.bound_rgb(want, S))
            res["pad_zero"] = bool((np.ascontiguousarray(rgb[:, c.rgb_n:]).view(np.uint32) == 0).all())
        if c.fuse == 3:
            check_tap(c, res, r["V"], r.get("pool"), stored32, ref, d["tap_coef"], cl.epi_exact(c))
        if cl.chain_applies(c):
            if unfused is None:
                unfused = launch(c.name, cl.run_layer, ctx.lib, ctx.handle, c, d, fuse=0)
                assert unfused["form"] == r["form"]
            p = launch(c.name, cl.run_split_post, ctx.lib, ctx.handle, c, unfused["out"], d["tap_coef"])
            res["chain_guards_ok"] = guards_ok(p["guards"])
            if c.fuse == 1:
                res["chain_equal"] = p["act"] == r["out"]
            else:
                res["chain_equal"] = bool(p["act"] == unfused["out"] and np.array_equal(p["V"], r["V"]) and
                                          (not c.tap_pool or np.array_equal(p["pool"], r["pool"])))
            res["chain_sat_equal"] = (unfused["sat_delta"] > 0) == (r["sat_delta"] > 0)
        out[c.name] = res
    del cache, memo

# ------------------------------------------------------------------------------------------ what the launcher must refuse
for c in cl.REFUSE_CASES:
    d = cl.make_epi_inputs(c)
    try:
        r = cl.run_layer(ctx.lib, ctx.handle, c, d)
        out[c.name] = {"refused": False, "form": r["form"]}
    except RuntimeError as e:
        out[c.name] = {"refused": True, "message": str(e)}

# ------------------------------------------------------------------------------------------------ the stand-alone kernels
for key, group in itertools.groupby(sorted(cl.POST_CASES, key=lambda c: c.key), key=lambda c: c.key):
    group = list(group)
    d = cl.make_post_inputs(group[0])
    stored32 = d["stored"]
    true = stored32.astype(np.float64) / cl.ACT_SCALE
    act = cl.encode_split(stored32)
    cache = {}
    memo = lambda k, f: cache[k] if k in cache else cache.setdefault(k, f())
    for c in group:
        p = launch(c.name, cl.run_split_post, ctx.lib, ctx.handle, c, act, d["tap_coef"])
        res = {"out_guards_ok": guards_ok(p["guards"])}
        if c.op == 0:
            hi, lo = cl.split_halves(p["act"], c.positions, c.C)
            dev = cl.halves_value(hi, lo)
            want = cl.ref_pixelnorm(true) * cl.ACT_SCALE
            res["finite"] = bool(np.isfinite(dev).all())
            res["ratio"] = ratio(dev, want, cl.bound_split(want))
            if c.inputs == "exact":
                against_oracle(res, "pn_oracle", [hi, lo], lambda: cl.oracle_pixelnorm(stored32))
        else:
            res["input_untouched"] = p["act"] == act
            check_tap(c, res, p["V"], p["pool"], stored32, true, d["tap_coef"], c.inputs == "exact")
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
    for k in ("GL_H3_XONCE", "GL_H3_T4", "GL_H3_HALO", "GL_H3_TILE128", "GL_HALO_RING", "GL_HALO_DIAG", "GL_TAP_FUSE", "GL_PIXNORM_FUSE", "GL_RGB_FUSE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    line = [l for l in r.stdout.decode().splitlines() if l.startswith("RESULT ")][-1]
    out = json.loads(line[7:])
    print(json.dumps(out, indent=1))
    return out


CHILD_TIMEOUT = 180             # the child takes ~18 s on an MI355X (measured, see the docstring), most of it the host-side decoding


def common_checks(c, r):
    assert "error" not in r, r
    assert r["form"] == c.form, "case written for form 0x%x ran as 0x%x" % (c.form, r["form"])
    assert r["in_guards_ok"] and r["out_guards_ok"], r
    assert r["finite"], r
    print("%s: largest error / bound %.3f" % (c.name, r["ratio"]))
    assert r["ratio"] <= 1.0, r
    if cl.epi_exact(c):
        assert r["nbad"] == 0, r                                  # device halves == the oracle's, zero tolerance
    if cl.chain_applies(c):
        assert r["chain_guards_ok"], r
        assert r["chain_equal"], "fused and unfused bytes differ: %r" % (r,)
        assert r["chain_sat_equal"], r


@pytest.mark.parametrize("c", [c for c in cl.PN_CASES if c.sat is None], ids=repr)
def test_fused_pixelnorm(c, result):
    """exact cases: the stored halves equal the oracle's; act 2: within |ref| 2^-21 + 2^-24 of float64; 64 / 128 channels: == unfused + pixelnorm_split_kernel"""
    r = result[c.name]
    common_checks(c, r)
    assert r["sat_delta"] == 0, r


def test_fused_pixelnorm_counts_the_pass_1_clamp_exactly_when_it_happens(result):
    lo, hi = result["pn_sat_below"], result["pn_sat_above"]
    common_checks(cl.EPI_BY_NAME["pn_sat_below"], lo)
    common_checks(cl.EPI_BY_NAME["pn_sat_above"], hi)             # against the reference of the CLAMPED activations: only the one value differs
    assert lo["sat_delta"] == 0 and hi["sat_delta"] > 0, (lo, hi)


@pytest.mark.parametrize("c", cl.RGB_CASES, ids=repr)
def test_fused_torgb(c, result):
    """rgb_out within S 2^-20 + 2^-24 |ref| of b + W . v_norm in float64; columns >= rgb_n exactly 0; `out` not written"""
    r = result[c.name]
    common_checks(c, r)
    assert r["out_untouched"] and r["pad_zero"], r
    assert r["sat_delta"] == 0, r


@pytest.mark.parametrize("c", cl.TAP_CASES, ids=repr)
def test_fused_tap(c, result):
    """V rows (and the pooled tensor) equal the oracle's halves at tap_row0 + img, tap_off + pin * cols + ch in every format and layout; the rest
    of the V buffer and `out` keep the sentinel; 64 / 128 channels: == unfused + lpips_tap(_pool)_split_kernel"""
    r = result[c.name]
    common_checks(c, r)
    assert r["out_untouched"] and r["v_rest_sentinel"], r
    if c.tap_pool:
        assert r["nbad_pool"] == 0, r
    assert r["sat_delta"] == 0, r


@pytest.mark.parametrize("switch", ["GL_PIXNORM_FUSE", "GL_TAP_FUSE"])
def test_switching_a_fused_epilogue_off_changes_no_bit_of_a_network(switch, result):
    """PGGAN (128 channels, 64 x 64, split-fp16) images under GL_PIXNORM_FUSE=0 (toRGB unfused in both arms: the fused toRGB needs the fused
    PixelNorm), VGG16 + LPIPS rows (32 x 32 images, split and search rows) under GL_TAP_FUSE=0: equal to the fused arm's, bit for bit"""
    r = result["switches"]
    assert r["pggan_finite"] and r["saturations"] == 0, r
    assert r[switch], r


def test_unfused_torgb_stays_within_the_generators_tolerance(result):
    """GL_RGB_FUSE=0 runs toRGB as a split-fp16 convolution with split weights instead of the epilogue's float32 fma chain: not the same bits (the
    arms really differ), but within tests/test_gpu_pggan.py's 5e-5 on images in (-1, 1).  Measured: 1.1e-6"""
    d = result["switches"]["GL_RGB_FUSE_maxdiff"]
    print("GL_RGB_FUSE=0 against the default: largest difference %.3g" % d)
    assert 0.0 < d < 5e-5


@pytest.mark.parametrize("c", cl.REFUSE_CASES, ids=repr)
def test_launcher_refuses(c, result):
    r = result[c.name]
    assert r["refused"] and c.refused in r["message"], r


@pytest.mark.parametrize("c", cl.POST_CASES, ids=repr)
def test_stand_alone_kernel(c, result):
    r = result[c.name]
    assert "error" not in r, r
    assert r["out_guards_ok"] and r["finite"], r
    print("%s: largest error / bound %.3f" % (c.name, r["ratio"]))
    assert r["ratio"] <= 1.0, r
    if c.inputs == "exact":
        assert r["nbad"] == 0, r
    if c.op:
        assert r["input_untouched"] and r["v_rest_sentinel"], r
    if c.op == 2:
        assert r["nbad_pool"] == 0, r



EXACT_CASES = [c for c in cl.EPI_CASES if cl.epi_exact(c)] + [c for c in cl.POST_CASES if c.inputs == "exact"]


@pytest.mark.parametrize("c", EXACT_CASES, ids=repr)
def test_exact_case_equals_the_correctly_rounded_oracle(c, result):
    """device halves == the oracle whose float32 steps (/, sqrt, +, *) are each correctly rounded (numpy float32), zero tolerance: the check
    that found the 1-ulp square root, on its own so that it names the case"""
    r = result[c.name]
    assert "error" not in r, r
    assert r["nbad"] == 0, r
