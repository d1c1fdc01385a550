"""Cases, host references and the GPU entry of the per-kernel tests of attention_core_kernel<C, SPLIT> (csrc/gl_dcgan.hip).  No GPU needed to import.

The kernel, per image of T = 256 positions:  energy_ij = q_i . k_j,  p = softmax_j(energy),  out_i = sum_j p_ij v_j,  y = gamma * out + x,
with q, k (C / 8 channels) and v (C channels) read from fp32 rows [position][q | k | v], and x / y either fp32 NHWC or the split-fp16
activation layout (stored value = true value * 16; per position and 32-channel chunk 32 hi halves, then 32 lo halves).

Every case has n = 3 images: image 1 differs from images 0 and 2, which are equal (their outputs must be equal bit for bit, and equal to
the n = 1 run of image 0).  Exact cases are built so that every value the kernel can form, in any order, is exactly representable
(tests/test_attention_cpu.py asserts those preconditions); real-valued cases come with a float64 reference, a float32 torch evaluation of
the same formula and a host-side allowance for the hardware exponential.
"""
import ctypes

import numpy as np

import conv_layer_common as cl

T = 256
N_IMG = 3
ACT_SCALE = 16.0
F16_MAX = 65504.0
SENTINEL = 0xA5
POISON = 64.0
GUARD = 4096
SLACK = 4.0                 # tests/test_gpu_wb.py: device error <= SLACK * the float32 CPU evaluation's
LOG2E = 1.4426950408889634
EXP_ZERO_GAP = 104          # exp2(fl32(t * log2 e)) is 0 in float32 for t <= -104: 104 * log2 e = 150.04 > 150 (half the smallest subnormal)


def code(j):
    """{-1, +1}^8 from the bits of j"""
    j = np.asarray(j)
    return (((j[..., None] >> np.arange(8)) & 1) * 2 - 1).astype(np.float32)


def perm(img):
    """pi(i) = (97 i + 41) mod 256 (image 1: + 128): a bijection without fixed point (96 i = -41 or -169 mod 256 has no solution: odd) that
    moves rows across the 32-row blocks and the lane halves"""
    return (97 * np.arange(T) + 41 + (128 if img == 1 else 0)) % T


class Case:
    def __init__(self, kind, C, split, gamma, b=None, temp=None, x_zero=False):
        self.kind, self.C, self.split, self.gamma, self.b, self.temp, self.x_zero = kind, C, bool(split), float(gamma), b, temp, x_zero
        self.DK = C // 8
        self.base = kind + ("_b%d" % b if b is not None else "") + ("_%s" % temp if temp else "") + ("_x0" if x_zero else "")
        self.name = "%s_c%d_%s" % (self.base, C, "split" if split else "f32")
        self.exact = kind != "real"

    def __repr__(self):
        return self.name


TEMPS = {"mild": 0.9, "peaked": 12.0, "extreme": 1500.0}      # standard deviation of the energies
ALL_CASES = []
for _C in (64, 128):
    for _split in (False, True):
        ALL_CASES += [Case("uniform", _C, _split, 0.5), Case("uniform_lo", _C, _split, 0.5), Case("onehot", _C, _split, 2.0),
                      Case("twohot", _C, _split, 0.25, b=2), Case("twohot", _C, _split, -1.0, b=5)]
        if _split:
            ALL_CASES += [Case("clamp_at", _C, True, 1.0), Case("clamp_over", _C, True, 1.0)]
        for _t in TEMPS:
            ALL_CASES += [Case("real", _C, _split, 0.7, temp=_t, x_zero=True), Case("real", _C, _split, 0.7, temp=_t)]
EXACT_CASES = [c for c in ALL_CASES if c.exact]
REAL_CASES = [c for c in ALL_CASES if not c.exact]
BY_NAME = {c.name: c for c in ALL_CASES}
CLAMP_V, CLAMP_X_AT, CLAMP_X_OVER = 4000.0, 1504.0, 1520.0    # 16 * 4000 + 1504 = 65504 (the largest fp16), + 1520 = 65520


def clamp_sites(img):
    """(position, channel, sign) of the two extreme elements of an image (image 2 is image 0)"""
    img %= 2
    return [(10 + 50 * img, 5, 1.0), (200 - 50 * img, 26 + img, -1.0)]


def split_round(x):
    """float32 true values -> what the split layout holds for them (float64)"""
    sh = x.shape
    return cl.decode_split(cl.encode_split(x.reshape(-1, sh[-1]) * np.float32(ACT_SCALE)), x.size // sh[-1], sh[-1]).reshape(sh) / ACT_SCALE


def make_inputs(c):
    """dict(q [n][T][DK], k, v [n][T][C], x [n][T][C]) float32 true values; x is representable in the layout of the case"""
    import zlib
    rng = np.random.default_rng(zlib.crc32(c.base.encode()) + c.C)       # fp32 and split share the draws
    n, C, DK = N_IMG, c.C, c.DK
    q, k = np.zeros((n, T, DK), np.float32), np.zeros((n, T, DK), np.float32)
    if c.exact:
        v = rng.integers(1, 9, (n, T, C)).astype(np.float32) * rng.choice([-1.0, 1.0], (n, T, C)).astype(np.float32)
        lim = 4095 if c.kind == "uniform_lo" else 2047                   # stored x = integer: above 2048 an odd one needs its lo half
        xs = rng.integers(1, lim + 1, (n, T, C)).astype(np.float32) * rng.choice([-1.0, 1.0], (n, T, C)).astype(np.float32)
        if c.kind == "uniform_lo":
            xs[:, ::3, 1::2] = np.sign(xs[:, ::3, 1::2]) * (2049 + 2 * (np.abs(xs[:, ::3, 1::2]) % 1023))     # odd, in (2048, 4095]
        for img in range(n):
            p = perm(img)
            if c.kind.startswith("uniform"):
                k[img] = rng.integers(-9, 10, (T, DK))
            else:
                k[img, :, :8] = 8 * code(np.arange(T))
                q[img, :, :8] = 8 * code(p) if c.kind != "twohot" else 8 * (code(p) + code(p ^ (1 << c.b)))
            if c.kind.startswith("clamp"):
                for (i, ch, s) in clamp_sites(img):
                    v[img, p[i], ch] = s * CLAMP_V
                    xs[img, i, ch] = s * (CLAMP_X_AT if c.kind == "clamp_at" else CLAMP_X_OVER)
        x = xs / np.float32(ACT_SCALE)
    else:
        s = np.sqrt(TEMPS[c.temp] / np.sqrt(DK))
        q = (rng.standard_normal((n, T, DK)) * s).astype(np.float32)
        k = (rng.standard_normal((n, T, DK)) * s).astype(np.float32)
        v = rng.standard_normal((n, T, C)).astype(np.float32)
        x = rng.standard_normal((n, T, C)).astype(np.float32)
        if c.x_zero:
            x[:] = 0
        elif c.split:
            x = split_round(x).astype(np.float32)
    d = {"q": q, "k": k, "v": v, "x": x}
    for a in d.values():
        a[2] = a[0]
    return d


def reference64(c, d):
    """float64 softmax attention -> (y [n][T][C], p [n][T][T], t = energy - row max, out)"""
    q, k, v, x = (d[n].astype(np.float64) for n in ("q", "k", "v", "x"))
    e = np.einsum("nid,njd->nij", q, k)
    t = e - e.max(axis=2, keepdims=True)
    p = np.exp(t)
    p /= p.sum(axis=2, keepdims=True)
    out = np.einsum("nij,njc->nic", p, v)
    return c.gamma * out + x, p, t, out


def reference32(c, d):
    """the same formula in float32, torch on the CPU -> float64 array"""
    import torch
    q, k, v, x = (torch.from_numpy(np.array(d[n])) for n in ("q", "k", "v", "x"))
    p = torch.softmax(torch.bmm(q, k.transpose(1, 2)), dim=-1)
    return (np.float32(c.gamma) * torch.bmm(p, v) + x).numpy().astype(np.float64)


def closed_form(c, d):
    """what an exact case must give, written without a softmax (float64; clamp_over: before the clamp)"""
    v, x = d["v"].astype(np.float64), d["x"].astype(np.float64)
    if c.kind.startswith("uniform"):
        return c.gamma / 256.0 * v.sum(axis=1, keepdims=True) + x
    y = np.empty_like(x)
    for img in range(N_IMG):
        p = perm(img)
        y[img] = c.gamma * v[img, p] + x[img] if c.kind != "twohot" else c.gamma / 2.0 * (v[img, p] + v[img, p ^ (1 << c.b)]) + x[img]
    return y


def expected_exact(c, d):
    """closed form with the split store's clamp applied"""
    y = closed_form(c, d)
    return np.clip(y * ACT_SCALE, -F16_MAX, F16_MAX) / ACT_SCALE if c.split else y


def weights32(d):
    """the float32 weights exp2(fl32((e - max) * log2 e)) of integer energies (exact in float32) -> (weights, sorted energies)"""
    e = np.einsum("nid,njd->nij", d["q"].astype(np.float64), d["k"].astype(np.float64))
    assert np.array_equal(e, e.astype(np.float32))
    t = (e - e.max(axis=2, keepdims=True)).astype(np.float32)
    return np.exp2((t * np.float32(LOG2E)).astype(np.float32)).astype(np.float32), np.sort(e, axis=2)


def exactness_problems(c, d):
    bad = []
    q, k, v, x = (d[n].astype(np.float64) for n in ("q", "k", "v", "x"))
    for name, a in (("q", q), ("k", k), ("v", v), ("16 x", x * ACT_SCALE)):
        if not np.array_equal(a, np.round(a)):
            bad.append(name + " is not integer")
    if not np.einsum("nid,njd->nij", np.abs(q), np.abs(k)).max() < 2.0 ** 24:
        bad.append("sum of absolute q k products not below 2^24")
    if not np.abs(v).sum(axis=1).max() < 2.0 ** 24:
        bad.append("sum of |v| over j not below 2^24")
    m, e = np.frexp(abs(c.gamma))
    if m != 0.5:
        bad.append("gamma is no power of two")
    y = closed_form(c, d)
    if not np.array_equal(y.astype(np.float32).astype(np.float64), y):
        bad.append("result not a float32")
    if c.split:
        if not np.array_equal(split_round(d["x"]), x):
            bad.append("x not representable as hi + lo")
        yc = expected_exact(c, d)
        if not np.array_equal(split_round(yc.astype(np.float32)), yc):
            bad.append("result not representable as hi + lo")
        if c.kind != "clamp_over" and np.abs(y * ACT_SCALE).max() > F16_MAX:
            bad.append("result beyond the fp16 range")
    return bad


def exp_allowance(c, d, ref=None):
    """(b) of the bound, per image, in the row metric: a weight formed as exp2(fl32(t log2 e)), t = e - max <= 0, has relative error at most
    (|t| + 1) 2^-23, so the attention output moves by at most A[i, c] = 2^-23 sum_j p[i, j] (|t[i, j]| + 1) |v[j, c] - out[i, c]|"""
    y, p, t, out = ref if ref is not None else reference64(c, d)
    v = d["v"].astype(np.float64)
    w = p * (np.abs(t) + 1.0)
    res = np.empty(N_IMG)
    for img in range(N_IMG):
        A = np.empty((T, c.C))
        for i0 in range(0, T, 32):
            A[i0:i0 + 32] = np.einsum("ij,ijc->ic", w[img, i0:i0 + 32], np.abs(v[img][None, :, :] - out[img, i0:i0 + 32, None, :]))
        res[img] = np.linalg.norm(abs(c.gamma) * A * 2.0 ** -23) / np.linalg.norm(y[img])
    return res


def row_errors(got, want64):
    """the project's row metric (tests/wb_common.py), one row per image"""
    got, want64 = np.asarray(got, np.float64).reshape(len(got), -1), np.asarray(want64, np.float64).reshape(len(want64), -1)
    return np.linalg.norm(got - want64, axis=1) / np.linalg.norm(want64, axis=1)


# ------------------------------------------------------------------------------------------------------------ the GPU entry
def pack_qkv(d, imgs):
    return np.ascontiguousarray(np.concatenate([d["q"][imgs], d["k"][imgs], d["v"][imgs]], axis=2), np.float32)


def x_bytes(c, d, imgs):
    x = np.ascontiguousarray(d["x"][imgs], np.float32)
    return cl.encode_split(x.reshape(-1, c.C) * np.float32(ACT_SCALE)) if c.split else x.tobytes()


def decode_y(c, buf, n):
    """raw y bytes -> float64 true values [n][T][C]"""
    if c.split:
        return cl.decode_split(buf, n * T, c.C).reshape(n, T, c.C) / ACT_SCALE
    return np.frombuffer(buf, np.float32).astype(np.float64).reshape(n, T, c.C)


class TuneAttention(ctypes.Structure):          # csrc/gl_tune.hip GlTuneAttention
    _fields_ = [("C", ctypes.c_int32), ("split", ctypes.c_int32), ("n_img", ctypes.c_int64),
                ("gamma", ctypes.c_float), ("poison", ctypes.c_float), ("sentinel", ctypes.c_int32), ("reserved_i", ctypes.c_int32),
                ("qkv", ctypes.c_void_p), ("x", ctypes.c_void_p), ("y", ctypes.c_void_p), ("out_guards", ctypes.c_void_p),
                ("sat_delta", ctypes.c_int64)]


def run_attention(lib, ctx_handle, c, d, imgs):
    """one launch through gl_tune_attention on the images `imgs` -> dict(y=bytes, guards=(lo, hi), sat_delta)"""
    imgs = list(imgs)
    qkv = pack_qkv(d, imgs)
    xb = np.frombuffer(x_bytes(c, d, imgs), np.uint8).copy()
    assert qkv.shape == (len(imgs), T, 2 * c.DK + c.C) and len(xb) == len(imgs) * T * c.C * 4
    y = np.empty(len(xb), np.uint8)
    og = np.empty(2 * GUARD, np.uint8)
    a = TuneAttention()
    a.C, a.split, a.n_img, a.gamma, a.poison, a.sentinel = c.C, int(c.split), len(imgs), c.gamma, POISON, SENTINEL
    a.qkv, a.x, a.y, a.out_guards = qkv.ctypes.data, xb.ctypes.data, y.ctypes.data, og.ctypes.data
    lib.gl_tune_attention.restype = ctypes.c_int
    lib.gl_tune_attention.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    rc = lib.gl_tune_attention(ctx_handle, ctypes.byref(a))
    if rc != 0:
        lib.gl_last_error.restype = ctypes.c_char_p
        raise RuntimeError("gl_tune_attention(%s): %s" % (c.name, lib.gl_last_error().decode()))
    return {"y": y.tobytes(), "guards": (og[:GUARD].tobytes(), og[GUARD:].tobytes()), "sat_delta": int(a.sat_delta)}
