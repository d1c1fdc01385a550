"""One convolution layer against a plain float64 convolution: what tests/test_conv_layers_cpu.py and tests/test_gpu_conv_layers.py share.

A case is one GlGatherConv problem (csrc/gl_conv.h) for ONE launch of gl_launch_gather_conv (kernel "f32") or gl_launch_gather_conv_h3
(kernel "h3"), run through the tuning build's gl_tune_conv_layer (csrc/gl_tune.hip).  Here: the case table, the input generators, the
float64 reference (torch.nn.functional.conv2d on the NCHW view with explicit zero padding), the decoders of the split and planar output
layouts (the entry returns raw bytes, so the layouts are under test too) and the exactness preconditions.

Why the structural cases can be compared with ZERO tolerance: activations are integers in {1, 2, 3} (no zeros: a missing zero fill or a stale
LDS guard shows), weights integers in {-2, -1, 1, 2}, scale a power of two per channel, shift and residual small integers.  Every product and
every partial sum is then an integer multiple of one unit and below 2^24 units, so any summation order, on any matrix core, is exact, and so
is the one rounding of the epilogue's fma when the result is a float32 number: the device must return float32(reference) bit for bit.
The preconditions (sum of absolute products < 2^24 units, float32(ref) == ref, split output representable as hi + lo below the fp16 limit) are
asserted on the CPU from the reference alone.
"""
import ctypes
import os
import time

import numpy as np
import torch
import torch.nn.functional as F

ACT_SCALE = 16.0            # csrc/gl_dcgan.hip kActScale: what stored split activations carry
POISON = 64.0               # value of the input guards
SENTINEL = 0xA5             # byte the output and its guards are pre-filled with
OUT_GUARD = 4096
F16_MAX = 65504.0

FP32_WIDE, FP32_NARROW = 0x100, 0x101
H3, UP, T4, XONCE = 0x200, 0x10, 0x20, 0x40
HALO = 0x400
KY = [[1, 3], [0, 2]]       # ConvTranspose2d k4 s2 p1: kernel row of tap ty of output parity py (csrc/gl_dcgan.hip kKy), offsets below
DY = [[0, -1], [1, 0]]


def tap_sets(kind):
    """-> (taps per phase [(dy, dx)], oy, ox, omul)"""
    if kind == "c3":
        return [[(t // 3 - 1, t % 3 - 1) for t in range(9)]], [0], [0], 1
    if kind == "one":
        return [[(0, 0)]], [0], [0], 1
    assert kind == "ct"
    sets, oy, ox = [], [], []
    for py in range(2):
        for px in range(2):
            sets.append([(DY[py][ty], DY[px][tx]) for ty in range(2) for tx in range(2)])
            oy.append(py)
            ox.append(px)
    return sets, oy, ox, 2


class Case(object):
    def __init__(self, name, kernel, taps, n, H, W, Cin, cols, form, out="f32", cmod=None, act=0, up=0, residual=False, tail=False,
                 cols_pad=None, inputs="struct", env=None, big=False, sat=None, atol=None, data=None):
        self.name, self.kernel, self.kind, self.n, self.H, self.W, self.Cin, self.cols, self.form = name, kernel, taps, n, H, W, Cin, cols, form
        self.taps, self.oy, self.ox, self.omul = tap_sets(taps)
        self.phases, self.ntaps = len(self.taps), len(self.taps[0])
        self.Ho, self.Wo = H * self.omul, W * self.omul
        self.out = out                        # "f32" row-major, "planar", "split"
        self.cmod = cmod or cols
        self.act, self.up, self.residual, self.tail = act, up, residual, tail
        self.cols_pad = cols_pad or (cols + 127) // 128 * 128
        self.inputs = inputs                  # struct | arith_w | arith_x | real | act34
        self.env = env or {}                  # tuning switches for this launch
        self.big = big
        self.key = data or name               # cases with the same key (a tuning switch apart) share inputs and reference
        self.sat = sat                        # None | "below" | "above": the largest split value just inside / outside the fp16 range
        self.atol = atol                      # None: exact
        self.positions = n * H * W
        self.opos = n * self.Ho * self.Wo
        self.ld_planar = self.positions
        self.wexp = 11 if inputs in ("struct", "arith_x", "act34") else 12
        self.tail_wexp = 11

    @property
    def in_guard(self):
        g = (2 * (self.W + 1) * self.Cin * 4 + 4095) // 4096 * 4096
        row = self.Cin * 4
        return (g + row - 1) // row * row

    @property
    def out_bytes(self):
        if self.tail:
            return 48 * self.opos * 4
        if self.out == "planar":
            return self.cols * self.ld_planar * 4
        return self.opos * self.cols * 4

    def __repr__(self):
        return self.name


def _pad(cols, pad):
    """cols_pad the fp32 launcher maps to its wide (pad 128) / narrow (pad 64: a multiple of 64 that is none of 128) tile"""
    p = (cols + pad - 1) // pad * pad
    return p if pad == 128 or p % 128 else p + 64


def _cases():
    c = []
    # 1: h3 tile 0 (<2,2>, 128 x 128): 216 positions = a ragged second tile that starts mid-row and mid-image
    for cin in (32, 64):
        c.append(Case("t0_c3_cin%d_cols96_split" % cin, "h3", "c3", 3, 6, 12, cin, 96, H3 | 0, out="split"))
        c.append(Case("t0_c3_cin%d_cols96_f32" % cin, "h3", "c3", 3, 6, 12, cin, 96, H3 | 0))
        c.append(Case("t0_c3_cin%d_cols160_f32" % cin, "h3", "c3", 3, 6, 12, cin, 160, H3 | 0))
    # 2: h3 tile 1 (<1,4>): one tap, 300 positions
    c.append(Case("t1_one_cols48_f32", "h3", "one", 3, 10, 10, 32, 48, H3 | 1))
    c.append(Case("t1_one_cols48_planar", "h3", "one", 3, 10, 10, 32, 48, H3 | 1, out="planar"))
    c.append(Case("t1_one_cols64_split", "h3", "one", 3, 10, 10, 32, 64, H3 | 1, out="split"))
    # 3: the layer-0 form: H = W = 1, c % cmod wraps
    for n in (5, 131):
        c.append(Case("l0_n%d_split" % n, "h3", "one", n, 1, 1, 128, 256, H3 | 0, out="split", cmod=16))
        c.append(Case("l0_n%d_f32" % n, "h3", "one", n, 1, 1, 128, 256, H3 | 0, cmod=16))
    # 4: h3 tile 2 (<2,4,8,4>): 16192 positions is the smallest count over the >= 256 workgroups threshold; 252 images stay on tile 0
    c.append(Case("t2_ct_n253", "h3", "ct", 253, 8, 8, 32, 256, H3 | 2, out="split", big=True))
    c.append(Case("t2_ct_n252_is_tile0", "h3", "ct", 252, 8, 8, 32, 256, H3 | 0, out="split", big=True))
    # 5: T4, and the raster form of the same problems
    for env, form, tag in (({}, H3 | 2 | T4, "t4"), ({"GL_H3_T4": "0"}, H3 | 2, "t4off")):
        c.append(Case("%s_ct_n1011" % tag, "h3", "ct", 1011, 4, 4, 32, 256, form, out="split", env=env, big=True, data="t4_ct_n1011"))
        c.append(Case("%s_c3_n4081" % tag, "h3", "c3", 4081, 4, 4, 32, 256, form, out="split", env=env, big=True, data="t4_c3_n4081"))
    # 6: h3 tile 5 (<1,8,8,4>): 24 x 24 is no multiple of the halo kernel's 16 x 16 block
    c.append(Case("t5_c3_n455", "h3", "c3", 455, 24, 24, 32, 96, H3 | 5, out="split", big=True))
    # 7: UP (input stored at half the grid)
    c.append(Case("up_t0_c3", "h3", "c3", 3, 6, 12, 32, 96, H3 | 0 | UP, out="split", up=1))
    c.append(Case("up_t1_one", "h3", "one", 3, 10, 10, 32, 48, H3 | 1 | UP, up=1))
    c.append(Case("up_t2_ct_n253", "h3", "ct", 253, 8, 8, 32, 256, H3 | 2 | UP, out="split", up=1, big=True))
    c.append(Case("up_t5_c3_n455", "h3", "c3", 455, 24, 24, 32, 96, H3 | 5 | UP, out="split", up=1, big=True))
    # 8: halo: 171 images of 32 x 48 = 1026 blocks of 16 x 16, just over the 1024-block threshold; and the tap-gather form of the same
    for cin in (32, 64):
        for cols, wcols, off in ((64, 1, H3 | 1), (96, 2, H3 | 5)):
            c.append(Case("halo%d_cin%d_cols%d" % (wcols, cin, cols), "h3", "c3", 171, 32, 48, cin, cols, HALO | wcols, out="split", big=True))
            c.append(Case("halo%d_off_cin%d_cols%d" % (wcols, cin, cols), "h3", "c3", 171, 32, 48, cin, cols, off, out="split",
                          env={"GL_H3_HALO": "0"}, big=True, data="halo%d_cin%d_cols%d" % (wcols, cin, cols)))
    # 9: fused RGB tail (act 1, then the 48-column GEMM in the epilogue)
    for n in (1, 3):
        c.append(Case("tail_16x16_n%d_cols128_xonce" % n, "h3", "ct", n, 16, 16, 32, 128, H3 | 3 | XONCE, out="split", act=1, tail=True))
        c.append(Case("tail_16x16_n%d_cols128_xonce_off" % n, "h3", "ct", n, 16, 16, 32, 128, H3 | 3, out="split", act=1, tail=True,
                      env={"GL_H3_XONCE": "0"}, data="tail_16x16_n%d_cols128_xonce" % n))
        c.append(Case("tail_16x16_n%d_cols64" % n, "h3", "ct", n, 16, 16, 32, 64, H3 | 4, out="split", act=1, tail=True))
    c.append(Case("tail_8x8_n3_cols128", "h3", "ct", 3, 8, 8, 32, 128, H3 | 3, out="split", act=1, tail=True))
    c.append(Case("tail_8x8_n3_cols64", "h3", "ct", 3, 8, 8, 32, 64, H3 | 4, out="split", act=1, tail=True))
    # 10: the fp32 kernel, <2,2,2,2> (cols_pad 128) and <4,1,1,2> (cols_pad 64), on the shapes of cases 1 to 3
    for pad, form, tag in ((128, FP32_WIDE, "w"), (64, FP32_NARROW, "n")):
        for cin in (32, 64):
            c.append(Case("f32%s_c3_cin%d_cols96" % (tag, cin), "f32", "c3", 3, 6, 12, cin, 96, form, cols_pad=_pad(96, pad)))
        c.append(Case("f32%s_c3_cols160" % tag, "f32", "c3", 3, 6, 12, 32, 160, form, cols_pad=_pad(160, pad)))
        c.append(Case("f32%s_one_cols48" % tag, "f32", "one", 3, 10, 10, 32, 48, form, cols_pad=_pad(48, pad)))
        c.append(Case("f32%s_one_cols48_planar" % tag, "f32", "one", 3, 10, 10, 32, 48, form, out="planar", cols_pad=_pad(48, pad)))
        c.append(Case("f32%s_c3_planar" % tag, "f32", "c3", 3, 6, 12, 32, 96, form, out="planar", cols_pad=_pad(96, pad)))
        c.append(Case("f32%s_l0_n5" % tag, "f32", "one", 5, 1, 1, 128, 256, form, cmod=16, cols_pad=_pad(256, pad)))
        c.append(Case("f32%s_l0_n131" % tag, "f32", "one", 131, 1, 1, 128, 256, form, cmod=16, cols_pad=_pad(256, pad)))
        c.append(Case("f32%s_ct_residual_cmod1" % tag, "f32", "ct", 3, 6, 12, 32, 96, form, cmod=1, residual=True,
                      cols_pad=_pad(96, pad)))
        c.append(Case("f32%s_up_c3" % tag, "f32", "c3", 3, 6, 12, 32, 96, form, up=1, cols_pad=_pad(96, pad)))
        c.append(Case("f32%s_up_ct" % tag, "f32", "ct", 3, 6, 12, 32, 96, form, up=1, cols_pad=_pad(96, pad)))
    return c


def _arith_cases():
    """split arithmetic: one operand carries a low half (1 + b 2^-12), the other is an integer; fp32 output, act 0; shapes of cases 1, 5, 8"""
    c = []
    for kind in ("arith_w", "arith_x"):
        c.append(Case("%s_t0_c3_cin64" % kind, "h3", "c3", 3, 6, 12, 64, 96, H3 | 0, inputs=kind))
        c.append(Case("%s_t4_ct_n1011" % kind, "h3", "ct", 1011, 4, 4, 32, 256, H3 | 2 | T4, inputs=kind, big=True))
        c.append(Case("%s_t4_c3_n4081" % kind, "h3", "c3", 4081, 4, 4, 32, 256, H3 | 2 | T4, inputs=kind, big=True))
        c.append(Case("%s_halo1_cin64" % kind, "h3", "c3", 171, 32, 48, 64, 64, HALO | 1, inputs=kind, big=True))
        c.append(Case("%s_halo2_cin64" % kind, "h3", "c3", 171, 32, 48, 64, 96, HALO | 2, inputs=kind, big=True))
    return c


def _act_cases():
    c = []
    for act in (1, 2):
        c.append(Case("act%d_h3_t0" % act, "h3", "c3", 3, 6, 12, 32, 96, H3 | 0, act=act))
        c.append(Case("act%d_f32w" % act, "f32", "c3", 3, 6, 12, 32, 96, FP32_WIDE, act=act))
        c.append(Case("act%d_f32n" % act, "f32", "c3", 3, 6, 12, 32, 96, FP32_NARROW, act=act, cols_pad=192))
    c.append(Case("act1_h3_split", "h3", "c3", 3, 6, 12, 32, 96, H3 | 0, act=1, out="split"))
    for act in (3, 4):                # fp32 kernel only; the project's golden tolerance against float64
        c.append(Case("act%d_f32w" % act, "f32", "c3", 3, 6, 12, 32, 96, FP32_WIDE, act=act, inputs="act34", atol=2e-5))
        c.append(Case("act%d_f32n_residual" % act, "f32", "ct", 3, 6, 12, 32, 96, FP32_NARROW, act=act, inputs="act34", atol=2e-5, residual=True,
                      cols_pad=192))
    c.append(Case("sat_below", "h3", "c3", 3, 6, 12, 32, 96, H3 | 0, out="split", sat="below"))
    c.append(Case("sat_above", "h3", "c3", 3, 6, 12, 32, 96, H3 | 0, out="split", sat="above"))
    return c


def _real_cases():
    """Gaussian activations after ReLU, He-scale weights, scale 1, shift 0: error against float64 relative to a float32 CPU conv2d's"""
    return [Case("real_t0_c3_cin64", "h3", "c3", 3, 6, 12, 64, 96, H3 | 0, inputs="real"),
            Case("real_t2_ct_n253", "h3", "ct", 253, 8, 8, 32, 256, H3 | 2, inputs="real", big=True),
            Case("real_halo2_cin64", "h3", "c3", 171, 32, 48, 64, 96, HALO | 2, inputs="real", big=True),
            Case("real_halo1_cin32", "h3", "c3", 171, 32, 48, 32, 64, HALO | 1, inputs="real", big=True),
            Case("real_tail_xonce", "h3", "ct", 3, 16, 16, 32, 128, H3 | 3 | XONCE, out="split", act=1, tail=True, inputs="real"),
            Case("real_tail_cols64", "h3", "ct", 3, 16, 16, 32, 64, H3 | 4, out="split", act=1, tail=True, inputs="real"),
            Case("real_f32w_c3_cin64", "f32", "c3", 3, 6, 12, 64, 96, FP32_WIDE, inputs="real"),
            Case("real_f32n_c3_cin64", "f32", "c3", 3, 6, 12, 64, 96, FP32_NARROW, inputs="real", cols_pad=192)]


STRUCT_CASES = _cases()
ARITH_CASES = _arith_cases()
ACT_CASES = _act_cases()
REAL_CASES = _real_cases()
ALL_CASES = STRUCT_CASES + ARITH_CASES + ACT_CASES + REAL_CASES
BY_NAME = dict((c.name, c) for c in ALL_CASES)
assert len(BY_NAME) == len(ALL_CASES)
RATIO_GATE = 4.0            # tests/test_gpu_wb.py's margin for the same comparison (kernel error / float32 CPU error)


# ------------------------------------------------------------------------------------------------------------------ inputs
def make_inputs(c, seed=None):
    rng = np.random.default_rng(sum(c.key.encode()) * 7919 + len(c.key) if seed is None else seed)
    Hs, Ws = c.H >> c.up, c.W >> c.up
    xs, ws = (c.n, Hs, Ws, c.Cin), (c.phases, c.cols, c.ntaps, c.Cin)
    pick = lambda vals, shape: np.asarray(vals, np.float32)[rng.integers(0, len(vals), size=shape)]
    lowhalf = lambda shape: (1.0 + pick([-3, -2, -1, 1, 2, 3], shape).astype(np.float64) * 2.0 ** -12).astype(np.float32)
    d = {}
    if c.inputs == "real":
        d["x"] = np.maximum(rng.standard_normal(xs), 0).astype(np.float32)
        d["w"] = (rng.standard_normal(ws) * np.sqrt(2.0 / (c.ntaps * c.Cin))).astype(np.float32)
        d["scale"], d["shift"] = np.ones(c.cmod, np.float32), np.zeros(c.cmod, np.float32)
        # like csrc/gl_dcgan.hip: max |w| 2^wexp in [2^12, 2^13)
        c.wexp = int(np.floor(np.log2(8191.0 / np.abs(d["w"]).max())))
    else:
        d["x"] = lowhalf(xs) if c.inputs == "arith_x" else pick([1, 2, 3], xs)
        d["w"] = lowhalf(ws) * pick([-1, 1], ws) if c.inputs == "arith_w" else pick([-2, -1, 1, 2], ws)
        if c.inputs in ("arith_w", "arith_x"):
            d["scale"], d["shift"] = np.ones(c.cmod, np.float32), np.zeros(c.cmod, np.float32)
        elif c.inputs == "act34":
            d["scale"], d["shift"] = pick([2.0 ** -6, 2.0 ** -5], c.cmod), pick([-1, 0, 1], c.cmod)
        else:
            d["scale"], d["shift"] = pick([0.25, 0.5, 1, 2], c.cmod), pick([-3, -2, -1, 0, 1, 2, 3], c.cmod)
    if c.residual:
        d["residual"] = pick(list(range(-8, 9)), (c.n, c.Ho, c.Wo, c.cols))
    if c.tail:
        if c.inputs == "real":
            d["tail_w"] = (rng.standard_normal((48, c.cols)) * np.sqrt(1.0 / c.cols)).astype(np.float32)
            c.tail_wexp = int(np.floor(np.log2(8191.0 / np.abs(d["tail_w"]).max())))
        else:
            d["tail_w"] = pick([-2, -1, 1, 2], (48, c.cols))
    if c.sat:
        # move the channel that holds the largest value so that this value * ACT_SCALE lies just inside (4093 * 16 = 65488) or outside
        # (4095 * 16 = 65520) the fp16 range; every other channel stays far below
        ref = reference(c, d)
        ch = int(np.unravel_index(np.argmax(ref), ref.shape)[-1])
        assert c.cmod == c.cols
        d["shift"][ch] += np.float32((4093.0 if c.sat == "below" else 4095.0) - ref.max())
    return d


# --------------------------------------------------------------------------------------------------------------- reference
def accumulate(c, x, w, dtype=torch.float64):
    """raw convolution sums, scattered: [n][Ho][Wo][cols] (torch, `dtype`); x [n][H >> up][W >> up][Cin], w [phases][cols][ntaps][Cin]"""
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).permute(0, 3, 1, 2)
    if c.up:
        xt = xt.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)         # nearest-neighbour x2
    wt = torch.from_numpy(np.ascontiguousarray(w)).to(dtype)
    out = torch.zeros((c.n, c.Ho, c.Wo, c.cols), dtype=dtype)
    for ph, taps in enumerate(c.taps):
        ly, hy = max(0, -min(t[0] for t in taps)), max(0, max(t[0] for t in taps))
        lx, hx = max(0, -min(t[1] for t in taps)), max(0, max(t[1] for t in taps))
        k = torch.zeros((c.cols, c.Cin, ly + hy + 1, lx + hx + 1), dtype=dtype)
        for t, (dy, dx) in enumerate(taps):
            k[:, :, dy + ly, dx + lx] += wt[ph, :, t, :]
        acc = F.conv2d(F.pad(xt, (lx, hx, ly, hy)), k)                          # explicit zero padding; [n][cols][H][W]
        out[:, c.oy[ph]:c.oy[ph] + c.H * c.omul:c.omul, c.ox[ph]:c.ox[ph] + c.W * c.omul:c.omul, :] = acc.permute(0, 2, 3, 1)
    return out


def activate(v, act):
    if act == 1:
        return torch.clamp(v, min=0)
    if act == 2:                  # the kernel's max(v, float32(0.2) * v) with the product rounded to float32
        prod = (v.to(torch.float32) * torch.tensor(0.2, dtype=torch.float32)).to(v.dtype)
        return torch.where(v >= 0, v, prod)
    if act == 3:
        return torch.tanh(v)
    if act == 4:
        return torch.sigmoid(v)
    return v


def reference(c, d, dtype=torch.float64, hidden=False):
    """float64 (or `dtype`) result in the logical shape: [n][Ho][Wo][cols], or for the fused tail [48][n * Ho * Wo]
    (hidden=True: the activated layer in front of the tail instead)"""
    acc = accumulate(c, d["x"], d["w"], dtype)
    ch = np.arange(c.cols) % c.cmod
    s = torch.from_numpy(d["scale"][ch]).to(dtype)
    t = torch.from_numpy(d["shift"][ch]).to(dtype)
    v = activate(acc * s + t, c.act)
    if c.residual:
        v = v + torch.from_numpy(d["residual"]).to(dtype)
    if c.tail and not hidden:
        v = (v.reshape(-1, c.cols) @ torch.from_numpy(d["tail_w"]).to(dtype).t()).t().contiguous()
    return v.numpy()


def abs_sum(c, d):
    """largest sum of absolute products over all outputs (and of the tail's, if any), in float64"""
    m = float(accumulate(c, np.abs(d["x"]), np.abs(d["w"])).max())
    mt = 0.0
    if c.tail:
        h = np.abs(reference(c, d, hidden=True)).reshape(-1, c.cols)
        mt = float((h @ np.abs(d["tail_w"]).astype(np.float64).T).max())
    return m, mt


def timed_reference(c, d):
    t0 = time.perf_counter()
    r = reference(c, d)
    return r, time.perf_counter() - t0


# ------------------------------------------------------------------------------------------------------------------ layouts
def encode_split(v):
    """[rows][d] float32 (d % 32 == 0) -> split layout bytes [rows][d / 32][32 hi halves | 32 lo halves], as the device stores it"""
    v = np.clip(np.asarray(v, np.float32), -F16_MAX, F16_MAX)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    rows, d = v.shape
    out = np.empty((rows, d // 32, 2, 32), np.float16)
    out[:, :, 0, :] = hi.reshape(rows, d // 32, 32)
    out[:, :, 1, :] = lo.reshape(rows, d // 32, 32)
    return out.tobytes()


def decode_split(buf, rows, d):
    """split layout bytes -> [rows][d] float64 hi + lo (exact)"""
    a = np.frombuffer(buf, np.float16).reshape(rows, d // 32, 2, 32).astype(np.float64)
    return (a[:, :, 0, :] + a[:, :, 1, :]).reshape(rows, d)


def decode_output(c, buf):
    """raw output bytes of gl_tune_conv_layer -> float64 in the shape reference() returns, true values"""
    if c.tail:
        return np.frombuffer(buf, np.float32).reshape(48, c.opos).astype(np.float64)
    if c.out == "split":
        return decode_split(buf, c.opos, c.cols).reshape(c.n, c.Ho, c.Wo, c.cols) / ACT_SCALE
    a = np.frombuffer(buf, np.float32).astype(np.float64)
    if c.out == "planar":
        return a.reshape(c.cols, c.ld_planar)[:, :c.positions].T.reshape(c.n, c.Ho, c.Wo, c.cols)
    return a.reshape(c.n, c.Ho, c.Wo, c.cols)


def expected_in_guard(c):
    """bytes of one input guard as the entry leaves it: POISON per value, split like the input on the split path"""
    vals = np.full((c.in_guard // (c.Cin * 4), c.Cin), POISON, np.float32)
    return encode_split(vals * np.float32(ACT_SCALE)) if c.kernel == "h3" else vals.tobytes()


# ------------------------------------------------------------------------------------------------------------ preconditions
def unit_of(c):
    """the unit every product and partial sum is an integer multiple of"""
    return 2.0 ** -12 if c.inputs in ("arith_w", "arith_x") else 1.0


def exactness_problems(c, d, ref):
    """the preconditions under which device == float32(reference) bit for bit; -> list of violations (empty = exact comparison is sound)"""
    bad = []
    m, mt = abs_sum(c, d)
    if not m / unit_of(c) < 2.0 ** 24:
        bad.append("sum of absolute products %g is not below 2^24 units" % m)
    if not np.array_equal(ref.astype(np.float32).astype(np.float64), ref):
        bad.append("float32(ref) != ref")
    if c.out == "split" or c.tail:
        h = reference(c, d, hidden=True) if c.tail else ref
        if c.sat != "above":
            if not np.abs(h).max() * ACT_SCALE < F16_MAX:
                bad.append("split value %g * %g reaches the fp16 limit" % (np.abs(h).max(), ACT_SCALE))
            flat = (h * ACT_SCALE).reshape(-1, c.cols)
            if not np.array_equal(decode_split(encode_split(flat), len(flat), c.cols), flat):
                bad.append("split output not representable as hi + lo")
    if c.tail:
        su = min(1.0, float(np.min(d["scale"])))              # unit of the hidden activations (shift is an integer)
        if not mt / su < 2.0 ** 24:
            bad.append("tail sum of absolute products %g is not below 2^24 units" % mt)
    if c.inputs in ("arith_w", "arith_x") and c.ntaps * c.Cin > 576:
        bad.append("K > 576")
    return bad


# ------------------------------------------------------------------------------------------------------------ the GPU entry
class TuneConvLayer(ctypes.Structure):          # csrc/gl_tune.hip GlTuneConvLayer
    _fields_ = [("kernel", ctypes.c_int32), ("phases", ctypes.c_int32), ("ntaps", ctypes.c_int32), ("up", ctypes.c_int32),
                ("n_img", ctypes.c_int64),
                ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("Cin", ctypes.c_int32), ("cols", ctypes.c_int32), ("cols_pad", ctypes.c_int32),
                ("Ho", ctypes.c_int32), ("Wo", ctypes.c_int32), ("omul", ctypes.c_int32),
                ("tap_dy", ctypes.c_uint32 * 4), ("tap_dx", ctypes.c_uint32 * 4), ("oy", ctypes.c_int32 * 4), ("ox", ctypes.c_int32 * 4),
                ("planar", ctypes.c_int32), ("out_mode", ctypes.c_int32), ("cmod", ctypes.c_int32), ("act", ctypes.c_int32),
                ("ld_planar", ctypes.c_int64),
                ("wexp", ctypes.c_int32), ("tail_wexp", ctypes.c_int32),
                ("x", ctypes.c_void_p), ("w", ctypes.c_void_p), ("scale", ctypes.c_void_p), ("shift", ctypes.c_void_p),
                ("residual", ctypes.c_void_p), ("tail_w", ctypes.c_void_p),
                ("poison", ctypes.c_float), ("sentinel", ctypes.c_int32),
                ("in_guard", ctypes.c_int64), ("out_bytes", ctypes.c_int64),
                ("out", ctypes.c_void_p), ("in_guards", ctypes.c_void_p), ("out_guards", ctypes.c_void_p),
                ("sat_delta", ctypes.c_int64), ("form", ctypes.c_int32), ("reserved_i", ctypes.c_int32 * 7), ("reserved_p", ctypes.c_void_p * 8)]


def run_layer(lib, ctx_handle, c, d):
    """one launch through gl_tune_conv_layer -> dict(out=bytes, in_guards=(lo, hi), out_guards=(lo, hi), sat_delta, form)"""
    q = TuneConvLayer()
    q.kernel, q.phases, q.ntaps, q.up, q.n_img = (1 if c.kernel == "h3" else 0), c.phases, c.ntaps, c.up, c.n
    q.H, q.W, q.Cin, q.cols, q.cols_pad, q.Ho, q.Wo, q.omul = c.H, c.W, c.Cin, c.cols, c.cols_pad, c.Ho, c.Wo, c.omul
    for ph, taps in enumerate(c.taps):
        q.tap_dy[ph] = sum((dy + 1) << (2 * t) for t, (dy, dx) in enumerate(taps))
        q.tap_dx[ph] = sum((dx + 1) << (2 * t) for t, (dy, dx) in enumerate(taps))
        q.oy[ph], q.ox[ph] = c.oy[ph], c.ox[ph]
    q.planar, q.out_mode, q.cmod, q.act, q.ld_planar = int(c.out == "planar"), (2 if c.out == "split" else 0), c.cmod, c.act, c.ld_planar
    q.wexp, q.tail_wexp = c.wexp, c.tail_wexp
    keep = {}
    def ptr(name):
        if name not in d:
            return None
        a = keep[name] = np.ascontiguousarray(d[name], np.float32)
        return a.ctypes.data
    q.x, q.w, q.scale, q.shift, q.residual, q.tail_w = ptr("x"), ptr("w"), ptr("scale"), ptr("shift"), ptr("residual"), ptr("tail_w")
    q.poison, q.sentinel, q.in_guard, q.out_bytes = POISON, SENTINEL, c.in_guard, c.out_bytes
    out = np.empty(c.out_bytes, np.uint8)
    ig = np.empty(2 * c.in_guard, np.uint8)
    og = np.empty(2 * OUT_GUARD, np.uint8)
    q.out, q.in_guards, q.out_guards = out.ctypes.data, ig.ctypes.data, og.ctypes.data
    for k in c.env:
        os.environ[k] = c.env[k]
    try:
        lib.gl_tune_conv_layer.restype = ctypes.c_int
        lib.gl_tune_conv_layer.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        rc = lib.gl_tune_conv_layer(ctx_handle, ctypes.byref(q))
    finally:
        for k in c.env:
            os.environ.pop(k, None)
    if rc != 0:
        lib.gl_last_error.restype = ctypes.c_char_p
        raise RuntimeError("gl_tune_conv_layer(%s): %s" % (c.name, lib.gl_last_error().decode()))
    return {"out": out.tobytes(), "in_guards": (ig[:c.in_guard].tobytes(), ig[c.in_guard:].tobytes()),
            "out_guards": (og[:OUT_GUARD].tobytes(), og[OUT_GUARD:].tobytes()), "sat_delta": int(q.sat_delta), "form": int(q.form)}
