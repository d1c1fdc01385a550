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
                 cols_pad=None, inputs="struct", env=None, big=False, sat=None, atol=None, data=None, fuse=0, rgb_n=0, tap_fmt=0, tap_pool=False,
                 tap_layout="row", tap_row0=0, tap_off=0, refused=None):
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
        # fused epilogues (the second half of this file): 0 none, 1 PixelNorm, 2 PixelNorm + toRGB, 3 LPIPS tap, 4 tap + PixelNorm (refused)
        self.fuse, self.rgb_n, self.tap_fmt, self.tap_pool, self.tap_layout = fuse, rgb_n, tap_fmt, tap_pool, tap_layout
        self.tap_row0, self.tap_off = tap_row0, tap_off
        self.refused = refused                # None, or a piece of the error message the launcher must refuse the case with

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
                ("sat_delta", ctypes.c_int64), ("form", ctypes.c_int32),
                ("fuse", ctypes.c_int32), ("rgb_n", ctypes.c_int32), ("tap_fmt", ctypes.c_int32), ("tap_pool", ctypes.c_int32),
                ("reserved_i", ctypes.c_int32 * 3),
                ("rgb_w", ctypes.c_void_p), ("rgb_b", ctypes.c_void_p), ("tap_coef", ctypes.c_void_p),
                ("rgb_out", ctypes.c_void_p), ("tap_V", ctypes.c_void_p), ("pool_out", ctypes.c_void_p), ("aux_guards", ctypes.c_void_p),
                ("reserved_p", ctypes.c_void_p * 1),
                ("tap_ldv", ctypes.c_int64), ("tap_off", ctypes.c_int64), ("tap_row0", ctypes.c_int64), ("v_bytes", ctypes.c_int64)]


def run_layer(lib, ctx_handle, c, d, fuse=None):
    """one launch through gl_tune_conv_layer -> dict(out=bytes, in_guards=(lo, hi), out_guards=(lo, hi), sat_delta, form) and, for a fused
    epilogue, rgb / V / pool = raw bytes, aux_guards = [(lo, hi)] * 3 in that order.  fuse=0: the same case without its fused epilogue"""
    fuse = c.fuse if fuse is None else fuse
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
    q.fuse = fuse
    aux = {}
    if fuse:
        ag = aux["aux_guards"] = np.empty(6 * OUT_GUARD, np.uint8)
        q.aux_guards = ag.ctypes.data
    if fuse == 2:
        rw = keep["rgb_w"] = np.ascontiguousarray(d["rgb_w"][:c.rgb_n], np.float32)
        rb = keep["rgb_b"] = np.ascontiguousarray(d["rgb_b"][:c.rgb_n], np.float32)
        aux["rgb"] = np.empty(c.opos * 16, np.uint8)
        q.rgb_w, q.rgb_b, q.rgb_n, q.rgb_out = rw.ctypes.data, rb.ctypes.data, c.rgb_n, aux["rgb"].ctypes.data
    if fuse in (3, 4):
        tc = keep["tap_coef"] = np.ascontiguousarray(d["tap_coef"], np.float32)
        ldv, vb = v_geometry(c)
        aux["V"] = np.empty(vb, np.uint8)
        q.tap_coef, q.tap_V, q.tap_fmt, q.tap_ldv, q.tap_off, q.tap_row0, q.v_bytes = tc.ctypes.data, aux["V"].ctypes.data, c.tap_fmt, ldv, c.tap_off, c.tap_row0, vb
        if c.tap_pool:
            aux["pool"] = np.empty(c.n * (c.Ho // 2) * (c.Wo // 2) * c.cols * 4, np.uint8)
            q.tap_pool, q.pool_out = 1, aux["pool"].ctypes.data
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
    r = {"out": out.tobytes(), "in_guards": (ig[:c.in_guard].tobytes(), ig[c.in_guard:].tobytes()),
         "out_guards": (og[:OUT_GUARD].tobytes(), og[OUT_GUARD:].tobytes()), "sat_delta": int(q.sat_delta), "form": int(q.form)}
    if fuse:
        ag = aux.pop("aux_guards")
        r["aux_guards"] = [(ag[2 * b * OUT_GUARD:(2 * b + 1) * OUT_GUARD].tobytes(), ag[(2 * b + 1) * OUT_GUARD:(2 * b + 2) * OUT_GUARD].tobytes()) for b in range(3)]
        r.update(aux)                           # rgb / V / pool stay numpy uint8 arrays (the V buffers are large)
    return r


# ====================================================================================================================================
# The fused epilogues of csrc/gl_conv_h3_epi.h (PixelNorm, PixelNorm + toRGB, LPIPS tap + 2 x 2 max-pool) and their stand-alone siblings
# (pixelnorm_split_kernel, lpips_tap_split_kernel, lpips_tap_pool_split_kernel): what tests/test_conv_epilogues_cpu.py and
# tests/test_gpu_conv_epilogues.py share.
#
# References: float64, from the float64 activations of reference() -- PixelNorm v / sqrt(mean_c v^2 + 1e-8), toRGB b + W . v_norm,
# tap v / (sqrt(sum_c v^2) + 1e-10) * coef * 16384, pool the plain 2 x 2 max.
#
# Exact cases: structural inputs with Cin = 32 and act 0 or 1.  The stored activations (value * ACT_SCALE) are then integer multiples of one
# power of two (`stored_unit`), the sum of squares of a position is below 2^24 unit^2 and therefore exact in float32 IN ANY ORDER, and everything
# after it is a fixed sequence of correctly rounded float32 operations (/, sqrt, +, *), which numpy's float32 reproduces; the fma residual of
# PixelNorm's low half is computed in float64, where product and difference are exact, then rounded float32 -> float16 like the device's.
# So the device bytes must equal the oracle's bit for bit.
# Bounded cases (toRGB, act 2, the clamped pair, real-valued inputs): elementwise against float64,
#     split values  |ref| 2^-21 + 2^-24 (stored units)       fp16 rows  |ref| (2^-11 + 2^-21) + 2^-25
#     toRGB         S 2^-20 + 2^-24 |ref|,  S = sum_ch |w_ch v_ch|   (2^-21 relative per normalised value, <= 9 float32 roundings on any path)
V_SCALE = 16384.0                                        # csrc/gl_feat_pair.h kVScale
TAP_EPS = np.float32(1e-10) * np.float32(ACT_SCALE)      # normalize_tensor's eps in stored units
PIX_EPS = np.float32(1e-8) * np.float32(ACT_SCALE) * np.float32(ACT_SCALE)
TAP_OFF = 128                                            # non-zero multiple of 64
HALO_SHAPE = (171, 32, 48)


def v_geometry(c):
    """-> (tap_ldv, v_bytes) of the V buffer a tap case writes into: room for rows [0, tap_row0 + n] and one unwritten chunk behind every row;
    K-blocked: cells = ceil(K / 64) passed as a negative tap_ldv, whole 256-row blocks"""
    k_end = c.tap_off + c.Ho * c.Wo * c.cols
    if c.tap_layout == "blocked":
        assert c.tap_fmt == 1
        cells = (k_end + 63) // 64
        return -cells, (c.tap_row0 + c.n + 255) // 256 * cells * 32768
    ldv = k_end * 4 + 128 if c.tap_fmt == 0 else k_end * 2 + 64
    return ldv, (c.tap_row0 + c.n + 1) * ldv


TAP_VARIANTS = [(pool, fmt, layout) for pool in (False, True) for fmt, layout in ((0, "row"), (1, "row"), (1, "blocked"))]


def _epi_cases():
    pn, rgb, tap, refuse = [], [], [], []
    shapes = {"t0": ((3, 6, 12), H3 | 0), "t1": ((3, 10, 10), H3 | 1)}

    def conv(name, shape, cols, form, key, **kw):
        n, H, W = shape
        return Case(name, "h3", "c3", n, H, W, 32, cols, form, out="split", data=key, big=shape == HALO_SHAPE, **kw)
    # ---- PixelNorm (mode 1): every fusable form, ragged tiles, cols below the tile's channels, UP, halo
    for tile, colss in (("t0", (128, 96)), ("t1", (64, 32))):
        shape, form = shapes[tile]
        for cols in colss:
            pn.append(conv("pn_%s_cols%d" % (tile, cols), shape, cols, form, "epi_%s_cols%d" % (tile, cols), fuse=1))
            pn.append(conv("pn_up_%s_cols%d" % (tile, cols), shape, cols, form | UP, "epi_up_%s_cols%d" % (tile, cols), fuse=1, up=1, act=1))
        pn.append(conv("pn_%s_cols%d_act2" % (tile, colss[0]), shape, colss[0], form, "epi_%s_cols%d_act2" % (tile, colss[0]), fuse=1, act=2))
    for cols, wc in ((64, 1), (96, 2), (128, 2)):
        pn.append(conv("pn_halo%d_cols%d" % (wc, cols), HALO_SHAPE, cols, HALO | wc, "epi_halo_cols%d" % cols, fuse=1))
    pn.append(conv("pn_up_halo1_cols64", HALO_SHAPE, 64, HALO | 1, "epi_up_halo_cols64", fuse=1, up=1, act=1))
    for sat in ("below", "above"):
        pn.append(conv("pn_sat_%s" % sat, shapes["t0"][0], 128, H3 | 0, "epi_sat_%s" % sat, fuse=1, sat=sat))
    # ---- PixelNorm + toRGB (mode 2)
    for name, tile, cols, rn, act in (("rgb_t0_cols128", "t0", 128, 3, 0), ("rgb_t0_cols96", "t0", 96, 1, 0), ("rgb_t1_cols64", "t1", 64, 1, 0),
                                      ("rgb_t1_cols32", "t1", 32, 3, 0), ("rgb_t0_cols128_act2", "t0", 128, 3, 2), ("rgb_t1_cols64_act2", "t1", 64, 3, 2)):
        shape, form = shapes[tile]
        rgb.append(conv(name, shape, cols, form, "epi_%s_cols%d%s" % (tile, cols, "_act2" if act else ""), fuse=2, rgb_n=rn, act=act))
    rgb.append(conv("rgb_halo1_cols64", HALO_SHAPE, 64, HALO | 1, "epi_halo_cols64", fuse=2, rgb_n=3))
    rgb.append(conv("rgb_halo2_cols96", HALO_SHAPE, 96, HALO | 2, "epi_halo_cols96", fuse=2, rgb_n=3))
    rgb.append(conv("rgb_halo2_cols128", HALO_SHAPE, 128, HALO | 2, "epi_halo_cols128", fuse=2, rgb_n=1))
    # ---- LPIPS tap (mode 3), act 1 like VGG16's ReLU.  W = 16, n = 2, H = 6: 192 positions, the image boundary at 96 lies inside the second wave's
    # 64 positions and the tile is ragged; W = 32: the pool partner is two position tiles away
    tshapes = [("tap_t1_w16_cols64", (2, 6, 16), 64, H3 | 1), ("tap_t1_w32_cols64", (3, 2, 32), 64, H3 | 1),
               ("tap_t0_w16_cols128", (2, 6, 16), 128, H3 | 0), ("tap_t0_w16_cols96", (2, 6, 16), 96, H3 | 0),
               ("tap_t0_w32_cols128", (1, 6, 32), 128, H3 | 0),
               ("tap_halo1_cols64", HALO_SHAPE, 64, HALO | 1), ("tap_halo2_cols128", HALO_SHAPE, 128, HALO | 2)]
    for name, shape, cols, form in tshapes:
        for pool, fmt, layout in TAP_VARIANTS:
            # K-blocked: the images cross the 256-row block boundary (rows 250 ... 420 of the halo shape, 255 ... of the small ones; a single
            # image sits in the second block); row-major rows of the halo shape start at 2, to keep the buffer small
            row0 = (250 if layout == "blocked" else 2) if shape == HALO_SHAPE else 255 if shape[0] > 1 else 257
            tap.append(conv("%s_%s%s%s" % (name, "f16" if fmt else "split", "_blocked" if layout == "blocked" else "", "_pool" if pool else ""), shape, cols,
                            form, "epi_" + name, fuse=3, act=1, tap_fmt=fmt, tap_layout=layout, tap_pool=pool, tap_row0=row0, tap_off=TAP_OFF))
    # ---- what the launcher must refuse (an error, no convolution launch)
    refuse.append(conv("refuse_pn_cols160_tile0", (3, 6, 12), 160, H3 | 0, "epi_refuse_cols160", fuse=1, refused="all 160 channels in one tile"))
    refuse.append(conv("refuse_pn_tile5", (455, 24, 24), 96, H3 | 5, "epi_refuse_tile5", fuse=1, refused="all 96 channels in one tile"))
    refuse.append(conv("refuse_tap_w12", (3, 6, 12), 128, H3 | 0, "epi_refuse_w12", fuse=3, act=1, tap_off=TAP_OFF, refused="tap cannot be fused"))
    refuse.append(conv("refuse_tap_with_pixelnorm", (2, 6, 16), 128, H3 | 0, "epi_refuse_both", fuse=4, act=1, tap_off=TAP_OFF, refused="tap cannot be fused"))
    refuse.append(conv("refuse_tap_switched_off", (2, 6, 16), 128, H3 | 0, "epi_refuse_switch", fuse=3, act=1, tap_off=TAP_OFF, env={"GL_TAP_FUSE": "0"},
                       refused="tap cannot be fused"))
    return pn, rgb, tap, refuse


PN_CASES, RGB_CASES, TAP_CASES, REFUSE_CASES = _epi_cases()
EPI_CASES = PN_CASES + RGB_CASES + TAP_CASES
EPI_BY_NAME = dict((c.name, c) for c in EPI_CASES + REFUSE_CASES)
assert len(EPI_BY_NAME) == len(EPI_CASES) + len(REFUSE_CASES) and not set(EPI_BY_NAME) & set(BY_NAME)


def epi_exact(c):
    """whether the case is compared bit for bit with the host oracle (else: with float64 under the derived bounds)"""
    return c.fuse in (1, 3) and c.act in (0, 1) and c.sat is None and c.inputs == "struct"


def chain_applies(c):
    """fused == unfused, bit for bit: the stand-alone kernels exist for 64 and 128 channels (the tap's; PixelNorm's takes any C % 16 == 0)"""
    return c.fuse in (1, 3) and c.cols in (64, 128)


def make_epi_inputs(c):
    """make_inputs + what the epilogue needs; the additions come from a generator of their own, so that the convolution's operands are those
    of every other case of the key"""
    d = make_inputs(c)
    rng = np.random.default_rng(sum(c.key.encode()) * 104729 + 17)
    d["tap_coef"] = rng.uniform(0.01, 1.0, size=c.cols).astype(np.float32)
    d["rgb_w"] = (np.asarray([-2, -1, 1, 2], np.float32)[rng.integers(0, 4, size=(4, c.cols))] / np.float32(8)).astype(np.float32)
    d["rgb_b"] = rng.integers(-3, 4, size=4).astype(np.float32)
    return d


# --------------------------------------------------------------------------------------------------------- float64 references
def ref_clamped(c, ref):
    """the activations as pass 1 of the fused PixelNorm / tap keeps them: clamped to the fp16 range of the stored value"""
    return np.clip(ref, -F16_MAX / ACT_SCALE, F16_MAX / ACT_SCALE)


def ref_pixelnorm(v):
    """[..., C] float64 true values -> v / sqrt(mean_c v^2 + 1e-8)"""
    return v / np.sqrt(np.mean(v * v, axis=-1, keepdims=True) + 1e-8)


def ref_rgb(vn, w, b):
    """-> (b + W . v_norm [positions][rgb_n], S = sum_ch |w_ch v_ch| [positions][rgb_n])"""
    vn = vn.reshape(-1, vn.shape[-1])
    w = np.asarray(w, np.float64)
    return np.asarray(b, np.float64)[None, :] + vn @ w.T, np.abs(vn) @ np.abs(w).T


def ref_tap(v, coef):
    """[..., C] float64 true values -> the V values (stored units: * 16384)"""
    return v / (np.sqrt(np.sum(v * v, axis=-1, keepdims=True)) + 1e-10) * np.asarray(coef, np.float64) * V_SCALE


def pool2(v):
    """[n][H][W][C] -> [n][H / 2][W / 2][C], the plain 2 x 2 max"""
    n, H, W, C = v.shape
    return v.reshape(n, H // 2, 2, W // 2, 2, C).max(axis=(2, 4))


def bound_split(ref_stored):
    return np.abs(ref_stored) * 2.0 ** -21 + 2.0 ** -24


def bound_f16(ref_stored):
    return np.abs(ref_stored) * (2.0 ** -11 + 2.0 ** -21) + 2.0 ** -25


def bound_rgb(ref, S):
    return S * 2.0 ** -20 + 2.0 ** -24 * np.abs(ref)


# ------------------------------------------------------------------------------------------------------------ the exact oracle
def stored_unit(c, d):
    """the power of two every stored activation of a structural case is an integer multiple of (shift and sums are integers)"""
    return ACT_SCALE * min(1.0, float(np.min(d["scale"])))


def sumsq_problems(stored, unit):
    """stored [positions][C] float64: the preconditions of the oracle -> list of violations"""
    bad = []
    if not np.array_equal(np.round(stored / unit) * unit, stored):
        bad.append("stored values are no multiples of %g" % unit)
    ss = float(np.max(np.sum(stored * stored, axis=-1))) / (unit * unit)
    if not ss < 2.0 ** 24:
        bad.append("sum of squares %g unit^2 is not below 2^24" % ss)
    if not np.array_equal(decode_split(encode_split(stored), len(stored), stored.shape[1]), stored):
        bad.append("stored values not representable as hi + lo")
    return bad


def _sumsq32(stored):
    ss = np.sum(stored.astype(np.float64) ** 2, axis=-1)
    assert np.array_equal(ss.astype(np.float32).astype(np.float64), ss)      # exact by the precondition
    return ss.astype(np.float32)


def _halves(t32):
    """float32 -> (hi, lo) float16 as a split store of t makes them"""
    hi = t32.astype(np.float16)
    return hi, (t32 - hi.astype(np.float32)).astype(np.float16)


def oracle_pixelnorm(stored):
    """stored [positions][C] float32 (exact sums) -> (hi, lo) float16 of the normalised stored values, as both the fused epilogue and
    pixelnorm_split_kernel compute them: inv = A / sqrt(ss / C + 1e-8 A A), hi = half(v * inv), lo = half(fma(v, inv, -hi))"""
    stored = np.asarray(stored, np.float32)
    A = np.float32(ACT_SCALE)
    inv = A / np.sqrt(_sumsq32(stored) / np.float32(stored.shape[1]) + PIX_EPS)
    assert inv.dtype == np.float32
    prod = stored.astype(np.float64) * inv.astype(np.float64)[:, None]        # 24 x 24 bits: exact
    hi = np.clip(prod.astype(np.float32), -F16_MAX, F16_MAX).astype(np.float16)
    lo = (prod - hi.astype(np.float64)).astype(np.float32).astype(np.float16)  # the difference is exact in float64; fma rounds it once to float32
    return hi, lo


def oracle_tap(stored, coef):
    """-> (hi, lo) float16 of the V values: inv = 16384 / (sqrt(ss) + eps), t = (v * inv) * coef with both products rounded to float32"""
    stored = np.asarray(stored, np.float32)
    inv = np.float32(V_SCALE) / (np.sqrt(_sumsq32(stored)) + TAP_EPS)
    t = (stored * inv[:, None]) * np.asarray(coef, np.float32)[None, :]
    assert t.dtype == np.float32
    return _halves(t)


def oracle_pool(stored_nhwc):
    """[n][H][W][C] float32 stored values -> (hi, lo) float16 [n * H/2 * W/2][C]"""
    m = pool2(np.asarray(stored_nhwc, np.float32))
    return _halves(m.reshape(-1, m.shape[-1]))


# ------------------------------------------------------------------------------------------------------------------- decoders
def split_halves(buf, rows, d):
    """split layout bytes [rows][d / 32][32 hi | 32 lo] -> (hi, lo) float16 [rows][d]"""
    a = np.frombuffer(buf, np.float16).reshape(rows, d // 32, 2, 32)
    return a[:, :, 0, :].reshape(rows, d), a[:, :, 1, :].reshape(rows, d)


def halves_value(hi, lo):
    return hi.astype(np.float64) + lo.astype(np.float64)


def decode_rgb(buf, opos):
    return np.frombuffer(buf, np.float32).reshape(opos, 4)


def vrow_half_index(fmt, ldv, rows, ks):
    """position, counted in halves from the start of the V buffer, of half k of buffer row r -> int64 [len(rows)][len(ks)]
    fmt 0: split rows of ldv bytes, chunks of [32 hi | 32 lo] (the index is the hi half's; lo: + 32)
    fmt 1, ldv >= 0: fp16 rows of ldv bytes;  ldv < 0: K-blocked [row / 256][-ldv cells][row % 256][64 halves]"""
    r = np.asarray(rows, np.int64)[:, None]
    k = np.asarray(ks, np.int64)[None, :]
    if fmt == 0:
        return r * (ldv // 2) + (k // 32) * 64 + k % 32
    if ldv >= 0:
        return r * (ldv // 2) + k
    return ((r // 256) * (-ldv) + k // 64) * 16384 + (r % 256) * 64 + k % 64


def decode_vrows(buf, fmt, ldv, row0, n, off, K):
    """V buffer (uint8 array) -> (hi [n][K] float16, lo or None, whether every half outside the written range still holds the sentinel)"""
    h = np.asarray(buf).view(np.uint16)
    idx = vrow_half_index(fmt, ldv, np.arange(row0, row0 + n), np.arange(off, off + K))
    written = np.zeros(len(h), bool)
    written[idx] = True
    hi = h[idx].view(np.float16)
    lo = None
    if fmt == 0:
        written[idx + 32] = True
        lo = h[idx + 32].view(np.float16)
    rest_ok = bool(np.all(h[~written] == SENTINEL * 0x101))
    return hi, lo, rest_ok


# ------------------------------------------------------------------------------------------------- the stand-alone kernels
class PostCase(object):
    """one launch of gl_tune_split_post: op 0 pixelnorm_split_kernel, 1 lpips_tap_split_kernel, 2 lpips_tap_pool_split_kernel"""
    def __init__(self, name, op, shape, C, inputs, tap_fmt=0, tap_layout="row", tap_row0=0, tap_off=0):
        self.name, self.op, self.C, self.inputs = name, op, C, inputs
        self.n, self.H, self.W = shape
        self.Ho, self.Wo, self.cols = self.H, self.W, C                       # what v_geometry reads
        self.tap_fmt, self.tap_layout, self.tap_row0, self.tap_off, self.tap_pool = tap_fmt, tap_layout, tap_row0, tap_off, op == 2
        self.positions = self.n * self.H * self.W
        self.key = "post_%s_%dx%dx%d_C%d" % ((inputs,) + tuple(shape) + (C,))

    def __repr__(self):
        return self.name


def _post_cases():
    c = []
    for inputs in ("exact", "real"):
        # 216 positions: a ragged last workgroup of 4 waves; C = 512: two sweeps of 256 channels
        for C in (32, 64, 96, 128, 256, 512):
            c.append(PostCase("post_pn_%s_C%d" % (inputs, C), 0, (3, 6, 12), C, inputs))
        # 3 x 5 x 5 = 75 positions: ragged for 8, 4, 2 and 1 positions per wave;  3 x 6 x 10: 45 windows
        for C in (64, 128, 256, 512):
            for fmt, layout in ((0, "row"), (1, "row"), (1, "blocked")):
                tag = "%s%s" % ("f16" if fmt else "split", "_blocked" if layout == "blocked" else "")
                c.append(PostCase("post_tap_%s_C%d_%s" % (inputs, C, tag), 1, (3, 5, 5), C, inputs, fmt, layout, 255, TAP_OFF))
                c.append(PostCase("post_tappool_%s_C%d_%s" % (inputs, C, tag), 2, (3, 6, 10), C, inputs, fmt, layout, 255, TAP_OFF))
    return c


POST_CASES = _post_cases()
POST_BY_NAME = dict((c.name, c) for c in POST_CASES)
assert len(POST_BY_NAME) == len(POST_CASES)


def make_post_inputs(c):
    """-> dict(stored [positions][C] float32: what the split activation holds, tap_coef)
    exact: small non-zero integers and ONE odd integer in [2049, 3001] per position, which needs its low half; the sum of squares stays below
    512 * 64 + 3001^2 < 2^24 for every C.  real: ReLU'd Gaussians * 16, rounded to hi + lo"""
    rng = np.random.default_rng(sum(c.key.encode()) * 7919 + len(c.key))
    if c.inputs == "exact":
        v = rng.integers(1, 9, size=(c.positions, c.C)) * rng.choice([-1, 1], size=(c.positions, c.C))
        v[np.arange(c.positions), rng.integers(0, c.C, size=c.positions)] = 2049 + 2 * rng.integers(0, 477, size=c.positions)
        stored = v.astype(np.float32)
    else:
        raw = (np.maximum(rng.standard_normal((c.positions, c.C)), -0.25) * ACT_SCALE).astype(np.float32)
        stored = decode_split(encode_split(raw), c.positions, c.C).astype(np.float32)
    return {"stored": stored, "tap_coef": rng.uniform(0.01, 1.0, size=c.C).astype(np.float32)}


class TuneSplitPost(ctypes.Structure):          # csrc/gl_tune.hip GlTuneSplitPost
    _fields_ = [("op", ctypes.c_int32), ("C", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("n_img", ctypes.c_int64),
                ("tap_fmt", ctypes.c_int32), ("sentinel", ctypes.c_int32),
                ("tap_ldv", ctypes.c_int64), ("tap_off", ctypes.c_int64), ("tap_row0", ctypes.c_int64), ("v_bytes", ctypes.c_int64),
                ("tap_eps", ctypes.c_float), ("reserved_i", ctypes.c_int32),
                ("act", ctypes.c_void_p), ("tap_coef", ctypes.c_void_p),
                ("act_out", ctypes.c_void_p), ("tap_V", ctypes.c_void_p), ("pool_out", ctypes.c_void_p), ("guards", ctypes.c_void_p)]


def run_split_post(lib, ctx_handle, c, act_bytes, coef):
    """one launch through gl_tune_split_post on the split activation `act_bytes` [n * H * W][C]; `c`: a PostCase, or a fused Case whose
    stand-alone counterpart (same tap parameters) is meant -> dict(act=bytes, V, pool = uint8 arrays or None, guards=[(lo, hi)] * 3)"""
    q = TuneSplitPost()
    op = c.op if isinstance(c, PostCase) else (0 if c.fuse == 1 else 2 if c.tap_pool else 1)
    q.op, q.C, q.H, q.W, q.n_img, q.sentinel = op, c.cols, c.Ho, c.Wo, c.n, SENTINEL
    src = np.frombuffer(act_bytes, np.uint8)
    assert len(src) == c.n * c.Ho * c.Wo * c.cols * 4
    act_out = np.empty(len(src), np.uint8)
    guards = np.empty(6 * OUT_GUARD, np.uint8)
    q.act, q.act_out, q.guards = src.ctypes.data, act_out.ctypes.data, guards.ctypes.data
    V = pool = None
    if op:
        tc = np.ascontiguousarray(coef, np.float32)
        ldv, vb = v_geometry(c)
        V = np.empty(vb, np.uint8)
        q.tap_coef, q.tap_V, q.tap_fmt, q.tap_ldv, q.tap_off, q.tap_row0, q.v_bytes = tc.ctypes.data, V.ctypes.data, c.tap_fmt, ldv, c.tap_off, c.tap_row0, vb
        q.tap_eps = float(TAP_EPS)
    if op == 2:
        pool = np.empty(c.n * (c.Ho // 2) * (c.Wo // 2) * c.cols * 4, np.uint8)
        q.pool_out = pool.ctypes.data
    lib.gl_tune_split_post.restype = ctypes.c_int
    lib.gl_tune_split_post.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    if lib.gl_tune_split_post(ctx_handle, ctypes.byref(q)) != 0:
        lib.gl_last_error.restype = ctypes.c_char_p
        raise RuntimeError("gl_tune_split_post(%s): %s" % (c.name, lib.gl_last_error().decode()))
    return {"act": act_out.tobytes(), "V": V, "pool": pool,
            "guards": [(guards[2 * b * OUT_GUARD:(2 * b + 1) * OUT_GUARD].tobytes(), guards[(2 * b + 1) * OUT_GUARD:(2 * b + 2) * OUT_GUARD].tobytes())
                       for b in range(3)]}
