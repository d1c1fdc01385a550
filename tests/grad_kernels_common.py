"""Cases, host restatements and the GPU entry of the per-kernel tests of the white-box backward kernels.  No GPU needed to import; imports nothing
from the product.

    csrc/gl_dcgan_grad.hip   tanh_grad_kernel<L2>, patch_rgb_kernel, relu_bn_grad_kernel<PLANAR>
    csrc/gl_pggan_grad.hip   pg_out_grad_kernel<L2>, pg_rgb_grad_kernel, pg_pn_grad_kernel, pg_leaky_grad_kernel, pg_rowpn_grad_kernel
    csrc/gl_lpips_grad.hip   lg_conv1_kernel<T>, lg_maxpool_kernel, lg_ref_kernel<J>, lg_act_grad_kernel<J>, lg_conv1_grad_kernel, lg_loss_kernel

Each kernel is launched once through gl_tune_grad_op of the tuning build (csrc/gl_tune.hip), which goes through the launcher the production pass
calls, so the grid, its cap and the template instance are the production ones.  Every case has n = 3 images, image 2 equal to image 0 (equal outputs
bit for bit, and equal to the n = 1 run of image 0), image 1 different.

Every kernel is restated here twice: the float64 formula of its header comment (`ref64`), and a float32 numpy restatement that rounds where the
source rounds (`ref32`): __f*_rn intrinsics one by one, fmaf chains and the xor butterfly 32 .. 1.  fma() here is a float64 product-sum rounded
to float32, i.e. rounded twice: it is the device's fmaf bit for bit only where the float64 value is exact, which the exact cases guarantee; in the
real-valued cases it is a float32-class evaluation that sets the bound, not a bit-faithful one.  An exact case is one whose values make every partial result
exactly representable, so `ref32` must be met bit for bit (tests/test_grad_kernels_cpu.py asserts the preconditions); a real-valued case measures
|g - g64|_2 / |g64|_2 per image and per position for `ref32` and allows the device SLACK = 4 times the largest such value.
"""
import ctypes
import zlib

import numpy as np

N_IMG, GUARD, SENTINEL, POISON, SLACK = 3, 4096, 0xA5, 64.0, 4.0
F32, F64 = np.float32, np.float64
CONV_CHUNK = 128            # kConvChunk of gl_pggan_grad.hip and gl_lpips_grad.hip
PG_K0 = 1024                # kGradK0 of gl_pggan_grad.hip
LP_EPS = F32(1e-10)
LP_SHIFT = np.array([-.030, -.088, -.188], F32)
LP_SCALE = np.array([.458, .448, .450], F32)
FAM_DCGAN, FAM_PGGAN, FAM_LPIPS = 0, 1, 2


# ------------------------------------------------------------------------------------------------------------ float32 building blocks
def fma(a, b, c):
    """a * b + c in float64, then rounded to float32: two roundings, not fmaf's one (module docstring)"""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def wave_sum(s):
    """the xor butterfly 32 .. 1 over the last axis (64 lanes): every lane ends with the same value"""
    idx = np.arange(64)
    s = np.asarray(s, F32)
    for o in (32, 16, 8, 4, 2, 1):
        s = (s + s[..., idx ^ o]).astype(F32)
    return s[..., 0]


def lanes(x, J):
    """[..., 64 J] -> [..., J, 64]: a lane holds channels lane + 64 j"""
    return x.reshape(x.shape[:-1] + (J, 64))


def unchunk(flat, positions, C, kc=CONV_CHUNK, chunked=True):
    """[chunk][pos][<= kc] -> [pos][C]"""
    flat = np.asarray(flat).reshape(-1)
    if not chunked:
        return flat.reshape(positions, C).copy()
    out = np.empty((positions, C), flat.dtype)
    for c0 in range(0, C, kc):
        cc = min(kc, C - c0)
        out[:, c0:c0 + cc] = flat[c0 * positions:c0 * positions + positions * cc].reshape(positions, cc)
    return out


def pixel_of_u8(u):
    return (2.0 * (u.astype(F64) / 255.0) - 1.0).astype(F32)           # attack_models/utils.py:82, as lg_*: in double, rounded once


def target_f32(u):
    """2.0f * (u / 255.0f) - 1.0f as tanh_grad_kernel / pg_out_grad_kernel form it: a rounded division, an exact doubling, a rounded subtraction"""
    return ((u.astype(F32) / F32(255.0)).astype(F32) * F32(2.0) - F32(1.0)).astype(F32)


def cells(x):
    """[n][h][w][C] -> [n][h/2][w/2][4 = qy * 2 + qx][C]"""
    n, h, w, C = x.shape
    return x.reshape(n, h // 2, 2, w // 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(n, h // 2, w // 2, 4, C)


def uncells(x):
    n, h2, w2, _, C = x.shape
    return x.reshape(n, h2, w2, 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(n, 2 * h2, 2 * w2, C)


# ------------------------------------------------------------------------------------------------------------ restatements: gl_lpips_grad.hip
def conv1_fwd(img, w, bias, dtype):
    """lg_conv1_kernel.  img [n][3][H][W] (float32 values or 8-bit codes), w [64][3][3][3], bias [64] -> [n][H W][64]"""
    n, _, H, W = img.shape
    px = pixel_of_u8(img) if img.dtype == np.uint8 else img.astype(F32)
    sh, sc = LP_SHIFT.reshape(1, 3, 1, 1), LP_SCALE.reshape(1, 3, 1, 1)
    if dtype == F32:
        v = ((px - sh).astype(F32) / sc).astype(F32)
    else:
        v = (px.astype(F64) - sh.astype(F64)) / sc.astype(F64)
    vp = np.zeros((n, 3, H + 2, W + 2), dtype)
    vp[:, :, 1:-1, 1:-1] = v
    acc = np.broadcast_to(bias.astype(dtype), (n, H, W, 64)).copy()
    for t in range(9):
        for c in range(3):
            tap = vp[:, c, t // 3:t // 3 + H, t % 3:t % 3 + W][..., None]
            wt = w[:, c, t // 3, t % 3].astype(dtype)
            acc = fma(tap, wt, acc) if dtype == F32 else acc + tap * wt
    return np.maximum(acc, dtype(0)).reshape(n, H * W, 64)


def maxpool(x, swap_yx=False):
    """lg_maxpool_kernel.  [n][H][W][C] -> [n][H/2][W/2][C]"""
    if swap_yx:
        n, H, W, C = x.shape
        x = x.reshape(n, W, H, C)
    return cells(x).max(axis=3)


def tap_norm32(av, J):
    """-> r, r + eps of every position; av [..., 64 J]"""
    L = lanes(av, J)
    ss = np.zeros(L.shape[:-2] + (64,), F32)
    for j in range(J):
        ss = fma(L[..., j, :], L[..., j, :], ss)
    r = np.sqrt(wave_sum(ss)).astype(F32)
    return r, (r + LP_EPS).astype(F32)


def ref_rows(f, dtype):
    """lg_ref_kernel.  f [n][hw][C] -> f / (|f|_c + 1e-10)"""
    if dtype == F32:
        _, den = tap_norm32(f, f.shape[-1] // 64)
        return (f / den[..., None]).astype(F32)
    f = f.astype(F64)
    return f / (np.sqrt((f * f).sum(axis=-1, keepdims=True)) + F64(LP_EPS))


def first_max_mask(a, variant=None):
    """[n][h][w][C] -> 1 where the position is the first maximum of its 2 x 2 cell in row-major order"""
    c = cells(a)
    if variant == "tie_all":                # >= against the earlier positions as well: every maximum takes the gradient
        m = (c == c.max(axis=3, keepdims=True))
    else:
        k = 3 - np.flip(c, axis=3).argmax(axis=3) if variant == "last_max" else c.argmax(axis=3)
        m = np.arange(4).reshape(1, 1, 1, 4, 1) == k[:, :, :, None, :]
    return uncells(m.astype(a.dtype))


def act_grad(a, D, mode, ref, lin, dtype, variant=None, before_mask=False):
    """lg_act_grad_kernel.  a [n][h][w][C]; D [n][h][w][C] (mode 1), [n][h/2][w/2][C] (mode 2) or None; ref [n][h][w][C] or None; lin [C]
    -> out [n][h w][C], part [n][h w] (None without a tap); before_mask: g [n][h][w][C] as it is before the ReLU mask instead of out"""
    n, h, w, C = a.shape
    J = C // 64
    if mode == 1:
        g = D.astype(dtype)
    elif mode == 2:
        up = np.repeat(np.repeat(D, 2, axis=1), 2, axis=2).astype(dtype)
        g = up * first_max_mask(a, variant).astype(dtype)
    else:
        g = np.zeros(a.shape, dtype)
    part = None
    if ref is not None:
        if dtype == F32:
            coef = F32(0.4 / (float(h) * w))
            r, den = tap_norm32(a, J)
            dn_ = den[..., None]
            nv = (a / dn_).astype(F32)
            diff = (nv - ref).astype(F32)
            wd = (lin * diff).astype(F32)
            dn = (coef * wd).astype(F32)
            sq, dot = np.zeros(a.shape[:-1] + (64,), F32), np.zeros(a.shape[:-1] + (64,), F32)
            for j in range(J):
                sq = fma(lanes(wd, J)[..., j, :], lanes(diff, J)[..., j, :], sq)
                dot = fma(lanes(nv, J)[..., j, :], lanes(dn, J)[..., j, :], dot)
            sq, dot = wave_sum(sq), wave_sum(dot)
            proj = np.where(r > 0, (dot * (r / den).astype(F32)).astype(F32), F32(0))
            g = (g + ((dn - (nv * proj[..., None]).astype(F32)).astype(F32) / dn_).astype(F32)).astype(F32)
            part = sq
        else:
            a64, ref64_, lin64 = a.astype(F64), ref.astype(F64), lin.astype(F64)
            r = np.sqrt((a64 * a64).sum(axis=-1, keepdims=True))
            den = r + F64(LP_EPS)
            nv = a64 / den
            diff = nv - ref64_
            dn = 0.4 / (float(h) * w) * lin64 * diff
            dot = (nv * dn).sum(axis=-1, keepdims=True)
            if variant == "proj_kept":      # torch's graph: d sqrt at 0 is infinite, the direction f / r is 0 / 0
                with np.errstate(invalid="ignore", divide="ignore"):
                    g = g + (dn - (a64 / r) * dot * r / den) / den
            else:
                g = g + (dn - nv * np.where(r > 0, dot * r / den, 0.0)) / den
            part = (lin64 * diff * diff).sum(axis=-1)
        part = part.reshape(n, h * w)
    if before_mask:
        return g, part
    mask = (a >= 0) if variant == "relu_ge" else (a > 0)
    return np.where(mask, g, dtype(0)).reshape(n, h * w, C), part


def conv1_grad(gpre, w, y, target, dtype, variant=None):
    """lg_conv1_grad_kernel.  gpre [n][H][W][64], w [64][3][3][3], y [n][3][H][W], target codes -> cot [n][3][H][W]"""
    n, H, W, _ = gpre.shape
    if variant == "swap_yx":
        gpre = gpre.reshape(n, W, H, 64)
        H, W = W, H
    gp = np.zeros((n, H + 2, W + 2, 64), dtype)
    gp[:, 1:-1, 1:-1] = gpre
    s = np.zeros((n, 3, H, W, 64), dtype)
    for t in range(9):
        dy, dx = t // 3 - 1, t % 3 - 1
        if variant == "not_mirrored":
            dy, dx = -dy, -dx
        gv = gp[:, 1 - dy:1 - dy + H, 1 - dx:1 - dx + W]                 # the output position that read this pixel through tap t
        for c in range(3):
            wt = (w[:, t // 3, t % 3, c] if variant == "transposed" else w[:, c, t // 3, t % 3]).astype(dtype)
            s[:, c] = fma(gv, wt, s[:, c]) if dtype == F32 else s[:, c] + gv * wt
    if variant == "swap_yx":
        s = s.reshape(n, 3, W, H, 64)
        H, W = W, H
    two_over_d = F32(2.0 / (3.0 * H * W))
    diff = (y - pixel_of_u8(target)).astype(F32)
    sc = LP_SCALE.reshape(1, 3, 1, 1)
    if dtype == F32:
        return ((wave_sum(s) / sc).astype(F32) + (two_over_d * diff).astype(F32)).astype(F32)
    return s.sum(axis=-1) / sc.astype(F64) + 2.0 / (3.0 * H * W) * diff.astype(F64)


def lpips_loss64(part, hws, y, target):
    """lg_loss_kernel in float64 (the differences as the kernel forms them: one float32 subtraction).  part [n][sum hws] -> [n]"""
    n = part.shape[0]
    acc, off = np.zeros(n), 0
    for hw in hws:
        acc += part[:, off:off + hw].astype(F64).sum(axis=1) * (0.2 / hw)
        off += hw
    diff = (y - pixel_of_u8(target)).astype(F32).astype(F64).reshape(n, -1)
    return acc + (diff * diff).sum(axis=1) / diff.shape[1]


# ------------------------------------------------------------------------------------------------------------ restatements: gl_dcgan_grad.hip / gl_pggan_grad.hip
def out_grad(y, cot, target, use_tanh, dtype):
    """tanh_grad_kernel / pg_out_grad_kernel -> g, loss [n] (float64, None without a target)"""
    loss = None
    if target is not None:
        diff = (y - target_f32(target)).astype(F32)
        loss = (diff.astype(F64) ** 2).reshape(len(y), -1).sum(axis=1)
        c = (F32(2.0) * diff).astype(dtype)
    else:
        c = cot.astype(dtype)
    yy = y.astype(dtype)
    if not use_tanh:
        return c, loss
    if dtype == F32:
        return (c * (F32(1.0) - (yy * yy).astype(F32)).astype(F32)).astype(F32), loss
    return c * (1.0 - yy * yy), loss


def patch_rgb(g4):
    """patch_rgb_kernel.  g4 [n][3][64][64] -> [n][1024][64]"""
    n = g4.shape[0]
    gp = np.zeros((n, 3, 66, 66), g4.dtype)
    gp[:, :, 1:-1, 1:-1] = g4
    out = np.zeros((n, 32, 32, 64), g4.dtype)
    for t in range(16):
        ky, kx = t >> 2, t & 3
        for co in range(3):
            out[:, :, :, t * 3 + co] = gp[:, co, ky:ky + 64:2, kx:kx + 64:2]          # 2 y + ky - 1, + 1 for the padding
    return out.reshape(n, 1024, 64)


def relu_bn(dA, a, scale, dtype=F32, variant=None):
    """dA * [a > 0] * scale[c], [n][Ho][Wo][C]"""
    prod = (dA.astype(dtype) * scale.astype(dtype)).astype(dtype)
    return np.where((a >= 0) if variant == "relu_ge" else (a > 0), prod, dtype(0))


def planar_unpack(flat, n, Ho, Wo, C, variant=None):
    """[py * 2 + px][n][Ho/2][Wo/2][C] -> [n][Ho][Wo][C]"""
    p = np.asarray(flat).reshape(2, 2, n, Ho // 2, Wo // 2, C)
    if variant == "phase_swapped":
        p = p.transpose(1, 0, 2, 3, 4, 5)
    return p.transpose(2, 3, 0, 4, 1, 5).reshape(n, Ho, Wo, C)


def rows_unchunk(flat, n, K, kc, chunked=True):
    """[chunk][n][<= kc] with every chunk at a stride of n * kc_full -> [n][K]"""
    flat = np.asarray(flat).reshape(-1)
    if not chunked:
        return flat.reshape(n, K).copy()
    out = np.empty((n, K), flat.dtype)
    for ch, k0 in enumerate(range(0, K, kc)):
        cc = min(kc, K - k0)
        out[:, k0:k0 + cc] = flat[ch * n * kc:ch * n * kc + n * cc].reshape(n, cc)
    return out


def rgb_grad(gout, w, H, pool, factor, dtype):
    """pg_rgb_grad_kernel.  gout [n][nc][R][R], w [nc][C] -> dA [n][H][H][C]"""
    factor = F32(factor)
    g = gout.astype(dtype)
    if pool:
        g = ((g[:, :, 0::2, 0::2] + g[:, :, 0::2, 1::2]).astype(dtype) + (g[:, :, 1::2, 0::2] + g[:, :, 1::2, 1::2]).astype(dtype)).astype(dtype)
    d = (dtype(factor) * g).astype(dtype)
    acc = np.zeros((g.shape[0], H, H, w.shape[1]), dtype)
    for o in range(w.shape[0]):
        acc = fma(d[:, o][..., None], w[o], acc) if dtype == F32 else acc + d[:, o][..., None] * w[o].astype(F64)
    return acc


def pool_sum(dA, dtype):
    """(00 + 01) + (10 + 11) of every 2 x 2 cell, [n][2H][2H][C] -> [n][H][H][C]"""
    d = dA.astype(dtype)
    return ((d[:, 0::2, 0::2] + d[:, 0::2, 1::2]).astype(dtype) + (d[:, 1::2, 0::2] + d[:, 1::2, 1::2]).astype(dtype)).astype(dtype)


def pn_grad(dA, a, inv, extra, pool, dtype, variant=None):
    """pg_pn_grad_kernel.  a [n][H][H][C], inv [n][H][H] -> gpre [n][H H][C]"""
    n, H, _, C = a.shape
    d = pool_sum(dA, dtype) if pool else dA.astype(dtype)
    if extra is not None:
        d = (d + extra.astype(dtype)).astype(dtype)
    slope = F32(0.2) if dtype == F32 else F64(0.2)
    at0 = dtype(0.0) if variant == "slope0" else slope          # the variant: slope 0 at exactly zero
    if dtype == F32:
        s = np.zeros((n, H, H, 64), F32)
        for c0 in range(0, C, 64):
            k = min(64, C - c0)
            s[..., :k] = fma(d[..., c0:c0 + k], a[..., c0:c0 + k], s[..., :k])
        mean = (wave_sum(s) / F32(C)).astype(F32)[..., None]
        t = (inv[..., None] * (d - (a * mean).astype(F32)).astype(F32)).astype(F32)
        out = np.where(a > 0, t, np.where(a == 0, (at0 * t).astype(F32), (slope * t).astype(F32)))
    else:
        a64 = a.astype(F64)
        mean = (d * a64).sum(axis=-1, keepdims=True) / C
        t = inv.astype(F64)[..., None] * (d - a64 * mean)
        out = np.where(a > 0, t, np.where(a == 0, at0 * t, slope * t))
    return out.reshape(n, H * H, C)


def leaky_grad(dA, h, variant=None):
    """pg_leaky_grad_kernel, [n][K]: one rounded multiply"""
    out = np.where(h > 0, dA, (F32(0.2) * dA).astype(F32))
    return np.where(h == 0, F32(0), out) if variant == "slope0" else out


def rowpn_grad(z, g, dtype):
    """pg_rowpn_grad_kernel.  z, g [n][d]"""
    n, d = z.shape
    if dtype == F64:
        z, g = z.astype(F64), g.astype(F64)
        inv = 1.0 / np.sqrt((z * z).mean(axis=1, keepdims=True) + 1e-8)
        zn = z * inv
        return inv * (g - zn * (g * zn).mean(axis=1, keepdims=True))
    ss, s = np.zeros((n, 64), F32), np.zeros((n, 64), F32)
    for c0 in range(0, d, 64):
        k = min(64, d - c0)
        ss[:, :k] = fma(z[:, c0:c0 + k], z[:, c0:c0 + k], ss[:, :k])
    inv = (F32(1.0) / np.sqrt(((wave_sum(ss) / F32(d)).astype(F32) + F32(1e-8)).astype(F32)).astype(F32)).astype(F32)[:, None]
    zn = (z * inv).astype(F32)
    for c0 in range(0, d, 64):
        k = min(64, d - c0)
        s[:, :k] = fma(g[:, c0:c0 + k], zn[:, c0:c0 + k], s[:, :k])
    mean = (wave_sum(s) / F32(d)).astype(F32)[:, None]
    return (inv * (g - (zn * mean).astype(F32)).astype(F32)).astype(F32)


# ------------------------------------------------------------------------------------------------------------ cases
class Case:
    """One launch.  make() -> inputs, every per-image array [3][...] with image 2 = image 0.  launch(d, imgs) -> (ip, f0, inputs, output shapes, copy_in).
    unpack(d, raw, n, variant) -> (dict name -> [n][P][C], bytes that must still be the sentinel).  expect(d, dtype, variant) -> the same dict for all 3
    images.  `exact`: expect(F32) is met bit for bit.  variants: named wrong restatements the case's own comparison must tell from the right one."""
    exact, family, op, variants, same_ok, ulp = True, 0, 0, (), False, ()

    def __init__(self, name, **kw):
        self.name = name
        self.__dict__.update(kw)
        self.rng_seed = zlib.crc32(name.encode())

    def __repr__(self):
        return self.name

    def rng(self):
        return np.random.default_rng(self.rng_seed)


def _tie(d, names):
    for k in names:
        d[k][2] = d[k][0]
    return d


def small_ints(rng, shape, lo=1, hi=9):
    return (rng.integers(lo, hi, shape) * rng.choice([-1, 1], shape)).astype(F32)


# ---- gl_lpips_grad.hip
class ActGrad(Case):
    """lg_act_grad_kernel<C / 64>.  kind: ties (mode 2, all 81 patterns of a cell over {0, 1, 2}), mask (modes 0, 1: a in {-0, 0, 1, 2}), tap (real-valued)"""
    family, op = FAM_LPIPS, 4

    def __init__(self, kind, C, mode, h, w):
        Case.__init__(self, "act_grad_%s_c%d_mode%d_%dx%d" % (kind, C, mode, h, w), kind=kind, C=C, mode=mode, h=h, w=w)
        self.exact = kind != "tap"
        self.same_ok = kind == "mask" and mode == 0
        self.variants = {"ties": ("last_max", "tie_all") + (("not_chunked",) if C > CONV_CHUNK else ()) + (("swap_yx",) if h != w else ()),
                         "mask": ("relu_ge",) if mode == 1 else (), "tap": ("relu_ge",)}[kind]

    def make(self):
        rng, n, h, w, C = self.rng(), N_IMG, self.h, self.w, self.C
        d = {"D": None, "ref": None, "lin": None}
        if self.kind == "ties":
            ncell = (h // 2) * (w // 2)
            pat = (np.arange(ncell * C).reshape(1, ncell, C) + np.array([0, 40, 0]).reshape(3, 1, 1)) % 81
            digits = np.stack([(pat // 3 ** q) % 3 for q in range(4)], axis=2).astype(F32)          # [n][cell][4][C]
            d["a"] = uncells(digits.reshape(n, h // 2, w // 2, 4, C))
            d["D"] = (1 + np.arange(ncell * C).reshape(1, h // 2, w // 2, C) + 4096 * np.array([0, 1, 0]).reshape(3, 1, 1, 1)).astype(F32)
        elif self.kind == "mask":
            d["a"] = rng.choice(np.array([-0.0, 0.0, 1.0, 2.0], F32), (n, h, w, C))
            d["a"][:, 0, 0, :4] = np.array([-0.0, 0.0, 1.0, 2.0], F32)
            if self.mode == 1:
                d["D"] = small_ints(rng, (n, h, w, C), 1, 1000)
        else:
            a = np.maximum(rng.standard_normal((n, h, w, C)), 0).astype(F32)
            a[:, 0, 1, :] = 0                                       # an all-zero position
            a[:, 1, 1, :] = 0
            a[:, 1, 0, :] = 0                                       # one positive channel
            a[:, 1, 0, C - 3] = 5.0                                  # above every other value of its pool cell: it takes what arrives in mode 2
            a[:, 2:4, 0:2, 5] = F32(0.75)                           # one tied pool cell per image (channel 5), positive
            a[:, 2:4, 0:2, 6] = 0                                   # and one tied at zero
            d["a"] = a
            d["ref"] = ref_rows(np.maximum(rng.standard_normal((n, h * w, C)), 0).astype(F32), F32).reshape(n, h, w, C)
            d["lin"] = np.abs(rng.standard_normal(C)).astype(F32) * F32(0.1)
            if self.mode == 1:
                d["D"] = (rng.standard_normal((n, h, w, C)) * 0.05).astype(F32)
            elif self.mode == 2:
                d["D"] = (rng.standard_normal((n, h // 2, w // 2, C)) * 0.05).astype(F32)
        return _tie(d, [k for k in ("a", "D", "ref") if d[k] is not None])

    def launch(self, d, imgs):
        n, hw, C = len(imgs), self.h * self.w, self.C
        tap = d["ref"] is not None
        # the tap's values sit inside longer rows, as in the production buffers: 7 floats / 3 positions in front, 5 / 2 behind
        ref = None
        if tap:
            ref = np.full((n, 7 + hw * C + 5), POISON, F32)
            ref[:, 7:7 + hw * C] = d["ref"][imgs].reshape(n, -1)
        ins = [d["a"][imgs], None if d["D"] is None else d["D"][imgs], ref, d["lin"]]
        outs = [(n * hw * C,), (n, 3 + hw + 2) if tap else None]
        return [n, self.h, self.w, C, self.mode, 7 + hw * C + 5, 7, 3 + hw + 2, 3], 0.0, ins, outs, -1

    def unpack(self, d, raw, n, variant=None):
        hw = self.h * self.w
        out = {"out": unchunk(raw[0], n * hw, self.C, chunked=variant != "not_chunked").reshape(n, hw, self.C)}
        rest = []
        if raw[1] is not None:
            out["part"] = raw[1][:, 3:3 + hw].reshape(n, hw, 1)
            rest = [raw[1][:, :3], raw[1][:, 3 + hw:]]
        return out, rest

    def expect(self, d, dtype=F32, variant=None):
        a, D = d["a"], d["D"]
        if variant == "swap_yx":
            n, h, w, C = a.shape
            a = a.reshape(n, w, h, C)
            D = D.reshape(n, w // 2, h // 2, C)
        o, part = act_grad(a, D, self.mode, d["ref"], d["lin"], dtype, variant)
        return {"out": o} if part is None else {"out": o, "part": part[..., None]}


class MaxPool(Case):
    family, op = FAM_LPIPS, 2

    def __init__(self, kind, C, h, w):
        Case.__init__(self, "maxpool_%s_c%d_%dx%d" % (kind, C, h, w), kind=kind, C=C, h=h, w=w)
        self.variants = ("swap_yx",) if h != w else ()

    def make(self):
        rng, shape = self.rng(), (N_IMG, self.h, self.w, self.C)
        x = rng.integers(0, 3, shape).astype(F32) if self.kind == "ties" else np.maximum(rng.standard_normal(shape), 0).astype(F32)
        return _tie({"x": x}, ["x"])

    def launch(self, d, imgs):
        n = len(imgs)
        return [n, self.h, self.w, self.C], 0.0, [d["x"][imgs]], [(n, (self.h // 2) * (self.w // 2), self.C)], -1

    def unpack(self, d, raw, n, variant=None):
        return {"out": raw[0]}, []

    def expect(self, d, dtype=F32, variant=None):
        return {"out": maxpool(d["x"], variant == "swap_yx").reshape(N_IMG, -1, self.C)}


class RefRows(Case):
    """lg_ref_kernel<C / 64>: integer rows (sum of squares below 2^24), all-zero and one-hot positions; written into longer rows at an offset"""
    family, op = FAM_LPIPS, 3

    def __init__(self, C, h, w):
        Case.__init__(self, "ref_rows_c%d_%dx%d" % (C, h, w), C=C, h=h, w=w)

    def make(self):
        rng, n, hw, C = self.rng(), N_IMG, self.h * self.w, self.C
        f = rng.integers(0, 8, (n, hw, C)).astype(F32)
        f[:, 1] = 0
        f[:, hw - 1] = 0
        f[:, 2] = 0
        f[:, 2, C - 2] = 3
        f[1, 3] = 0
        f[1, 3, 64 % C] = 1
        return _tie({"f": f}, ["f"])

    def launch(self, d, imgs):
        n, hw, C = len(imgs), self.h * self.w, self.C
        return [n, self.h, self.w, C, 11 + hw * C + 6, 11], 0.0, [d["f"][imgs]], [(n, 11 + hw * C + 6)], -1

    def unpack(self, d, raw, n, variant=None):
        hw, C = self.h * self.w, self.C
        return {"out": raw[0][:, 11:11 + hw * C].reshape(n, hw, C)}, [raw[0][:, :11], raw[0][:, 11 + hw * C:]]

    def expect(self, d, dtype=F32, variant=None):
        return {"out": ref_rows(d["f"], dtype)}


class Conv1(Case):
    """lg_conv1_kernel<float | uint8_t>, real-valued"""
    family, exact = FAM_LPIPS, False

    def __init__(self, u8, h, w):
        Case.__init__(self, "conv1_%s_%dx%d" % ("u8" if u8 else "f32", h, w), u8=u8, h=h, w=w)
        self.op = 1 if u8 else 0

    def make(self):
        rng, shape = self.rng(), (N_IMG, 3, self.h, self.w)
        if self.u8:
            img = rng.integers(0, 256, shape).astype(np.uint8)
            if img[0].size >= 256:
                img[0].reshape(-1)[rng.permutation(img[0].size)[:256]] = np.arange(256)
        else:
            img = np.tanh(rng.standard_normal(shape)).astype(F32)
        return _tie({"img": img, "w": (rng.standard_normal((64, 3, 3, 3)) * 0.2).astype(F32), "b": (rng.standard_normal(64) * 0.1).astype(F32)}, ["img"])

    def launch(self, d, imgs):
        n = len(imgs)
        return [n, self.h, self.w, 64], 0.0, [d["img"][imgs], d["w"], d["b"]], [(n, self.h * self.w, 64)], -1

    def unpack(self, d, raw, n, variant=None):
        return {"out": raw[0]}, []

    def expect(self, d, dtype=F32, variant=None):
        return {"out": conv1_fwd(d["img"], d["w"], d["b"], dtype)}


class Conv1Grad(Case):
    """lg_conv1_grad_kernel: integer gpre and weights (every weight different), y at the target's own value (image 0 / 2) and away from it (image 1)"""
    family, op = FAM_LPIPS, 5

    def __init__(self, h, w):
        Case.__init__(self, "conv1_grad_%dx%d" % (h, w), h=h, w=w)
        self.variants = ("not_mirrored", "transposed") + (("swap_yx",) if h != w else ())

    def make(self):
        rng, n, h, w = self.rng(), N_IMG, self.h, self.w
        target = rng.integers(0, 256, (n, 3, h, w)).astype(np.uint8)
        y = pixel_of_u8(target)
        y[1] = np.tanh(rng.standard_normal((3, h, w))).astype(F32)
        y[0, :, 0, 0] += F32(0.25)
        d = {"gpre": rng.integers(-2, 3, (n, h, w, 64)).astype(F32), "w": (np.arange(64 * 27) - 864).astype(F32).reshape(64, 3, 3, 3), "y": y, "target": target}
        return _tie(d, ["gpre", "y", "target"])

    def launch(self, d, imgs):
        n = len(imgs)
        return [n, self.h, self.w, 64], 0.0, [d["gpre"][imgs], d["w"], d["y"][imgs], d["target"][imgs]], [(n, 3, self.h * self.w)], -1

    def unpack(self, d, raw, n, variant=None):
        return {"out": raw[0]}, []

    def expect(self, d, dtype=F32, variant=None):
        return {"out": conv1_grad(d["gpre"], d["w"], d["y"], d["target"], dtype, variant).reshape(N_IMG, 3, -1)}


class LpipsLoss(Case):
    """lg_loss_kernel: float64 sum rounded to float32, within 1 ulp"""
    family, op, exact, ulp = FAM_LPIPS, 6, False, ("loss",)

    def __init__(self, name, hws, dimg):
        Case.__init__(self, "lpips_loss_" + name, hws=hws, dimg=dimg)

    def make(self):
        rng, n = self.rng(), N_IMG
        d = {"part": np.abs(rng.standard_normal((n, sum(self.hws) + 3))).astype(F32), "y": np.tanh(rng.standard_normal((n, self.dimg))).astype(F32),
             "target": rng.integers(0, 256, (n, self.dimg)).astype(np.uint8)}
        return _tie(d, ["part", "y", "target"])

    def launch(self, d, imgs):
        n = len(imgs)
        return [n, self.dimg, sum(self.hws) + 3, 0] + list(self.hws), 0.0, [d["part"][imgs], d["y"][imgs], d["target"][imgs]], [(n, 1, 1)], -1

    def unpack(self, d, raw, n, variant=None):
        return {"loss": raw[0]}, []

    def expect(self, d, dtype=F32, variant=None):
        return {"loss": lpips_loss64(d["part"], self.hws, d["y"], d["target"]).astype(dtype).reshape(N_IMG, 1, 1)}


# ---- gl_dcgan_grad.hip and gl_pggan_grad.hip
class OutGrad(Case):
    """tanh_grad_kernel<L2> (family 0: 3 x 64 x 64 images) and pg_out_grad_kernel<L2> (family 1: any size, use_tanh)"""

    def __init__(self, family, l2, img, use_tanh=1):
        Case.__init__(self, "%s_%s_img%d%s" % ("tanh_grad" if family == FAM_DCGAN else "pg_out_grad", "l2" if l2 else "cot", img, "" if use_tanh else "_notanh"),
                      l2=l2, img=img, use_tanh=use_tanh)
        self.family, self.op, self.exact = family, 1 if l2 else 0, not l2
        self.ulp = ("loss",) if l2 else ()

    def make(self):
        rng, shape = self.rng(), (N_IMG, self.img)
        if self.l2:
            t = rng.integers(0, 256, shape).astype(np.uint8)
            t[:, :256] = np.arange(256)
            t[1, :256] = np.arange(256)[::-1]
            return _tie({"y": np.tanh(rng.standard_normal(shape)).astype(F32), "cot": None, "target": t}, ["y", "target"])
        return _tie({"y": rng.choice(np.array([0, 0.5, -0.5, 1, -1], F32), shape), "cot": small_ints(rng, shape, 1, 1000), "target": None}, ["y", "cot"])

    def launch(self, d, imgs):
        n = len(imgs)
        second = d["target"][imgs] if self.l2 else d["cot"][imgs]
        ip = [n] if self.family == FAM_DCGAN else [n, self.img, self.use_tanh]
        return ip, 0.0, [d["y"][imgs], second], [(n, self.img, 1), (n, 1, 1) if self.l2 else None], -1

    def unpack(self, d, raw, n, variant=None):
        return ({"g": raw[0], "loss": raw[1]} if self.l2 else {"g": raw[0]}), []

    def expect(self, d, dtype=F32, variant=None):
        g, loss = out_grad(d["y"], d["cot"], d["target"], self.use_tanh, dtype)
        out = {"g": g.reshape(N_IMG, self.img, 1)}
        if loss is not None:
            out["loss"] = loss.astype(dtype).reshape(N_IMG, 1, 1)
        return out


class PatchRgb(Case):
    family, op = FAM_DCGAN, 2

    def make(self):
        g4 = (1 + np.arange(3 * 3 * 64 * 64)).astype(F32).reshape(3, 3, 64, 64)
        return _tie({"g4": g4}, ["g4"])

    def launch(self, d, imgs):
        n = len(imgs)
        return [n], 0.0, [d["g4"][imgs]], [(n, 1024, 64)], -1

    def unpack(self, d, raw, n, variant=None):
        return {"patch": raw[0]}, []

    def expect(self, d, dtype=F32, variant=None):
        return {"patch": patch_rgb(d["g4"])}


class ReluBn(Case):
    """relu_bn_grad_kernel<PLANAR>: distinct integer dA, power-of-two scales, a in {0, 1} (and -0)"""
    family, op = FAM_DCGAN, 3

    def __init__(self, planar, C, kc=0):
        Case.__init__(self, "relu_bn_grad_%s_c%d" % ("planar" if planar else "rows_kc%d" % kc, C), planar=planar, C=C, kc=kc)
        self.variants = ("relu_ge", "phase_swapped" if planar else "not_chunked")

    def make(self):
        rng, n, C = self.rng(), N_IMG, self.C
        dA = (1 + np.arange(n * 16 * C)).astype(F32).reshape(n, 4, 4, C)
        a = rng.choice(np.array([0.0, 1.0, -0.0], F32), (n, 4, 4, C))
        return _tie({"dA": dA, "a": a, "scale": np.ldexp(1.0, rng.integers(-3, 4, C)).astype(F32)}, ["dA", "a"])

    def launch(self, d, imgs):
        n = len(imgs)
        return [n, 4, 4, self.C, 1 if self.planar else 0, self.kc], 0.0, [d["dA"][imgs], d["a"][imgs], d["scale"]], [(n * 16 * self.C,)], -1

    def unpack(self, d, raw, n, variant=None):
        if self.planar:
            return {"gpre": planar_unpack(raw[0], n, 4, 4, self.C, variant).reshape(n, 16, self.C)}, []
        return {"gpre": rows_unchunk(raw[0], n, 16 * self.C, self.kc, variant != "not_chunked").reshape(n, 16, self.C)}, []

    def expect(self, d, dtype=F32, variant=None):
        return {"gpre": relu_bn(d["dA"], d["a"], d["scale"], dtype, variant).reshape(N_IMG, 16, self.C)}


class RgbGrad(Case):
    """pg_rgb_grad_kernel: integer g and weights, a power-of-two factor"""
    family, op = FAM_PGGAN, 2

    def __init__(self, pool, nc, H=4, C=32):
        Case.__init__(self, "pg_rgb_grad_%s_nc%d" % ("pool" if pool else "plain", nc), pool=pool, nc=nc, H=H, C=C)

    def make(self):
        rng, R = self.rng(), self.H * (2 if self.pool else 1)
        return _tie({"g": small_ints(rng, (N_IMG, self.nc, R, R), 1, 100), "w": small_ints(rng, (self.nc, self.C), 1, 100)}, ["g"])

    def launch(self, d, imgs):
        n = len(imgs)
        return [n, self.H, self.C, self.nc, 1 if self.pool else 0], 0.25, [d["g"][imgs], d["w"]], [(n, self.H * self.H, self.C)], -1

    def unpack(self, d, raw, n, variant=None):
        return {"dA": raw[0]}, []

    def expect(self, d, dtype=F32, variant=None):
        return {"dA": rgb_grad(d["g"], d["w"], self.H, self.pool, 0.25, dtype).reshape(N_IMG, -1, self.C)}


class PnGrad(Case):
    """pg_pn_grad_kernel, real-valued: units at exactly 0, one all-zero position, inv as the forward stores it"""
    family, op, exact = FAM_PGGAN, 3, False

    def __init__(self, C, pool, extra, H=4):
        Case.__init__(self, "pg_pn_grad_c%d_%s_%s" % (C, "pool" if pool else "plain", "extra" if extra else "noextra"), C=C, pool=pool, extra=extra, H=H)
        self.variants = ("slope0",) + (("not_chunked",) if C > CONV_CHUNK else ())

    def make(self):
        rng, n, H, C = self.rng(), N_IMG, self.H, self.C
        pre = rng.standard_normal((n, H, H, C)).astype(F32)
        leaky = np.where(pre > 0, pre, (F32(0.2) * pre).astype(F32))
        leaky[:, :, :, 3] = 0                                        # units at exactly 0 (and -0)
        leaky[:, 1, 2, 7] = -0.0
        leaky[:, 2, 1, :] = 0                                        # an all-zero position: inv = 1e4
        inv = (1.0 / np.sqrt((leaky.astype(F64) ** 2).mean(axis=-1) + 1e-8)).astype(F32)
        d = {"a": (leaky * inv[..., None]).astype(F32), "inv": inv, "dA": rng.standard_normal((n, H * (2 if self.pool else 1), H * (2 if self.pool else 1), C)).astype(F32),
             "extra": rng.standard_normal((n, H, H, C)).astype(F32) if self.extra else None}
        return _tie(d, [k for k in ("a", "inv", "dA", "extra") if d[k] is not None])

    def launch(self, d, imgs):
        n = len(imgs)
        ins = [d["dA"][imgs], d["a"][imgs], d["inv"][imgs], d["extra"][imgs] if self.extra else None]
        return [n, self.H, self.C, 1 if self.pool else 0], 0.0, ins, [(n * self.H * self.H * self.C,)], -1

    def unpack(self, d, raw, n, variant=None):
        P = n * self.H * self.H
        return {"gpre": unchunk(raw[0], P, self.C, chunked=variant != "not_chunked").reshape(n, self.H * self.H, self.C)}, []

    def expect(self, d, dtype=F32, variant=None):
        return {"gpre": pn_grad(d["dA"], d["a"], d["inv"], d["extra"], self.pool, dtype, variant)}


class LeakyGrad(Case):
    """pg_leaky_grad_kernel: K = 1536 = a chunk of 1024 and a ragged one of 512"""
    family, op, variants = FAM_PGGAN, 4, ("slope0", "not_chunked")

    def __init__(self, K):
        Case.__init__(self, "pg_leaky_grad_k%d" % K, K=K)

    def make(self):
        rng, shape = self.rng(), (N_IMG, self.K)
        return _tie({"dA": small_ints(rng, shape, 1, 1000), "h": rng.choice(np.array([-1.0, -0.0, 0.0, 1.0], F32), shape)}, ["dA", "h"])

    def launch(self, d, imgs):
        n = len(imgs)
        return [n, self.K], 0.0, [d["dA"][imgs], d["h"][imgs]], [(n * self.K,)], -1

    def unpack(self, d, raw, n, variant=None):
        return {"gpre": rows_unchunk(raw[0], n, self.K, PG_K0, variant != "not_chunked").reshape(n, 1, self.K)}, []

    def expect(self, d, dtype=F32, variant=None):
        return {"gpre": leaky_grad(d["dA"], d["h"], variant).reshape(N_IMG, 1, self.K)}


class RowPn(Case):
    """pg_rowpn_grad_kernel, in place on the gradient rows"""
    family, op, exact = FAM_PGGAN, 5, False

    def __init__(self, dim):
        Case.__init__(self, "pg_rowpn_grad_d%d" % dim, dim=dim)

    def make(self):
        rng, shape = self.rng(), (N_IMG, self.dim)
        return _tie({"z": rng.standard_normal(shape).astype(F32), "g": rng.standard_normal(shape).astype(F32)}, ["z", "g"])

    def launch(self, d, imgs):
        n = len(imgs)
        return [n, self.dim], 0.0, [d["z"][imgs], d["g"][imgs]], [(n, 1, self.dim)], 1

    def unpack(self, d, raw, n, variant=None):
        return {"dz": raw[0]}, []

    def expect(self, d, dtype=F32, variant=None):
        return {"dz": rowpn_grad(d["z"], d["g"], dtype).reshape(N_IMG, 1, self.dim)}


J_WIDTHS = (64, 128, 256, 512)
ALL_CASES = []
for _C in J_WIDTHS:
    ALL_CASES += [ActGrad("ties", _C, 2, 4, 4), ActGrad("mask", _C, 1, 4, 2), RefRows(_C, 4, 2 if _C in (64, 256) else 4)]
    ALL_CASES += [ActGrad("tap", _C, _m, 4, 2 if _m == 1 else 4) for _m in (0, 1, 2)]
ALL_CASES += [ActGrad("ties", 64, 2, 4, 2), ActGrad("ties", 256, 2, 4, 2), ActGrad("mask", 128, 0, 4, 4), ActGrad("tap", 256, 2, 4, 2),
              MaxPool("ties", 64, 4, 2), MaxPool("real", 256, 4, 4),
              Conv1(False, 4, 4), Conv1(False, 4, 2), Conv1(True, 12, 8), Conv1(True, 4, 2), Conv1Grad(4, 2), Conv1Grad(4, 4),
              LpipsLoss("16x16", (256, 64, 16, 4, 1), 3 * 16 * 16), LpipsLoss("odd", (300, 77, 1, 5, 257), 777),
              OutGrad(FAM_DCGAN, False, 3 * 64 * 64), OutGrad(FAM_DCGAN, True, 3 * 64 * 64), PatchRgb("patch_rgb"),
              ReluBn(True, 32), ReluBn(True, 64), ReluBn(False, 32, kc=64),
              OutGrad(FAM_PGGAN, False, 192), OutGrad(FAM_PGGAN, False, 16, use_tanh=0), OutGrad(FAM_PGGAN, True, 768), OutGrad(FAM_PGGAN, True, 300, use_tanh=0),
              RgbGrad(False, 1), RgbGrad(False, 3), RgbGrad(True, 1), RgbGrad(True, 3)]
ALL_CASES += [PnGrad(_C, _p, _e) for _C in (32, 64, 160) for _p in (0, 1) for _e in (0, 1)]
ALL_CASES += [LeakyGrad(1536), RowPn(64), RowPn(100)]
EXACT_CASES = [c for c in ALL_CASES if c.exact]
REAL_CASES = [c for c in ALL_CASES if not c.exact]
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)


# ------------------------------------------------------------------------------------------------------------ comparison
def ulps(got, want32):
    """distance in float32 steps (both finite, same sign or zero)"""
    a, b = np.asarray(got, F32).view(np.int32).astype(np.int64), np.asarray(want32, F32).view(np.int32).astype(np.int64)
    return int(np.abs(a - b).max())


def image_errors(got, want64):
    """|g - g64|_2 / |g64|_2 per image -> [n]"""
    got, want64 = np.asarray(got, F64), np.asarray(want64, F64)
    n = len(got)
    return np.linalg.norm((got - want64).reshape(n, -1), axis=1) / np.linalg.norm(want64.reshape(n, -1), axis=1)


# A position at which the float32 restatement itself is this far from float64 (relative) is a cancellation, not a rounding.  The constant is chosen by
# hand, between float32's rounding (1e-7; the worst well-conditioned position of any case is 1.2e-5) and a lost position (1): tests/test_grad_kernels_cpu.py
# pins the only positions it may apply to (the one-hot position of the mode-0 tap cases) and that no other position of any case comes near it
ILL = 1e-3


def position_errors(got, want32, want64):
    """The same metric position by position (the norms over the last axis).  Three kinds of position, told apart on the reference side alone:
      * the float64 reference is all zero (an all-zero tap position behind the ReLU mask): `got` has to be exactly zero;
      * the float32 restatement is more than ILL away from float64: the formula cancels there beyond float32 (a position with ONE positive channel
        and nothing arriving from above: n is one-hot, dn - n (n . dn) r / (r + eps) = dn eps / (r + eps), and float32 gives 0) -- a relative
        error says nothing, so the absolute error of `got` is compared with the restatement's at the same position;
      * every other position: the relative error, the largest of them
    -> dict(dev, f32: largest relative errors; stray: non-zero values at all-zero positions; ill: number of cancelling positions; ill_ratio: largest
    absolute error of `got` over the restatement's at those)"""
    got, want32, want64 = np.asarray(got, F64), np.asarray(want32, F64), np.asarray(want64, F64)
    den = np.linalg.norm(want64, axis=-1)
    e_dev, e_f32 = np.linalg.norm(got - want64, axis=-1), np.linalg.norm(want32 - want64, axis=-1)
    live = den > 0
    ill = live & (e_f32 > ILL * den)
    ok = live & ~ill
    return {"dev": float((e_dev[ok] / den[ok]).max()), "f32": float((e_f32[ok] / den[ok]).max()), "stray": int((got[~live] != 0).sum()),
            "ill": int(ill.sum()), "ill_ratio": float((e_dev[ill] / e_f32[ill]).max()) if ill.any() else 0.0}


def evaluate(c, d, dev3, rest3, dev1, guards_ok, variant=None):
    """dev3 / dev1: the unpacked outputs of the n = 3 run and of image 0 alone; rest3: what must still be the sentinel -> the case's verdict (JSON-able)"""
    sent32 = np.frombuffer(bytes([SENTINEL]) * 4, np.uint32)[0]
    bits3 = {k: np.ascontiguousarray(v, F32).view(np.uint32) for k, v in dev3.items()}
    bits1 = {k: np.ascontiguousarray(v, F32).view(np.uint32) for k, v in dev1.items()}
    res = {"guards_ok": bool(guards_ok),
           "finite": all(bool(np.isfinite(v).all()) for v in dev3.values()),
           "written": all(bool((b != sent32).all()) for b in bits3.values()),
           "rest_untouched": all(bool((np.ascontiguousarray(r).view(np.uint8) == SENTINEL).all()) for r in rest3),
           "img0_eq_img2": all(bool(np.array_equal(b[0], b[2])) for b in bits3.values()),
           "img0_ne_img1": c.same_ok or any(not np.array_equal(b[0], b[1]) for b in bits3.values()),
           "n1_eq_img0": all(bool(np.array_equal(bits1[k][0], bits3[k][0])) for k in bits3)}
    want32 = c.expect(d, F32, variant)
    if c.exact:
        # == on values: -0 and +0 are one value (a kernel may form either where the formula gives zero); NaN equals nothing
        res["nbad"] = {k: int((np.asarray(dev3[k], F32) != want32[k]).sum()) for k in want32}
        return res
    want64 = c.expect(d, F64, variant)
    res["err_dev"], res["err_f32"], res["pos_dev"], res["pos_f32"], res["stray"], res["ulp"], res["ill"], res["ill_ratio"] = {}, {}, {}, {}, {}, {}, {}, {}
    for k in want64:
        if k in c.ulp:
            res["ulp"][k] = ulps(dev3[k], want64[k].astype(F32)) if np.isfinite(dev3[k]).all() else -1
            continue
        res["err_dev"][k], res["err_f32"][k] = image_errors(dev3[k], want64[k]).tolist(), image_errors(want32[k], want64[k]).tolist()
        p = position_errors(dev3[k], want32[k], want64[k])
        res["pos_dev"][k], res["pos_f32"][k], res["stray"][k], res["ill"][k], res["ill_ratio"][k] = p["dev"], p["f32"], p["stray"], p["ill"], p["ill_ratio"]
    return res


def verdict(c, r):
    """-> list of what is wrong with a case's result (empty: it passes)"""
    if "error" in r:
        return ["error: " + r["error"]]
    bad = [k for k in ("guards_ok", "finite", "written", "rest_untouched", "img0_eq_img2", "img0_ne_img1", "n1_eq_img0") if not r.get(k)]
    if c.exact:
        return bad + ["%s: %d values differ" % (k, v) for k, v in r["nbad"].items() if v]
    for k, v in r["ulp"].items():
        if not 0 <= v <= 1:
            bad.append("%s: %d ulp from the float64 sum" % (k, v))
    for k in r["err_dev"]:
        a = max(r["err_f32"][k])
        if not all(e <= SLACK * a for e in r["err_dev"][k]):
            bad.append("%s: image error %.3e > %g x %.3e" % (k, max(r["err_dev"][k]), SLACK, a))
        if not r["pos_dev"][k] <= SLACK * r["pos_f32"][k]:
            bad.append("%s: position error %.3e > %g x %.3e" % (k, r["pos_dev"][k], SLACK, r["pos_f32"][k]))
        if not r["ill_ratio"][k] <= SLACK:
            bad.append("%s: at a cancelling position the absolute error is %.2f x the float32 restatement's" % (k, r["ill_ratio"][k]))
        if r["stray"][k]:
            bad.append("%s: %d non-zero values where the reference is all zero" % (k, r["stray"][k]))
    return bad


# ------------------------------------------------------------------------------------------------------------ the GPU entry
class TuneGradOp(ctypes.Structure):          # csrc/gl_tune.hip GlTuneGradOp
    _fields_ = [("family", ctypes.c_int32), ("op", ctypes.c_int32), ("sentinel", ctypes.c_int32), ("copy_in", ctypes.c_int32),
                ("poison", ctypes.c_float), ("f0", ctypes.c_float), ("ip", ctypes.c_int64 * 12),
                ("in_", ctypes.c_void_p * 4), ("in_bytes", ctypes.c_int64 * 4), ("out", ctypes.c_void_p * 2), ("out_bytes", ctypes.c_int64 * 2),
                ("out_guards", ctypes.c_void_p)]


STRUCT_LAYOUT = {"size": 224, "ip": 24, "in_": 120, "in_bytes": 152, "out": 184, "out_bytes": 200, "out_guards": 216}      # the static_assert of gl_tune.hip


def run_case(lib, ctx_handle, c, d, imgs):
    """one launch through gl_tune_grad_op on the images `imgs` -> (unpacked outputs, rest, guards all sentinel)"""
    imgs = list(imgs)
    ip, f0, ins, out_shapes, copy_in = c.launch(d, imgs)
    ins = [None if a is None else np.ascontiguousarray(a) for a in ins]
    raw = [None if s is None else np.empty(s, F32) for s in out_shapes] + [None] * (2 - len(out_shapes))
    og = np.empty(4 * GUARD, np.uint8)
    q = TuneGradOp()
    q.family, q.op, q.sentinel, q.copy_in, q.poison, q.f0 = c.family, c.op, SENTINEL, copy_in, POISON, f0
    for i, v in enumerate(ip):
        q.ip[i] = int(v)
    for i, a in enumerate(ins):
        q.in_[i], q.in_bytes[i] = (a.ctypes.data, a.nbytes) if a is not None else (None, 0)
    for i, a in enumerate(raw):
        q.out[i], q.out_bytes[i] = (a.ctypes.data, a.nbytes) if a is not None else (None, 0)
    q.out_guards = og.ctypes.data
    lib.gl_tune_grad_op.restype = ctypes.c_int
    lib.gl_tune_grad_op.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    rc = lib.gl_tune_grad_op(ctx_handle, ctypes.byref(q))
    if rc != 0:
        lib.gl_last_error.restype = ctypes.c_char_p
        raise RuntimeError("gl_tune_grad_op(%s): %s" % (c.name, lib.gl_last_error().decode()))
    out, rest = c.unpack(d, raw, len(imgs))
    return out, rest, bool((og == SENTINEL).all())
