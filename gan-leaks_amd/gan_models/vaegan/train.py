"""Counterpart of the `Generator` class of the reference's gan_models/vaegan/train.py:109-135 (with `SpectralNorm`
and `SelfAttention` from gan_models/vaegan/ops.py:23-75,86-120) and of its `Encoder` class (train.py:61-106), for inference.
Discriminators and training are out of scope.

    Generator(z_dim, d=64)(x[N,z_dim,1,1]) -> [N,3,64,64]
    4 x [SpectralNorm(ConvTranspose2d + bias) -> BatchNorm2d -> ReLU], SelfAttention after the third, ConvTranspose2d -> tanh

SpectralNorm is STATEFUL at inference in the reference: every forward runs one power iteration that overwrites
`weight_u` / `weight_v` (ops.py:32-44,73-75), also under `.eval()`.  This class reproduces that: each call of
`forward` advances u, v once per wrapped layer (host side, fp32 like the reference), folds 1/sigma, the
ConvTranspose bias and BatchNorm(eval) into the convolution epilogue and runs the stack on the HIP generator.
`state_dict()` returns the advanced u, v so a run can be continued or compared.

`Generator.frozen(k)` -> `FrozenGenerator`: the same generator with the state of its k-th next forward held for good, a fixed function of z
with gradients with respect to z -- what the partial-black-box and the white-box attack take (the plain Generator stays stateful and refused).

    Encoder(z_dim, d=64).encode(x[N,3,64,64]) -> (z_mu, z_var) [N,z_dim]
    4 x [Conv2d(k4, s2, p1) -> BatchNorm2d -> ReLU], then two heads Linear(8192, 4 z) -> BatchNorm1d -> ReLU -> Linear(4 z, z)
on the HIP encoder (csrc/gl_vaegan_enc.hip): what the reconstruction attack (recon.py) and `--encoder_path` of pbb.py / wb.py read.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ..._lib import Context, DeviceArray, as_device, check

_p = ctypes.c_void_p


def _np(v):
    if type(v).__module__.startswith("torch"):
        v = v.detach().cpu().numpy()
    return np.ascontiguousarray(v, dtype=np.float32)


def _load(lib, h, sd, chans, d, power_iterations, state=None):
    """install a reference state dict in the gl_dcgan handle h; state: spectral-norm vectors that take the place of sd's (state_dict()'s keys).
    -> the float32 arrays that were installed, by key, so that a frozen view can be loaded from them"""
    state = state or {}
    kept = {}

    def get(key):
        kept[key] = _np(state[key] if key in state else sd[key])
        return kept[key]

    for l in range(4):
        name = "deconv%d" % (l + 1)
        w = get(name + ".module.weight_bar")
        if w.shape != (chans[l], chans[l + 1], 4, 4):
            raise ValueError("%s.module.weight_bar has shape %s" % (name, w.shape))
        u, v, bias = (get(name + ".module." + k) for k in ("weight_u", "weight_v", "bias"))
        g, b, mu, var = (get("%s_bn.%s" % (name, k)) for k in ("weight", "bias", "running_mean", "running_var"))
        # BatchNorm(eval) and the ConvTranspose bias fold into y = conv(x, w_bar) * (bn_s / sigma) + shift; sigma is advanced on the device
        bn_s = g.astype(np.float64) / np.sqrt(var.astype(np.float64) + 1e-5)
        shift = ((bias.astype(np.float64) - mu) * bn_s + b).astype(np.float32)
        bn_s = bn_s.astype(np.float32)
        check(lib.gl_dcgan_set_spectral_norm(h, l, w.ctypes.data_as(_p), u.ctypes.data_as(_p), v.ctypes.data_as(_p), bn_s.ctypes.data_as(_p),
                                             shift.ctypes.data_as(_p), int(power_iterations)))
    w5, b5 = get("deconv5.weight"), get("deconv5.bias")
    check(lib.gl_dcgan_set_conv_weight(h, 4, w5.ctypes.data_as(_p)))
    check(lib.gl_dcgan_set_out_bias(h, b5.ctypes.data_as(_p)))
    C = 2 * d
    att = [get("sa1.%s_conv.%s" % (n, k)) for n in ("query", "key", "value") for k in ("weight", "bias")]
    wq, bq, wk, bk, wv, bv = att
    if wq.shape != (C // 8, C, 1, 1) or wv.shape != (C, C, 1, 1):
        raise ValueError("sa1 conv weights have shapes %s / %s" % (wq.shape, wv.shape))
    gamma = float(get("sa1.gamma").reshape(-1)[0])
    check(lib.gl_dcgan_set_attention(h, *[a.ctypes.data_as(_p) for a in (wq, bq, wk, bk, wv, bv)], ctypes.c_float(gamma)))
    return kept


def _spectral_state(lib, h, chans):
    out = {}
    for l in range(4):
        u = np.empty(chans[l], np.float32)
        v = np.empty(chans[l + 1] * 16, np.float32)
        check(lib.gl_dcgan_get_spectral_state(h, l, u.ctypes.data_as(_p), v.ctypes.data_as(_p)))
        out["deconv%d.module.weight_u" % (l + 1)] = u
        out["deconv%d.module.weight_v" % (l + 1)] = v
    return out


class Generator:
    def __init__(self, z_dim, d=64, ctx=None):
        self.z_dim, self.d = int(z_dim), int(d)
        if self.d % 32 != 0:
            raise ValueError("d must be a multiple of 32")
        self._ctx = ctx
        self._handle = None
        self._loaded = False
        self.power_iterations = 1
        self._precision = 1
        self.chans = [self.z_dim, 8 * self.d, 4 * self.d, 2 * self.d, self.d, 3]

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = Context.get()
        return self._ctx

    def _ensure(self):
        if self._handle is None:
            h = _p()
            # the ConvTranspose stack is the DCGAN one with features_g = d / 2
            check(self.ctx.lib.gl_dcgan_create(self.ctx.handle, self.z_dim, 3, self.d // 2, ctypes.byref(h)))
            self._handle = h
        return self._handle

    def __del__(self):
        if getattr(self, "_handle", None) is not None:
            try:
                self.ctx.lib.gl_dcgan_destroy(self._handle)
            except Exception:  # noqa: BLE001
                pass

    def load_state_dict(self, sd, strict=True):
        self._arrays = _load(self.ctx.lib, self._ensure(), sd, self.chans, self.d, self.power_iterations)
        self._loaded = True
        return "<All keys matched successfully>"

    def state_dict(self):
        """the spectral-norm state after the forwards run so far (it lives on the device)"""
        return _spectral_state(self.ctx.lib, self._handle, self.chans)

    def frozen(self, forwards=1):
        """A generator that is a FIXED function of z: an independent object with its own device handle, loaded from this generator's weights
        and its current u, v, whose spectral-norm state is advanced `forwards` >= 1 times on the device and then held for good.  Its forward
        equals this generator's forwards-th next forward bit for bit (in the precision this generator has now); this generator is not touched.
        The view is what pbb_attack, wb_attack and their l2-lpips forms take (-> FrozenGenerator)."""
        if int(forwards) != forwards or forwards < 1:
            raise ValueError("forwards must be an integer >= 1, got %r" % (forwards,))
        if not self._loaded:
            raise RuntimeError("Generator: load_state_dict() has not been called")
        return FrozenGenerator(self, int(forwards))

    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    def cuda(self, *a, **k):                 # vaegan/sample.py:36 calls .cuda(); the weights already live on the device
        return self

    def train(self, mode=True):              # inference only: BatchNorm always uses its running statistics
        return self

    def set_precision(self, mode):
        """1 (default) = split-fp16 convolutions (three fp16 MFMAs per product), 0 = fp32 MFMA; the attention block is fp32 MFMA in both"""
        check(self.ctx.lib.gl_dcgan_set_precision(self._ensure(), int(mode)))
        self._precision = int(mode)

    def forward_device(self, x, want_f32=True, want_u8=False):
        if not self._loaded:
            raise RuntimeError("Generator: load_state_dict() has not been called")
        z = as_device(self.ctx, x, np.float32)
        n = z.shape[0]
        if int(np.prod(z.shape[1:], dtype=np.int64)) != self.z_dim:
            raise ValueError("expected z of shape [N,%d,1,1], got %s" % (self.z_dim, z.shape))
        # gl_dcgan_forward advances the spectral-norm state by one power iteration per call on the device, as the reference does
        shape = (n, 3, 64, 64)
        f32 = self.ctx.empty(shape, np.float32) if want_f32 else None
        u8 = self.ctx.empty(shape, np.uint8) if want_u8 else None
        check(self.ctx.lib.gl_dcgan_forward(self._handle, _p(z.ptr), n, _p(f32.ptr if f32 else 0), _p(u8.ptr if u8 else 0)))
        if self._precision == 1 and self.ctx.h3_saturations() > 0:
            # an activation left the fp16 range of the split layout: redo this call (same spectral-norm state) with fp32 products
            import warnings
            warnings.warn("split-fp16 generator path saturated for these weights; falling back to fp32 MFMA products")
            self.set_precision(0)
            check(self.ctx.lib.gl_dcgan_set_spectral_hold(self._handle, 1))
            try:
                check(self.ctx.lib.gl_dcgan_forward(self._handle, _p(z.ptr), n, _p(f32.ptr if f32 else 0), _p(u8.ptr if u8 else 0)))
            finally:
                check(self.ctx.lib.gl_dcgan_set_spectral_hold(self._handle, 0))
        return f32, u8

    def forward(self, input):
        f32, _ = self.forward_device(input, True, False)
        out = f32.numpy()
        if type(input).__module__.startswith("torch"):
            import torch
            return torch.from_numpy(out).to(input.device)
        return out

    __call__ = forward

    def generate_u8(self, x):
        """8-bit bank of the generator's samples (u8 DeviceArray [N,3,64,64], bank index = latent index), quantised as the image generate
        branches do (gan_models/dcgan/train_torch.py:154-158,172).  The reference's VAEGAN sampler keeps floats (vaegan/sample.py:55-59)
        and has no reader in fbb.py; this is what `attack(queries, GeneratedBank(generator, z))` consumes.  One forward =
        one spectral-norm step, like forward()."""
        return self.forward_device(x, False, True)[1]


class FrozenGenerator:
    """Generator.frozen(forwards): the VAEGAN generator with its spectral-norm state held, a fixed function of z.  It offers what the attacks and
    GeneratedBank take from the DCGAN / WGAN-GP generator (gan_models/dcgan/model_torch.py), the gradients with respect to z included: with sigma
    held, the stack is the DCGAN ConvTranspose stack plus the self-attention block, whose backward pass is csrc/gl_attention_grad.hip.  It has no
    `power_iterations`: that attribute is how the attacks tell a generator that changes with every forward."""
    image_shape = (3, 64, 64)
    channels_img = 3

    def __init__(self, parent, forwards):
        self.z_dim, self.d, self.forwards = parent.z_dim, parent.d, int(forwards)
        self.chans = list(parent.chans)
        self._ctx = parent.ctx
        self._handle = None
        lib = self._ctx.lib
        h = _p()
        check(lib.gl_dcgan_create(self._ctx.handle, self.z_dim, 3, self.d // 2, ctypes.byref(h)))
        self._handle = h
        _load(lib, h, parent._arrays, self.chans, self.d, parent.power_iterations, state=parent.state_dict())
        check(lib.gl_dcgan_advance_spectral(h, self.forwards))
        check(lib.gl_dcgan_set_spectral_hold(h, 1))
        self._precision = 1
        self.set_precision(parent._precision)

    @property
    def ctx(self):
        return self._ctx

    def __del__(self):
        if getattr(self, "_handle", None) is not None:
            try:
                self._ctx.lib.gl_dcgan_destroy(self._handle)
            except Exception:  # noqa: BLE001
                pass

    def state_dict(self):
        """the held u, v"""
        return _spectral_state(self._ctx.lib, self._handle, self.chans)

    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    def cuda(self, *a, **k):
        return self

    def train(self, mode=True):
        return self

    def set_precision(self, mode):
        """1 = split-fp16 convolutions, 0 = fp32 MFMA; the attention block is fp32 MFMA in both"""
        check(self._ctx.lib.gl_dcgan_set_precision(self._handle, int(mode)))
        self._precision = int(mode)

    def set_chunk(self, images_per_pass):
        check(self._ctx.lib.gl_dcgan_set_chunk(self._handle, int(images_per_pass)))

    def _z_device(self, x):
        z = as_device(self._ctx, x, np.float32)
        n = z.shape[0]
        if int(np.prod(z.shape[1:], dtype=np.int64)) != self.z_dim:
            raise ValueError("expected z of shape [N,%d,1,1], got %s" % (self.z_dim, z.shape))
        return z, n

    def forward_device(self, x, want_f32=True, want_u8=False, check_range=True):
        """z -> (f32 DeviceArray [N,3,64,64] or None, u8 DeviceArray or None).  With check_range (default) the call synchronises once to make
        sure the split-fp16 path did not clamp any activation"""
        z, n = self._z_device(x)
        shape = (n, 3, 64, 64)
        f32 = self._ctx.empty(shape, np.float32) if want_f32 else None
        u8 = self._ctx.empty(shape, np.uint8) if want_u8 else None
        lib = self._ctx.lib
        check(lib.gl_dcgan_forward(self._handle, _p(z.ptr), n, _p(f32.ptr if f32 else 0), _p(u8.ptr if u8 else 0)))
        if check_range and self._precision == 1 and self._ctx.h3_saturations() > 0:
            # an activation left the fp16 range of the split layout: redo this call with fp32 products; the state stays held
            import warnings
            warnings.warn("split-fp16 generator path saturated for these weights; falling back to fp32 MFMA products")
            self.set_precision(0)
            check(lib.gl_dcgan_forward(self._handle, _p(z.ptr), n, _p(f32.ptr if f32 else 0), _p(u8.ptr if u8 else 0)))
        return f32, u8

    def forward(self, input):
        f32, _ = self.forward_device(input, True, False)
        out = f32.numpy()
        if type(input).__module__.startswith("torch"):
            import torch
            return torch.from_numpy(out).to(input.device)
        return out

    __call__ = forward

    def generate_u8(self, x):
        """8-bit images of the latents (u8 DeviceArray [N,3,64,64]), quantised as the image generate branches do; the same z gives the same
        images in every call"""
        return self.forward_device(x, False, True)[1]

    # ---- gradients with respect to z (csrc/gl_dcgan_grad.hip, csrc/gl_attention_grad.hip), signatures of the DCGAN generator's
    def vjp_z(self, z, cot, want_output=False):
        """grad_z = (dG/dz)^T cot for cot [N,3,64,64] float32 -> DeviceArray [N, z_dim]; with want_output also G(z) of the fp32-product
        forward the gradient belongs to.  Precision and chunk stay as they are."""
        zd, n = self._z_device(z)
        cd = as_device(self._ctx, cot, np.float32)
        if cd.nbytes != n * 3 * 64 * 64 * 4:
            raise ValueError("expected a cotangent of shape [%d,3,64,64], got %s" % (n, cd.shape))
        grad = self._ctx.empty((n, self.z_dim), np.float32)
        out = self._ctx.empty((n, 3, 64, 64), np.float32) if want_output else None
        check(self._ctx.lib.gl_dcgan_vjp_z(self._handle, _p(zd.ptr), n, _p(cd.ptr), _p(grad.ptr), _p(out.ptr if out else 0)))
        return (grad, out) if want_output else grad

    def l2_grad_z(self, z, targets_u8):
        """loss[i] = sum (G(z_i) - x_i)^2, x = 2 u / 255 - 1 of targets_u8 [N,3,64,64] uint8, and grad = d loss / d z:
        -> (grad DeviceArray [N, z_dim], loss DeviceArray [N]), float32"""
        zd, n = self._z_device(z)
        td = as_device(self._ctx, targets_u8, np.uint8)
        if td.nbytes != n * 3 * 64 * 64:
            raise ValueError("expected targets of shape [%d,3,64,64] uint8, got %s" % (n, td.shape))
        grad, loss = self._ctx.empty((n, self.z_dim), np.float32), self._ctx.empty((n,), np.float32)
        check(self._ctx.lib.gl_dcgan_l2_grad_z(self._handle, _p(zd.ptr), _p(td.ptr), n, _p(grad.ptr), _p(loss.ptr)))
        return grad, loss


ENCODER_BN = ("weight", "bias", "running_mean", "running_var")


def encoder_keys(z_dim, d=64):
    """{key: shape} of the reference's Encoder(z_dim, d).state_dict() (train.py:61-85)"""
    ch = [3, d, 2 * d, 4 * d, 8 * d]
    keys = {}
    for l in range(4):
        keys["cv%d.weight" % (l + 1)] = (ch[l + 1], ch[l], 4, 4)
        keys["cv%d.bias" % (l + 1)] = (ch[l + 1],)
        for k in ENCODER_BN:
            keys["bn%d.%s" % (l + 1, k)] = (ch[l + 1],)
        keys["bn%d.num_batches_tracked" % (l + 1)] = ()
    for fc, bn in (("fc1", "bn6"), ("fc2", "bn7")):
        keys[fc + ".weight"] = (4 * z_dim, 512 * 4 * 4)
        keys[fc + ".bias"] = (4 * z_dim,)
        keys[fc + "_1.weight"] = (z_dim, 4 * z_dim)
        keys[fc + "_1.bias"] = (z_dim,)
        for k in ENCODER_BN:
            keys["%s.%s" % (bn, k)] = (4 * z_dim,)
        keys[bn + ".num_batches_tracked"] = ()
    return keys


class Encoder:
    """The reference's Encoder (train.py:61-106) for inference: encode(x) = (z_mu, z_var) of images x [N,3,64,64], BatchNorm in eval mode.
    d must be 64: the reference hard-wires 512 * 4 * 4 inputs to the heads, so no other width loads.  x: uint8 images, or float32 values (the
    reference feeds 2 u / 255 - 1); a byte u is read as float32(2 * (u / 255.) - 1), the library's 8-bit lattice, so both give the same bits on it."""
    image_shape = (3, 64, 64)

    def __init__(self, z_dim, d=64, ctx=None):
        self.z_dim, self.d = int(z_dim), int(d)
        if self.d != 64:
            raise ValueError("Encoder: d must be 64, got %r: the reference hard-wires 512 * 4 * 4 inputs to the encoder's heads "
                             "(gan_models/vaegan/train.py:79,83), so no other width loads" % (d,))
        if not 1 <= self.z_dim <= 4096:
            raise ValueError("Encoder: z_dim must be in 1..4096, got %r" % (z_dim,))
        self._ctx = ctx
        self._handle = None
        self._loaded = False

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = Context.get()
        return self._ctx

    def _ensure(self):
        if self._handle is None:
            h = _p()
            check(self.ctx.lib.gl_vaegan_enc_create(self.ctx.handle, self.z_dim, self.d, ctypes.byref(h)))
            self._handle = h
        return self._handle

    def __del__(self):
        if getattr(self, "_handle", None) is not None:
            try:
                self.ctx.lib.gl_vaegan_enc_destroy(self._handle)
            except Exception:  # noqa: BLE001
                pass

    def load_state_dict(self, sd, strict=True):
        """the reference's keys (encoder_keys); a missing key raises KeyError, a wrong shape ValueError naming the key; with strict, a key the
        reference's Encoder does not have raises KeyError as well.  num_batches_tracked is required and not used (eval mode)."""
        want = encoder_keys(self.z_dim, self.d)
        arrays = {}
        for key, shape in want.items():
            if key not in sd:
                raise KeyError("Encoder.load_state_dict: missing key %r" % key)
            if key.endswith("num_batches_tracked"):
                continue
            a = _np(sd[key])
            if a.shape != shape:
                raise ValueError("Encoder.load_state_dict: %s has shape %s, expected %s" % (key, a.shape, shape))
            arrays[key] = a
        if strict:
            extra = sorted(k for k in sd if k not in want)
            if extra:
                raise KeyError("Encoder.load_state_dict: unexpected key(s) %s" % ", ".join(repr(k) for k in extra))
        lib, h = self.ctx.lib, self._ensure()
        ptr = lambda key: arrays[key].ctypes.data_as(_p)   # noqa: E731
        for l in range(4):
            cv, bn = "cv%d" % (l + 1), "bn%d" % (l + 1)
            check(lib.gl_vaegan_enc_set_conv(h, l, ptr(cv + ".weight"), ptr(cv + ".bias"), *[ptr("%s.%s" % (bn, k)) for k in ENCODER_BN]))
        for i, (fc, bn) in enumerate((("fc1", "bn6"), ("fc2", "bn7"))):
            check(lib.gl_vaegan_enc_set_head(h, i, ptr(fc + ".weight"), ptr(fc + ".bias"), *[ptr("%s.%s" % (bn, k)) for k in ENCODER_BN],
                                             ptr(fc + "_1.weight"), ptr(fc + "_1.bias")))
        self._loaded = True
        return "<All keys matched successfully>"

    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    def cuda(self, *a, **k):
        return self

    def train(self, mode=True):              # inference only: BatchNorm always uses its running statistics
        return self

    def set_chunk(self, images_per_pass):
        """images per pass on the device (0 = the default); results do not depend on it"""
        check(self.ctx.lib.gl_vaegan_enc_set_chunk(self._ensure(), int(images_per_pass)))

    def encode_device(self, x):
        """x [N,3,64,64]: uint8 or float32, numpy / torch / DeviceArray -> (mu, logvar) float32 DeviceArrays [N, z_dim].  Before the weights
        are loaded the library refuses (GL_ERR_STATE) and names the missing part."""
        if not isinstance(x, DeviceArray) and not type(x).__module__.startswith("torch"):
            x = np.asarray(x)
            if x.dtype != np.uint8:
                x = x.astype(np.float32, copy=False)
        xd = as_device(self.ctx, x)
        if xd.dtype not in (np.dtype(np.uint8), np.dtype(np.float32)):
            raise TypeError("Encoder: images must be uint8 or float32, got %s" % xd.dtype)
        if tuple(xd.shape[1:]) != self.image_shape:
            raise ValueError("Encoder: expected images of shape [N,3,64,64], got %s" % (xd.shape,))
        n = xd.shape[0]
        mu, logvar = self.ctx.empty((n, self.z_dim), np.float32), self.ctx.empty((n, self.z_dim), np.float32)
        u8 = xd.dtype == np.dtype(np.uint8)
        check(self.ctx.lib.gl_vaegan_enc_encode(self._ensure(), _p(xd.ptr if u8 else 0), _p(0 if u8 else xd.ptr), n, _p(mu.ptr), _p(logvar.ptr)))
        return mu, logvar

    def encode(self, x):
        """-> (z_mu, z_var) float32 numpy arrays [N, z_dim] (the reference's names: z_var is what reparametrize calls logvar)"""
        mu, logvar = self.encode_device(x)
        return mu.numpy(), logvar.numpy()

    def forward(self, x, seed=0, query_base=0):
        """the reference's forward is reparametrize(encode(x)) = mu + exp(logvar) * eps with eps from torch's RNG stream.  That stream is NOT
        reproduced: eps here is the library's counter-based noise, draw j = 1 of recon_latents(mu, logvar, 1, seed, query_base), clamped to
        [-4, 4] like every latent the attacks draw.  -> float32 [N, z_dim]"""
        from ...recon import recon_latents
        mu, logvar = self.encode(x)
        z = recon_latents(mu, logvar, 1, seed=seed, query_base=query_base, ctx=self.ctx).numpy()
        return np.ascontiguousarray(z.reshape(len(mu), 2, self.z_dim)[:, 1])

    __call__ = forward
