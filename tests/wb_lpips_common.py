"""Host restatement for the white-box tests under 0.2 * LPIPS + L2 (csrc/gl_lpips_grad.hip, ganleaks_amd/wb.py pair_grad_z / pair_wb_attack):
the loss of Loss('l2-lpips') (attack_models/utils.py:166-176, networks_basic.py:134-181) as a torch graph over VGG16 built from a state dict,
in float64 (the reference) or float32 (its arithmetic class), differentiated by autograd; the preconditions of the GPU cases; the composed
graphs generator -> VGG16; a host search.  Nothing here imports the product."""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

import wb_common as wc
import wb_pggan_common as wp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, path):
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, path)
        sys.modules[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[name])
    return sys.modules[name]


lo = _load("gl_lpips_oracle", os.path.join(ROOT, "oracle", "lpips_oracle.py"))      # the cfg, the constants and normalize_tensor

GOLDEN = os.path.join(ROOT, "tests", "golden")


def lin_weights():
    z = np.load(os.path.join(GOLDEN, "lpips_lin_v0.1.npz"))
    return {"lin%d" % i: z["lin%d" % i] for i in range(5)}


class LpipsNet:
    """PNetLin (v0.1, net-lin, vgg, eval) + the L2 term from a VGG16 `features` state dict and the five lin weight vectors"""

    def __init__(self, sd, lin, dtype=torch.float64):
        self.dtype = dtype
        self.w = [torch.from_numpy(np.asarray(sd["%d.weight" % k])).to(dtype) for k in lo.VGG_KEYS]
        self.b = [torch.from_numpy(np.asarray(sd["%d.bias" % k])).to(dtype) for k in lo.VGG_KEYS]
        self.lin = [torch.from_numpy(np.asarray(lin["lin%d" % i], np.float64).reshape(-1)).to(dtype).view(1, -1, 1, 1) for i in range(5)]
        self.shift = torch.from_numpy(lo.SHIFT.astype(np.float64)).to(dtype).view(1, 3, 1, 1)
        self.scale = torch.from_numpy(lo.SCALE.astype(np.float64)).to(dtype).view(1, 3, 1, 1)

    def taps(self, img, pre=None, pooled=None):
        """img [n,3,H,W] in [-1,1] -> the five tapped activations; the input of every ReLU is appended to `pre`, the input of every max-pool
        to `pooled`"""
        h = (img - self.shift) / self.scale
        out, ci = [], 0
        for v in lo.VGG_CFG:
            if v == "M":
                if pooled is not None:
                    pooled.append(h)
                h = F.max_pool2d(h, 2, 2)
                continue
            h = F.conv2d(h, self.w[ci], self.b[ci], padding=1)
            if pre is not None:
                pre.append(h)
            h = F.relu(h)
            if ci in lo.TAP_AFTER_CONV:
                out.append(h)
            ci += 1
        return out

    def target(self, targets_u8):
        return torch.from_numpy(np.asarray(targets_u8).astype(np.float64)).to(self.dtype) * (2.0 / 255.0) - 1.0

    def loss(self, y, x):
        """[n]: 0.2 * LPIPS(y, x) + mean (y - x)^2"""
        ty, tx = self.taps(y), self.taps(x)
        lp = 0
        for l in range(5):
            d = (lo.normalize_tensor(ty[l]) - lo.normalize_tensor(tx[l])) ** 2
            lp = lp + (d * self.lin[l]).sum(dim=1).mean(dim=(1, 2))
        return 0.2 * lp + ((y - x) ** 2).reshape(len(y), -1).mean(dim=1)


def grad_image(net, y, targets_u8):
    """(d loss / d y [n,3,H,W], loss [n]) by autograd, in the module's dtype"""
    yt = torch.from_numpy(np.asarray(y, np.float32)).to(net.dtype).requires_grad_(True)
    loss = net.loss(yt, net.target(targets_u8))
    (g,) = torch.autograd.grad(loss.sum(), yt)
    return g.numpy(), loss.detach().numpy()


def distance64(net64, a_u8, b_u8):
    """[n]: the float64 distance between 8-bit images, row by row"""
    with torch.no_grad():
        return net64.loss(net64.target(a_u8), net64.target(b_u8)).numpy()


def preconditions(net64, net32, y):
    """what a GPU gradient case needs of its input y [n,3,H,W]: -> (flip_ok, near, zero_positions, tied_cells)
    flip_ok        wb_pggan_common.flip_margin_ok's rule at every ReLU input: units of the float64 module with |h| < 1e-3 rms(layer) have
                   their float32 value within |h| / 8, so no arithmetic of float32's class moves a unit across zero
    zero_positions tap positions whose channels are all zero (torch's gradient is NaN there; the device takes the projection term as 0)
    tied_cells     2 x 2 max-pool cells whose positive maximum is attained more than once, in either dtype (the first maximum takes the
                   gradient: a tie that one arithmetic has and another has not moves it to another position)
    Ties and all-zero positions are kept out of the end-to-end cases because float32 and float64 may disagree about them there -- a tie or a
    zero that one arithmetic has and the other has not changes the gradient by far more than rounding does -- not because the device's rules
    for them go unchecked: the tie rule (all 81 patterns of a cell), the all-zero tap position and the ReLU mask at exactly zero are pinned
    kernel by kernel in tests/test_gpu_grad_kernels.py, and tests/test_grad_kernels_cpu.py shows them to be torch's rules."""
    ok, near, zero, tied = True, 0, 0, 0
    y = np.asarray(y, np.float32)
    runs = []
    for net in (net64, net32):
        pre, pooled = [], []
        with torch.no_grad():
            taps = net.taps(torch.from_numpy(y).to(net.dtype), pre, pooled)
        runs.append([t.numpy() for t in pre])
        zero += sum(int(((t ** 2).sum(dim=1) == 0).sum()) for t in taps)
        for p in pooled:
            n, c, h, w = p.shape
            cells = p.reshape(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)
            mx = cells.max(dim=-1, keepdim=True).values
            tied += int((((cells == mx).sum(dim=-1) > 1) & (mx[..., 0] > 0)).sum())
    for h64, h32 in zip(*runs):
        small = np.abs(h64) < 1e-3 * np.sqrt(np.mean(h64 ** 2))
        near += int(small.sum())
        ok = ok and bool((np.abs(h32.astype(np.float64) - h64)[small] <= np.abs(h64)[small] / 8).all())
    return ok, near, zero, tied


# the GPU cases of grad_image: name -> (n, H, W).  16 x 16 is the smallest size the path takes (taps 16, 8, 4, 2 and 1 wide) and still has the
# 512-channel layers whose data gradient takes four launches; 32 x 16 is not square; 64 x 64 is the attacks' size.  The last entry seeds the
# noise: float32 torch itself moves a ReLU unit across zero on some seeds (at 64 x 64 on seven of the eight from 11 to 18), so each case has
# one at which tests/test_wb_lpips_cpu.py finds the preconditions to hold
IMAGE_CASES = {"16x16": (3, 16, 16, 11), "32x16": (2, 32, 16, 11), "64x64": (2, 64, 64, 14)}


def image_case(synth, name):
    """(targets_u8 [n,3,H,W], y float32 [n,3,H,W]): low-pass targets and y = clip(x + 0.1 N(0, 1))"""
    n, H, W, seed = IMAGE_CASES[name]
    targets = np.ascontiguousarray(synth.lowpass_u8_images(5, n, res=max(H, W))[:, :, :H, :W])
    x = (2.0 * (targets.astype(np.float64) / 255.0) - 1.0).astype(np.float32)
    y = np.clip(x + np.float32(0.1) * np.random.default_rng(seed).standard_normal(x.shape).astype(np.float32), -1.0, 1.0).astype(np.float32)
    return targets, y


def vgg_nets(synth):
    sd, lin = synth.vgg16_state_dict(7), lin_weights()
    return LpipsNet(sd, lin), LpipsNet(sd, lin, torch.float32)


# ---- generator -> VGG16
class Composed:
    """z -> G(z) -> loss against 8-bit targets, for the DCGAN module of wb_common or the PgganNet of wb_pggan_common at (steps, alpha)"""

    def __init__(self, gen, vgg, steps=None, alpha=None):
        self.gen, self.vgg, self.steps, self.alpha = gen, vgg, steps, alpha
        self.dtype = vgg.dtype

    def image(self, zt):
        return self.gen(zt) if self.steps is None else self.gen.run(zt, self.steps, self.alpha)

    def forward(self, z):
        with torch.no_grad():
            return self.image(self._z(z)).numpy()

    def quantize(self, y):
        return wc.quantize_u8(y) if self.steps is None else wp.quantize_u8(y)

    def _z(self, z, grad=False):
        z = np.asarray(z, np.float32)
        return torch.from_numpy(z).to(self.dtype).reshape(len(z), -1, 1, 1).requires_grad_(grad)

    def grad_z(self, z, targets_u8):
        """(d loss / d z [n, nz], loss [n]) by autograd through both networks"""
        zt = self._z(z, True)
        loss = self.vgg.loss(self.image(zt), self.vgg.target(targets_u8))
        (g,) = torch.autograd.grad(loss.sum(), zt)
        return g.reshape(len(z), -1).numpy(), loss.detach().numpy()


# the GPU cases of pair_grad_z: name -> (n, seed of the latents: as above, one at which the preconditions hold); composed_case gives the inputs
COMPOSED_CASES = {"dcgan16": (2, 35), "pggan_a1.0": (3, 37), "pggan_a0.4": (3, 37)}
PGGAN_SD = (100, 64, 64)          # synth.pggan_state_dict(seed, z_dim, in_channels): 16 x 16 images at steps = 2
DCGAN_SD = dict(seed=1234, features_g=16)


def composed_nets(synth, name):
    """(float64, float32) Composed of a case"""
    out = []
    for dtype in (torch.float64, torch.float32):
        vgg = LpipsNet(synth.vgg16_state_dict(7), lin_weights(), dtype)
        if name == "dcgan16":
            out.append(Composed(wc.dcgan_module(synth.dcgan_state_dict(DCGAN_SD["seed"], features_g=DCGAN_SD["features_g"]), dtype), vgg))
        else:
            out.append(Composed(wp.PgganNet(synth.pggan_state_dict(*PGGAN_SD), dtype), vgg, 2, float(name.split("_a")[1])))
    return out


def composed_case(net64, name):
    """(z [n, nz], targets_u8): the targets are the 8-bit images of latents 0.3 away from z, so that the loss is that of a descent under way"""
    n, seed = COMPOSED_CASES[name]
    nz = 100 if name == "dcgan16" else PGGAN_SD[1]
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, nz)).astype(np.float32)
    other = z + np.float32(0.3) * rng.standard_normal((n, nz)).astype(np.float32)
    return z, net64.quantize(net64.forward(other))


# ---- the search test: pggan at (2, 1.0), the latents of wb_common.search_latents
SEARCH_PG_STEPS, SEARCH_ALPHA, SEARCH_NZ = 2, 1.0, 64
SEARCH_STEPS, SEARCH_LR = 16, 0.05


def search(queries_u8, net64, z_init, steps, lr, beta1=0.9, beta2=0.999, eps=1e-8, z_max=4.0):
    """the whole attack on the host: float64 autograd gradients, the float32 Adam step, 8-bit images of the host module, the float64 distance
    and the elitist best-so-far -> (z_best float32, dist float64 [Q], trace float64 [steps + 1, Q])"""
    z = np.array(z_init, np.float32).reshape(len(queries_u8), -1)
    m, v = np.zeros_like(z), np.zeros_like(z)
    z_best = z.copy()
    score = lambda zz: distance64(net64.vgg, queries_u8, net64.quantize(net64.forward(zz)))      # noqa: E731
    S = score(z)
    trace = [S.copy()]
    for t in range(1, steps + 1):
        g, _ = net64.grad_z(z, queries_u8)
        c1, c2 = wc.bias_corrections(beta1, beta2, t)
        z, m, v = wc.adam_step(z, m, v, g.astype(np.float32), lr, beta1, beta2, eps, c1, c2, z_max)
        S_new = score(z)
        take = S_new < S
        z_best[take] = z[take]
        S = np.where(take, S_new, S)
        trace.append(S.copy())
    return z_best, S, np.stack(trace)
