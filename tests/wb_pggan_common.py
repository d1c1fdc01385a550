"""Host restatement of PGGAN's generator for the white-box tests (csrc/gl_pggan_grad.hip, pggan Generator.at): the graph of
gan_models/pggan/model_torch.py at a fixed (steps, alpha), built from a state dict in float64 (the reference) or float32 (its arithmetic class)
and differentiated by autograd; the inputs of every LeakyReLU for the slope-flip precondition; PGGAN's 8-bit code; a host search.
Nothing here imports the product."""
import numpy as np
import torch
import torch.nn.functional as F

from wb_common import adam_step, bias_corrections, ssd


class PgganNet:
    """Generator(z_dim, in_channels, img_channels).forward(z, steps, alpha) from a state dict"""

    def __init__(self, sd, dtype=torch.float64, prefix=""):
        self.dtype = dtype
        self.sd = {k[len(prefix):]: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd.items() if k.startswith(prefix)}

    def _ws(self, name, x, k):
        w = self.sd[name + ".conv.weight"]
        scale = (2.0 / (w.shape[1] * k * k)) ** 0.5                    # WSConv2d scales its input, not the bias
        return F.conv2d(x * scale, w, None, padding=k // 2) + self.sd[name + ".bias"].view(1, -1, 1, 1)

    @staticmethod
    def _pn(x):
        return x / torch.sqrt(torch.mean(x ** 2, dim=1, keepdim=True) + 1e-8)

    def run(self, zt, steps, alpha, taps=None):
        """zt [n, z_dim, 1, 1] -> [n, img_channels, R, R]; the input of every LeakyReLU is appended to `taps`"""
        def leaky(h):
            if taps is not None:
                taps.append(h)
            return F.leaky_relu(h, 0.2)
        x = leaky(F.conv_transpose2d(self._pn(zt), self.sd["initial.1.weight"], self.sd["initial.1.bias"]))
        out = self._pn(leaky(self._ws("initial.3", x, 3)))
        if steps == 0:
            return self._ws("initial_rgb", out, 1)
        for s in range(steps):
            up = F.interpolate(out, scale_factor=2, mode="nearest")
            out = self._pn(leaky(self._ws("prog_blocks.%d.conv1" % s, up, 3)))
            out = self._pn(leaky(self._ws("prog_blocks.%d.conv2" % s, out, 3)))
        a, b = self._ws("rgb_layers.%d" % steps, out, 1), self._ws("rgb_layers.%d" % (steps - 1), up, 1)
        return torch.tanh(alpha * a + (1 - alpha) * b)

    def _z(self, z, grad=False):
        z = np.asarray(z, np.float32)
        return torch.from_numpy(z).to(self.dtype).reshape(len(z), -1, 1, 1).requires_grad_(grad)


def forward(net, z, steps, alpha):
    with torch.no_grad():
        return net.run(net._z(z), steps, alpha).numpy()


def leaky_inputs(net, z, steps, alpha):
    """the input of every LeakyReLU, one array per layer, in the module's dtype"""
    taps = []
    with torch.no_grad():
        net.run(net._z(z), steps, alpha, taps)
    return [t.numpy() for t in taps]


def vjp_z(net, z, cot, steps, alpha):
    """(dG/dz)^T cot by autograd, in the module's dtype -> (grad [n, nz], G(z))"""
    zt = net._z(z, True)
    y = net.run(zt, steps, alpha)
    (g,) = torch.autograd.grad(y, zt, torch.from_numpy(np.asarray(cot, np.float32)).to(net.dtype).reshape(y.shape))
    return g.reshape(len(z), -1).numpy(), y.detach().numpy()


def l2_grad_z(net, z, targets_u8, steps, alpha):
    """loss[i] = sum (G(z_i) - x_i)^2, x = 2 u / 255 - 1, and d loss / d z by autograd, in the module's dtype"""
    zt = net._z(z, True)
    y = net.run(zt, steps, alpha)
    x = torch.from_numpy(np.asarray(targets_u8).reshape(y.shape).astype(np.float64)).to(net.dtype) * (2.0 / 255.0) - 1.0
    loss = ((y - x) ** 2).reshape(len(z), -1).sum(dim=1)
    (g,) = torch.autograd.grad(loss.sum(), zt)
    return g.reshape(len(z), -1).numpy(), loss.detach().numpy()


def quantize_u8(y):
    """PGGAN's generate branch: trunc((y * 0.5 + 0.5) * 255)"""
    return np.clip(np.trunc((np.asarray(y, np.float64) * 0.5 + 0.5) * 255.0), 0, 255).astype(np.uint8)


def flip_margin_ok(net64, net32, z, steps, alpha):
    """the precondition of a GPU gradient case: every LeakyReLU input of the float64 module with |h| < 1e-3 rms(layer) has a float32 value
    within |h| / 8 of it, so that no arithmetic of float32's class flips the unit's slope -> (ok, number of near-zero units)"""
    ok, near = True, 0
    for h64, h32 in zip(leaky_inputs(net64, z, steps, alpha), leaky_inputs(net32, z, steps, alpha)):
        small = np.abs(h64) < 1e-3 * np.sqrt(np.mean(h64 ** 2))
        near += int(small.sum())
        ok = ok and bool((np.abs(h32.astype(np.float64) - h64)[small] <= np.abs(h64)[small] / 8).all())
    return ok, near


# the GPU gradient cases: (weights seed, z_dim, in_channels, steps, n, latent seed, chunk); tests/test_wb_pggan_cpu.py asserts flip_margin_ok
# for every one of them at both alphas
CASES = {
    "steps0": (100, 64, 64, 0, 3, 0, 0),
    "steps1": (100, 64, 64, 1, 3, 0, 0),
    "steps2_chunk2": (100, 64, 64, 2, 5, 0, 2),
    "steps4": (100, 64, 64, 4, 2, 7, 0),
    "wide512": (101, 64, 512, 0, 2, 1, 0),
    # 160 = 128 + 32 channels in every 3 x 3 layer: the data gradients run a full chunk of gpre and then a shorter one (pack_grad_weights' index
    # arithmetic and pg_pn_grad_kernel's chunked output against each other), with 160 columns padded to 192
    "ragged160": (102, 64, 160, 1, 3, 0, 0),
    # block 3 is 384 -> 192 channels at 64 x 64: its data gradients run chunks of 128 + 64 (gpre of conv1 and conv2) against 128 + 128 + 128
    # columns, so the channel chunking (L.C) and the column arithmetic (L.cin) of pack_grad_weights see different numbers.  2.6 M LeakyReLU
    # units: float32 torch flips 8.6 of them per latent on average and about one latent in 5 000 passes flip_margin_ok; seeds 1022 and 3714 do.
    # At 1022 five units lie within 2.2 - 5.6 times their layer's float32 error (rms) of zero, and another float32 arithmetic does flip one: the
    # device the 5.6 one (the row moves by 2.974e-03, exactly what flipping that unit in float64 gives), float32 torch on another host the 2.2 one
    # (5.867e-05).  At 3714 the closest units are 3.8, 5.9 and 6.6 errors away and neither flips
    "ragged384": (102, 64, 384, 4, 1, 3714, 0),
}
ALPHAS = (1.0, 0.4)


def case_latents(name):
    _, nz, _, _, n, seed, _ = CASES[name]
    return np.random.default_rng(seed).standard_normal((n, nz, 1, 1)).astype(np.float32).reshape(n, nz)


def search(queries_u8, net, z_init, steps_pg, alpha, steps, lr, beta1=0.9, beta2=0.999, eps=1e-8, z_max=4.0):
    """the whole attack on the host: float64 autograd gradients, the float32 Adam step, 8-bit images of the host module, exact S and the
    elitist best-so-far -> (z_best float32, S int64, trace int64 [steps + 1, Q])"""
    q = np.asarray(queries_u8).reshape(len(queries_u8), -1)
    z = np.array(z_init, np.float32).reshape(len(q), -1)
    m, v = np.zeros_like(z), np.zeros_like(z)
    z_best = z.copy()
    S = ssd(quantize_u8(forward(net, z, steps_pg, alpha)), q)
    trace = [S.copy()]
    for t in range(1, steps + 1):
        g, _ = l2_grad_z(net, z, q, steps_pg, alpha)
        c1, c2 = bias_corrections(beta1, beta2, t)
        z, m, v = adam_step(z, m, v, g.astype(np.float32), lr, beta1, beta2, eps, c1, c2, z_max)
        S_new = ssd(quantize_u8(forward(net, z, steps_pg, alpha)), q)
        take = S_new < S
        z_best[take] = z[take]
        S = np.where(take, S_new, S)
        trace.append(S.copy())
    return z_best, S, np.stack(trace)
