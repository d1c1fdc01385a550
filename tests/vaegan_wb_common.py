"""Host restatement of the VAEGAN generator with its spectral-norm state held (gan_models/vaegan/train.py Generator.frozen(k)), for the tests of the
white-box and partial-black-box attacks on it: the graph in torch, differentiated by autograd (float64 is the reference, float32 its arithmetic
class), in the manner of wb_common.dcgan_module.  Nothing here imports the product.

    4 x [ConvTranspose2d(w_bar / sigma) + bias -> BatchNorm2d (eval) -> ReLU], self-attention after the third, ConvTranspose2d + bias -> tanh
    sigma: u, v advanced k times from the state dict (v = normalise(W^T u), u = normalise(W v), W = w_bar.view(C_in, -1)), sigma = u . W v, then constant
"""
import numpy as np
import torch
import torch.nn.functional as F

import wb_common as wc

GAMMA = 0.7                       # synth.vaegan_state_dict's
# (d, z_dim): attention width 2 d = 64 / 128 -- the two instances of the attention kernels; d = 32 is features_g 16 with z_pad 128 > z_dim
SMALL, WIDE = (32, 100), (64, 64)

# the attack test's inputs (tests/test_vaegan_wb_cpu.py asserts that descent works at them on the host, tests/test_gpu_wb_vaegan.py runs the device
# there): a bank of ATTACK_BANK latents, query q the 8-bit image of bank latent ATTACK_PICK[q] moved by ATTACK_DELTA * (a standard-normal direction)
ATTACK_Q, ATTACK_BANK, ATTACK_DELTA, ATTACK_STEPS, ATTACK_LR = 8, 64, 0.25, 8, 0.05
ATTACK_PICK = (3, 60, 17, 42, 8, 29, 51, 36)


def attack_latents(nz=100):
    """(z_bank [64, nz], z_query [8, nz]): the bank's latents and the latents whose images are the queries"""
    rng = np.random.default_rng(20251)
    z_bank = rng.standard_normal((ATTACK_BANK, nz)).astype(np.float32)
    step = rng.standard_normal((ATTACK_Q, nz)).astype(np.float32)
    return z_bank, z_bank[list(ATTACK_PICK)] + np.float32(ATTACK_DELTA) * step


class HeldVaegan:
    """G of the state dict `sd` at the spectral-norm state of its `forwards`-th forward, in `dtype`; call it with a tensor [n, nz, 1, 1]"""

    def __init__(self, sd, forwards, dtype=torch.float64):
        self.dtype = dtype
        t = lambda key: torch.from_numpy(np.asarray(sd[key])).to(dtype)            # noqa: E731
        self.w, self.b, self.bn, self.state = [], [], [], {}
        for l in range(1, 5):
            name = "deconv%d" % l
            w_bar, u = t(name + ".module.weight_bar"), t(name + ".module.weight_u")
            W = w_bar.reshape(w_bar.shape[0], -1)
            for _ in range(int(forwards)):
                v = W.t().mv(u)
                v = v / (v.norm() + 1e-12)
                u = W.mv(v)
                u = u / (u.norm() + 1e-12)
            sigma = u.dot(W.mv(v))
            self.state[name + ".module.weight_u"], self.state[name + ".module.weight_v"] = u.numpy(), v.numpy()
            self.w.append(w_bar / sigma)
            self.b.append(t(name + ".module.bias"))
            self.bn.append(tuple(t("%s_bn.%s" % (name, k)) for k in ("running_mean", "running_var", "weight", "bias")))
        self.w5, self.b5 = t("deconv5.weight"), t("deconv5.bias")
        self.att = {n: (t("sa1.%s_conv.weight" % n), t("sa1.%s_conv.bias" % n)) for n in ("query", "key", "value")}
        self.gamma = t("sa1.gamma")

    def attention(self, x):
        n, c, h, w = x.shape
        q, k, v = (F.conv2d(x, *self.att[name]).reshape(n, -1, h * w) for name in ("query", "key", "value"))
        p = torch.softmax(torch.bmm(q.transpose(1, 2), k), dim=-1)                   # [n][i][j]
        return self.gamma * torch.bmm(v, p.transpose(1, 2)).reshape(n, c, h, w) + x

    def __call__(self, z, pre=None):
        """pre: a list that receives the input of every ReLU"""
        x = z
        for l in range(4):
            x = F.conv_transpose2d(x, self.w[l], self.b[l], 1 if l == 0 else 2, 0 if l == 0 else 1)
            x = F.batch_norm(x, *self.bn[l], False, 0.0, 1e-5)
            if pre is not None:
                pre.append(x)
            x = F.relu(x)
            if l == 2:
                x = self.attention(x)
        return torch.tanh(F.conv_transpose2d(x, self.w5, self.b5, 2, 1))


# the gradient cases of tests/test_gpu_wb_vaegan.py: (model, n, chunk) -> seed of the latents.  A ReLU unit whose input is within rounding of zero
# takes its gradient mask from the arithmetic: one such unit of the last hidden layer is 1 % of a gradient row (seed 605, row 1: input
# -4.7e-8 of an rms of 1.1, the unit's share of the row 1.17e-2 -- float64 masks it, another float32 order does not).  So each case has a
# seed at which flip_margin_ok holds; tests/test_vaegan_wb_cpu.py asserts that, the GPU test draws its inputs with gradient_inputs
GRADIENT_CASES = {("small", 1, 0): 601, ("small", 3, 0): 603, ("small", 5, 2): 608, ("wide", 1, 0): 611, ("wide", 3, 0): 616, ("wide", 5, 2): 615}


def gradient_references(which, net64, net32, nz):
    """The host side of every gradient case of one generator, computed once: {(n, chunk): dict(z, cot, targets, g64, ref_vjp, lg64, l64, ref_grad,
    ref_loss)} and the loss yardstick.  ref_* are the errors of float32 autograd against float64, per row.  The gradient rows are gated case by
    case, as in tests/test_gpu_wb.py.  The loss of an image is ONE float32 number, and a single float32 evaluation lands within a fraction of an ulp
    of the float64 value often enough that the maximum over the one to five rows of a case is no yardstick (5.8e-8, half an ulp, at n = 1); so the
    loss yardstick is the maximum of the same float32 error over ALL nine rows of the generator's three cases -- reference side only."""
    out = {}
    for (m, n, chunk), seed in GRADIENT_CASES.items():
        if m != which:
            continue
        z, cot, targets = gradient_inputs(net64, nz, n, seed)
        g64, _ = vjp_z(net64, z, cot)
        g32, _ = vjp_z(net32, z, cot)
        lg64, l64 = l2_grad_z(net64, z, targets)
        lg32, l32 = l2_grad_z(net32, z, targets)
        out[(n, chunk)] = dict(z=z, cot=cot, targets=targets, g64=g64, ref_vjp=wc.row_errors(g32, g64), lg64=lg64, l64=l64,
                               ref_grad=wc.row_errors(lg32, lg64), ref_loss=np.abs(l32.astype(np.float64) - l64) / l64)
    return out, max(float(c["ref_loss"].max()) for c in out.values())


def gradient_inputs(net64, nz, n, seed):
    """(z [n, nz], cot [n, 3, 64, 64], targets_u8: the 8-bit images of latents 0.2 away from z)"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, nz)).astype(np.float32)
    cot = rng.standard_normal((n, 3, 64, 64)).astype(np.float32)
    targets = wc.quantize_u8(forward(net64, z + np.float32(0.2) * rng.standard_normal((n, nz)).astype(np.float32)))
    return z, cot, targets


def flip_margin_ok(net64, net32, z):
    """wb_lpips_common.preconditions' rule at every ReLU input: units of the float64 module with |h| < 1e-3 rms(layer) have their float32 value
    within |h| / 8, so no arithmetic of float32's class moves a unit across zero -> (ok, number of such units, smallest |h| / rms)"""
    runs = []
    for net in (net64, net32):
        pre = []
        with torch.no_grad():
            net(_z(net, z), pre)
        runs.append([t.numpy().astype(np.float64) for t in pre])
    ok, near, smallest = True, 0, np.inf
    for h64, h32 in zip(*runs):
        rms = np.sqrt(np.mean(h64 ** 2))
        small = np.abs(h64) < 1e-3 * rms
        near += int(small.sum())
        smallest = min(smallest, float(np.abs(h64).min() / rms))
        ok = ok and bool((np.abs(h32 - h64)[small] <= np.abs(h64)[small] / 8).all())
    return ok, near, smallest


def _z(net, z):
    z = np.asarray(z, np.float32)
    return torch.from_numpy(z).to(net.dtype).reshape(len(z), -1, 1, 1)


def forward(net, z):
    with torch.no_grad():
        return net(_z(net, z)).numpy()


def vjp_z(net, z, cot):
    """(dG/dz)^T cot by autograd, in the module's dtype -> (grad [n, nz], G(z))"""
    zt = _z(net, z).requires_grad_(True)
    y = net(zt)
    (g,) = torch.autograd.grad(y, zt, torch.from_numpy(np.asarray(cot, np.float32)).to(net.dtype))
    return g.reshape(len(z), -1).numpy(), y.detach().numpy()


def l2_grad_z(net, z, targets_u8):
    """loss[i] = sum (G(z_i) - x_i)^2, x = 2 u / 255 - 1, and d loss / d z by autograd, in the module's dtype"""
    zt = _z(net, z).requires_grad_(True)
    x = torch.from_numpy(np.asarray(targets_u8).reshape(len(z), 3, 64, 64).astype(np.float64)).to(net.dtype) * (2.0 / 255.0) - 1.0
    loss = ((net(zt) - x) ** 2).reshape(len(z), -1).sum(dim=1)
    (g,) = torch.autograd.grad(loss.sum(), zt)
    return g.reshape(len(z), -1).numpy(), loss.detach().numpy()


def search(queries_u8, net, z_init, steps, lr, beta1=0.9, beta2=0.999, eps=1e-8, z_max=4.0):
    """wb_common.search with this module's gradient and images, in the module's dtype -> (z_best float32, S int64, trace int64 [steps + 1, Q])"""
    q = np.asarray(queries_u8).reshape(len(queries_u8), -1)
    z = np.array(z_init, np.float32).reshape(len(q), -1)
    m, v = np.zeros_like(z), np.zeros_like(z)
    z_best = z.copy()
    S = wc.ssd(wc.quantize_u8(forward(net, z)), q)
    trace = [S.copy()]
    for t in range(1, steps + 1):
        g, _ = l2_grad_z(net, z, q)
        c1, c2 = wc.bias_corrections(beta1, beta2, t)
        z, m, v = wc.adam_step(z, m, v, g.astype(np.float32), lr, beta1, beta2, eps, c1, c2, z_max)
        S_new = wc.ssd(wc.quantize_u8(forward(net, z)), q)
        take = S_new < S
        z_best[take] = z[take]
        S = np.where(take, S_new, S)
        trace.append(S.copy())
    return z_best, S, np.stack(trace)
