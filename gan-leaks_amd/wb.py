"""The white-box attack of GAN-Leaks (section 5.4 of the paper): the attacker holds the generator's weights, finds
z* = argmin_z L(x, G(z)) by gradient descent and scores the query x by L(x, G(z*)).  For all queries at once, one step is

    l2_grad_z           d/dz sum (G(z) - x)^2 at the iterate: the generator's own fp32-product forward and its backward pass
                        (csrc/gl_dcgan_grad.hip, csrc/gl_pggan_grad.hip), as device arrays
    gl_wb_adam_step     one Adam update of the iterate, clamped to [-z_max, z_max] (csrc/gl_wb.hip)
    generate_u8         the 8-bit images of the new iterate, with the generator's own precision setting: exactly the images the
                        full-black-box and the partial-black-box attack score
    gl_pbb_group_min    exact S = sum (a - b)^2 of every query against its one image (lambda = 1)
    gl_pbb_accept       into a separate best-so-far (z_best, S_best) where S is strictly smaller; the Adam iterate itself goes on

Step 0 scores the starting point, so the score of a query never rises, S == SSD(generate_u8(z_star), query) exactly, and started from the
nearest bank latent (pbb_init_from_bank) the attack can only lower the full-black-box answer.  The scoring forward per step is what makes
the three attacks report the same quantity.  Every query's trajectory depends on that query alone, so results do not depend on block_images.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import DeviceArray, check
from .attack import _dist32, prepare_images

_p = ctypes.c_void_p
_f = ctypes.c_float

GL_PBB_PARTIAL_BYTES = 16    # include/ganleaks.h


def _check_arguments(generator, z_init, steps, lr, beta1, beta2, eps, z_max, block_images, distance):
    """everything that can be refused without a GPU; -> z_init float32 [Q, nz]"""
    if distance == "l2-lpips":
        raise NotImplementedError("wb_attack is built for distance='l2'; 0.2 * LPIPS + L2 needs the backward pass of the VGG16 features and is "
                                  "not built")
    if distance != "l2":
        raise ValueError("distance must be 'l2', got %r" % (distance,))
    if getattr(generator, "power_iterations", None) is not None:
        raise NotImplementedError("VAEGAN's generator (spectral normalisation advanced by every forward, self-attention) has no backward pass")
    if not hasattr(generator, "l2_grad_z") or not hasattr(generator, "generate_u8"):
        raise NotImplementedError("%s.%s has no l2_grad_z: the backward pass is built for the DCGAN / WGAN-GP generator and for PGGAN at a "
                                  "fixed depth -- hand over pggan's Generator.at(steps, alpha)" % (type(generator).__module__, type(generator).__name__))
    if int(steps) != steps or steps < 0:
        raise ValueError("steps must be an integer >= 0, got %r" % (steps,))
    for name, v in (("lr", lr), ("eps", eps), ("z_max", z_max)):
        if not (np.isfinite(v) and v > 0):
            raise ValueError("%s must be finite and positive, got %r" % (name, v))
    for name, v in (("beta1", beta1), ("beta2", beta2)):
        if not (np.isfinite(v) and 0 <= v < 1):
            raise ValueError("%s must lie in [0, 1), got %r" % (name, v))
    if int(block_images) < 1:
        raise ValueError("block_images must be at least 1, got %r" % (block_images,))
    if type(z_init).__module__.startswith("torch"):
        z_init = z_init.detach().cpu().numpy()
    z = np.asarray(z_init, np.float32)
    if z.ndim == 4 and z.shape[2:] == (1, 1):
        z = z.reshape(z.shape[0], z.shape[1])
    if z.ndim != 2 or z.shape[1] < 1:
        raise ValueError("z_init must be [Q, nz] or [Q, nz, 1, 1], got shape %r" % (z.shape,))
    return np.ascontiguousarray(z)


def wb_attack(queries, generator, z_init, steps=64, lr=0.05, beta1=0.9, beta2=0.999, eps=1e-8, z_max=4.0, block_images=4096, history=False,
              distance="l2"):
    """gradient descent on the latent for every query.

    queries   : [Q,C,H,W] 8-bit images (u8, or floats on the lattice 2*(u/255.)-1); numpy / torch / DeviceArray; [Q,3,64,64] for DCGAN
    generator : the DCGAN / WGAN-GP Generator, or PGGAN's Generator.at(steps, alpha) (l2_grad_z and generate_u8); where it has an
                `image_shape`, queries of another shape are refused
    z_init    : [Q, nz] or [Q, nz, 1, 1] starting latents (pbb_init_from_bank gives the nearest bank latents)
    steps, lr, beta1, beta2, eps: Adam on sum (G(z) - x)^2, float32; z_max: the iterate is clamped to [-z_max, z_max]
    block_images: queries go in blocks of that many; each block runs all its steps on the device
    returns (dist float32 [Q] -- the float32 attack() reports for the same S --, z_star float32 [Q, nz], S int64 [Q]), and with
    history=True also trace int64 [steps + 1, Q]: the best S after every step, trace[0] the starting point's."""
    z_host = _check_arguments(generator, z_init, steps, lr, beta1, beta2, eps, z_max, block_images, distance)
    steps = int(steps)
    Q, nz = z_host.shape
    if len(queries) != Q:
        raise ValueError("%d queries but %d starting latents" % (len(queries), Q))
    image_shape = tuple(int(v) for v in (queries.shape if hasattr(queries, "shape") else np.shape(queries))[1:])
    want_shape = getattr(generator, "image_shape", None)
    if want_shape is not None and image_shape != tuple(want_shape):
        raise ValueError("the queries are images of shape %r, the generator makes %r" % (image_shape, tuple(want_shape)))
    ctx = generator.ctx
    lib = ctx.lib
    qu8 = prepare_images(ctx, queries)                   # raises ValueError off the 8-bit lattice
    d = qu8.shape[1]
    z_star = np.empty((Q, nz), np.float32)
    S_out = np.empty((Q,), np.int64)
    trace = np.empty((steps + 1, Q), np.int64) if history else None
    per_block = int(block_images)

    def images(z_dev, n):
        u8 = generator.generate_u8(z_dev)
        if not isinstance(u8, DeviceArray) or u8.dtype != np.uint8 or u8.nbytes != n * d:
            raise ValueError("generate_u8 gave %s for %d latents; the queries hold %d values each" % (getattr(u8, "shape", None), n, d))
        return u8

    for lo in range(0, Q, per_block):
        nb = min(per_block, Q - lo)
        q_dev = qu8.view((nb, d), offset_bytes=lo * d)
        z, z_best = ctx.to_device(z_host[lo:lo + nb]), ctx.to_device(z_host[lo:lo + nb])
        m, v = ctx.zeros((nb, nz), np.float32), ctx.zeros((nb, nz), np.float32)
        one = ctx.to_device(np.ones((nb,), np.float32))                    # gl_pbb_accept's step width: not used here, stays 1
        S_best, S_new = ctx.empty((nb,), np.uint64), ctx.empty((nb,), np.uint64)
        j_new, accepted = ctx.empty((nb,), np.int32), ctx.empty((nb,), np.uint8)
        work = ctx.empty((GL_PBB_PARTIAL_BYTES * nb,), np.uint8)
        # step 0: the starting point itself, straight into S_best
        u8 = images(z, nb)
        check(lib.gl_pbb_group_min(ctx.handle, _p(q_dev.ptr), _p(u8.ptr), nb, 1, d, _p(S_best.ptr), _p(j_new.ptr), _p(work.ptr)))
        if history:
            trace[0, lo:lo + nb] = S_best.numpy().astype(np.int64)
        for t in range(1, steps + 1):
            grad, _ = generator.l2_grad_z(z, q_dev.view((nb,) + image_shape))
            c1, c2 = 1.0 / (1.0 - float(beta1) ** t), 1.0 / (1.0 - float(beta2) ** t)
            check(lib.gl_wb_adam_step(ctx.handle, _p(z.ptr), _p(m.ptr), _p(v.ptr), _p(grad.ptr), nb, nz, _f(lr), _f(beta1), _f(beta2), _f(eps), _f(c1),
                                      _f(c2), _f(z_max)))
            u8 = images(z, nb)
            check(lib.gl_pbb_group_min(ctx.handle, _p(q_dev.ptr), _p(u8.ptr), nb, 1, d, _p(S_new.ptr), _p(j_new.ptr), _p(work.ptr)))
            check(lib.gl_pbb_accept(ctx.handle, _p(z_best.ptr), _p(one.ptr), _p(S_best.ptr), _p(z.ptr), _p(S_new.ptr), _p(j_new.ptr), nb, nz, 1,
                                    _f(1.0), _f(1.0), _f(1.0), _f(1.0), _p(accepted.ptr)))
            if history:
                trace[t, lo:lo + nb] = S_best.numpy().astype(np.int64)
        z_star[lo:lo + nb] = z_best.numpy()
        S_out[lo:lo + nb] = S_best.numpy().astype(np.int64)
        del u8
    dist = _dist32(S_out, d, "u8")
    return (dist, z_star, S_out, trace) if history else (dist, z_star, S_out)
