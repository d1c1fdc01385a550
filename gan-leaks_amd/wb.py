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

optimizer="lbfgs" is the paper's optimiser with a parallel line search (csrc/gl_wb_lbfgs.hip).  A step, again for all queries at once:

    l2_grad_z               as above
    gl_wb_lbfgs_push        the pair (z - z_prev, g - g_prev) of a query that moved goes into its ring of `memory` pairs iff s.y > 0
    gl_wb_lbfgs_direction   p = -H g by the two-loop recursion; -g with an empty ring or where -H g is no descent direction
    gl_wb_lbfgs_candidates  the ladder z + (t 2^-j) p, j < `ladder`, clamped; t = 1 for a quasi-Newton step, step0 / |g| at first for -g
    generate_u8             on all nb * ladder candidates, and gl_pbb_group_min with lambda = ladder: every query's best rung
    gl_pbb_accept           the winner replaces the iterate where it is strictly closer: the iterate is itself the best so far
    gl_wb_lbfgs_advance     a rejected quasi-Newton step drops the ring; steepest descent carries its width up or down the ladder

The same driver (_lbfgs_block) runs both distances; what differs is the gradient and the scoring of a block of candidates.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import DeviceArray, check
from .attack import _dist32, prepare_images, refuse_pair_for_tables

_p = ctypes.c_void_p
_f = ctypes.c_float

GL_PBB_PARTIAL_BYTES = 16    # include/ganleaks.h
GL_WB_LBFGS_MAX_M = 16
GL_WB_LBFGS_MAX_LADDER = 32


def _check_arguments(generator, z_init, steps, lr, beta1, beta2, eps, z_max, block_images, distance, gradient="l2_grad_z"):
    """everything that can be refused without a GPU; -> z_init float32 [Q, nz].  gradient: the method the caller needs of the generator"""
    if gradient == "l2_grad_z":
        if distance == "l2-lpips":
            raise NotImplementedError("wb_attack is built for distance='l2'; 0.2 * LPIPS + L2 needs the backward pass of the VGG16 features and is "
                                      "not built into wb_attack: pair_wb_attack runs the descent under that distance")
        if distance != "l2":
            raise ValueError("distance must be 'l2', got %r" % (distance,))
    else:
        if distance == "l2":
            raise ValueError("pair_wb_attack is built for distance='l2-lpips'; wb_attack runs the descent on exact 'l2'")
        if distance != "l2-lpips":
            raise ValueError("distance must be 'l2-lpips', got %r" % (distance,))
    if getattr(generator, "power_iterations", None) is not None:
        raise NotImplementedError("VAEGAN's generator (spectral normalisation advanced by every forward, self-attention) has no backward pass "
                                  "while its state moves: hand over Generator.frozen(k), the same generator with that state held")
    if not hasattr(generator, gradient) or not hasattr(generator, "generate_u8"):
        raise NotImplementedError("%s.%s has no %s: the backward pass is built for the DCGAN / WGAN-GP generator and for PGGAN at a "
                                  "fixed depth -- hand over pggan's Generator.at(steps, alpha)"
                                  % (type(generator).__module__, type(generator).__name__, gradient))
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


def _check_optimizer(optimizer, memory, ladder, step0):
    """the optimiser's keywords, refused without a GPU; -> (memory, ladder) as ints"""
    if optimizer not in ("adam", "lbfgs"):
        raise ValueError("optimizer must be 'adam' or 'lbfgs', got %r" % (optimizer,))
    for name, v, hi in (("memory", memory, GL_WB_LBFGS_MAX_M), ("ladder", ladder, GL_WB_LBFGS_MAX_LADDER)):
        if isinstance(v, bool) or int(v) != v or not 1 <= v <= hi:
            raise ValueError("%s must be an integer in 1..%d, got %r" % (name, hi, v))
    if not (np.isfinite(step0) and step0 > 0):
        raise ValueError("step0 must be finite and positive, got %r" % (step0,))
    return int(memory), int(ladder)


def _lbfgs_block(ctx, z0, steps, memory, ladder, step0, z_max, gradient, score, record):
    """L-BFGS with a ladder line search for one block of queries, on the device (csrc/gl_wb_lbfgs.hip, include/ganleaks.h).

    z0 [nb, nz] float32 on the host; gradient(z_dev) -> the gradient at z, a DeviceArray [nb, nz]; score(latents_dev, lam, S_dev, j_dev)
    writes every query's smallest key over its own lam consecutive latents and the rung that attains it, in the form gl_pbb_accept compares;
    record(step, S_cur_dev) is called after the start (step 0) and after every step.  -> (z, S_cur) DeviceArrays"""
    lib = ctx.lib
    nb, nz = z0.shape
    z = ctx.to_device(z0)
    S_cur, S_new = ctx.empty((nb,), np.uint64), ctx.empty((nb,), np.uint64)
    j_new, accepted = ctx.zeros((nb,), np.int32), ctx.zeros((nb,), np.uint8)
    score(z, 1, S_cur, j_new)                                             # step 0: the starting point itself, straight into S_cur
    record(0, S_cur)
    if not steps:
        return z, S_cur
    z_prev, g_prev = ctx.zeros((nb, nz), np.float32), ctx.zeros((nb, nz), np.float32)
    S_hist, Y_hist = ctx.zeros((nb, memory, nz), np.float32), ctx.zeros((nb, memory, nz), np.float32)
    count, head, flag = ctx.zeros((nb,), np.int32), ctx.zeros((nb,), np.int32), ctx.zeros((nb,), np.uint8)
    t = ctx.to_device(np.ones((nb,), np.float32))
    one = ctx.to_device(np.ones((nb,), np.float32))                       # gl_pbb_accept's step width: not used here, stays 1
    p, cand = ctx.empty((nb, nz), np.float32), ctx.empty((nb * ladder, nz), np.float32)
    for k in range(1, steps + 1):
        grad = gradient(z)
        check(lib.gl_wb_lbfgs_push(ctx.handle, _p(z.ptr), _p(grad.ptr), _p(z_prev.ptr), _p(g_prev.ptr), _p(S_hist.ptr), _p(Y_hist.ptr), _p(count.ptr),
                                   _p(head.ptr), _p(accepted.ptr), nb, nz, memory))
        check(lib.gl_wb_lbfgs_direction(ctx.handle, _p(grad.ptr), _p(S_hist.ptr), _p(Y_hist.ptr), _p(count.ptr), _p(head.ptr), _p(t.ptr), _p(flag.ptr),
                                        nb, nz, memory, _f(step0), _p(p.ptr)))
        check(lib.gl_wb_lbfgs_candidates(ctx.handle, _p(z.ptr), _p(p.ptr), _p(t.ptr), nb, nz, ladder, _f(z_max), _p(cand.ptr)))
        score(cand, ladder, S_new, j_new)
        check(lib.gl_pbb_accept(ctx.handle, _p(z.ptr), _p(one.ptr), _p(S_cur.ptr), _p(cand.ptr), _p(S_new.ptr), _p(j_new.ptr), nb, nz, ladder,
                                _f(1.0), _f(1.0), _f(1.0), _f(1.0), _p(accepted.ptr)))
        check(lib.gl_wb_lbfgs_advance(ctx.handle, _p(t.ptr), _p(count.ptr), _p(head.ptr), _p(flag.ptr), _p(accepted.ptr), _p(j_new.ptr), nb, ladder))
        record(k, S_cur)
    return z, S_cur


def wb_attack(queries, generator, z_init, steps=64, lr=0.05, beta1=0.9, beta2=0.999, eps=1e-8, z_max=4.0, block_images=4096, history=False,
              distance="l2", optimizer="adam", memory=8, ladder=8, step0=1.0):
    """gradient descent on the latent for every query.

    queries   : [Q,C,H,W] 8-bit images (u8, or floats on the lattice 2*(u/255.)-1); numpy / torch / DeviceArray; [Q,3,64,64] for DCGAN
    generator : the DCGAN / WGAN-GP Generator, or PGGAN's Generator.at(steps, alpha) (l2_grad_z and generate_u8); where it has an
                `image_shape`, queries of another shape are refused
    z_init    : [Q, nz] or [Q, nz, 1, 1] starting latents (pbb_init_from_bank gives the nearest bank latents)
    steps, lr, beta1, beta2, eps: Adam on sum (G(z) - x)^2, float32; z_max: the iterate is clamped to [-z_max, z_max]
    block_images: queries go in blocks of that many; each block runs all its steps on the device
    optimizer : 'adam' (the default) or 'lbfgs', the paper's optimiser: L-BFGS over the last `memory` (1..16) pairs, every step scoring a
                ladder of `ladder` (1..32) step widths t 2^-j along its direction in one batched forward; a steepest-descent step (the first
                one, and after a rejected step) tries length `step0` in latent space first.  steps is the number of gradient evaluations under
                both optimisers; lr, beta1, beta2 and eps are not used by 'lbfgs', memory, ladder and step0 not by 'adam'.  A step scores
                nb * ladder images: the block is capped at pbb.POPULATION_IMAGES // ladder queries, which does not change the results.
    returns (dist float32 [Q] -- the float32 attack() reports for the same S --, z_star float32 [Q, nz], S int64 [Q]), and with
    history=True also trace int64 [steps + 1, Q]: the best S after every step, trace[0] the starting point's."""
    z_host = _check_arguments(generator, z_init, steps, lr, beta1, beta2, eps, z_max, block_images, distance)
    memory, ladder = _check_optimizer(optimizer, memory, ladder, step0)
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

    if optimizer == "lbfgs":
        from .pbb import GL_PBB_GROUP, POPULATION_IMAGES
        per_block = min(per_block, max(1, POPULATION_IMAGES // ladder))
        for lo in range(0, Q, per_block):
            nb = min(per_block, Q - lo)
            q_dev = qu8.view((nb, d), offset_bytes=lo * d)
            work = ctx.empty((GL_PBB_PARTIAL_BYTES * nb * (-(-ladder // GL_PBB_GROUP)),), np.uint8)

            def score(latents, lam, S, j):
                u8 = images(latents, nb * lam)
                check(lib.gl_pbb_group_min(ctx.handle, _p(q_dev.ptr), _p(u8.ptr), nb, lam, d, _p(S.ptr), _p(j.ptr), _p(work.ptr)))

            def record(k, S):
                if history:
                    trace[k, lo:lo + nb] = S.numpy().astype(np.int64)

            z, S_cur = _lbfgs_block(ctx, z_host[lo:lo + nb], steps, memory, ladder, step0, z_max,
                                    lambda z_dev: generator.l2_grad_z(z_dev, q_dev.view((nb,) + image_shape))[0], score, record)
            z_star[lo:lo + nb] = z.numpy()
            S_out[lo:lo + nb] = S_cur.numpy().astype(np.int64)
        dist = _dist32(S_out, d, "u8")
        return (dist, z_star, S_out, trace) if history else (dist, z_star, S_out)

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


# ---------------------------------------------------------------------------------------------------------------------------------------
# the same descent under 0.2 * LPIPS + L2, the distance fbb.py hard-wires and the paper's white-box loss (section 5.4)
PAIR_BLOCK = 256        # queries scored per gl_feat_pair_dist* call: one tile of the pair kernels, and one block of K-blocked search rows


def _forward_f32(generator, z_dev):
    """G(z) of the generator's fp32-product forward -- the values vjp_z differentiates -- as a DeviceArray, with the precision setting the
    caller sees put back"""
    owner = getattr(generator, "generator", generator)             # pggan's Generator.at(steps, alpha) is a view of its Generator
    before = owner._precision
    owner.set_precision(0)
    try:
        if owner is generator:
            y, _ = generator.forward_device(z_dev, True, False, check_range=False)
        else:
            y, _ = owner.forward_device(z_dev, generator.steps, generator.alpha, True, False, check_range=False)
    finally:
        owner.set_precision(before)
    return y


def pair_grad_z(generator, z, targets_u8, lpips=None, ref=None):
    """loss[i] = 0.2 * LPIPS(G(z_i), x_i) + mean (G(z_i) - x_i)^2, x = 2 u / 255 - 1 of targets_u8 [n,3,H,W] uint8, and grad = d loss / d z:
    -> (grad DeviceArray [n, nz], loss DeviceArray [n]), float32.  G(z) is the generator's fp32-product forward, the image gradient is
    LpipsModel.grad_image's (csrc/gl_lpips_grad.hip) and the last step the generator's own vjp_z (DCGAN / WGAN-GP, pggan's
    Generator.at(steps, alpha)).  lpips: the LpipsModel (default: lpips.default_model()); ref: its reference_rows(targets_u8)."""
    refuse_pair_for_tables(generator, "pair_grad_z")
    from . import lpips as _lp
    from ._lib import as_device
    if not hasattr(generator, "vjp_z"):
        raise NotImplementedError("%s.%s has no vjp_z" % (type(generator).__module__, type(generator).__name__))
    model = lpips if lpips is not None else _lp.default_model()
    z_dev = as_device(generator.ctx, z, np.float32)
    y = _forward_f32(generator, z_dev)
    n = z_dev.shape[0]
    shape = tuple(int(v) for v in targets_u8.shape)
    cot, loss = model.grad_image(y.view((n,) + shape[1:]), targets_u8, ref)
    out = generator.vjp_z(z_dev, cot)                              # DCGAN: grad; the PGGAN view: (grad, y)
    return (out[0] if isinstance(out, tuple) else out), loss


def _pair_keys(ctx, model, fq, lo, u8_images, keys):
    """keys[i] = bits(D32(query lo + i, image i)) for the nb images of a block: the images' bank rows, pair distances of blocks of PAIR_BLOCK
    queries against the same block of images, and their diagonals"""
    lib = ctx.lib
    nb = u8_images.shape[0]
    fb = model.features(u8_images, role=model.search_role("bank"), fmt=fq.fmt)
    if fb.K != fq.K or fb.fmt != fq.fmt:
        raise ValueError("the images' rows and the queries' rows differ in layout")
    M = ctx.empty((PAIR_BLOCK, PAIR_BLOCK), np.float32)
    esz = 2 if fq.role else 4
    for b0 in range(0, nb, PAIR_BLOCK):
        m = min(PAIR_BLOCK, nb - b0)
        # where the rows are stored K-blocked, lo and b0 are multiples of PAIR_BLOCK = 256: whole blocks, each contiguous
        qV = fq.V.ptr + (lo + b0) * fq.K * esz
        bV = fb.V.ptr + b0 * fb.K * esz
        qn, bn = fq.norms.ptr + (lo + b0) * 4, fb.norms.ptr + b0 * 4
        if fq.role:
            check(lib.gl_feat_pair_dist_h1_scaled(ctx.handle, _p(bV), _p(bn), m, _p(qV), _p(qn), m, fb.K, _f(fb.scale), _p(M.ptr), PAIR_BLOCK))
        else:
            check(lib.gl_feat_pair_dist(ctx.handle, _p(bV), _p(bn), m, _p(qV), _p(qn), m, fb.K, _p(M.ptr), PAIR_BLOCK))
        check(lib.gl_wb_diag_keys(ctx.handle, _p(M.ptr), m, PAIR_BLOCK, _p(keys.ptr + b0 * 8)))
    ctx.sync()                                                      # fb and M are released on return
    return keys


def pair_wb_attack(queries, generator, z_init, steps=64, lr=0.05, beta1=0.9, beta2=0.999, eps=1e-8, z_max=4.0, block_images=1024, history=False,
                   distance="l2-lpips", lpips=None, optimizer="adam", memory=8, ladder=8, step0=1.0):
    """wb_attack under 0.2 * LPIPS + L2: gradient descent on the latent for every query, scored by the distance attack(distance='l2-lpips')
    searches.

    queries, generator, z_init, steps .. z_max, history: as wb_attack; the generator needs vjp_z and generate_u8, H and W multiples of 16
    lpips: the LpipsModel (default: lpips.default_model(), weights from local files)
    One step is pair_grad_z -> gl_wb_adam_step -> generate_u8 -> the pair distance D32(query, its image) of the search's own kernels, on the
    search's own row formats -> gl_pbb_accept into a separate best-so-far, the key being the uint32 pattern of D32 (D32 >= +0: the unsigned
    order of the patterns is the order of the floats).  Step 0 scores the start, so a score never rises, and started from the nearest bank
    latent under l2-lpips the attack can only lower attack(distance='l2-lpips')'s answer.  block_images: queries per block (rounded up to a
    multiple of 256 for images from 96 x 96, whose search rows are stored in blocks of 256); results do not depend on it.
    optimizer, memory, ladder, step0: as wb_attack.  With 'lbfgs' a step scores the nb * ladder candidates as pair_pbb_attack scores its
    population (their search rows, gl_feat_pair_dist* per tile of 256 queries, gl_pbb_group_min_keys), the iterate is itself the best so
    far, the block is capped at pbb.PAIR_POPULATION_IMAGES // ladder queries, and lr, beta1, beta2 and eps are not used.
    returns (dist float32 [Q] -- the float whose pattern is key --, z_star float32 [Q, nz], key int64 [Q]), and with history=True also
    trace int64 [steps + 1, Q]: the best key after every step, trace[0] the starting point's."""
    refuse_pair_for_tables(generator, "pair_wb_attack")
    z_host = _check_arguments(generator, z_init, steps, lr, beta1, beta2, eps, z_max, block_images, distance, gradient="vjp_z")
    memory, ladder = _check_optimizer(optimizer, memory, ladder, step0)
    steps = int(steps)
    Q, nz = z_host.shape
    if len(queries) != Q:
        raise ValueError("%d queries but %d starting latents" % (len(queries), Q))
    image_shape = tuple(int(v) for v in (queries.shape if hasattr(queries, "shape") else np.shape(queries))[1:])
    want_shape = getattr(generator, "image_shape", None)
    if want_shape is not None and image_shape != tuple(want_shape):
        raise ValueError("the queries are images of shape %r, the generator makes %r" % (image_shape, tuple(want_shape)))
    if len(image_shape) != 3 or image_shape[0] != 3 or image_shape[1] % 16 or image_shape[2] % 16 or min(image_shape[1:]) < 16:
        raise ValueError("the l2-lpips path needs [Q,3,H,W] images with H and W multiples of 16, got %r" % (image_shape,))
    from . import lpips as _lp
    ctx = generator.ctx
    lib = ctx.lib
    model = lpips if lpips is not None else _lp.default_model()
    qu8 = prepare_images(ctx, queries)                   # raises ValueError off the 8-bit lattice
    d = qu8.shape[1]
    z_star = np.empty((Q, nz), np.float32)
    key_out = np.empty((Q,), np.int64)
    trace = np.empty((steps + 1, Q), np.int64) if history else None
    per_block = int(block_images)
    fq = model.features(qu8.view((Q,) + image_shape), role="query" if model.search_role("bank") else None) if Q else None
    if Q and fq.blocked and per_block < Q:
        per_block = -(-per_block // PAIR_BLOCK) * PAIR_BLOCK            # K-blocked rows (images from 96 x 96) come in blocks of 256

    def images(z_dev, n):
        u8 = generator.generate_u8(z_dev)
        if not isinstance(u8, DeviceArray) or u8.dtype != np.uint8 or u8.nbytes != n * d:
            raise ValueError("generate_u8 gave %s for %d latents; the queries hold %d values each" % (getattr(u8, "shape", None), n, d))
        return u8.view((n,) + image_shape)

    if optimizer == "lbfgs" and Q:
        from .pbb import PAIR_POPULATION_IMAGES, _pair_blocking, _pair_group_min, _pair_population_buffers
        per_block, tile = _pair_blocking(fq, Q, min(int(block_images), max(1, PAIR_POPULATION_IMAGES // ladder)))
        M = _pair_population_buffers(ctx, fq, per_block, ladder, tile, nz, "ladder")[1] if steps else None
        rows = [None]                                                    # the candidates' search rows: the first block's, reused
        for lo in range(0, Q, per_block):
            nb = min(per_block, Q - lo)
            q_dev = qu8.view((nb,) + image_shape, offset_bytes=lo * d)
            ref = model.reference_rows(q_dev) if steps else None

            def score(latents, lam, S, j):
                if lam == 1:
                    _pair_keys(ctx, model, fq, lo, images(latents, nb), S)
                else:
                    rows[0] = _pair_group_min(ctx, model, fq, lo, images(latents, nb * lam), lam, tile, M, rows[0], S, j)

            def record(k, S):
                if history:
                    trace[k, lo:lo + nb] = S.numpy().astype(np.int64)

            z, S_cur = _lbfgs_block(ctx, z_host[lo:lo + nb], steps, memory, ladder, step0, z_max,
                                    lambda z_dev: pair_grad_z(generator, z_dev, q_dev, model, ref)[0], score, record)
            z_star[lo:lo + nb] = z.numpy()
            key_out[lo:lo + nb] = S_cur.numpy().astype(np.int64)
        dist = key_out.astype(np.uint32).view(np.float32)
        return (dist, z_star, key_out, trace) if history else (dist, z_star, key_out)

    for lo in range(0, Q, per_block):
        nb = min(per_block, Q - lo)
        q_dev = qu8.view((nb,) + image_shape, offset_bytes=lo * d)
        ref = model.reference_rows(q_dev) if steps else None
        z, z_best = ctx.to_device(z_host[lo:lo + nb]), ctx.to_device(z_host[lo:lo + nb])
        m, v = ctx.zeros((nb, nz), np.float32), ctx.zeros((nb, nz), np.float32)
        one = ctx.to_device(np.ones((nb,), np.float32))                    # gl_pbb_accept's step width: not used here, stays 1
        S_best, S_new = ctx.empty((nb,), np.uint64), ctx.empty((nb,), np.uint64)
        j_new, accepted = ctx.zeros((nb,), np.int32), ctx.empty((nb,), np.uint8)
        # step 0: the starting point itself, straight into S_best
        _pair_keys(ctx, model, fq, lo, images(z, nb), S_best)
        if history:
            trace[0, lo:lo + nb] = S_best.numpy().astype(np.int64)
        for t in range(1, steps + 1):
            grad, _ = pair_grad_z(generator, z, q_dev, model, ref)
            c1, c2 = 1.0 / (1.0 - float(beta1) ** t), 1.0 / (1.0 - float(beta2) ** t)
            check(lib.gl_wb_adam_step(ctx.handle, _p(z.ptr), _p(m.ptr), _p(v.ptr), _p(grad.ptr), nb, nz, _f(lr), _f(beta1), _f(beta2), _f(eps), _f(c1),
                                      _f(c2), _f(z_max)))
            _pair_keys(ctx, model, fq, lo, images(z, nb), S_new)
            check(lib.gl_pbb_accept(ctx.handle, _p(z_best.ptr), _p(one.ptr), _p(S_best.ptr), _p(z.ptr), _p(S_new.ptr), _p(j_new.ptr), nb, nz, 1,
                                    _f(1.0), _f(1.0), _f(1.0), _f(1.0), _p(accepted.ptr)))
            if history:
                trace[t, lo:lo + nb] = S_best.numpy().astype(np.int64)
        z_star[lo:lo + nb] = z_best.numpy()
        key_out[lo:lo + nb] = S_best.numpy().astype(np.int64)
    dist = key_out.astype(np.uint32).view(np.float32)
    return (dist, z_star, key_out, trace) if history else (dist, z_star, key_out)
