"""The partial-black-box attack of GAN-Leaks (section 5.3 of the paper): the attacker holds the generator, searches its latent space for
z* = argmin_z L(x, G(z)) without gradients and scores the query x by L(x, G(z*)).  The paper runs Powell's method per query; the GPU-native
form of a gradient-free search is population-based, so this is a (1 + lambda) evolution strategy for all queries at once.  A round:

    gl_pbb_candidates   lambda latents around every query's incumbent: z + sigma * eps, eps a counter-based noise (a pure function of
                        seed, round, global query index, j, c -- csrc/gl_pbb.hip, include/ganleaks.h)
    generate_u8         the generator on all Q * lambda latents, as device arrays: the candidates never visit the host
    gl_pbb_group_min    every query against its OWN lambda images: exact S = sum (a - b)^2, the minimum of (S, j)
    gl_pbb_accept       the winner replaces the incumbent where it is strictly closer; sigma *= up on success, *= down otherwise

The strategy is elitist, so the score of a query never rises from round to round, and round 0 evaluates the starting point: started from
the nearest bank latent (pbb_init_from_bank) the attack refines the full-black-box answer and can only lower it.  Distances are exact
integers and the noise is integer arithmetic up to one rounded product, so results do not depend on block_images or on how the queries are
sharded (query_base).
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import DeviceArray, check
from .attack import GeneratedBank, _dist32, attack, prepare_images

_p = ctypes.c_void_p
_f = ctypes.c_float

GL_PBB_GROUP = 16            # include/ganleaks.h
GL_PBB_PARTIAL_BYTES = 16


def _check_arguments(generator, z_init, rounds, population, sigma, distance, up, down, sigma_min, sigma_max, z_max, block_images, query_base):
    """everything that can be refused without a GPU; -> z_init float32 [Q, nz]"""
    if distance == "l2-lpips":
        raise NotImplementedError("pbb_attack is built for distance='l2' (exact integer S on 8-bit images); 0.2 * LPIPS + L2 needs the VGG16 "
                                  "features of every candidate and is not built")
    if distance != "l2":
        raise ValueError("distance must be 'l2', got %r" % (distance,))
    if not hasattr(generator, "generate_u8"):
        raise TypeError("generator must provide generate_u8(z, ...) -> u8 DeviceArray")
    if getattr(generator, "power_iterations", None) is not None:
        raise NotImplementedError("VAEGAN's generator advances its spectral-norm state with every forward, so G is not a fixed function of z: "
                                  "the result of a latent search would depend on how the candidates are blocked")
    if int(rounds) != rounds or rounds < 0:
        raise ValueError("rounds must be an integer >= 0, got %r" % (rounds,))
    if int(population) != population or population < 1:
        raise ValueError("population must be an integer >= 1, got %r" % (population,))
    if not (np.isfinite(sigma) and sigma > 0):
        raise ValueError("sigma must be finite and positive, got %r" % (sigma,))
    for name, v in (("up", up), ("down", down), ("sigma_min", sigma_min), ("sigma_max", sigma_max), ("z_max", z_max)):
        if not (np.isfinite(v) and v > 0):
            raise ValueError("%s must be finite and positive, got %r" % (name, v))
    if sigma_min > sigma_max:
        raise ValueError("sigma_min %r exceeds sigma_max %r" % (sigma_min, sigma_max))
    if int(block_images) < 1:
        raise ValueError("block_images must be at least 1, got %r" % (block_images,))
    if type(z_init).__module__.startswith("torch"):
        z_init = z_init.detach().cpu().numpy()
    z = np.asarray(z_init, np.float32)
    if z.ndim == 4 and z.shape[2:] == (1, 1):
        z = z.reshape(z.shape[0], z.shape[1])
    if z.ndim != 2 or z.shape[1] < 1:
        raise ValueError("z_init must be [Q, nz] or [Q, nz, 1, 1], got shape %r" % (z.shape,))
    if int(query_base) < 0 or int(query_base) + len(z) > 1 << 32:
        raise ValueError("query_base + Q must stay within 2^32 (the noise counter holds 32 bits of the query index)")
    return np.ascontiguousarray(z)


def pbb_attack(queries, generator, z_init, rounds=32, population=64, sigma=0.5, seed=0, up=1.5, down=1.5 ** -0.25, sigma_min=1e-4, sigma_max=4.0,
               z_max=4.0, block_images=16384, query_base=0, history=False, distance="l2", **generate_kwargs):
    """gradient-free latent search for every query.

    queries   : [Q,C,H,W] 8-bit images (u8, or floats on the lattice 2*(u/255.)-1); numpy / torch / DeviceArray
    generator : anything with generate_u8(z, **generate_kwargs) -> u8 DeviceArray (DCGAN / WGAN-GP / PGGAN Generator)
    z_init    : [Q, nz] or [Q, nz, 1, 1] starting latents (pbb_init_from_bank gives the nearest bank latents)
    rounds, population: number of rounds and candidates per query and round (lambda); sigma: the initial step width
    seed, query_base  : the noise of query q is a function of (seed, round, query_base + q, j, c): the queries of a larger set can be
                submitted in parts and give the same results
    up, down, sigma_min, sigma_max: the step-width rule (float32 arithmetic); z_max: candidates are clamped to [-z_max, z_max]
    block_images: queries go in blocks of max(1, block_images // population); each block runs all its rounds on the device
    returns (dist float32 [Q] -- the float32 attack() reports for the same S --, z_star float32 [Q, nz], S int64 [Q]), and with
    history=True also trace int64 [rounds + 1, Q]: S after every round, trace[0] the starting point's."""
    z_host = _check_arguments(generator, z_init, rounds, population, sigma, distance, up, down, sigma_min, sigma_max, z_max, block_images,
                              query_base)
    rounds, lam, seed, query_base = int(rounds), int(population), int(seed) & 0xFFFFFFFFFFFFFFFF, int(query_base)
    Q, nz = z_host.shape
    if len(queries) != Q:
        raise ValueError("%d queries but %d starting latents" % (len(queries), Q))
    ctx = generator.ctx
    lib = ctx.lib
    qu8 = prepare_images(ctx, queries)                   # raises ValueError off the 8-bit lattice
    d = qu8.shape[1]
    z_star = np.empty((Q, nz), np.float32)
    S_out = np.empty((Q,), np.int64)
    trace = np.empty((rounds + 1, Q), np.int64) if history else None
    per_block = max(1, int(block_images) // lam)

    def images(z_dev, n):
        u8 = generator.generate_u8(z_dev, **generate_kwargs)
        if not isinstance(u8, DeviceArray) or u8.dtype != np.uint8 or u8.nbytes != n * d:
            raise ValueError("generate_u8 gave %s for %d latents; the queries hold %d values each" % (getattr(u8, "shape", None), n, d))
        return u8

    for lo in range(0, Q, per_block):
        nb = min(per_block, Q - lo)
        q_dev = qu8.view((nb, d), offset_bytes=lo * d)
        z = ctx.to_device(z_host[lo:lo + nb])
        sig = ctx.to_device(np.full((nb,), sigma, np.float32))
        S_cur, S_new = ctx.empty((nb,), np.uint64), ctx.empty((nb,), np.uint64)
        j_new, accepted = ctx.empty((nb,), np.int32), ctx.empty((nb,), np.uint8)
        work = ctx.empty((GL_PBB_PARTIAL_BYTES * nb * ((lam + GL_PBB_GROUP - 1) // GL_PBB_GROUP),), np.uint8)
        cand = ctx.empty((nb * lam, nz), np.float32) if rounds else None
        # round 0: the starting point itself (lambda = 1), straight into S_cur
        u8 = images(z, nb)
        check(lib.gl_pbb_group_min(ctx.handle, _p(q_dev.ptr), _p(u8.ptr), nb, 1, d, _p(S_cur.ptr), _p(j_new.ptr), _p(work.ptr)))
        if history:
            trace[0, lo:lo + nb] = S_cur.numpy().astype(np.int64)
        for r in range(1, rounds + 1):
            check(lib.gl_pbb_candidates(ctx.handle, _p(z.ptr), _p(sig.ptr), nb, nz, lam, ctypes.c_uint64(seed), ctypes.c_uint32(r), query_base + lo,
                                        _f(z_max), _p(cand.ptr)))
            u8 = images(cand, nb * lam)
            check(lib.gl_pbb_group_min(ctx.handle, _p(q_dev.ptr), _p(u8.ptr), nb, lam, d, _p(S_new.ptr), _p(j_new.ptr), _p(work.ptr)))
            check(lib.gl_pbb_accept(ctx.handle, _p(z.ptr), _p(sig.ptr), _p(S_cur.ptr), _p(cand.ptr), _p(S_new.ptr), _p(j_new.ptr), nb, nz, lam,
                                    _f(up), _f(down), _f(sigma_min), _f(sigma_max), _p(accepted.ptr)))
            if history:
                trace[r, lo:lo + nb] = S_cur.numpy().astype(np.int64)
        z_star[lo:lo + nb] = z.numpy()
        S_out[lo:lo + nb] = S_cur.numpy().astype(np.int64)
        del u8
    dist = _dist32(S_out, d, "u8")
    return (dist, z_star, S_out, trace) if history else (dist, z_star, S_out)


def pbb_init_from_bank(queries, generator, z_bank, batch_size=64, **generate_kwargs):
    """the natural start of the search: the latent of every query's nearest bank sample under exact L2 -- the full-black-box answer,
    attack(queries, GeneratedBank(generator, z_bank), distance='l2').  -> (z_bank[idx] float32 [Q, nz], idx int64 [Q])"""
    if type(z_bank).__module__.startswith("torch"):
        z_bank = z_bank.detach().cpu().numpy()
    z_bank = np.asarray(z_bank, np.float32)
    _, idx = attack(queries, GeneratedBank(generator, z_bank, **generate_kwargs), distance="l2", batch_size=batch_size)
    return np.ascontiguousarray(z_bank[idx].reshape(len(idx), -1)), idx
