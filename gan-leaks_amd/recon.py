"""The reconstruction attack for VAE-type models (Hilprecht et al., "Monte Carlo and Reconstruction Membership Inference Attacks against
Generative Models", the paper of mc.py's attacks): the attacker holds the WHOLE VAEGAN, encoder and generator, and scores a query x by how
well the model reconstructs it -- the distance between x and G(z) for z at the encoder's posterior mean, and averaged over draws from the
posterior.  Per block of queries:

    Encoder.encode_device   mu, logvar of every query (csrc/gl_vaegan_enc.hip), straight from the queries' bytes
    gl_recon_latents        samples + 1 latents per query: row 0 the clamped mean, rows j >= 1 mu + std * eps with the counter-based noise of
                            the partial-black-box attack (a pure function of seed, query_base + q, j, c -- include/ganleaks.h)
    generate_u8             the generator on all Q * (samples + 1) latents, as device arrays
    gl_pbb_group_S          every query against its OWN samples + 1 images: the exact integer S = sum (a - b)^2 of each

It is the cheapest attack here -- no bank of samples and no search, samples + 1 generator forwards per query -- and its z_mu is a starting
latent for wb_attack / pbb_attack that needs no bank either.  Distances are exact integers and the noise is integer arithmetic up to one
rounded product, so results do not depend on block_images or on how the queries are split (query_base).

std = exp(logvar), NOT exp(logvar / 2): the reference's Encoder.reparametrize (gan_models/vaegan/train.py:98-101) computes
logvar.mul(1.0).exp_(), and the quirk is kept.  It is computed on the host in float32 (np.exp) and uploaded.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import Context, DeviceArray, check
from .attack import _dist32, prepare_images
from .pbb import POPULATION_IMAGES, _check_arguments

_p = ctypes.c_void_p
_f = ctypes.c_float

IMAGE_SHAPE = (3, 64, 64)


def _host(a):
    if isinstance(a, DeviceArray):
        return a.numpy()
    if type(a).__module__.startswith("torch"):
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def _check_draws(samples, z_max, query_base, Q):
    if isinstance(samples, bool) or int(samples) != samples or samples < 0:
        raise ValueError("samples must be an integer >= 0, got %r" % (samples,))
    if not (np.isfinite(z_max) and z_max > 0):
        raise ValueError("z_max must be finite and positive, got %r" % (z_max,))
    if int(query_base) < 0 or int(query_base) + Q > 1 << 32:
        raise ValueError("query_base + Q must stay within 2^32 (the noise counter holds 32 bits of the query index)")


def posterior_std(logvar):
    """the reference's std = exp(logvar) (its quirk: not exp(logvar / 2)), float32 on the host"""
    return np.exp(np.ascontiguousarray(logvar, dtype=np.float32))


def recon_latents(mu, logvar, samples, seed=0, query_base=0, z_max=4.0, ctx=None):
    """mu, logvar [Q, nz] (Encoder.encode's) -> float32 DeviceArray [Q * (samples + 1), nz]: row q * (samples + 1) is the mean of query q
    clamped to [-z_max, z_max], the rows j = 1 .. samples after it are clamp(fl(mu + fl(exp(logvar) * eps(seed, query_base + q, j, c)))) with
    the noise gl_pbb_candidates documents at round 0.  ValueError where exp(logvar) is not finite in float32."""
    mu = np.ascontiguousarray(_host(mu), dtype=np.float32)
    logvar = np.ascontiguousarray(_host(logvar), dtype=np.float32)
    if mu.ndim != 2 or mu.shape[1] < 1 or logvar.shape != mu.shape:
        raise ValueError("mu and logvar must both be [Q, nz], got shapes %r and %r" % (mu.shape, logvar.shape))
    Q, nz = mu.shape
    _check_draws(samples, z_max, query_base, Q)
    with np.errstate(over="ignore"):
        std = posterior_std(logvar)
    if not (np.isfinite(std).all() and np.isfinite(mu).all()):
        raise ValueError("mu or exp(logvar) is not finite in float32")
    ctx = ctx if ctx is not None else Context.get()
    lam = int(samples) + 1
    out = ctx.empty((Q * lam, nz), np.float32)
    mu_dev, std_dev = ctx.to_device(mu), ctx.to_device(std)
    check(ctx.lib.gl_recon_latents(ctx.handle, _p(mu_dev.ptr), _p(std_dev.ptr), Q, nz, lam, ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                                   int(query_base), _f(z_max), _p(out.ptr)))
    return out


def _check_attack(queries, encoder, generator, samples, z_max, block_images, query_base):
    """everything recon_attack refuses without a GPU; -> (Q, nz)"""
    if getattr(generator, "row_kind", None) == "int":
        raise NotImplementedError("recon_attack: the encoder reads 3 x 64 x 64 images, so a table generator (row_kind 'int') has no reconstruction attack")
    nz = int(getattr(generator, "z_dim", -1))
    # the generator checks of the partial-black-box attack (generate_u8, the stateful VAEGAN Generator -> Generator.frozen(k)), z_max, block_images
    _check_arguments(generator, np.zeros((0, max(nz, 1)), np.float32), 0, 1, 1.0, "l2", 1.0, 1.0, 1.0, 1.0, z_max, block_images, 0)
    if int(getattr(encoder, "z_dim", -2)) != nz:
        raise ValueError("the encoder gives latents of %r values, the generator takes %r" % (getattr(encoder, "z_dim", None), getattr(generator, "z_dim", None)))
    shape = tuple(int(v) for v in (queries.shape if hasattr(queries, "shape") else np.shape(queries)))
    if len(shape) != 4 or shape[1:] != IMAGE_SHAPE:
        raise ValueError("recon_attack needs [Q,3,64,64] images (what the VAEGAN encoder reads), got shape %r" % (shape,))
    if tuple(getattr(generator, "image_shape", IMAGE_SHAPE)) != IMAGE_SHAPE:
        raise ValueError("the generator makes images of shape %r, the encoder reads 3 x 64 x 64" % (tuple(generator.image_shape),))
    _check_draws(samples, z_max, query_base, shape[0])
    return shape[0], nz


def recon_attack(queries, encoder, generator, samples=16, seed=0, query_base=0, z_max=4.0, block_images=POPULATION_IMAGES, **generate_kwargs):
    """the reconstruction attack on every query.

    queries   : [Q,3,64,64] 8-bit images (u8, or floats on the lattice 2*(u/255.)-1); numpy / torch / DeviceArray
    encoder   : gan_models.vaegan.train.Encoder (anything with z_dim and encode_device(u8 DeviceArray) -> (mu, logvar) DeviceArrays)
    generator : anything pbb_attack takes for images: for VAEGAN Generator.frozen(k) -- the plain Generator advances its spectral-norm state
                with every forward and is refused with pbb_attack's message; a table generator is refused (the encoder reads images)
    samples   : posterior draws per query; every query costs samples + 1 generator forwards.  seed, query_base: the noise of query q is a
                function of (seed, query_base + q, j, c), so the queries of a larger set can be submitted in parts and give the same results
    block_images: queries go in blocks of max(1, block_images // (samples + 1)); the results do not depend on it
    returns (loss float64 [Q]    -- the mean over the draws j >= 1 of the float32 distances of S[:, j], taken in float64; dist_mu where samples = 0,
             dist_mu float32 [Q] -- the float32 attack() reports for S[:, 0], the distance to the reconstruction at the posterior mean,
             S int64 [Q, samples + 1] -- exact sums of squared byte differences, column 0 against G(mu),
             z_mu float32 [Q, nz] -- the clamped posterior means: a z_init for wb_attack / pbb_attack that needs no bank)"""
    Q, nz = _check_attack(queries, encoder, generator, samples, z_max, block_images, query_base)
    lam, seed, query_base = int(samples) + 1, int(seed) & 0xFFFFFFFFFFFFFFFF, int(query_base)
    ctx = generator.ctx
    lib = ctx.lib
    qu8 = prepare_images(ctx, queries)                   # raises ValueError off the 8-bit lattice
    d = qu8.shape[1]
    S = np.empty((Q, lam), np.int64)
    z_mu = np.empty((Q, nz), np.float32)
    per_block = max(1, int(block_images) // lam)
    for lo in range(0, Q, per_block):
        nb = min(per_block, Q - lo)
        q_dev = qu8.view((nb, d), offset_bytes=lo * d)
        mu, logvar = encoder.encode_device(q_dev.view((nb,) + IMAGE_SHAPE))
        lat = recon_latents(mu, logvar, lam - 1, seed=seed, query_base=query_base + lo, z_max=z_max, ctx=ctx)
        u8 = generator.generate_u8(lat, **generate_kwargs)
        if not isinstance(u8, DeviceArray) or u8.dtype != np.uint8 or u8.nbytes != nb * lam * d:
            raise ValueError("generate_u8 gave %s for %d latents; the queries hold %d values each" % (getattr(u8, "shape", None), nb * lam, d))
        S_dev = ctx.empty((nb, lam), np.uint64)
        check(lib.gl_pbb_group_S(ctx.handle, _p(q_dev.ptr), _p(u8.ptr), nb, lam, d, _p(S_dev.ptr)))
        S[lo:lo + nb] = S_dev.numpy().astype(np.int64)
        z_mu[lo:lo + nb] = lat.numpy().reshape(nb, lam, nz)[:, 0]
        del u8
    dist = _dist32(S, d, "u8")
    dist_mu = np.ascontiguousarray(dist[:, 0])
    loss = dist[:, 1:].astype(np.float64).mean(axis=1) if lam > 1 else dist_mu.astype(np.float64)
    return loss, dist_mu, S, z_mu
