"""The partial-black-box attack of GAN-Leaks (section 5.3 of the paper): the attacker holds the generator, searches its latent space for
z* = argmin_z L(x, G(z)) without gradients and scores the query x by L(x, G(z*)).  The paper runs Powell's method per query; the default
here is population-based, a (1 + lambda) evolution strategy for all queries at once, and optimizer="powell" is the paper's method with
every line search turned into a batched ladder (below).  A round of the evolution strategy:

    gl_pbb_candidates   lambda latents around every query's incumbent: z + sigma * eps, eps a counter-based noise (a pure function of
                        seed, round, global query index, j, c -- csrc/gl_pbb.hip, include/ganleaks.h)
    generate_u8         the generator on all Q * lambda latents, as device arrays: the candidates never visit the host
    gl_pbb_group_min    every query against its OWN lambda images: exact S = sum (a - b)^2, the minimum of (S, j)
    gl_pbb_accept       the winner replaces the incumbent where it is strictly closer; sigma *= up on success, *= down otherwise

The strategy is elitist, so the score of a query never rises from round to round, and round 0 evaluates the starting point: started from
the nearest bank latent (pbb_init_from_bank) the attack refines the full-black-box answer and can only lower it.  Distances are exact
integers and the noise is integer arithmetic up to one rounded product, so results do not depend on block_images or on how the queries are
sharded (query_base).

pair_pbb_attack is the same strategy under 0.2 * LPIPS + L2, the distance fbb.py hard-wires: the candidates' images go through VGG16 into
the search's own rows (LpipsModel.features), gl_feat_pair_dist* scores a tile of 256 queries against the tile's candidates, and
gl_pbb_group_min_keys takes every query's minimum over its OWN lambda columns on the uint32 pattern of the float32 distance -- the score
attack(distance='l2-lpips') reports for that pair, bit for bit.  pair_pbb_init_from_bank is its start.

optimizer="powell" (both entries) is Powell's conjugate-direction method, all queries of a block in lock-step (csrc/gl_pbb_powell.hip).  Per
query the direction set U [nz + 1][nz] (the identity at first) and one trial width per direction stay on the device.  A sweep:

    gl_pbb_powell_begin        z0 = z, f0 = the key at the sweep's start
    for line i = 0 .. nz - 1:
        gl_pbb_powell_candidates   the ladder z + (+-2^-k t[i]) U[i]: `ladder` rungs, both signs of ladder / 2 widths, clamped
        generate_u8, gl_pbb_group_min (or the pair path's rows and gl_pbb_group_min_keys) with lambda = ladder, gl_pbb_accept
        gl_pbb_powell_advance      t[i] up or down the ladder; the largest decrease on one line and where it happened
    gl_pbb_powell_extrapolate  the sweep's displacement z - z0 and the point z + (z - z0), scored with lambda = 1
    gl_pbb_powell_decide       Numerical Recipes' test: does the displacement replace the direction of the largest decrease?
    line nz along the displacement (width 0 where the test failed: the block stays in lock-step), gl_pbb_powell_replace

Scoring and acceptance are the evolution strategy's, so a key never rises and the results are a pure function of the inputs: no noise, no
dependence on block_images.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import DeviceArray, check
from .attack import GeneratedBank, _dist32, _prepare_for, attack, prepare_images, refuse_pair_for_tables, table_as_float_rows

_p = ctypes.c_void_p
_f = ctypes.c_float

GL_PBB_GROUP = 16            # include/ganleaks.h
GL_PBB_PARTIAL_BYTES = 16
GL_PBB_POWELL_MAX_LADDER = 32
POPULATION_IMAGES = 16384    # candidate images of one block of pbb_attack, and of one ladder of wb_attack(optimizer="lbfgs")
PAIR_POPULATION_IMAGES = 4096    # the same for pair_pbb_attack and pair_wb_attack(optimizer="lbfgs"): every image also has its search row


def _check_arguments(generator, z_init, rounds, population, sigma, distance, up, down, sigma_min, sigma_max, z_max, block_images, query_base,
                     pair=False):
    """everything that can be refused without a GPU; -> z_init float32 [Q, nz].  pair: the caller is pair_pbb_attack"""
    if pair:
        if distance == "l2":
            raise ValueError("pair_pbb_attack is built for distance='l2-lpips'; pbb_attack runs the search on exact 'l2'")
        if distance != "l2-lpips":
            raise ValueError("distance must be 'l2-lpips', got %r" % (distance,))
    else:
        if distance == "l2-lpips":
            raise NotImplementedError("pbb_attack is built for distance='l2' (exact integer S on 8-bit images); 0.2 * LPIPS + L2 needs the VGG16 "
                                      "features of every candidate and is not built into pbb_attack: pair_pbb_attack runs the search under "
                                      "that distance")
        if distance != "l2":
            raise ValueError("distance must be 'l2', got %r" % (distance,))
    if not hasattr(generator, "generate_u8"):
        raise TypeError("generator must provide generate_u8(z, ...) -> u8 DeviceArray")
    if getattr(generator, "power_iterations", None) is not None:
        raise NotImplementedError("VAEGAN's generator advances its spectral-norm state with every forward, so G is not a fixed function of z: "
                                  "the result of a latent search would depend on how the candidates are blocked -- hand over "
                                  "Generator.frozen(k), the same generator with that state held")
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


_ES_DEFAULTS = (("population", 64), ("sigma", 0.5), ("up", 1.5), ("down", 1.5 ** -0.25))      # the keywords only the evolution strategy reads
_POWELL_DEFAULTS = (("sweeps", 2), ("ladder", 8), ("step0", 1.0))                               # and the ones only Powell's method reads


def _check_optimizer(optimizer, sweeps, ladder, step0, population, sigma, up, down):
    """the optimiser's keywords, refused without a GPU; -> (sweeps, ladder) as ints"""
    if optimizer not in ("es", "powell"):
        raise ValueError("optimizer must be 'es' or 'powell', got %r" % (optimizer,))
    own, other = (_ES_DEFAULTS, _POWELL_DEFAULTS) if optimizer == "es" else (_POWELL_DEFAULTS, _ES_DEFAULTS)
    given = dict(sweeps=sweeps, ladder=ladder, step0=step0, population=population, sigma=sigma, up=up, down=down)
    for name, default in other:
        v = given[name]
        if isinstance(v, bool) or not (v == default):
            raise ValueError("%s=%r belongs to optimizer=%r and is not used by optimizer=%r" % (name, v, "powell" if optimizer == "es" else "es", optimizer))
    if optimizer == "es":
        return int(sweeps), int(ladder)
    if isinstance(sweeps, bool) or not np.isfinite(sweeps) or int(sweeps) != sweeps or sweeps < 0:
        raise ValueError("sweeps must be an integer >= 0, got %r" % (sweeps,))
    if isinstance(ladder, bool) or not np.isfinite(ladder) or int(ladder) != ladder or not 2 <= ladder <= GL_PBB_POWELL_MAX_LADDER or int(ladder) % 2:
        raise ValueError("ladder must be an even integer in 2..%d (a rung for either sign of every width), got %r" % (GL_PBB_POWELL_MAX_LADDER, ladder))
    if isinstance(step0, bool) or not (np.isfinite(step0) and step0 > 0):
        raise ValueError("step0 must be finite and positive, got %r" % (step0,))
    return int(sweeps), int(ladder)


def _powell_fits(ctx, nb, nz, ladder):
    """ValueError where a block's direction rows and candidates do not fit the device"""
    need, avail = nb * (nz + 1) * nz * 4 + nb * ladder * nz * 4, ctx.mem_info()[0]
    if need > avail:
        raise ValueError("a block of %d queries needs %d bytes for its direction sets [%d][%d] and its %d candidates each; %d are available: "
                         "lower block_images" % (nb, need, nz + 1, nz, ladder, avail))


def _powell_block(ctx, z0, sweeps, ladder, step0, t_min, t_max, z_max, key_kind, score, record):
    """Powell's method with a ladder line search for one block of queries, on the device (csrc/gl_pbb_powell.hip, include/ganleaks.h).

    z0 [nb, nz] float32 on the host; score(latents_dev, lam, S_dev, j_dev) writes every query's smallest key over its own lam consecutive
    latents and the rung that attains it, in the form gl_pbb_accept compares; key_kind: 0 where the keys are exact integers, 1 where they
    are float32 patterns; record(sweep, S_cur_dev) is called after the start (sweep 0) and after every sweep.  -> (z, S_cur) DeviceArrays"""
    lib = ctx.lib
    nb, nz = z0.shape
    z = ctx.to_device(z0)
    S_cur, S_new = ctx.empty((nb,), np.uint64), ctx.empty((nb,), np.uint64)
    j_new, accepted = ctx.zeros((nb,), np.int32), ctx.zeros((nb,), np.uint8)
    score(z, 1, S_cur, j_new)                                             # sweep 0: the starting point itself, straight into S_cur
    record(0, S_cur)
    if not sweeps:
        return z, S_cur
    U, t = ctx.empty((nb, nz + 1, nz), np.float32), ctx.empty((nb, nz + 1), np.float32)
    z_start, z_e, cand = ctx.empty((nb, nz), np.float32), ctx.empty((nb, nz), np.float32), ctx.empty((nb * ladder, nz), np.float32)
    f0, S_prev, S_e = ctx.empty((nb,), np.uint64), ctx.empty((nb,), np.uint64), ctx.empty((nb,), np.uint64)
    drop_best, i_best, flag = ctx.empty((nb,), np.float64), ctx.empty((nb,), np.int32), ctx.empty((nb,), np.uint8)
    one = ctx.to_device(np.ones((nb,), np.float32))                       # gl_pbb_accept's step width: not used here, stays 1
    check(lib.gl_pbb_powell_init(ctx.handle, _p(U.ptr), _p(t.ptr), nb, nz, _f(step0)))

    def line(i):
        check(lib.gl_pbb_powell_candidates(ctx.handle, _p(z.ptr), _p(U.ptr), _p(t.ptr), nb, nz, i, ladder, _f(z_max), _p(cand.ptr)))
        score(cand, ladder, S_new, j_new)
        check(lib.gl_pbb_accept(ctx.handle, _p(z.ptr), _p(one.ptr), _p(S_cur.ptr), _p(cand.ptr), _p(S_new.ptr), _p(j_new.ptr), nb, nz, ladder,
                                _f(1.0), _f(1.0), _f(1.0), _f(1.0), _p(accepted.ptr)))
        check(lib.gl_pbb_powell_advance(ctx.handle, _p(t.ptr), _p(accepted.ptr), _p(j_new.ptr), _p(S_cur.ptr), _p(S_prev.ptr), _p(drop_best.ptr),
                                        _p(i_best.ptr), nb, nz, i, ladder, key_kind, _f(t_min), _f(t_max)))

    for k in range(1, sweeps + 1):
        check(lib.gl_pbb_powell_begin(ctx.handle, _p(z.ptr), _p(S_cur.ptr), _p(z_start.ptr), _p(f0.ptr), _p(S_prev.ptr), _p(drop_best.ptr),
                                      _p(i_best.ptr), nb, nz))
        for i in range(nz):
            line(i)
        check(lib.gl_pbb_powell_extrapolate(ctx.handle, _p(z.ptr), _p(z_start.ptr), _p(U.ptr), nb, nz, _f(z_max), _p(z_e.ptr)))
        score(z_e, 1, S_e, j_new)
        check(lib.gl_pbb_powell_decide(ctx.handle, _p(U.ptr), _p(t.ptr), _p(f0.ptr), _p(S_cur.ptr), _p(S_e.ptr), _p(drop_best.ptr), _p(flag.ptr),
                                       nb, nz, key_kind))
        line(nz)
        check(lib.gl_pbb_powell_replace(ctx.handle, _p(U.ptr), _p(t.ptr), _p(flag.ptr), _p(i_best.ptr), nb, nz))
        record(k, S_cur)
    return z, S_cur


def pbb_attack(queries, generator, z_init, rounds=32, population=64, sigma=0.5, seed=0, up=1.5, down=1.5 ** -0.25, sigma_min=1e-4, sigma_max=4.0,
               z_max=4.0, block_images=POPULATION_IMAGES, query_base=0, history=False, distance="l2", optimizer="es", sweeps=2, ladder=8, step0=1.0,
               **generate_kwargs):
    """gradient-free latent search for every query.

    queries   : [Q,C,H,W] 8-bit images (u8, or floats on the lattice 2*(u/255.)-1); numpy / torch / DeviceArray
    generator : anything with generate_u8(z, **generate_kwargs) -> u8 DeviceArray (DCGAN / WGAN-GP / PGGAN Generator)
                A table generator (row_kind 'int': medgan's table_generator, whose bytes are the values themselves) takes a 2-D table
                [Q, F] of whole numbers 0..255 -- float rows on the integer lattice or uint8 holding the values; S is then the number of
                differing columns of 0/1 rows and dist = fl32(S / F), what attack() reports for such rows
    z_init    : [Q, nz] or [Q, nz, 1, 1] starting latents (pbb_init_from_bank gives the nearest bank latents)
    rounds, population: number of rounds and candidates per query and round (lambda); sigma: the initial step width
    seed, query_base  : the noise of query q is a function of (seed, round, query_base + q, j, c): the queries of a larger set can be
                submitted in parts and give the same results
    up, down, sigma_min, sigma_max: the step-width rule (float32 arithmetic); z_max: candidates are clamped to [-z_max, z_max]
    block_images: queries go in blocks of max(1, block_images // population); each block runs all its rounds on the device
    optimizer : 'es' (the default, everything above) or 'powell', the paper's optimiser: `sweeps` sweeps of Powell's conjugate-direction
                method, every line search a two-sided ladder of `ladder` (even, 2..32) step widths +-t 2^-k scored in one batched forward;
                every direction starts at width `step0`, and sigma_min / sigma_max bound the widths (t_min / t_max).  A sweep costs
                (nz + 1) * ladder + 1 forwards per query.  Powell's method draws no noise: seed and query_base have no effect, rounds is
                not used, and population, sigma, up and down are refused unless left at their defaults, as sweeps, ladder and step0 are
                under 'es'.  Queries go in blocks of max(1, block_images // ladder), which does not change the results; ValueError where
                a block's direction sets (nz + 1) * nz floats per query do not fit the device.
    returns (dist float32 [Q] -- the float32 attack() reports for the same S --, z_star float32 [Q, nz], S int64 [Q]), and with
    history=True also trace int64 [rounds + 1, Q]: S after every round, trace[0] the starting point's ([sweeps + 1, Q] and every sweep
    under 'powell')."""
    z_host = _check_arguments(generator, z_init, rounds, population, sigma, distance, up, down, sigma_min, sigma_max, z_max, block_images,
                              query_base)
    sweeps, ladder = _check_optimizer(optimizer, sweeps, ladder, step0, population, sigma, up, down)
    rounds, lam, seed, query_base = int(rounds), int(population), int(seed) & 0xFFFFFFFFFFFFFFFF, int(query_base)
    Q, nz = z_host.shape
    if len(queries) != Q:
        raise ValueError("%d queries but %d starting latents" % (len(queries), Q))
    ctx = generator.ctx
    lib = ctx.lib
    qu8, kind = _prepare_for(generator, ctx, queries)    # raises ValueError off the 8-bit lattice (a table generator: the integer lattice)
    d = qu8.shape[1]
    if kind == "int" and (d,) != tuple(generator.image_shape):
        raise ValueError("the queries are rows of %d columns, the generator makes %d" % (d, generator.image_shape[0]))
    z_star = np.empty((Q, nz), np.float32)
    S_out = np.empty((Q,), np.int64)
    trace = np.empty((rounds + 1, Q), np.int64) if history else None
    per_block = max(1, int(block_images) // lam)

    def images(z_dev, n):
        u8 = generator.generate_u8(z_dev, **generate_kwargs)
        if not isinstance(u8, DeviceArray) or u8.dtype != np.uint8 or u8.nbytes != n * d:
            raise ValueError("generate_u8 gave %s for %d latents; the queries hold %d values each" % (getattr(u8, "shape", None), n, d))
        return u8

    if optimizer == "powell":
        trace = np.empty((sweeps + 1, Q), np.int64) if history else None
        per_block = max(1, int(block_images) // ladder)
        if sweeps and Q:
            _powell_fits(ctx, min(per_block, Q), nz, ladder)
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

            z, S_cur = _powell_block(ctx, z_host[lo:lo + nb], sweeps, ladder, step0, sigma_min, sigma_max, z_max, 0, score, record)
            z_star[lo:lo + nb] = z.numpy()
            S_out[lo:lo + nb] = S_cur.numpy().astype(np.int64)
        dist = _dist32(S_out, d, kind)
        return (dist, z_star, S_out, trace) if history else (dist, z_star, S_out)

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
    dist = _dist32(S_out, d, kind)
    return (dist, z_star, S_out, trace) if history else (dist, z_star, S_out)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the same search under 0.2 * LPIPS + L2, the distance fbb.py hard-wires and the loss of the paper (section 5.3)
def _pair_blocking(fq, Q, per_block):
    """(queries per block, queries per gl_feat_pair_dist* call) for a wish of per_block queries: K-blocked rows (images from 96 x 96) come
    in blocks of PAIR_BLOCK = 256, and the block of pair distances M is [tile][tile * lambda]"""
    from .wb import PAIR_BLOCK
    if fq.blocked and per_block < Q:
        per_block = -(-per_block // PAIR_BLOCK) * PAIR_BLOCK
    per_block = min(per_block, Q)
    return per_block, min(PAIR_BLOCK, per_block)


def _pair_population_buffers(ctx, fq, per_block, lam, tile, nz, what):
    """(cand [per_block * lam, nz] float32, M [tile, tile * lam] float32) of one block, allocated once; ValueError where the candidates' rows
    and the block of pair distances do not fit the device.  what: the keyword that sets lam, for the message"""
    esz = 2 if fq.role else 4
    rows = per_block * lam
    cap = int(ctx.lib.gl_lpips_search_rows_capacity(rows, fq.K)) if fq.role else rows
    need, avail = cap * fq.K * esz + tile * tile * lam * 4, ctx.mem_info()[0]
    if need > avail:
        raise ValueError("a block of %d queries x %d candidates needs %d bytes for the candidates' rows and their pair distances; %d are "
                         "available: lower %s or block_images" % (per_block, lam, need, avail, what))
    return ctx.empty((rows, nz), np.float32), ctx.empty((tile, tile * lam), np.float32)


def _pair_group_min(ctx, model, fq, lo, u8_images, lam, tile, M, fb, S_new, j_new):
    """every query of the block that starts at query lo against its OWN lam images under 0.2 * LPIPS + L2: the images' search rows (the
    bank's role, written into fb where given), per tile of queries one gl_feat_pair_dist* call of the tile's queries against the tile's
    images, and gl_pbb_group_min_keys over every query's own lam columns into S_new, j_new.  u8_images [nb * lam, 3, H, W].
    -> the rows (the first block is the largest: its rows are the buffer every later call writes into)"""
    lib = ctx.lib
    nb = u8_images.shape[0] // lam
    esz = 2 if fq.role else 4
    fb = model.features(u8_images, role=model.search_role("bank"), fmt=fq.fmt, out=fb)
    if fb.K != fq.K or fb.fmt != fq.fmt:
        raise ValueError("the candidates' rows and the queries' rows differ in layout")
    for b0 in range(0, nb, tile):
        m = min(tile, nb - b0)
        # where the rows are stored K-blocked, tile = 256 and lo is a multiple of 256: lo + b0 and b0 * lambda are whole blocks
        qV, qn = fq.V.ptr + (lo + b0) * fq.K * esz, fq.norms.ptr + (lo + b0) * 4
        bV, bn = fb.V.ptr + b0 * lam * fb.K * esz, fb.norms.ptr + b0 * lam * 4
        if fq.role:
            check(lib.gl_feat_pair_dist_h1_scaled(ctx.handle, _p(bV), _p(bn), m * lam, _p(qV), _p(qn), m, fb.K, _f(fb.scale), _p(M.ptr), tile * lam))
        else:
            check(lib.gl_feat_pair_dist(ctx.handle, _p(bV), _p(bn), m * lam, _p(qV), _p(qn), m, fb.K, _p(M.ptr), tile * lam))
        check(lib.gl_pbb_group_min_keys(ctx.handle, _p(M.ptr), m, lam, tile * lam, _p(S_new.ptr + b0 * 8), _p(j_new.ptr + b0 * 4)))
    return fb


def pair_pbb_attack(queries, generator, z_init, rounds=32, population=64, sigma=0.5, seed=0, up=1.5, down=1.5 ** -0.25, sigma_min=1e-4,
                    sigma_max=4.0, z_max=4.0, block_images=PAIR_POPULATION_IMAGES, query_base=0, history=False, distance="l2-lpips", lpips=None,
                    optimizer="es", sweeps=2, ladder=8, step0=1.0, **generate_kwargs):
    """pbb_attack under 0.2 * LPIPS + L2: the same (1 + lambda) strategy, scored by the distance attack(distance='l2-lpips') searches.

    queries, generator, z_init, rounds .. z_max, seed, query_base, history, generate_kwargs: as pbb_attack; [Q,3,H,W] images, H and W
    multiples of 16.  lpips: the LpipsModel (default: lpips.default_model(), weights from local files)
    A round is gl_pbb_candidates (the candidates pbb_attack would draw for the same seed, query_base and incumbents) -> generate_u8 on all
    nb * lambda latents -> their search rows (LpipsModel.features, the bank's role) -> per tile of 256 queries one gl_feat_pair_dist* call of
    the tile's queries against the tile's candidates and gl_pbb_group_min_keys over every query's own lambda columns -> gl_pbb_accept.  The
    key is the uint32 pattern of D32(query, image) out of the search's own pair kernels (D32 >= +0: the unsigned order of the patterns is
    the order of the floats), so key == bits(pair_distances(query, generate_u8(z_star))).  Round 0 scores the start, the strategy is
    elitist: a key never rises, and started from pair_pbb_init_from_bank the attack can only lower attack(distance='l2-lpips')'s answer.
    D32 is a function of the two rows alone and the noise one of the global query index, so results do not depend on block_images or on
    how the queries are split with query_base.
    block_images: candidate images generated and turned into rows at a time -- queries go in blocks of max(1, block_images // population)
    (rounded up to a multiple of 256 for images from 96 x 96, whose search rows are stored in blocks of 256).  One block's candidate rows
    (1 MB per 64 x 64 image) and its block of pair distances are allocated once and reused by every round; ValueError before the first
    round when they do not fit the device.
    optimizer, sweeps, ladder, step0: as pbb_attack.  With 'powell' a line scores the nb * ladder candidates as a round scores its
    population, queries go in blocks of max(1, block_images // ladder) (rounded up as above), f(key) of the acceptance test is the float32
    distance itself, and the trace is [sweeps + 1, Q].
    returns (dist float32 [Q] -- the float whose pattern is key --, z_star float32 [Q, nz], key int64 [Q]), and with history=True also
    trace int64 [rounds + 1, Q]: the key after every round, trace[0] the starting point's."""
    refuse_pair_for_tables(generator, "pair_pbb_attack")
    z_host = _check_arguments(generator, z_init, rounds, population, sigma, distance, up, down, sigma_min, sigma_max, z_max, block_images,
                              query_base, pair=True)
    sweeps, ladder = _check_optimizer(optimizer, sweeps, ladder, step0, population, sigma, up, down)
    rounds, lam, seed, query_base = int(rounds), int(population), int(seed) & 0xFFFFFFFFFFFFFFFF, int(query_base)
    Q, nz = z_host.shape
    if len(queries) != Q:
        raise ValueError("%d queries but %d starting latents" % (len(queries), Q))
    image_shape = tuple(int(v) for v in (queries.shape if hasattr(queries, "shape") else np.shape(queries))[1:])
    if len(image_shape) != 3 or image_shape[0] != 3 or image_shape[1] % 16 or image_shape[2] % 16 or min(image_shape[1:]) < 16:
        raise ValueError("the l2-lpips path needs [Q,3,H,W] images with H and W multiples of 16, got %r" % (image_shape,))
    from . import lpips as _lp
    from .wb import _pair_keys
    ctx = generator.ctx
    lib = ctx.lib
    model = lpips if lpips is not None else _lp.default_model()
    qu8 = prepare_images(ctx, queries)                   # raises ValueError off the 8-bit lattice
    d = qu8.shape[1]
    z_star = np.empty((Q, nz), np.float32)
    key_out = np.empty((Q,), np.int64)
    trace = np.empty(((sweeps if optimizer == "powell" else rounds) + 1, Q), np.int64) if history else None
    if Q == 0:
        dist = key_out.astype(np.uint32).view(np.float32)
        return (dist, z_star, key_out, trace) if history else (dist, z_star, key_out)
    bank_role = model.search_role("bank")
    fq = model.features(qu8.view((Q,) + image_shape), role="query" if bank_role else None)

    def images(z_dev, n):
        u8 = generator.generate_u8(z_dev, **generate_kwargs)
        if not isinstance(u8, DeviceArray) or u8.dtype != np.uint8 or u8.nbytes != n * d:
            raise ValueError("generate_u8 gave %s for %d latents; the queries hold %d values each" % (getattr(u8, "shape", None), n, d))
        return u8.view((n,) + image_shape)

    if optimizer == "powell":
        per_block, tile = _pair_blocking(fq, Q, max(1, int(block_images) // ladder))
        M = None
        if sweeps:
            _powell_fits(ctx, per_block, nz, ladder)
            M = _pair_population_buffers(ctx, fq, per_block, ladder, tile, nz, "ladder")[1]
        rows = [None]                                                    # the candidates' search rows: the first block's, reused
        for lo in range(0, Q, per_block):
            nb = min(per_block, Q - lo)

            def score(latents, n, S, j):
                if n == 1:
                    _pair_keys(ctx, model, fq, lo, images(latents, nb), S)
                else:
                    rows[0] = _pair_group_min(ctx, model, fq, lo, images(latents, nb * n), n, tile, M, rows[0], S, j)

            def record(k, S):
                if history:
                    trace[k, lo:lo + nb] = S.numpy().astype(np.int64)

            z, S_cur = _powell_block(ctx, z_host[lo:lo + nb], sweeps, ladder, step0, sigma_min, sigma_max, z_max, 1, score, record)
            z_star[lo:lo + nb] = z.numpy()
            key_out[lo:lo + nb] = S_cur.numpy().astype(np.int64)
        dist = key_out.astype(np.uint32).view(np.float32)
        return (dist, z_star, key_out, trace) if history else (dist, z_star, key_out)

    per_block, tile = _pair_blocking(fq, Q, max(1, int(block_images) // lam))
    cand = fb = M = None
    if rounds:
        cand, M = _pair_population_buffers(ctx, fq, per_block, lam, tile, nz, "population")

    for lo in range(0, Q, per_block):
        nb = min(per_block, Q - lo)
        z = ctx.to_device(z_host[lo:lo + nb])
        sig = ctx.to_device(np.full((nb,), sigma, np.float32))
        S_cur, S_new = ctx.empty((nb,), np.uint64), ctx.empty((nb,), np.uint64)
        j_new, accepted = ctx.empty((nb,), np.int32), ctx.empty((nb,), np.uint8)
        # round 0: the starting point itself (lambda = 1), straight into S_cur
        _pair_keys(ctx, model, fq, lo, images(z, nb), S_cur)
        if history:
            trace[0, lo:lo + nb] = S_cur.numpy().astype(np.int64)
        cz = cand.view((nb * lam, nz)) if rounds else None
        for r in range(1, rounds + 1):
            check(lib.gl_pbb_candidates(ctx.handle, _p(z.ptr), _p(sig.ptr), nb, nz, lam, ctypes.c_uint64(seed), ctypes.c_uint32(r), query_base + lo,
                                        _f(z_max), _p(cz.ptr)))
            # the first block is the largest: its rows are the buffer every later round and block writes into
            fb = _pair_group_min(ctx, model, fq, lo, images(cz, nb * lam), lam, tile, M, fb, S_new, j_new)
            check(lib.gl_pbb_accept(ctx.handle, _p(z.ptr), _p(sig.ptr), _p(S_cur.ptr), _p(cz.ptr), _p(S_new.ptr), _p(j_new.ptr), nb, nz, lam,
                                    _f(up), _f(down), _f(sigma_min), _f(sigma_max), _p(accepted.ptr)))
            if history:
                trace[r, lo:lo + nb] = S_cur.numpy().astype(np.int64)
        z_star[lo:lo + nb] = z.numpy()
        key_out[lo:lo + nb] = S_cur.numpy().astype(np.int64)
    dist = key_out.astype(np.uint32).view(np.float32)
    return (dist, z_star, key_out, trace) if history else (dist, z_star, key_out)


def pair_pbb_init_from_bank(queries, generator, z_bank, batch_size=64, lpips=None, **generate_kwargs):
    """the start of pair_pbb_attack: the latent of every query's nearest bank sample under 0.2 * LPIPS + L2 -- the full-black-box answer,
    attack(queries, GeneratedBank(generator, z_bank), distance='l2-lpips', batch_size=..., lpips=...).
    -> (z_bank[idx] float32 [Q, nz], idx int64 [Q])"""
    refuse_pair_for_tables(generator, "pair_pbb_init_from_bank")
    if type(z_bank).__module__.startswith("torch"):
        z_bank = z_bank.detach().cpu().numpy()
    z_bank = np.asarray(z_bank, np.float32)
    _, idx = attack(queries, GeneratedBank(generator, z_bank, **generate_kwargs), distance="l2-lpips", batch_size=batch_size, lpips=lpips)
    return np.ascontiguousarray(z_bank[idx].reshape(len(idx), -1)), idx


def pbb_init_from_bank(queries, generator, z_bank, batch_size=64, **generate_kwargs):
    """the natural start of the search: the latent of every query's nearest bank sample under exact L2 -- the full-black-box answer,
    attack(queries, GeneratedBank(generator, z_bank), distance='l2').  -> (z_bank[idx] float32 [Q, nz], idx int64 [Q])"""
    if type(z_bank).__module__.startswith("torch"):
        z_bank = z_bank.detach().cpu().numpy()
    z_bank = np.asarray(z_bank, np.float32)
    if getattr(generator, "row_kind", None) == "int":
        queries = table_as_float_rows(generator.ctx, queries)       # a uint8 table holds the values; attack() reads uint8 as image codes
    _, idx = attack(queries, GeneratedBank(generator, z_bank, **generate_kwargs), distance="l2", batch_size=batch_size)
    return np.ascontiguousarray(z_bank[idx].reshape(len(idx), -1)), idx
