"""GPU: the partial-black-box attack (csrc/gl_pbb.hip, ganleaks_amd/pbb.py) against the host restatements of tests/pbb_common.py.

The noise is integer arithmetic up to one rounded product and the distances are exact integers, so every comparison is array_equal: the
candidates on their uint32 views, S and j as integers, and whole searches (z*, S, trace) against a numpy search whose only outside call is
the generator itself."""
import ctypes

import numpy as np
import pytest

import gpu_common  # noqa: F401
import pbb_common as pc

pytestmark = pytest.mark.gpu
_p = ctypes.c_void_p
KW = dict(up=1.5, down=1.5 ** -0.25, sigma_min=1e-4, sigma_max=4.0, z_max=4.0)
LAM, SEED = 37, 77


@pytest.fixture(scope="module")
def gl():
    import ganleaks_amd
    return ganleaks_amd


@pytest.fixture(scope="module")
def dcgan(gl):
    """the small DCGAN, 23 starting latents and 23 queries of three kinds.  q % 3 == 0: G(z_init[q]) itself -- S = 0 from the start, no
    candidate is ever accepted and sigma only shrinks.  q % 3 == 1: the image of an unrelated latent -- candidates may or may not be closer.
    q % 3 == 2: the image of candidate q % LAM of round 1 under SEED -- accepted in round 1 with S = 0, so sigma grows once, then shrinks."""
    from ganleaks_amd.gan_models.dcgan.model_torch import Generator
    gen = Generator(100, 3, 16)
    gen.load_state_dict(gl.synth.dcgan_state_dict(1234, features_g=16))
    z_init = gl.synth.latent(21, 23).reshape(23, 100)
    queries = gen.generate_u8(z_init).numpy()
    queries[1::3] = gen.generate_u8(gl.synth.latent(22, 23).reshape(23, 100)).numpy()[1::3]
    cz = pc.candidates(z_init, np.full(23, 0.5, np.float32), LAM, SEED, 1, 0, KW["z_max"])
    planted = gen.generate_u8(cz).numpy()[np.arange(23) * LAM + np.arange(23) % LAM]
    queries[2::3] = planted[2::3]
    return gen, z_init, queries


def _candidates(ctx, z, sigma, lam, seed, rnd, query_base, z_max):
    nq, nz = z.shape
    out = ctx.empty((nq * lam, nz), np.float32)
    zd, sd = ctx.to_device(z), ctx.to_device(np.asarray(sigma, np.float32))
    from ganleaks_amd._lib import check
    check(ctx.lib.gl_pbb_candidates(ctx.handle, _p(zd.ptr), _p(sd.ptr), nq, nz, lam, ctypes.c_uint64(seed), ctypes.c_uint32(rnd), query_base,
                                    ctypes.c_float(z_max), _p(out.ptr)))
    return out.numpy()


def _group_min(ctx, queries, cand, lam, q_dev=None, c_dev=None):
    from ganleaks_amd._lib import check
    nq, d = queries.shape
    q_dev = ctx.to_device(queries) if q_dev is None else q_dev
    c_dev = ctx.to_device(cand) if c_dev is None else c_dev
    S, j = ctx.empty((nq,), np.uint64), ctx.empty((nq,), np.int32)
    work = ctx.empty((16 * nq * ((lam + 15) // 16),), np.uint8)
    check(ctx.lib.gl_pbb_group_min(ctx.handle, _p(q_dev.ptr), _p(c_dev.ptr), nq, lam, d, _p(S.ptr), _p(j.ptr), _p(work.ptr)))
    return S.numpy().astype(np.int64), j.numpy()


def test_candidates_bit_for_bit(gl):
    ctx = gl.Context.get()
    seed, lam, rnd = 0x0123456789ABCDEF, 37, 3
    z = gl.synth.latent(5, 7).reshape(7, 100)
    sigma = np.array([0.5, 1e-4, 4.0, 0.25, 40.0, 1.0, 0.03], np.float32)       # 40: z_max clamps
    want = pc.candidates(z, sigma, lam, seed, rnd, 5, 4.0)
    assert (np.abs(want[4 * lam:5 * lam]) == 4.0).any() and (np.abs(want[:lam]) < 4.0).all()
    got = _candidates(ctx, z, sigma, lam, seed, rnd, 5, 4.0)
    assert got.shape == (7 * lam, 100) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the same rows when the 7 queries are submitted as 3 + 4
    parts = np.concatenate([_candidates(ctx, z[:3], sigma[:3], lam, seed, rnd, 5, 4.0), _candidates(ctx, z[3:], sigma[3:], lam, seed, rnd, 8, 4.0)])
    assert np.array_equal(parts.view(np.uint32), want.view(np.uint32))
    # other rounds and seeds give other rows; the high word of the seed is part of the key
    for s, r in ((seed, 4), (seed ^ 1, rnd), (seed ^ (1 << 40), rnd)):
        other = _candidates(ctx, z, sigma, lam, s, r, 5, 4.0)
        assert np.array_equal(other.view(np.uint32), pc.candidates(z, sigma, lam, s, r, 5, 4.0).view(np.uint32))
        assert not np.array_equal(other, got)
    # zero queries: nothing happens; query_base + nq beyond 2^32: refused
    assert _candidates(ctx, z[:0], sigma[:0], lam, seed, rnd, 0, 4.0).shape == (0, 100)
    assert _candidates(ctx, z[:1], sigma[:1], 1, seed, rnd, (1 << 32) - 1, 4.0).shape == (1, 100)
    with pytest.raises(gl.GanLeaksError, match="2\\^32"):
        _candidates(ctx, z[:2], sigma[:2], 1, seed, rnd, (1 << 32) - 1, 4.0)


@pytest.mark.parametrize("nq,lam,d", [(3, 5, 300), (23, 37, 12288), (2, 3, 70001), (4, 1, 12288), (3, 1, 77)])
def test_group_min_exact(gl, nq, lam, d):
    """ragged d (bytes) and d % 16 == 0 (16-byte loads), one and several K chunks, one and several candidate groups with a ragged last one,
    lambda = 1; ties inside a wave, across waves and across groups go to the lower j"""
    ctx = gl.Context.get()
    rng = np.random.default_rng(100 + d + lam)
    q = rng.integers(0, 256, size=(nq, d), dtype=np.uint8)
    c = rng.integers(0, 256, size=(nq, lam, d), dtype=np.uint8)
    if lam >= 5:
        # near copies of the query, twice each: (1, 2) share a wave, (3, 4) straddle two waves; with 37 candidates (5, 30) straddle groups
        for qi, (a, b) in enumerate([(1, 2), (3, 4), (5, 30) if lam > 30 else (0, 4)][:nq]):
            near = q[qi].copy()
            near[::7] ^= 3
            c[qi, a] = c[qi, b] = near
    c = c.reshape(nq * lam, d)
    S, j, allS = pc.group_min(q, c, lam)
    if lam >= 5:
        assert (np.sort(allS, axis=1)[:min(nq, 3), 0] == np.sort(allS, axis=1)[:min(nq, 3), 1]).all() and j[0] == 1 and j[1] == 3
    gS, gj = _group_min(ctx, q, c, lam)
    assert np.array_equal(gS, S) and np.array_equal(gj, j), (gS, S, gj, j)


def test_group_min_beyond_32_bits_and_unaligned(gl):
    ctx = gl.Context.get()
    # an all-0 query against all-255 candidates: S = 65025 d > 2^32 at d = 70000 (d % 16 == 0: the 16-byte path, five K chunks)
    d = 70000
    q = np.zeros((2, d), np.uint8)
    c = np.full((6, d), 255, np.uint8)
    c[4, 69999] = 254                                           # query 1: candidate 1 is closer by 2 * 255 - 1
    gS, gj = _group_min(ctx, q, c, 3)
    assert 65025 * d > 1 << 32
    assert gS.tolist() == [65025 * d, 65025 * d - 509] and gj.tolist() == [0, 1]
    # d % 16 == 0 but rows that do not start on 16-byte boundaries (a view 4 bytes into a buffer): the byte path, same answers
    rng = np.random.default_rng(9)
    q = rng.integers(0, 256, size=(3, 304), dtype=np.uint8)
    c = rng.integers(0, 256, size=(3 * 5, 304), dtype=np.uint8)
    S, j, _ = pc.group_min(q, c, 5)
    buf = ctx.to_device(np.concatenate([np.zeros(4, np.uint8), q.reshape(-1)]))
    gS, gj = _group_min(ctx, q, c, 5, q_dev=buf.view((3, 304), offset_bytes=4))
    assert np.array_equal(gS, S) and np.array_equal(gj, j)
    assert _group_min(ctx, q[:0], c[:0], 5)[0].shape == (0,)


def test_accept_kernel(gl):
    from ganleaks_amd._lib import check
    ctx = gl.Context.get()
    rng = np.random.default_rng(3)
    nq, nz, lam = 9, 100, 5
    z = rng.standard_normal((nq, nz)).astype(np.float32)
    cand = rng.standard_normal((nq * lam, nz)).astype(np.float32)
    sigma = np.array([0.5, 0.5, 3.9, 1.1e-4, 1.0, 2.0, 0.3, 0.7, 4.0], np.float32)
    S_cur = np.array([10, 10, 10, 10, 1 << 40, 0, 5, (1 << 63) + 5, 7], np.uint64)
    S_new = np.array([9, 10, 0, 11, (1 << 40) - 1, 0, 4, 1 << 63, 8], np.uint64)
    j_new = rng.integers(0, lam, size=nq).astype(np.int32)
    # (the restatement compares int64: the two values beyond 2^63 are compared by hand)
    want_take = np.array([True, False, True, False, True, False, True, True, False])
    zd, sd, cd, nd, jd = (ctx.to_device(a) for a in (z, sigma, S_cur, S_new, j_new))
    cz, acc = ctx.to_device(cand), ctx.empty((nq,), np.uint8)
    check(ctx.lib.gl_pbb_accept(ctx.handle, _p(zd.ptr), _p(sd.ptr), _p(cd.ptr), _p(cz.ptr), _p(nd.ptr), _p(jd.ptr), nq, nz, lam,
                                ctypes.c_float(KW["up"]), ctypes.c_float(KW["down"]), ctypes.c_float(1e-4), ctypes.c_float(4.0), _p(acc.ptr)))
    assert np.array_equal(acc.numpy().astype(bool), want_take)
    assert np.array_equal(cd.numpy(), np.where(want_take, S_new, S_cur))
    rows = cand.reshape(nq, lam, nz)[np.arange(nq), j_new]
    assert np.array_equal(zd.numpy().view(np.uint32), np.where(want_take[:, None], rows, z).view(np.uint32))
    s = sigma * np.where(want_take, np.float32(KW["up"]), np.float32(KW["down"])).astype(np.float32)
    want_sigma = np.minimum(np.maximum(s, np.float32(1e-4)), np.float32(4.0))
    assert want_sigma[2] == 4.0 and want_sigma[3] == np.float32(1e-4)
    assert np.array_equal(sd.numpy().view(np.uint32), want_sigma.view(np.uint32))


def test_two_rounds_end_to_end(gl, dcgan):
    gen, z_init, queries = dcgan
    lam, seed = LAM, SEED
    calls = []

    def generate(z):
        calls.append(len(z))
        return gen.generate_u8(np.ascontiguousarray(z)).numpy()          # one call for all candidates of a round

    z_want, S_want, trace_want, sig = pc.search(queries, generate, z_init, 2, lam, 0.5, seed, query_base=0, **KW)
    assert calls == [23, 23 * lam, 23 * lam]
    f32, up, down = np.float32, np.float32(KW["up"]), np.float32(KW["down"])
    # never accepted: sigma shrinks twice; planted: accepted in round 1 (sigma grows), nothing beats S = 0 in round 2 (sigma shrinks)
    assert (trace_want[:, 0::3] == 0).all() and (sig[0::3] == f32(f32(f32(0.5) * down) * down)).all()
    assert (trace_want[0, 2::3] > 0).all() and (trace_want[1:, 2::3] == 0).all() and (sig[2::3] == f32(f32(f32(0.5) * up) * down)).all()
    assert not np.array_equal(z_want[2::3], z_init[2::3]) and np.array_equal(z_want[0::3], z_init[0::3])
    print("acceptances per round among the 8 queries with unrelated images:", (np.diff(trace_want[:, 1::3], axis=0) < 0).sum(axis=1))
    dist, z_star, S, trace = gl.pbb_attack(queries, gen, z_init, rounds=2, population=lam, sigma=0.5, seed=seed, block_images=5 * lam, history=True,
                                           **KW)
    assert trace.dtype == np.int64 and trace.shape == (3, 23) and S.dtype == np.int64 and dist.dtype == np.float32 and z_star.dtype == np.float32
    assert np.array_equal(trace, trace_want) and np.array_equal(S, S_want) and np.array_equal(S, trace[-1])
    assert np.array_equal(z_star.view(np.uint32), z_want.view(np.uint32))
    from ganleaks_amd.attack import _dist32
    assert np.array_equal(dist, _dist32(S, 12288, "u8"))
    # rounds = 0 scores the starting point; history off returns three values
    d0, z0, S0 = gl.pbb_attack(queries, gen, z_init.reshape(23, 100, 1, 1), rounds=0)
    assert np.array_equal(S0, trace_want[0]) and np.array_equal(z0, z_init)


def test_planted_answers(gl, dcgan):
    gen, z_init, _ = dcgan
    lam, seed = 37, 4242
    cz = pc.candidates(z_init, np.full(23, 0.5, np.float32), lam, seed, 1, 0, KW["z_max"])
    imgs = gen.generate_u8(cz).numpy()
    pick = np.arange(23) * lam + np.arange(23) % lam
    queries = imgs[pick]
    dist, z_star, S, trace = gl.pbb_attack(queries, gen, z_init, rounds=1, population=lam, sigma=0.5, seed=seed, history=True, **KW)
    assert (trace[0] > 0).all() and (S == 0).all() and (dist == 0).all()
    assert np.array_equal(z_star.view(np.uint32), cz[pick].view(np.uint32))


def test_invariants(gl, dcgan):
    gen, _, queries = dcgan
    lam, seed = 37, 5
    z_bank = gl.synth.latent(31, 130).reshape(130, 100)
    z_init, idx = gl.pbb_init_from_bank(queries, gen, z_bank, batch_size=64)
    fbb_dist, fbb_idx = gl.attack(queries, gl.GeneratedBank(gen, z_bank), distance="l2", batch_size=64)
    assert np.array_equal(idx, fbb_idx) and idx.max() < 128 and np.array_equal(z_init, z_bank[idx])
    run = lambda q, z, **kw: gl.pbb_attack(q, gen, z, rounds=3, population=lam, sigma=0.5, seed=seed, history=True, **KW, **kw)   # noqa: E731
    dist, z_star, S, trace = run(queries, z_init)
    assert (np.diff(trace, axis=0) <= 0).all() and np.array_equal(trace[-1], S)
    from ganleaks_amd.attack import _dist32
    assert np.array_equal(_dist32(trace[0], 12288, "u8"), fbb_dist) and (dist <= fbb_dist).all()
    for block in (lam, 5 * lam):
        for a, b in zip(run(queries, z_init, block_images=block), (dist, z_star, S, trace)):
            assert np.array_equal(a, b), block
    lo, hi = run(queries[:9], z_init[:9]), run(queries[9:], z_init[9:], query_base=9)
    assert np.array_equal(np.concatenate([lo[1], hi[1]]), z_star) and np.array_equal(np.concatenate([lo[3], hi[3]], axis=1), trace)
    # without query_base the second part draws the noise of queries 0..13
    assert not np.array_equal(run(queries[9:], z_init[9:])[1], z_star[9:])
    # off the 8-bit lattice: refused as prepare_images refuses
    with pytest.raises(ValueError, match="lattice"):
        gl.pbb_attack(np.full((23, 3, 64, 64), 0.123, np.float32), gen, z_init, rounds=1, population=2)
    with pytest.raises(ValueError, match="generate_u8 gave"):
        gl.pbb_attack(queries[:, :, :32], gen, z_init, rounds=1, population=2)


def test_pggan_through_generate_kwargs(gl):
    from ganleaks_amd.gan_models.pggan.model_torch import Generator
    gen = Generator(64, 64, 3)
    gen.load_state_dict(gl.synth.pggan_state_dict(100, 64, 64))
    z_init = gl.synth.latent(41, 4, 64).reshape(4, 64)
    queries = gen.generate_u8(gl.synth.latent(42, 4, 64), steps=2, alpha=1.0).numpy()
    assert queries.shape == (4, 3, 16, 16)
    run = lambda: gl.pbb_attack(queries, gen, z_init, rounds=2, population=8, seed=1, history=True, steps=2, alpha=1.0)   # noqa: E731
    dist, z_star, S, trace = run()
    assert trace.shape == (3, 4) and (np.diff(trace, axis=0) <= 0).all()
    for a, b in zip(run(), (dist, z_star, S, trace)):
        assert np.array_equal(a, b)
