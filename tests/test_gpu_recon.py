"""GPU: the reconstruction attack's two kernels (gl_pbb_group_S, gl_recon_latents in csrc/gl_pbb.hip) against their numpy restatements, and
recon_attack on a frozen VAEGAN generator: S against numpy, invariance under block_images and query splits, and its z_mu as the start of the
white-box attack."""
import ctypes

import numpy as np
import pytest

import gpu_common  # noqa: F401
import recon_common as rc

pytestmark = pytest.mark.gpu
_p = ctypes.c_void_p
NZ, D = 100, 32


@pytest.fixture(scope="module")
def ctx():
    import ganleaks_amd as gl
    return gl.Context.get()


def _group_S(ctx, q_dev, c_dev, nq, lam, d):
    from ganleaks_amd._lib import check
    out = ctx.empty((nq, lam), np.uint64)
    check(ctx.lib.gl_pbb_group_S(ctx.handle, _p(q_dev.ptr if hasattr(q_dev, "ptr") else q_dev), _p(c_dev.ptr if hasattr(c_dev, "ptr") else c_dev),
                                 nq, lam, d, _p(out.ptr)))
    return out.numpy().astype(np.int64)


@pytest.mark.parametrize("d", [1, 15, 16, 17, 12288])
def test_group_S_matches_numpy(ctx, d):
    from ganleaks_amd._lib import check
    rng = np.random.default_rng(d)
    for lam in (1, 2, 17, 33):
        for nq in (1, 3, 5):
            q = rng.integers(0, 256, size=(nq, d), dtype=np.uint8)
            c = rng.integers(0, 256, size=(nq * lam, d), dtype=np.uint8)
            c[0] = q[0]                                                   # an exact hit: S = 0
            want = rc.group_S(q, c, lam)
            qd, cd = ctx.to_device(q), ctx.to_device(c)
            got = _group_S(ctx, qd, cd, nq, lam, d)
            assert np.array_equal(got, want), (d, lam, nq)
            # its row minimum and the smallest j that attains it are gl_pbb_group_min's
            S, j = ctx.empty((nq,), np.uint64), ctx.empty((nq,), np.int32)
            work = ctx.empty((16 * nq * (-(-lam // 16)),), np.uint8)
            check(ctx.lib.gl_pbb_group_min(ctx.handle, _p(qd.ptr), _p(cd.ptr), nq, lam, d, _p(S.ptr), _p(j.ptr), _p(work.ptr)))
            assert np.array_equal(S.numpy().astype(np.int64), got.min(axis=1)) and np.array_equal(j.numpy(), got.argmin(axis=1).astype(np.int32))


@pytest.mark.parametrize("d", [1, 17, 12288])
def test_group_S_extreme_and_unaligned(ctx, d):
    lam, nq = 3, 2
    q = np.zeros((nq, d), np.uint8)
    c = np.full((nq * lam, d), 255, np.uint8)
    assert (_group_S(ctx, ctx.to_device(q), ctx.to_device(c), nq, lam, d) == 65025 * d).all()
    # base pointers offset by one byte: byte loads, the same sums
    rng = np.random.default_rng(7 + d)
    q = rng.integers(0, 256, size=(nq, d), dtype=np.uint8)
    c = rng.integers(0, 256, size=(nq * lam, d), dtype=np.uint8)
    qd = ctx.to_device(np.concatenate([[0], q.reshape(-1)]).astype(np.uint8))
    cd = ctx.to_device(np.concatenate([[0], c.reshape(-1)]).astype(np.uint8))
    assert np.array_equal(_group_S(ctx, qd.ptr + 1, cd.ptr + 1, nq, lam, d), rc.group_S(q, c, lam))
    assert ctx.lib.gl_pbb_group_S(ctx.handle, _p(0), _p(0), 0, lam, d, _p(0)) == 0          # nq == 0


@pytest.mark.parametrize("nz", [1, 3, 100])
@pytest.mark.parametrize("lam", [1, 2, 17])
def test_recon_latents_match_numpy(ctx, nz, lam):
    import ganleaks_amd as gl
    rng = np.random.default_rng(nz * 100 + lam)
    nq = 5
    mu = rng.standard_normal((nq, nz)).astype(np.float32)
    logvar = rng.normal(0.0, 1.5, size=(nq, nz)).astype(np.float32)
    logvar[0] = 3.0                                                       # std = 20: the clamp bites
    mu[1, 0] = 7.5                                                        # and the mean itself is clamped
    std = np.exp(logvar)
    got = gl.recon_latents(mu, logvar, lam - 1, seed=(1 << 40) + 3, query_base=1000, z_max=4.0).numpy()
    want = rc.recon_latents(mu, std, lam, (1 << 40) + 3, 1000, 4.0)
    assert got.shape == (nq * lam, nz) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got.reshape(nq, lam, nz)[:, 0], np.clip(mu, -4.0, 4.0))
    if lam > 1:
        assert (np.abs(got.reshape(nq, lam, nz)[0, 1:]) == 4.0).any()
    # a split through query_base
    part = gl.recon_latents(mu[2:], logvar[2:], lam - 1, seed=(1 << 40) + 3, query_base=1002, z_max=4.0).numpy()
    assert np.array_equal(part, got.reshape(nq, lam, nz)[2:].reshape(-1, nz))
    assert gl.recon_latents(mu[:0], logvar[:0], lam - 1).shape == (0, nz)


@pytest.fixture(scope="module")
def model(synth):
    from ganleaks_amd.gan_models.vaegan.train import Encoder, Generator
    parent = Generator(NZ, d=D)
    parent.load_state_dict(synth.vaegan_state_dict(z_dim=NZ, d=D))
    view = parent.frozen(1)
    enc = Encoder(NZ)
    enc.load_state_dict(synth.vaegan_encoder_state_dict(778, NZ))
    z = synth.latent(61, 5, NZ).reshape(5, NZ)
    queries = synth.perturb_u8(62, view.generate_u8(z).numpy(), 6.0)
    return enc, view, queries


def test_recon_attack(model):
    import ganleaks_amd as gl
    from ganleaks_amd.attack import _dist32
    enc, view, q = model
    loss, dist_mu, S, z_mu = gl.recon_attack(q, enc, view, samples=3, seed=4, query_base=10)
    assert S.shape == (5, 4) and S.dtype == np.int64 and loss.dtype == np.float64 and dist_mu.dtype == np.float32 and z_mu.shape == (5, NZ)
    mu, logvar = enc.encode(q)
    lat = gl.recon_latents(mu, logvar, 3, seed=4, query_base=10)
    assert np.array_equal(z_mu, lat.numpy().reshape(5, 4, NZ)[:, 0]) and np.array_equal(z_mu, np.clip(mu, -4.0, 4.0))
    want = rc.group_S(q, view.generate_u8(lat).numpy(), 4)
    assert np.array_equal(S, want)
    d32 = _dist32(want, 3 * 64 * 64, "u8")
    assert np.array_equal(dist_mu, d32[:, 0]) and np.array_equal(loss, d32[:, 1:].astype(np.float64).mean(axis=1))
    # block_images and a split of the queries change nothing
    for kw in (dict(block_images=1), dict(block_images=9)):
        other = gl.recon_attack(q, enc, view, samples=3, seed=4, query_base=10, **kw)
        assert all(np.array_equal(a, b) for a, b in zip(other, (loss, dist_mu, S, z_mu)))
    a = gl.recon_attack(q[:2], enc, view, samples=3, seed=4, query_base=10)
    b = gl.recon_attack(q[2:], enc, view, samples=3, seed=4, query_base=12)
    assert all(np.array_equal(np.concatenate([x, y]), w) for x, y, w in zip(a, b, (loss, dist_mu, S, z_mu)))
    # no draws: the reconstruction at the mean alone
    l0, d0, S0, z0 = gl.recon_attack(q, enc, view, samples=0)
    assert S0.shape == (5, 1) and np.array_equal(S0[:, 0], S[:, 0]) and np.array_equal(l0, d0.astype(np.float64)) and np.array_equal(z0, z_mu)
    # floats on the lattice are the same queries
    assert np.array_equal(gl.recon_attack(rc.lattice(q), enc, view, samples=1, seed=4)[2], gl.recon_attack(q, enc, view, samples=1, seed=4)[2])


def test_z_mu_starts_the_white_box_attack(model):
    import ganleaks_amd as gl
    enc, view, q = model
    _, _, S, z_mu = gl.recon_attack(q, enc, view, samples=0)
    dist, z_star, S_wb, trace = gl.wb_attack(q, view, z_mu, steps=2, history=True)
    assert np.array_equal(trace[0], S[:, 0]) and (S_wb <= S[:, 0]).all()
