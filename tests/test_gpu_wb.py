"""GPU: the white-box attack -- the generator's gradient with respect to z (csrc/gl_dcgan_grad.hip) against float64 autograd of the same
graph, the Adam step (csrc/gl_wb.hip) bit for bit against numpy float32, and wb_attack (ganleaks_amd/wb.py) on the inputs at which
tests/test_wb_cpu.py shows descent to work on the host.

The bound on a gradient row is not a chosen number: the same metric, |g - g64|_2 / |g64|_2, is measured for float32 torch autograd of the
graph on the CPU (the reference's arithmetic class) on the test's own inputs, its maximum over the rows is taken, and the device may be 4x
that (another summation order, fp32 accumulation in the matrix cores).  Every row is counted.  Measured on one MI355X:
see the figures each test prints."""
import ctypes

import numpy as np
import pytest
import torch

import gpu_common  # noqa: F401
import wb_common as wc

pytestmark = pytest.mark.gpu
_p = ctypes.c_void_p
_f = ctypes.c_float
SLACK = 4.0


@pytest.fixture(scope="module")
def gl():
    import ganleaks_amd
    return ganleaks_amd


def _make(gl, z_dim, fg, seed):
    from ganleaks_amd.gan_models.dcgan.model_torch import Generator
    sd = gl.synth.dcgan_state_dict(seed, z_dim=z_dim, features_g=fg)
    gen, gen0 = Generator(z_dim, 3, fg), Generator(z_dim, 3, fg)
    gen.load_state_dict(sd)
    gen0.load_state_dict(sd)
    gen0.set_precision(0)
    return gen, gen0, wc.dcgan_module(sd), wc.dcgan_module(sd, torch.float32)


@pytest.fixture(scope="module")
def small(gl):
    """Generator(100, 3, 16): z_pad = 128 > z_dim, channels 256 / 128 / 64 / 32; (the generator under test with its default split-fp16
    precision, one at precision 0 for comparison, the float64 and the float32 host modules)"""
    return _make(gl, 100, 16, 1234)


@pytest.fixture(scope="module")
def wide(gl):
    """Generator(64, 3, 32): z_dim a multiple of 32, 512 channels in the first layer, a 64-channel last layer (the fused tail at precision 1)"""
    return _make(gl, 64, 32, 77)


def _check_vjp(gl, models, n, chunk, seed):
    gen, gen0, net64, net32 = models
    nz = gen.z_dim
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, nz)).astype(np.float32)
    cot = rng.standard_normal((n, 3, 64, 64)).astype(np.float32)
    g64, _ = wc.vjp_z(net64, z, cot)
    g32, _ = wc.vjp_z(net32, z, cot)
    ref = wc.row_errors(g32, g64)
    before = gen.generate_u8(z).numpy()
    try:
        if chunk:
            gen.set_chunk(chunk)
            gen0.set_chunk(chunk)
        grad, out = gen.vjp_z(z, cot, want_output=True)
        grad, out = grad.numpy(), out.numpy()
        after = gen.generate_u8(z).numpy()
        out0 = gen0.forward(z.reshape(n, nz, 1, 1))
    finally:
        gen.set_chunk(0)
        gen0.set_chunk(0)
    err = wc.row_errors(grad, g64)
    print("vjp_z n=%d chunk=%s nz=%d: float32 autograd max %.3e, device rows %s, bound %.3e" % (n, chunk, nz, ref.max(), err, SLACK * ref.max()))
    assert grad.shape == (n, nz) and np.isfinite(grad).all()
    assert (err <= SLACK * ref.max()).all()
    assert np.array_equal(out, out0)                       # the fp32-product forward's output
    assert np.array_equal(after, before)                   # precision, fuse_tail and chunk are as they were
    assert np.array_equal(gen.generate_u8(z).numpy(), before)


@pytest.mark.parametrize("n,chunk", [(1, 0), (3, 0), (5, 2)])
def test_vjp_against_autograd(gl, small, n, chunk):
    _check_vjp(gl, small, n, chunk, 500 + n)


def test_vjp_wide_generator(gl, wide):
    _check_vjp(gl, wide, 2, 0, 510)


def test_l2_grad_against_autograd(gl, small):
    gen, gen0, net64, net32 = small
    z = gl.synth.latent(61, 6).reshape(6, 100)
    targets = gen.generate_u8(gl.synth.latent(62, 6)).numpy()
    targets[3] = gen.generate_u8(z[3:4]).numpy()[0]                                     # G(z) quantised: a small, finite gradient
    targets[4:] = gen.generate_u8(z[4:] + np.float32(0.2) * gl.synth.latent(63, 2).reshape(2, 100)).numpy()
    g64, l64 = wc.l2_grad_z(net64, z, targets)
    g32, l32 = wc.l2_grad_z(net32, z, targets)
    ref_g, ref_l = wc.row_errors(g32, g64), np.abs(l32.astype(np.float64) - l64) / l64
    grad, loss = gen.l2_grad_z(z, targets)
    grad, loss = grad.numpy(), loss.numpy()
    err_g, err_l = wc.row_errors(grad, g64), np.abs(loss.astype(np.float64) - l64) / l64
    print("l2_grad_z: float32 autograd rows %s max %.3e, device rows %s" % (ref_g, ref_g.max(), err_g))
    print("loss: float32 rows %s max %.3e, device rows %s" % (ref_l, ref_l.max(), err_l))
    assert grad.dtype == np.float32 and grad.shape == (6, 100) and loss.shape == (6,)
    assert np.isfinite(grad).all() and np.isfinite(loss).all() and 0 < np.abs(grad[3]).max() < np.abs(grad[0]).max()
    assert (err_g <= SLACK * ref_g.max()).all()
    assert (err_l <= SLACK * ref_l.max()).all()


def test_gradient_rows_do_not_depend_on_the_batch(gl, small):
    gen = small[0]
    z = gl.synth.latent(64, 5).reshape(5, 100)
    targets = gen.generate_u8(gl.synth.latent(65, 5)).numpy()
    cot = np.random.default_rng(66).standard_normal((5, 3, 64, 64)).astype(np.float32)
    bits = lambda pair: [a.numpy().view(np.uint32) for a in pair]        # noqa: E731
    together = bits(gen.l2_grad_z(z, targets))
    parts = [bits(gen.l2_grad_z(z[:2], targets[:2])), bits(gen.l2_grad_z(z[2:], targets[2:]))]
    vjp = gen.vjp_z(z, cot).numpy().view(np.uint32)
    try:
        gen.set_chunk(2)
        chunked = bits(gen.l2_grad_z(z, targets))
        vjp_chunked = gen.vjp_z(z, cot).numpy().view(np.uint32)
    finally:
        gen.set_chunk(0)
    for k in (0, 1):
        assert np.array_equal(np.concatenate([parts[0][k], parts[1][k]]), together[k])
        assert np.array_equal(chunked[k], together[k])
    assert np.array_equal(vjp_chunked, vjp) and np.array_equal(gen.vjp_z(z[3:], cot[3:]).numpy().view(np.uint32), vjp[3:])


def test_adam_step_bit_for_bit(gl):
    from ganleaks_amd._lib import check
    ctx = gl.Context.get()
    rng = np.random.default_rng(8)
    nq, nz = 7, 33                                                       # 231 values: no multiple of the 256 threads of a workgroup
    z = rng.standard_normal((nq, nz)).astype(np.float32)
    z[2, 4] = 3.99
    m, v = np.zeros_like(z), np.zeros_like(z)
    zd, md, vd = ctx.to_device(z), ctx.to_device(m), ctx.to_device(v)
    lr, b1, b2, eps, z_max = 0.5, 0.9, 0.999, 1e-8, 4.0
    for t in (1, 2, 3):
        g = (rng.standard_normal((nq, nz)) * 10.0 ** rng.integers(-3, 4, size=(nq, 1))).astype(np.float32)
        g[:, 5] = 0.0                                                    # a column without gradient
        g[2, 4] = -1e15                                                  # a huge gradient: 3.99 + 0.5 runs into z_max
        c1, c2 = wc.bias_corrections(b1, b2, t)
        z, m, v = wc.adam_step(z, m, v, g, lr, b1, b2, eps, c1, c2, z_max)
        gd = ctx.to_device(g)
        check(ctx.lib.gl_wb_adam_step(ctx.handle, _p(zd.ptr), _p(md.ptr), _p(vd.ptr), _p(gd.ptr), nq, nz, _f(lr), _f(b1), _f(b2), _f(eps), _f(c1), _f(c2),
                                      _f(z_max)))
        for name, dev, want in (("z", zd, z), ("m", md, m), ("v", vd, v)):
            assert np.array_equal(dev.numpy().view(np.uint32), want.view(np.uint32)), (name, t)
    assert z[2, 4] == np.float32(4.0) and np.abs(z).max() <= 4.0 and np.isfinite(v).all()
    # nothing to do, and what is refused
    check(ctx.lib.gl_wb_adam_step(ctx.handle, _p(0), _p(0), _p(0), _p(0), 0, nz, _f(lr), _f(b1), _f(b2), _f(eps), _f(1.0), _f(1.0), _f(z_max)))
    for bad in (dict(lr=0.0), dict(b1=1.0), dict(c1=float("nan")), dict(z_max=0.0)):
        a = dict(lr=lr, b1=b1, b2=b2, eps=eps, c1=1.0, c2=1.0, z_max=z_max)
        a.update(bad)
        with pytest.raises(gl.GanLeaksError):
            check(ctx.lib.gl_wb_adam_step(ctx.handle, _p(zd.ptr), _p(md.ptr), _p(vd.ptr), _p(gd.ptr), nq, nz, _f(a["lr"]), _f(a["b1"]), _f(a["b2"]),
                                          _f(a["eps"]), _f(a["c1"]), _f(a["c2"]), _f(a["z_max"])))
    with pytest.raises(gl.GanLeaksError, match="NULL"):
        check(ctx.lib.gl_wb_adam_step(ctx.handle, _p(zd.ptr), _p(0), _p(vd.ptr), _p(gd.ptr), nq, nz, _f(lr), _f(b1), _f(b2), _f(eps), _f(1.0), _f(1.0),
                                      _f(z_max)))


def test_search(gl, small):
    from ganleaks_amd.attack import _dist32
    gen = small[0]
    z_init, z_image = wc.search_latents()
    queries = gen.generate_u8(z_image).numpy()
    start = wc.ssd(gen.generate_u8(z_init).numpy(), queries)
    kw = dict(steps=wc.SEARCH_STEPS, lr=wc.SEARCH_LR, history=True)
    dist, z_star, S, trace = gl.wb_attack(queries, gen, z_init, **kw)
    print("start", start.tolist(), "final", S.tolist())
    assert trace.dtype == np.int64 and trace.shape == (wc.SEARCH_STEPS + 1, 12) and S.dtype == np.int64 and dist.dtype == np.float32
    assert z_star.dtype == np.float32 and z_star.shape == (12, 100)
    assert (np.diff(trace, axis=0) <= 0).all() and np.array_equal(trace[0], start) and np.array_equal(trace[-1], S)
    assert np.array_equal(S, wc.ssd(gen.generate_u8(z_star).numpy(), queries))
    assert np.array_equal(dist, _dist32(S, 12288, "u8"))
    # the queries that are the image of their own start: S = 0 from the start, nothing is accepted
    assert (trace[:, 0::3] == 0).all() and np.array_equal(z_star[0::3], z_init[0::3])
    assert (start[2::3] > 0).all() and (2 * S[2::3] <= start[2::3]).all()
    # 12 queries as 5 + 5 + 2
    for a, b in zip(gl.wb_attack(queries, gen, z_init, block_images=5, **kw), (dist, z_star, S, trace)):
        assert np.array_equal(a, b)
    # steps = 0 returns the start; history off returns three values
    d0, z0, S0 = gl.wb_attack(queries, gen, z_init.reshape(12, 100, 1, 1), steps=0)
    assert np.array_equal(S0, start) and np.array_equal(z0, z_init) and np.array_equal(d0, _dist32(start, 12288, "u8"))
    with pytest.raises(ValueError, match="lattice"):
        gl.wb_attack(np.full((12, 3, 64, 64), 0.123, np.float32), gen, z_init, steps=1)


def test_never_above_the_full_black_box_score(gl, small):
    gen = small[0]
    queries = gen.generate_u8(gl.synth.latent(71, 6)).numpy()
    z_bank = gl.synth.latent(72, 130).reshape(130, 100)
    z_init, _ = gl.pbb_init_from_bank(queries, gen, z_bank, batch_size=64)
    fbb_dist, _ = gl.attack(queries, gl.GeneratedBank(gen, z_bank), distance="l2", batch_size=64)
    dist, _, _ = gl.wb_attack(queries, gen, z_init, steps=4)
    assert (dist <= fbb_dist).all() and (dist < fbb_dist).any()


def test_refusals(gl, small):
    from ganleaks_amd._lib import check
    from ganleaks_amd.gan_models.dcgan.model_torch import Generator
    from ganleaks_amd.gan_models.pggan.model_torch import Generator as PgganGenerator
    from ganleaks_amd.gan_models.vaegan.train import Generator as VaeganGenerator
    ctx = gl.Context.get()
    lib = ctx.lib
    q = np.zeros((2, 3, 64, 64), np.uint8)
    pg = PgganGenerator(64, 64, 3)
    pg.load_state_dict(gl.synth.pggan_state_dict(100, 64, 64))
    with pytest.raises(NotImplementedError, match="l2_grad_z"):
        gl.wb_attack(q, pg, np.zeros((2, 64), np.float32))
    with pytest.raises(NotImplementedError, match="VAEGAN"):
        gl.wb_attack(q, VaeganGenerator(100), np.zeros((2, 100), np.float32))
    # the C calls: nothing to do, NULL pointers, unloaded weights, a spectrally normalised layer
    gen = small[0]
    z, t = ctx.to_device(np.zeros((2, 100), np.float32)), ctx.to_device(q)
    cot, grad, loss = ctx.zeros((2, 3, 64, 64), np.float32), ctx.empty((2, 100), np.float32), ctx.empty((2,), np.float32)
    check(lib.gl_dcgan_vjp_z(gen._handle, _p(0), 0, _p(0), _p(0), _p(0)))
    check(lib.gl_dcgan_l2_grad_z(gen._handle, _p(0), _p(0), 0, _p(0), _p(0)))
    for call in (lambda: lib.gl_dcgan_vjp_z(gen._handle, _p(z.ptr), 2, _p(0), _p(grad.ptr), _p(0)),
                 lambda: lib.gl_dcgan_vjp_z(gen._handle, _p(z.ptr), 2, _p(cot.ptr), _p(0), _p(0)),
                 lambda: lib.gl_dcgan_vjp_z(None, _p(z.ptr), 2, _p(cot.ptr), _p(grad.ptr), _p(0)),
                 lambda: lib.gl_dcgan_l2_grad_z(gen._handle, _p(0), _p(t.ptr), 2, _p(grad.ptr), _p(loss.ptr)),
                 lambda: lib.gl_dcgan_l2_grad_z(gen._handle, _p(z.ptr), _p(t.ptr), 2, _p(grad.ptr), _p(0)),
                 lambda: lib.gl_dcgan_l2_grad_z(gen._handle, _p(z.ptr), _p(t.ptr), -1, _p(grad.ptr), _p(loss.ptr))):
        with pytest.raises(gl.GanLeaksError) as e:
            check(call())
        assert e.value.code == -1
    empty = Generator(100, 3, 16)
    with pytest.raises(gl.GanLeaksError, match="not loaded") as e:
        check(lib.gl_dcgan_l2_grad_z(empty._ensure(), _p(z.ptr), _p(t.ptr), 2, _p(grad.ptr), _p(loss.ptr)))
    assert e.value.code == -4
    with pytest.raises(RuntimeError, match="load_state_dict"):
        empty.l2_grad_z(np.zeros((2, 100), np.float32), q)
    sn = Generator(100, 3, 16)
    sd = gl.synth.dcgan_state_dict(1234, features_g=16)
    sn.load_state_dict(sd)
    w = np.ascontiguousarray(sd["gen.0.0.weight"], np.float32)
    rng = np.random.default_rng(1)
    u, v = rng.standard_normal(100).astype(np.float32), rng.standard_normal(256 * 16).astype(np.float32)
    ones, zeros = np.ones(256, np.float32), np.zeros(256, np.float32)
    check(lib.gl_dcgan_set_spectral_norm(sn._handle, 0, w.ctypes.data_as(_p), u.ctypes.data_as(_p), v.ctypes.data_as(_p), ones.ctypes.data_as(_p),
                                         zeros.ctypes.data_as(_p), 1))
    for call in (lambda: sn.l2_grad_z(np.zeros((2, 100), np.float32), q), lambda: sn.vjp_z(np.zeros((2, 100), np.float32), cot)):
        with pytest.raises(gl.GanLeaksError, match="spectral") as e:
            call()
        assert e.value.code == -4
