"""GPU: the white-box attack on PGGAN -- the generator's gradient with respect to z at a fixed depth (csrc/gl_pggan_grad.hip, Generator.at)
against float64 autograd of the same graph, and wb_attack on the inputs at which tests/test_wb_pggan_cpu.py shows descent to work on the host.

The bound on a gradient row is the rule of tests/test_gpu_wb.py: the same metric, |g - g64|_2 / |g64|_2, is measured for float32 torch autograd
of the graph on the CPU on the test's own inputs, its maximum over the rows is taken, and the device may be 4x that.  Every row is counted.
The cases are those of wb_pggan_common.CASES, at which no LeakyReLU unit is close enough to zero for float32 to flip its slope (asserted on the
CPU).  Measured on one MI355X: see the figures each test prints."""
import ctypes

import numpy as np
import pytest
import torch

import gpu_common  # noqa: F401
import wb_common as wc
import wb_pggan_common as wp

pytestmark = pytest.mark.gpu
_p = ctypes.c_void_p
_f = ctypes.c_float
SLACK = 4.0
_models = {}


@pytest.fixture(scope="module")
def gl():
    import ganleaks_amd
    return ganleaks_amd


def _make(gl, seed, nz, C):
    """(the generator under test with its default split-fp16 precision, one at precision 0, the float64 and the float32 host modules)"""
    key = (seed, nz, C)
    if key not in _models:
        from ganleaks_amd.gan_models.pggan.model_torch import Generator
        sd = gl.synth.pggan_state_dict(seed, nz, C)
        gen, gen0 = Generator(nz, C, 3), Generator(nz, C, 3)
        gen.load_state_dict(sd)
        gen0.load_state_dict(sd)
        gen0.set_precision(0)
        _models[key] = (gen, gen0, wp.PgganNet(sd), wp.PgganNet(sd, torch.float32))
    return _models[key]


@pytest.fixture(scope="module")
def small(gl):
    return _make(gl, 100, 64, 64)


@pytest.mark.parametrize("name,alpha", [(n, a) for n in sorted(wp.CASES) for a in wp.ALPHAS if a == 1.0 or wp.CASES[n][3] > 0])
def test_vjp_against_autograd(gl, name, alpha):
    seed, nz, C, steps, n, _, chunk = wp.CASES[name]
    gen, gen0, net64, net32 = _make(gl, seed, nz, C)
    R = 4 * 2 ** steps
    z = wp.case_latents(name)
    cot = np.random.default_rng(900 + steps).standard_normal((n, 3, R, R)).astype(np.float32)
    g64, _ = wp.vjp_z(net64, z, cot, steps, alpha)
    g32, _ = wp.vjp_z(net32, z, cot, steps, alpha)
    ref = wc.row_errors(g32, g64)
    view = gen.at(steps, alpha)
    before = view.generate_u8(z).numpy()
    try:
        if chunk:
            gen.set_chunk(chunk)
        grad, out = view.vjp_z(z, cot)
        grad, out = grad.numpy(), out.numpy()
        after = view.generate_u8(z).numpy()
    finally:
        gen.set_chunk(0)
    out0 = gen0.forward(z.reshape(n, nz, 1, 1), steps, alpha)
    err = wc.row_errors(grad, g64)
    print("vjp_z %s alpha=%s: float32 autograd max %.3e, device rows %s max %.3e, ratio %.2f, bound %.3e"
          % (name, alpha, ref.max(), err, err.max(), err.max() / ref.max(), SLACK * ref.max()))
    assert grad.shape == (n, nz) and grad.dtype == np.float32 and np.isfinite(grad).all() and out.shape == (n, 3, R, R)
    assert (err <= SLACK * ref.max()).all()
    assert np.array_equal(out.view(np.uint32), out0.view(np.uint32))      # the fp32-product forward's output: keep mode moves no bit
    assert gen._precision == 1 and np.array_equal(after, before)          # the precision found before the call is there after it
    assert np.array_equal(view.generate_u8(z).numpy(), before)


@pytest.mark.parametrize("steps,alpha", [(2, 0.4)])
def test_l2_grad_against_autograd(gl, small, steps, alpha):
    gen, gen0, net64, net32 = small
    view = gen.at(steps, alpha)
    z = wp.case_latents("steps2_chunk2")                                               # 5 latents that flip no slope at steps <= 2
    targets = view.generate_u8(np.random.default_rng(62).standard_normal((5, 64)).astype(np.float32)).numpy()
    targets[3] = view.generate_u8(z[3:4]).numpy()[0]                                   # G(z) quantised: a small, finite gradient
    g64, l64 = wp.l2_grad_z(net64, z, targets, steps, alpha)
    g32, l32 = wp.l2_grad_z(net32, z, targets, steps, alpha)
    ref_g, ref_l = wc.row_errors(g32, g64), np.abs(l32.astype(np.float64) - l64) / l64
    grad, loss = view.l2_grad_z(z, targets)
    grad, loss = grad.numpy(), loss.numpy()
    err_g, err_l = wc.row_errors(grad, g64), np.abs(loss.astype(np.float64) - l64) / l64
    print("l2_grad_z steps=%d: float32 autograd rows %s max %.3e, device rows %s" % (steps, ref_g, ref_g.max(), err_g))
    print("loss: float32 rows %s max %.3e, device rows %s" % (ref_l, ref_l.max(), err_l))
    assert grad.dtype == np.float32 and grad.shape == (5, 64) and loss.dtype == np.float32 and loss.shape == (5,)
    assert np.isfinite(grad).all() and np.isfinite(loss).all()
    assert 0 < np.abs(grad[3]).max() < np.abs(grad[0]).max()
    assert (err_g <= SLACK * ref_g.max()).all()
    assert (err_l <= SLACK * ref_l.max()).all()


def test_gradient_rows_do_not_depend_on_the_batch(gl, small):
    gen = small[0]
    view = gen.at(2, 0.4)
    rng = np.random.default_rng(64)
    z = rng.standard_normal((5, 64)).astype(np.float32)
    targets = view.generate_u8(rng.standard_normal((5, 64)).astype(np.float32)).numpy()
    cot = rng.standard_normal((5, 3, 16, 16)).astype(np.float32)
    bits = lambda pair: [a.numpy().view(np.uint32) for a in pair]        # noqa: E731
    together, vjp = bits(view.l2_grad_z(z, targets)), bits(view.vjp_z(z, cot))
    parts = [bits(view.l2_grad_z(z[:2], targets[:2])), bits(view.l2_grad_z(z[2:], targets[2:]))]
    try:
        gen.set_chunk(2)
        chunked, vjp_chunked = bits(view.l2_grad_z(z, targets)), bits(view.vjp_z(z, cot))
    finally:
        gen.set_chunk(0)
    for k in (0, 1):
        assert np.array_equal(np.concatenate([parts[0][k], parts[1][k]]), together[k])
        assert np.array_equal(chunked[k], together[k]) and np.array_equal(vjp_chunked[k], vjp[k])
        assert np.array_equal(bits(view.vjp_z(z[3:], cot[3:]))[k], vjp[k][3:])


def gen_channels(s, in_channels=64):
    """output channels of block s (model_torch.py: factors 1, 1, 1, 1, 1/2, 1/4, ... from the initial block on)"""
    factors = [1, 1, 1, 1, 1 / 2, 1 / 4, 1 / 8, 1 / 16, 1 / 32]
    return int(in_channels * factors[s + 1])


def _source_constants(path, function):
    """the integer literals of one function of a csrc file, and the file's kKeepBytes in MiB: the caps below are read from the code under test"""
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gan-leaks_amd", "csrc", path)).read()
    body = text[text.index(function):]
    body = body[:body.index("\n}\n")]
    return body, int(re.search(r"kKeepBytes = (\d+)ull << 20", text).group(1))


def test_grid_stride_loop_wraps(gl, small):
    """17 images at 64 x 64 in ONE pass: pg_pn_grad_kernel is launched with at most 16384 workgroups of 4 waves, one wave per position, so at the two
    64 x 64 layers the second trip of its loop runs.  Rows do not depend on the pass (above): passes of 4 stay under the cap and must give the
    same bits"""
    gen = small[0]
    steps, n = 4, 17
    R = 4 << steps
    import re
    body, keep_mib = _source_constants("gl_pggan_grad.hip", "void launch_pn_grad(")
    blocks_cap = int(re.search(r"if \(blocks > (\d+)\) blocks = \1;", body).group(1))
    per_block = int(re.search(r"gl_ceil_div\(positions, (\d+)\)", body).group(1))
    wave_cap = blocks_cap * per_block                        # 16384 workgroups of 4 waves
    assert n * R * R > wave_cap and 4 * R * R <= wave_cap
    # the default pass holds all 17: grad_sizes() keeps hw^2 (C + 1) floats per layer -- two 4 x 4 layers of 64 channels, then two layers per block
    widths = [64, 64] + [c for s in range(steps) for c in (gen_channels(s),) * 2]
    grids = [4, 4] + [4 << (s + 1) for s in range(steps) for _ in (0, 1)]
    kept = sum(h * h * (c + 1) for h, c in zip(grids, widths))
    assert n * kept * 4 <= keep_mib << 20
    view = gen.at(steps, 0.4)
    rng = np.random.default_rng(65)
    z = rng.standard_normal((n, 64)).astype(np.float32)
    targets = view.generate_u8(rng.standard_normal((n, 64)).astype(np.float32)).numpy()
    cot = rng.standard_normal((n, 3, R, R)).astype(np.float32)
    bits = lambda pair: [a.numpy().view(np.uint32) for a in pair]        # noqa: E731
    together, vjp = bits(view.l2_grad_z(z, targets)), bits(view.vjp_z(z, cot))
    try:
        gen.set_chunk(4)
        chunked, vjp_chunked = bits(view.l2_grad_z(z, targets)), bits(view.vjp_z(z, cot))
    finally:
        gen.set_chunk(0)
    assert np.isfinite(together[0].view(np.float32)).all() and not np.array_equal(together[0][0], together[0][16])
    for k in (0, 1):
        assert np.array_equal(chunked[k], together[k]) and np.array_equal(vjp_chunked[k], vjp[k])


def test_search(gl, small):
    from ganleaks_amd.attack import _dist32
    gen = small[0]
    view = gen.at(2, 0.4)
    z_init, z_image = wc.search_latents(64)
    queries = view.generate_u8(z_image).numpy()
    start = wc.ssd(view.generate_u8(z_init).numpy(), queries)
    kw = dict(steps=wc.SEARCH_STEPS, lr=wc.SEARCH_LR, history=True)
    dist, z_star, S, trace = gl.wb_attack(queries, view, z_init, **kw)
    print("start", start.tolist(), "final", S.tolist())
    assert trace.dtype == np.int64 and trace.shape == (wc.SEARCH_STEPS + 1, 12) and S.dtype == np.int64 and dist.dtype == np.float32
    assert z_star.dtype == np.float32 and z_star.shape == (12, 64)
    assert (np.diff(trace, axis=0) <= 0).all() and np.array_equal(trace[0], start) and np.array_equal(trace[-1], S)
    assert np.array_equal(S, wc.ssd(view.generate_u8(z_star).numpy(), queries))
    assert np.array_equal(dist, _dist32(S, 3 * 16 * 16, "u8"))
    # the queries that are the image of their own start: S = 0 from the start, nothing is accepted
    assert (trace[:, 0::3] == 0).all() and np.array_equal(z_star[0::3], z_init[0::3])
    assert (start[2::3] > 0).all() and (2 * S[2::3] <= start[2::3]).all()
    # 12 queries as 5 + 5 + 2
    for a, b in zip(gl.wb_attack(queries, view, z_init, block_images=5, **kw), (dist, z_star, S, trace)):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError, match="shape"):
        gl.wb_attack(queries, gen.at(1), z_init, steps=1)


def test_never_above_the_full_black_box_score(gl, small):
    gen = small[0]
    view = gen.at(2)
    rng = np.random.default_rng(71)
    queries = view.generate_u8(rng.standard_normal((6, 64)).astype(np.float32)).numpy()
    z_bank = rng.standard_normal((130, 64)).astype(np.float32)
    z_init, _ = gl.pbb_init_from_bank(queries, view, z_bank, batch_size=64)
    fbb_dist, _ = gl.attack(queries, gl.GeneratedBank(view, z_bank), distance="l2", batch_size=64)
    dist, _, _ = gl.wb_attack(queries, view, z_init, steps=4)
    assert (dist <= fbb_dist).all() and (dist < fbb_dist).any()
    # the view is a generator for the partial-black-box search too, without generate_kwargs
    d_pbb, _, _ = gl.pbb_attack(queries, view, z_init, rounds=2, population=8)
    assert (d_pbb <= fbb_dist).all()


def test_refusals(gl, small):
    from ganleaks_amd._lib import check
    from ganleaks_amd.gan_models.pggan.model_torch import Generator
    ctx = gl.Context.get()
    lib = ctx.lib
    gen = small[0]
    h = gen._handle
    one = _f(1.0)
    z, t = ctx.to_device(np.zeros((2, 64), np.float32)), ctx.to_device(np.zeros((2, 3, 4, 4), np.uint8))
    cot, grad, loss = ctx.zeros((2, 3, 4, 4), np.float32), ctx.empty((2, 64), np.float32), ctx.empty((2,), np.float32)
    check(lib.gl_pggan_vjp_z(h, _p(0), 0, 0, one, _p(0), _p(0), _p(0)))
    check(lib.gl_pggan_l2_grad_z(h, _p(0), _p(0), 0, 0, one, _p(0), _p(0)))
    for call in (lambda: lib.gl_pggan_vjp_z(h, _p(z.ptr), 2, 0, one, _p(0), _p(grad.ptr), _p(0)),
                 lambda: lib.gl_pggan_vjp_z(h, _p(z.ptr), 2, 0, one, _p(cot.ptr), _p(0), _p(0)),
                 lambda: lib.gl_pggan_vjp_z(None, _p(z.ptr), 2, 0, one, _p(cot.ptr), _p(grad.ptr), _p(0)),
                 lambda: lib.gl_pggan_l2_grad_z(h, _p(0), _p(t.ptr), 2, 0, one, _p(grad.ptr), _p(loss.ptr)),
                 lambda: lib.gl_pggan_l2_grad_z(h, _p(z.ptr), _p(t.ptr), 2, 0, one, _p(grad.ptr), _p(0)),
                 lambda: lib.gl_pggan_l2_grad_z(h, _p(z.ptr), _p(t.ptr), -1, 0, one, _p(grad.ptr), _p(loss.ptr)),
                 lambda: lib.gl_pggan_l2_grad_z(h, _p(z.ptr), _p(t.ptr), 2, 9, one, _p(grad.ptr), _p(loss.ptr)),
                 # block 4 has 32 -> 16 channels at in_channels = 64: the depth the forward refuses
                 lambda: lib.gl_pggan_l2_grad_z(h, _p(z.ptr), _p(t.ptr), 2, 5, one, _p(grad.ptr), _p(loss.ptr)),
                 lambda: lib.gl_pggan_vjp_z(h, _p(z.ptr), 2, 5, one, _p(cot.ptr), _p(grad.ptr), _p(0))):
        with pytest.raises(gl.GanLeaksError) as e:
            check(call())
        assert e.value.code == -1
    with pytest.raises(gl.GanLeaksError, match="channels"):
        gen.forward(np.zeros((2, 64, 1, 1), np.float32), 5, 1.0)
    # an unloaded block: only the initial block and its toRGB are there
    sd = gl.synth.pggan_state_dict(100, 64, 64)
    part = Generator(64, 64, 3)
    a = lambda k: np.ascontiguousarray(sd[k], np.float32).ctypes.data_as(_p)      # noqa: E731
    check(lib.gl_pggan_set_initial(part._ensure(), a("initial.1.weight"), a("initial.1.bias"), a("initial.3.conv.weight"), a("initial.3.bias")))
    check(lib.gl_pggan_set_rgb(part._handle, 0, a("initial_rgb.conv.weight"), a("initial_rgb.bias")))
    check(lib.gl_pggan_set_rgb(part._handle, 1, a("rgb_layers.1.conv.weight"), a("rgb_layers.1.bias")))
    empty = Generator(64, 64, 3)
    t8, cot8 = ctx.to_device(np.zeros((2, 3, 8, 8), np.uint8)), ctx.zeros((2, 3, 8, 8), np.float32)
    for call in (lambda: lib.gl_pggan_l2_grad_z(part._handle, _p(z.ptr), _p(t8.ptr), 2, 1, one, _p(grad.ptr), _p(loss.ptr)),
                 lambda: lib.gl_pggan_vjp_z(part._handle, _p(z.ptr), 2, 1, one, _p(cot8.ptr), _p(grad.ptr), _p(0)),
                 lambda: lib.gl_pggan_vjp_z(empty._ensure(), _p(z.ptr), 2, 0, one, _p(cot.ptr), _p(grad.ptr), _p(0))):
        with pytest.raises(gl.GanLeaksError, match="not loaded") as e:
            check(call())
        assert e.value.code == -4
    check(lib.gl_pggan_l2_grad_z(part._handle, _p(z.ptr), _p(t.ptr), 2, 0, one, _p(grad.ptr), _p(loss.ptr)))     # depth 0 is complete
    with pytest.raises(RuntimeError, match="load_state_dict"):
        empty.at(0).l2_grad_z(np.zeros((2, 64), np.float32), np.zeros((2, 3, 4, 4), np.uint8))
