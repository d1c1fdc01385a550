"""GPU: the white-box attack under 0.2 * LPIPS + L2 -- the image gradient of the distance (csrc/gl_lpips_grad.hip, LpipsModel.grad_image)
and the latent gradient through generator and VGG16 (pair_grad_z) against float64 autograd of the same graphs, and pair_wb_attack on the
inputs at which tests/test_wb_lpips_cpu.py shows descent to work on the host.

The bound on a gradient row is the rule of tests/test_gpu_wb.py: the same metric, |g - g64|_2 / |g64|_2, is measured for float32 torch
autograd of the graph on the CPU on the test's own inputs, its maximum over the rows is taken, and the device may be 4x that; likewise the
relative error of the loss.  Every row is counted.  The cases are those of wb_lpips_common, at which no ReLU unit is close enough to zero for
float32 to move it across, no tap position is all zero and no max-pool cell has tied positive maxima (asserted on the CPU).  Measured on one
MI355X: see the figures each test prints."""
import ctypes
import os

import numpy as np
import pytest

import gpu_common  # noqa: F401
import wb_common as wc
import wb_lpips_common as wl

pytestmark = pytest.mark.gpu
_p = ctypes.c_void_p
SLACK = 4.0


@pytest.fixture(scope="module")
def gl():
    import ganleaks_amd
    return ganleaks_amd


@pytest.fixture(scope="module")
def model(gl, synth):
    from ganleaks_amd.lpips import LpipsModel
    return LpipsModel().load_state_dicts(synth.vgg16_state_dict(7), wl.lin_weights())


@pytest.fixture(scope="module")
def pggan(gl, synth):
    from ganleaks_amd.gan_models.pggan.model_torch import Generator
    gen = Generator(wl.PGGAN_SD[1], wl.PGGAN_SD[2], 3)
    gen.load_state_dict(synth.pggan_state_dict(*wl.PGGAN_SD))
    return gen


def _rows(a):
    return np.asarray(a).reshape(len(a), -1)


def _bits(pair):
    return [a.numpy().view(np.uint32) for a in pair]


@pytest.mark.parametrize("name", sorted(wl.IMAGE_CASES))
def test_grad_image_against_float64(synth, model, name):
    targets, y = wl.image_case(synth, name)
    n64, n32 = wl.vgg_nets(synth)
    g64, l64 = wl.grad_image(n64, y, targets)
    g32, l32 = wl.grad_image(n32, y, targets)
    ref_g, ref_l = wc.row_errors(_rows(g32), _rows(g64)), np.abs(l32.astype(np.float64) - l64) / l64
    before = model.features(targets).V.numpy()
    cot, loss = model.grad_image(y, targets)
    cot, loss = cot.numpy(), loss.numpy()
    err_g, err_l = wc.row_errors(_rows(cot), _rows(g64)), np.abs(loss.astype(np.float64) - l64) / l64
    print("grad_image %s: float32 autograd rows %s max %.3e, device rows %s max %.3e, ratio %.2f, bound %.3e"
          % (name, ref_g, ref_g.max(), err_g, err_g.max(), err_g.max() / ref_g.max(), SLACK * ref_g.max()))
    print("loss %s: float32 rows %s max %.3e, device rows %s, ratio %.2f" % (name, ref_l, ref_l.max(), err_l, err_l.max() / ref_l.max()))
    assert cot.shape == y.shape and cot.dtype == np.float32 and loss.shape == (len(y),) and loss.dtype == np.float32
    assert np.isfinite(cot).all() and np.isfinite(loss).all()
    assert (err_g <= SLACK * ref_g.max()).all()
    assert (err_l <= SLACK * ref_l.max()).all()
    # precision, calibration and chunk are what they were: the split-fp16 forward gives the bits it gave before
    assert model._precision == 1 and np.array_equal(model.features(targets).V.numpy().view(np.uint32), before.view(np.uint32))


def test_rows_do_not_depend_on_the_batch(synth, model):
    """bit for bit: a pass of 2 against the default pass, reference rows handed over against computed in the call, a row alone against the
    row inside a call of 5"""
    targets = np.ascontiguousarray(synth.lowpass_u8_images(6, 5, res=16))
    x = (2.0 * (targets.astype(np.float64) / 255.0) - 1.0).astype(np.float32)
    y = np.clip(x + np.float32(0.1) * np.random.default_rng(12).standard_normal(x.shape).astype(np.float32), -1.0, 1.0).astype(np.float32)
    together = _bits(model.grad_image(y, targets))
    try:
        model.set_chunk(2)
        chunked = _bits(model.grad_image(y, targets))
        ref_chunked = model.reference_rows(targets).numpy().view(np.uint32)
    finally:
        model.set_chunk(0)
    ref = model.reference_rows(targets)
    assert ref.shape == (5, model.ctx.lib.gl_lpips_ref_dim(16, 16)) and np.array_equal(ref.numpy().view(np.uint32), ref_chunked)
    given = _bits(model.grad_image(y, targets, ref))
    for k in (0, 1):
        assert np.array_equal(chunked[k], together[k]) and np.array_equal(given[k], together[k])
        for i in (0, 3, 4):
            assert np.array_equal(_bits(model.grad_image(y[i:i + 1], targets[i:i + 1]))[k], together[k][i:i + 1])
    with pytest.raises(ValueError, match="reference_rows"):
        model.grad_image(y[:2], targets[:2], ref)


def test_grid_stride_loops_wrap(synth, model):
    """65 images at 64 x 64 in ONE pass: the wave-per-position kernels (conv1_1, the reference rows, the activation gradients, conv1_1 backwards)
    are launched with at most 16384 workgroups of 4 waves and the max-pool with at most 4096 workgroups of 256 threads, one float4 each, so here
    the second trip of their grid-stride loops runs.  Rows do not depend on the pass (above), so the same call in passes of 8 -- whose launches
    stay under both caps -- must give the same bits; so must the reference rows"""
    n, H, W = 65, 64, 64
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gan-leaks_amd", "csrc", "gl_lpips_grad.hip")).read()
    wb = src[src.index("unsigned wave_blocks("):]
    wb = wb[:wb.index("\n}\n")]
    mp = src[src.index("void launch_maxpool("):]
    mp = mp[:mp.index("\n}\n")]
    # the caps as the code under test has them: 16384 workgroups of 4 waves, 4096 workgroups of kThreads = 256 items
    wave_cap = int(re.search(r"b > (\d+) \? \1 : b", wb).group(1)) * int(re.search(r"gl_ceil_div\(positions, (\d+)\)", wb).group(1))
    pool_cap = int(re.search(r"if \(blocks > (\d+)\) blocks = \1;", mp).group(1)) * int(re.search(r"constexpr int kThreads = (\d+);", src).group(1))
    keep_mib = int(re.search(r"kKeepBytes = (\d+)ull << 20", src).group(1))
    assert (wave_cap, pool_cap) == (16384 * 4, 4096 * 256)     # what the sizes below were chosen for
    kept = sum(h * h * c for h, c in ((64, 64), (64, 64), (32, 64), (32, 128), (32, 128), (16, 128), (16, 256), (16, 256), (16, 256), (8, 256),
                                      (8, 512), (8, 512), (8, 512), (4, 512), (4, 512), (4, 512), (4, 512)))      # the 13 outputs and the 4 pools
    assert n * kept * 4 < keep_mib << 20                       # the default pass holds all of them (kKeepBytes)
    assert n * H * W > wave_cap and n * (H // 2) * (W // 2) > wave_cap       # conv1_1, conv1_2 and the first tap; conv2_x: 66 560 positions
    assert n * (H // 2) * (W // 2) * (64 // 4) > pool_cap      # the first max-pool's float4 items
    assert 8 * H * W <= wave_cap and 8 * (H // 2) * (W // 2) * (64 // 4) <= pool_cap
    targets = np.ascontiguousarray(synth.lowpass_u8_images(8, n, res=64))
    x = (2.0 * (targets.astype(np.float64) / 255.0) - 1.0).astype(np.float32)
    y = np.clip(x + np.float32(0.1) * np.random.default_rng(13).standard_normal(x.shape).astype(np.float32), -1.0, 1.0).astype(np.float32)
    together = _bits(model.grad_image(y, targets))
    ref = model.reference_rows(targets).numpy().view(np.uint32)
    try:
        model.set_chunk(8)
        chunked = _bits(model.grad_image(y, targets))
        ref_chunked = model.reference_rows(targets).numpy().view(np.uint32)
    finally:
        model.set_chunk(0)
    assert np.isfinite(together[0].view(np.float32)).all() and np.isfinite(together[1].view(np.float32)).all()
    assert not np.array_equal(together[0][0], together[0][64])
    assert np.array_equal(together[0], chunked[0]) and np.array_equal(together[1], chunked[1])
    assert np.array_equal(ref, ref_chunked)


def test_all_lin_weights_zero(gl, synth):
    """without LPIPS the loss is the L2 term and the gradient 2 (y - x) / (3 H W): a failure here is in the tail, not in VGG16.  x is the
    float32 value of 2 u / 255 - 1, as the device forms it (against the exact x the difference of two close floats would carry x's rounding,
    6e-8, relative to a difference that may be 1e-3).  A gradient value is then a float32 difference, a float32 constant and a product --
    three roundings, 1.8e-7 -- and the loss a double sum of squares of such differences rounded once: 1e-6 covers both"""
    from ganleaks_amd.lpips import LpipsModel
    zero = LpipsModel().load_state_dicts(synth.vgg16_state_dict(7), {"lin%d" % i: np.zeros_like(v) for i, v in enumerate(wl.lin_weights().values())})
    targets, y = wl.image_case(synth, "32x16")
    cot, loss = zero.grad_image(y, targets)
    x32 = (2.0 * (targets.astype(np.float64) / 255.0) - 1.0).astype(np.float32)
    diff = y.astype(np.float64) - x32.astype(np.float64)
    assert np.allclose(cot.numpy(), 2.0 * diff / diff[0].size, rtol=1e-6, atol=0)
    assert np.allclose(loss.numpy(), (diff ** 2).reshape(len(y), -1).mean(axis=1), rtol=1e-6, atol=0)


def _generator(gl, synth, pggan, name):
    if name == "dcgan16":
        from ganleaks_amd.gan_models.dcgan.model_torch import Generator
        gen = Generator(100, 3, wl.DCGAN_SD["features_g"])
        gen.load_state_dict(synth.dcgan_state_dict(wl.DCGAN_SD["seed"], features_g=wl.DCGAN_SD["features_g"]))
        return gen, gen
    return pggan.at(2, float(name.split("_a")[1])), pggan


@pytest.mark.parametrize("name", sorted(wl.COMPOSED_CASES))
def test_pair_grad_z_against_autograd(gl, synth, model, pggan, name):
    c64, c32 = wl.composed_nets(synth, name)
    z, targets = wl.composed_case(c64, name)
    g64, l64 = c64.grad_z(z, targets)
    g32, l32 = c32.grad_z(z, targets)
    ref_g, ref_l = wc.row_errors(g32, g64), np.abs(l32.astype(np.float64) - l64) / l64
    gen, owner = _generator(gl, synth, pggan, name)
    before = gen.generate_u8(z).numpy()
    grad, loss = gl.pair_grad_z(gen, z, targets, model)
    grad, loss = grad.numpy(), loss.numpy()
    err_g, err_l = wc.row_errors(grad, g64), np.abs(loss.astype(np.float64) - l64) / l64
    print("pair_grad_z %s: float32 autograd rows %s max %.3e, device rows %s max %.3e, ratio %.2f, bound %.3e"
          % (name, ref_g, ref_g.max(), err_g, err_g.max(), err_g.max() / ref_g.max(), SLACK * ref_g.max()))
    print("loss %s: float32 rows %s max %.3e, device rows %s, ratio %.2f" % (name, ref_l, ref_l.max(), err_l, err_l.max() / ref_l.max()))
    assert grad.shape == z.shape and grad.dtype == np.float32 and loss.shape == (len(z),) and np.isfinite(grad).all() and np.isfinite(loss).all()
    assert (err_g <= SLACK * ref_g.max()).all()
    assert (err_l <= SLACK * ref_l.max()).all()
    assert owner._precision == 1 and np.array_equal(gen.generate_u8(z).numpy(), before)      # the generator's precision is what it was
    ref = model.reference_rows(targets)
    assert all(np.array_equal(a, b) for a, b in zip(_bits(gl.pair_grad_z(gen, z, targets, model, ref)), (grad.view(np.uint32), loss.view(np.uint32))))


def _pattern(dist):
    return np.ascontiguousarray(dist, np.float32).view(np.uint32).astype(np.int64)


def test_search(gl, model, pggan):
    view = pggan.at(wl.SEARCH_PG_STEPS, wl.SEARCH_ALPHA)
    z_init, z_image = wc.search_latents(wl.SEARCH_NZ)
    queries = view.generate_u8(z_image).numpy()
    kw = dict(steps=wl.SEARCH_STEPS, lr=wl.SEARCH_LR, history=True, lpips=model)
    dist, z_star, key, trace = gl.pair_wb_attack(queries, view, z_init, **kw)
    start = trace[0].astype(np.uint32).view(np.float32)
    print("start", start.tolist(), "final", dist.tolist(), "factor", (dist[2::3] / start[2::3]).tolist())
    assert trace.dtype == np.int64 and trace.shape == (wl.SEARCH_STEPS + 1, 12) and key.dtype == np.int64 and key.shape == (12,)
    assert dist.dtype == np.float32 and z_star.dtype == np.float32 and z_star.shape == (12, wl.SEARCH_NZ)
    assert (np.diff(trace, axis=0) <= 0).all() and np.array_equal(trace[-1], key) and (key >= 0).all()
    assert np.array_equal(_pattern(dist), key)
    # the key is the search's own distance between the query and the image of z_star, bit for bit
    images = view.generate_u8(z_star).numpy()
    recount = np.array([gl.pair_distances(queries[q:q + 1], images[q:q + 1], batch_size=1, lpips=model)[0, 0] for q in range(12)], np.float32)
    assert np.array_equal(_pattern(recount), key)
    first = np.array([gl.pair_distances(queries[q:q + 1], view.generate_u8(z_init[q:q + 1]).numpy(), batch_size=1, lpips=model)[0, 0]
                      for q in range(12)], np.float32)
    assert np.array_equal(_pattern(first), trace[0])
    # the displaced starts: the host restatement ends at 0.062 - 0.085 of the starting distance (tests/test_wb_lpips_cpu.py asserts a quarter)
    assert (start[2::3] > 0).all() and (2 * dist[2::3] <= start[2::3]).all()
    # 12 queries as 5 + 5 + 2
    for a, b in zip(gl.pair_wb_attack(queries, view, z_init, block_images=5, **kw), (dist, z_star, key, trace)):
        assert np.array_equal(a, b)
    # no steps: the start
    d0, z0, k0, t0 = gl.pair_wb_attack(queries, view, z_init, steps=0, history=True, lpips=model)
    assert np.array_equal(z0, z_init) and np.array_equal(k0, trace[0]) and np.array_equal(t0, trace[:1]) and np.array_equal(_pattern(d0), k0)
    with pytest.raises(ValueError, match="lattice"):
        gl.pair_wb_attack(queries.astype(np.float32) / 255.0 + np.float32(1e-3), view, z_init, steps=1, lpips=model)


def test_never_above_the_full_black_box_score(gl, model, pggan):
    view = pggan.at(2)
    rng = np.random.default_rng(71)
    queries = view.generate_u8(rng.standard_normal((6, 64)).astype(np.float32)).numpy()
    z_bank = rng.standard_normal((130, 64)).astype(np.float32)
    fbb_dist, idx = gl.attack(queries, gl.GeneratedBank(view, z_bank), distance="l2-lpips", batch_size=64, lpips=model)
    dist, _, key, trace = gl.pair_wb_attack(queries, view, z_bank[idx], steps=4, history=True, lpips=model)
    assert np.array_equal(trace[0], _pattern(fbb_dist))
    assert (dist <= fbb_dist).all() and (dist < fbb_dist).any()


def test_refusals(gl, model):
    from ganleaks_amd._lib import check
    from ganleaks_amd.lpips import LpipsModel
    ctx = gl.Context.get()
    lib = ctx.lib
    h = model._handle
    y, t = ctx.zeros((2, 3, 16, 16), np.float32), ctx.to_device(np.zeros((2, 3, 16, 16), np.uint8))
    cot, loss = ctx.empty((2, 3, 16, 16), np.float32), ctx.empty((2,), np.float32)
    ref = ctx.empty((2, lib.gl_lpips_ref_dim(16, 16)), np.float32)
    check(lib.gl_lpips_grad_image(h, _p(0), _p(0), _p(0), 0, 16, 16, _p(0), _p(0)))
    check(lib.gl_lpips_ref_rows_u8(h, _p(0), 0, 16, 16, _p(0)))
    check(lib.gl_wb_diag_keys(ctx.handle, _p(0), 0, 0, _p(0)))
    for call in (lambda: lib.gl_lpips_grad_image(h, _p(0), _p(t.ptr), _p(0), 2, 16, 16, _p(cot.ptr), _p(loss.ptr)),
                 lambda: lib.gl_lpips_grad_image(h, _p(y.ptr), _p(0), _p(0), 2, 16, 16, _p(cot.ptr), _p(loss.ptr)),
                 lambda: lib.gl_lpips_grad_image(h, _p(y.ptr), _p(t.ptr), _p(0), 2, 16, 16, _p(0), _p(loss.ptr)),
                 lambda: lib.gl_lpips_grad_image(h, _p(y.ptr), _p(t.ptr), _p(0), 2, 16, 16, _p(cot.ptr), _p(0)),
                 lambda: lib.gl_lpips_grad_image(None, _p(y.ptr), _p(t.ptr), _p(0), 2, 16, 16, _p(cot.ptr), _p(loss.ptr)),
                 lambda: lib.gl_lpips_grad_image(h, _p(y.ptr), _p(t.ptr), _p(0), -1, 16, 16, _p(cot.ptr), _p(loss.ptr)),
                 lambda: lib.gl_lpips_grad_image(h, _p(y.ptr), _p(t.ptr), _p(0), 2, 24, 16, _p(cot.ptr), _p(loss.ptr)),
                 lambda: lib.gl_lpips_ref_rows_u8(h, _p(t.ptr), 2, 16, 24, _p(ref.ptr)),
                 lambda: lib.gl_lpips_ref_rows_u8(h, _p(0), 2, 16, 16, _p(ref.ptr)),
                 lambda: lib.gl_lpips_ref_rows_u8(h, _p(t.ptr), 2, 16, 16, _p(0)),
                 lambda: lib.gl_wb_diag_keys(ctx.handle, _p(0), 2, 2, _p(loss.ptr)),
                 lambda: lib.gl_wb_diag_keys(ctx.handle, _p(y.ptr), 2, 1, _p(loss.ptr))):
        with pytest.raises(gl.GanLeaksError) as e:
            check(call())
        assert e.value.code == -1
    empty = LpipsModel()
    for call in (lambda: lib.gl_lpips_grad_image(empty._handle, _p(y.ptr), _p(t.ptr), _p(0), 2, 16, 16, _p(cot.ptr), _p(loss.ptr)),
                 lambda: lib.gl_lpips_ref_rows_u8(empty._handle, _p(t.ptr), 2, 16, 16, _p(ref.ptr))):
        with pytest.raises(gl.GanLeaksError, match="not loaded") as e:
            check(call())
        assert e.value.code == -4
    with pytest.raises(RuntimeError, match="not loaded"):
        empty.grad_image(np.zeros((2, 3, 16, 16), np.float32), np.zeros((2, 3, 16, 16), np.uint8))
    with pytest.raises(ValueError, match="multiples of 16"):
        model.grad_image(np.zeros((2, 3, 24, 16), np.float32), np.zeros((2, 3, 24, 16), np.uint8))
    # the diagonal of a small matrix
    M = np.arange(12, dtype=np.float32).reshape(3, 4)
    keys = ctx.empty((3,), np.uint64)
    check(lib.gl_wb_diag_keys(ctx.handle, _p(ctx.to_device(M).ptr), 3, 4, _p(keys.ptr)))
    assert np.array_equal(keys.numpy(), np.diag(M).view(np.uint32).astype(np.uint64))


def _write_pngs(d, imgs_u8_nchw, prefix="image_"):
    import PIL.Image
    os.makedirs(d, exist_ok=True)
    for i, im in enumerate(imgs_u8_nchw):
        PIL.Image.fromarray(im.transpose(1, 2, 0)).save(os.path.join(d, "%s%d.png" % (prefix, i)))


def test_wb_cli_pair_distance(gl, tmp_path, monkeypatch, synth, pggan):
    import torch
    from ganleaks_amd import lpips
    from ganleaks_amd.attack_models import eval_roc, utils, wb
    lin = wl.lin_weights()
    torch.save({"features.%s" % k: torch.from_numpy(v) for k, v in synth.vgg16_state_dict(7).items()}, tmp_path / "vgg16.pth")
    torch.save({"lin%d.model.1.weight" % i: torch.from_numpy(lin["lin%d" % i]).view(1, -1, 1, 1) for i in range(5)}, tmp_path / "vgg_lin.pth")
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in synth.pggan_state_dict(*wl.PGGAN_SD).items()}, tmp_path / "generator.pth")
    monkeypatch.setenv("GANLEAKS_VGG16_PATH", str(tmp_path / "vgg16.pth"))
    monkeypatch.setenv("GANLEAKS_LPIPS_LIN_PATH", str(tmp_path / "vgg_lin.pth"))
    view = pggan.at(2)
    z_bank = np.random.default_rng(3).standard_normal((64, 64)).astype(np.float32)       # what --num_init 64 --init_seed 3 draws
    pos = view.generate_u8(z_bank[:4] + np.float32(0.2) * synth.latent(52, 4, 64).reshape(4, 64)).numpy()
    neg = view.generate_u8(synth.latent(53, 4, 64).reshape(4, 64)).numpy()
    _write_pngs(tmp_path / "pos", pos)
    _write_pngs(tmp_path / "neg", neg)
    monkeypatch.chdir(tmp_path)
    base = ["--pos_data_dir", str(tmp_path / "pos"), "--neg_data_dir", str(tmp_path / "neg"), "--BATCH_SIZE", "64", "--gan", "pggan", "--pg_steps", "2",
            "--in_channels", "64", "--nz", "64", "--resolution", "16", "--generator_path", str(tmp_path / "generator.pth"),
            "--num_init", "64", "--init_seed", "3", "--steps", "4", "--pair_distance", "l2-lpips", "--exp_name", "run"]
    lpips.set_default_model(None)
    try:
        out = wb.main(wb.parse_arguments(base))[0]
        d = tmp_path / "wb_attack" / "run"
        assert out == str(d)
        names = ["%s_%s.npy" % (k, f) for k in ("pos", "neg") for f in ("loss", "z", "key", "init_loss", "trace")]
        assert sorted(os.listdir(d)) == sorted(["params.txt"] + names)
        order = lambda name: [int(os.path.basename(x)[6:-4]) for x in utils.get_filepaths_from_dir(str(tmp_path / name), "png")]   # noqa: E731
        both = np.concatenate([pos[order("pos")], neg[order("neg")]])
        model = lpips.default_model()
        _, idx = gl.attack(both, gl.GeneratedBank(view, z_bank), distance="l2-lpips", batch_size=64, lpips=model)
        dist, z_star, key = gl.pair_wb_attack(both, view, z_bank[idx], steps=4, lpips=model)
    finally:
        lpips.set_default_model(None)
    loss = np.concatenate([np.load(d / "pos_loss.npy"), np.load(d / "neg_loss.npy")])
    assert loss.dtype == np.float64 and loss.shape == (8, 1) and np.array_equal(loss[:, 0], dist.astype(np.float64))
    assert np.array_equal(np.concatenate([np.load(d / "pos_key.npy"), np.load(d / "neg_key.npy")])[:, 0], key)
    assert np.array_equal(np.concatenate([np.load(d / "pos_z.npy"), np.load(d / "neg_z.npy")]), z_star)
    assert (loss <= np.concatenate([np.load(d / "pos_init_loss.npy"), np.load(d / "neg_init_loss.npy")])).all()
    assert np.load(d / "pos_trace.npy").shape == (5, 4)
    assert "pair_distance:l2-lpips" in open(d / "params.txt").read().splitlines()
    auc, ap, precision = eval_roc.main(eval_roc.parse_arguments(["--attack_type", "wb", "-ldir", str(d)]))
    assert auc == eval_roc.plot_roc(-np.load(d / "pos_loss.npy")[:, 0], -np.load(d / "neg_loss.npy")[:, 0])[3] and 0.0 <= auc <= 1.0
