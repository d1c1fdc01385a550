"""GPU: the partial-black-box attack under 0.2 * LPIPS + L2 -- gl_pbb_group_min_keys (csrc/gl_pbb.hip) against the host restatement of
tests/pair_pbb_common.py, and pair_pbb_attack bit for bit against a search driven from the host that is built only from parts that existed
before it: pbb_common's candidates and accept rule, generate_u8, and one pair_distances call per round on all queries x all candidates,
of which entry [q, q * lambda + j] is used.  The inputs of the search test are those at which tests/test_pair_pbb_cpu.py shows the search
to make progress on the host."""
import ctypes
import os

import numpy as np
import pytest

import gpu_common  # noqa: F401
import pair_pbb_common as pp
import wb_common as wc
import wb_lpips_common as wl

pytestmark = pytest.mark.gpu
_p = ctypes.c_void_p


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


def _group_min_keys(gl, M, nq, lam, ld):
    from ganleaks_amd._lib import check
    ctx = gl.Context.get()
    keys, j = ctx.empty((max(nq, 1),), np.uint64), ctx.empty((max(nq, 1),), np.int32)
    check(ctx.lib.gl_pbb_group_min_keys(ctx.handle, _p(ctx.to_device(M).ptr), nq, lam, ld, _p(keys.ptr), _p(j.ptr)))
    return keys.numpy()[:nq].astype(np.int64), j.numpy()[:nq]


def test_group_min_keys(gl):
    from ganleaks_amd._lib import check
    ctx = gl.Context.get()
    lib = ctx.lib
    f32, inf = np.float32, np.float32(np.inf)
    # nq = 3, lambda = 4, ld = 13: ties, +inf, and smaller values in the columns a query must not read
    M = np.full((3, 13), 9.0, f32)
    M[0, 0:4] = [2.0, 1.0, 1.0, 3.0]
    M[1, 4:8] = [inf, 5.0, 7.0, 5.0]
    M[2, 8:12] = [6.0, 4.0, 4.0, 4.0]
    M[:, 12] = 0.0
    M[0, 4:12] = 0.0
    M[2, 0:8] = 0.0
    keys, j = _group_min_keys(gl, M, 3, 4, 13)
    want_k, want_j = pp.group_min_keys(M, 4)
    assert want_j.tolist() == [1, 1, 1] and np.array_equal(keys, want_k) and np.array_equal(j, want_j) and j.dtype == np.int32
    # more than one workgroup, lambda no power of two; values from a small set, so that ties are common
    rng = np.random.default_rng(17)
    R = rng.random((257, 257 * 3 + 5)).astype(f32)
    R[rng.random(R.shape) < 0.3] = f32(0.25)
    keys, j = _group_min_keys(gl, R, 257, 3, R.shape[1])
    want_k, want_j = pp.group_min_keys(R, 3)
    assert np.array_equal(keys, want_k) and np.array_equal(j, want_j)
    # more candidates than lanes: every lane strides
    W = rng.integers(0, 6, size=(5, 5 * 150)).astype(f32)
    keys, j = _group_min_keys(gl, W, 5, 150, 750)
    want_k, want_j = pp.group_min_keys(W, 150)
    assert np.array_equal(keys, want_k) and np.array_equal(j, want_j)
    # lambda = 1 is gl_wb_diag_keys
    D = rng.random((70, 75)).astype(f32)
    keys, j = _group_min_keys(gl, D, 70, 1, 75)
    diag = ctx.empty((70,), np.uint64)
    check(lib.gl_wb_diag_keys(ctx.handle, _p(ctx.to_device(D).ptr), 70, 75, _p(diag.ptr)))
    assert np.array_equal(keys, diag.numpy().astype(np.int64)) and (j == 0).all()
    # nothing to do
    check(lib.gl_pbb_group_min_keys(ctx.handle, _p(0), 0, 4, 0, _p(0), _p(0)))
    Md, kd, jd = ctx.to_device(M), ctx.empty((3,), np.uint64), ctx.empty((3,), np.int32)
    for call in (lambda: lib.gl_pbb_group_min_keys(ctx.handle, _p(Md.ptr), 3, 4, 11, _p(kd.ptr), _p(jd.ptr)),
                 lambda: lib.gl_pbb_group_min_keys(ctx.handle, _p(Md.ptr), 3, 0, 13, _p(kd.ptr), _p(jd.ptr)),
                 lambda: lib.gl_pbb_group_min_keys(ctx.handle, _p(Md.ptr), -1, 4, 13, _p(kd.ptr), _p(jd.ptr)),
                 lambda: lib.gl_pbb_group_min_keys(ctx.handle, _p(Md.ptr), 3, 1 << 31, 1 << 40, _p(kd.ptr), _p(jd.ptr)),
                 lambda: lib.gl_pbb_group_min_keys(ctx.handle, _p(Md.ptr), 3, 4, 1 << 62, _p(kd.ptr), _p(jd.ptr)),
                 lambda: lib.gl_pbb_group_min_keys(ctx.handle, _p(0), 3, 4, 13, _p(kd.ptr), _p(jd.ptr)),
                 lambda: lib.gl_pbb_group_min_keys(ctx.handle, _p(Md.ptr), 3, 4, 13, _p(0), _p(jd.ptr)),
                 lambda: lib.gl_pbb_group_min_keys(ctx.handle, _p(Md.ptr), 3, 4, 13, _p(kd.ptr), _p(0)),
                 lambda: lib.gl_pbb_group_min_keys(None, _p(Md.ptr), 3, 4, 13, _p(kd.ptr), _p(jd.ptr))):
        with pytest.raises(gl.GanLeaksError) as e:
            check(call())
        assert e.value.code == -1


def _driven(gl, model, gen, queries, z_init, rounds, lam, sigma, seed, query_base=0):
    shape = queries.shape[1:]
    generate = lambda z: gen.generate_u8(np.ascontiguousarray(z, np.float32)).numpy().reshape((len(z),) + shape)     # noqa: E731
    matrix = lambda q, images: gl.pair_distances(q, images, batch_size=1, lpips=model)                                  # noqa: E731
    return pp.driven_search(queries, generate, matrix, z_init, rounds, lam, sigma, seed, query_base)


@pytest.fixture(scope="module")
def search_case(gl, model, pggan):
    """the 12 queries of the precondition test, the attack's answer and the host-driven search's"""
    view = pggan.at(wl.SEARCH_PG_STEPS, wl.SEARCH_ALPHA)
    z_init, z_image = wc.search_latents(wl.SEARCH_NZ)
    queries = view.generate_u8(z_image).numpy()
    kw = dict(rounds=pp.SEARCH_ROUNDS, population=pp.SEARCH_LAMBDA, sigma=pp.SEARCH_SIGMA, seed=pp.SEARCH_SEED, history=True, lpips=model)
    got = gl.pair_pbb_attack(queries, view, z_init, **kw)
    want = _driven(gl, model, view, queries, z_init, pp.SEARCH_ROUNDS, pp.SEARCH_LAMBDA, pp.SEARCH_SIGMA, pp.SEARCH_SEED)
    return view, queries, z_init, kw, got, want


def test_search_against_the_host_driven_search(search_case):
    _, _, _, _, (dist, z_star, key, trace), (want_z, want_key, want_trace) = search_case
    assert np.array_equal(z_star, want_z) and np.array_equal(key, want_key) and np.array_equal(trace, want_trace)


def test_search_properties(gl, model, search_case):
    view, queries, z_init, kw, (dist, z_star, key, trace), _ = search_case
    start = trace[0].astype(np.uint32).view(np.float32)
    print("start", start.tolist(), "final", dist.tolist(), "factor", (dist[2::3] / start[2::3]).tolist())
    assert trace.dtype == np.int64 and trace.shape == (pp.SEARCH_ROUNDS + 1, 12) and key.dtype == np.int64 and key.shape == (12,)
    assert dist.dtype == np.float32 and dist.shape == (12,) and z_star.dtype == np.float32 and z_star.shape == (12, wl.SEARCH_NZ)
    assert (np.diff(trace, axis=0) <= 0).all() and np.array_equal(trace[-1], key) and (key >= 0).all()
    assert np.array_equal(pp.bits32(dist), key)
    # the key is the search's own distance between the query and the image of z_star, bit for bit
    images = view.generate_u8(z_star).numpy()
    recount = np.array([gl.pair_distances(queries[q:q + 1], images[q:q + 1], batch_size=1, lpips=model)[0, 0] for q in range(12)], np.float32)
    assert np.array_equal(pp.bits32(recount), key)
    # the displaced queries end strictly below their start.  (A query that is its own start need not sit at key 0 here: D32 of a row with
    # itself is the float32 rounding of |q|^2 + |q|^2 - 2 q.q, zero or a few 1e-8; the host search of the precondition has exact zeros.)
    assert (start[2::3] > 0).all() and (dist[2::3] < start[2::3]).all()
    assert (start[0::3] < start[2::3].min()).all()
    # no rounds: the start
    d0, z0, k0, t0 = gl.pair_pbb_attack(queries, view, z_init, **dict(kw, rounds=0))
    assert np.array_equal(z0, z_init) and np.array_equal(k0, trace[0]) and np.array_equal(t0, trace[:1]) and np.array_equal(pp.bits32(d0), k0)
    # without history: three results
    assert len(gl.pair_pbb_attack(queries[:2], view, z_init[:2], **dict(kw, rounds=1, history=False))) == 3
    # a block whose candidate rows cannot fit (10^8 candidates of one query: 64 KB of rows each) is refused before the first round
    with pytest.raises(ValueError, match=r"needs \d+ bytes.*\d+ are available.*population or block_images"):
        gl.pair_pbb_attack(queries, view, z_init, **dict(kw, rounds=1, population=10 ** 8))
    with pytest.raises(ValueError, match="lattice"):
        gl.pair_pbb_attack(queries.astype(np.float32) / 255.0 + np.float32(1e-3), view, z_init, **dict(kw, rounds=1))


def test_search_does_not_depend_on_the_blocks(gl, search_case):
    view, queries, z_init, kw, got, _ = search_case
    # 12 queries as 2 + 2 + ...
    for a, b in zip(gl.pair_pbb_attack(queries, view, z_init, block_images=2 * pp.SEARCH_LAMBDA, **kw), got):
        assert np.array_equal(a, b)
    # 12 queries as two calls
    head = gl.pair_pbb_attack(queries[:5], view, z_init[:5], query_base=0, **kw)
    tail = gl.pair_pbb_attack(queries[5:], view, z_init[5:], query_base=5, **kw)
    for a, b, c, axis in zip(head, tail, got, (0, 0, 0, 1)):
        assert np.array_equal(np.concatenate([a, b], axis=axis), c)


def test_never_above_the_full_black_box_score(gl, model, pggan):
    view = pggan.at(2)
    rng = np.random.default_rng(71)
    queries = view.generate_u8(rng.standard_normal((6, 64)).astype(np.float32)).numpy()
    z_bank = rng.standard_normal((130, 64)).astype(np.float32)
    fbb_dist, idx = gl.attack(queries, gl.GeneratedBank(view, z_bank), distance="l2-lpips", batch_size=64, lpips=model)
    z_init, idx2 = gl.pair_pbb_init_from_bank(queries, view, z_bank, batch_size=64, lpips=model)
    assert np.array_equal(idx2, idx) and np.array_equal(z_init, z_bank[idx]) and z_init.dtype == np.float32
    dist, _, key, trace = gl.pair_pbb_attack(queries, view, z_init, rounds=4, population=8, sigma=0.25, history=True, lpips=model)
    assert np.array_equal(trace[0], pp.bits32(fbb_dist))
    assert (dist <= fbb_dist).all()


def test_blocked_rows_and_a_tile_boundary(gl, synth, model):
    """128 x 128 images: search rows of 2 MiB or more are stored in blocks of 256 rows.  257 queries, lambda = 3, block_images = 3: a block
    of one query is rounded up to 256, so the second block starts at query 256 and candidate row 768 and holds one query"""
    from ganleaks_amd.gan_models.pggan.model_torch import Generator
    gen = Generator(64, 128, 3)                          # blocks of 128, 128, 128, 128 -> 64 -> 32 channels
    gen.load_state_dict(synth.pggan_state_dict(4321, 64, 128))
    view = gen.at(5)
    rng = np.random.default_rng(29)
    z_true = rng.standard_normal((257, 64)).astype(np.float32)
    z_init = (z_true + np.float32(0.25) * rng.standard_normal((257, 64)).astype(np.float32)).astype(np.float32)
    queries = view.generate_u8(z_true).numpy()
    assert queries.shape == (257, 3, 128, 128)
    assert model.features(queries[:1], role=model.search_role("bank")).blocked
    dist, z_star, key, trace = gl.pair_pbb_attack(queries, view, z_init, rounds=2, population=3, sigma=0.0625, seed=3, block_images=3, history=True,
                                                  lpips=model)
    want_z, want_key, want_trace = _driven(gl, model, view, queries, z_init, 2, 3, 0.0625, 3)
    assert np.array_equal(z_star, want_z) and np.array_equal(key, want_key) and np.array_equal(trace, want_trace)
    assert np.array_equal(pp.bits32(dist), key) and (np.diff(trace, axis=0) <= 0).all()
    # one block of 257 queries: the second tile starts at query 256 and candidate row 768 of the same buffers
    for a, b in zip(gl.pair_pbb_attack(queries, view, z_init, rounds=2, population=3, sigma=0.0625, seed=3, history=True, lpips=model),
                    (dist, z_star, key, trace)):
        assert np.array_equal(a, b)


def test_dcgan(gl, synth, model):
    from ganleaks_amd.gan_models.dcgan.model_torch import Generator
    gen = Generator(100, 3, wl.DCGAN_SD["features_g"])
    gen.load_state_dict(synth.dcgan_state_dict(wl.DCGAN_SD["seed"], features_g=wl.DCGAN_SD["features_g"]))
    rng = np.random.default_rng(31)
    z_true = rng.standard_normal((4, 100)).astype(np.float32)
    z_init = (z_true + np.float32(0.25) * rng.standard_normal((4, 100)).astype(np.float32)).astype(np.float32)
    queries = gen.generate_u8(z_true).numpy()
    assert queries.shape == (4, 3, 64, 64)
    dist, z_star, key, trace = gl.pair_pbb_attack(queries, gen, z_init, rounds=2, population=4, sigma=0.125, seed=5, history=True, lpips=model)
    want_z, want_key, want_trace = _driven(gl, model, gen, queries, z_init, 2, 4, 0.125, 5)
    assert np.array_equal(z_star, want_z) and np.array_equal(key, want_key) and np.array_equal(trace, want_trace)
    assert np.array_equal(pp.bits32(dist), key)


def _write_pngs(d, imgs_u8_nchw, prefix="image_"):
    import PIL.Image
    os.makedirs(d, exist_ok=True)
    for i, im in enumerate(imgs_u8_nchw):
        PIL.Image.fromarray(im.transpose(1, 2, 0)).save(os.path.join(d, "%s%d.png" % (prefix, i)))


def test_pbb_cli_pair_distance(gl, tmp_path, monkeypatch, synth, pggan):
    import torch
    from ganleaks_amd import lpips
    from ganleaks_amd.attack_models import eval_roc, pbb, utils
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
    base = ["--pos_data_dir", str(tmp_path / "pos"), "--neg_data_dir", str(tmp_path / "neg"), "--BATCH_SIZE", "64", "--gan", "pggan", "--steps", "2",
            "--in_channels", "64", "--nz", "64", "--resolution", "16", "--generator_path", str(tmp_path / "generator.pth"),
            "--num_init", "64", "--init_seed", "3", "--rounds", "3", "--population", "6", "--sigma", "0.25", "--seed", "9",
            "--pair_distance", "l2-lpips", "--exp_name", "run"]
    lpips.set_default_model(None)
    try:
        out = pbb.main(pbb.parse_arguments(base))[0]
        d = tmp_path / "pbb_attack" / "run"
        assert out == str(d)
        names = ["%s_%s.npy" % (k, f) for k in ("pos", "neg") for f in ("loss", "z", "key", "init_loss", "trace")]
        assert sorted(os.listdir(d)) == sorted(["params.txt"] + names)
        order = lambda name: [int(os.path.basename(x)[6:-4]) for x in utils.get_filepaths_from_dir(str(tmp_path / name), "png")]   # noqa: E731
        both = np.concatenate([pos[order("pos")], neg[order("neg")]])
        model = lpips.default_model()
        z_init, _ = gl.pair_pbb_init_from_bank(both, view, z_bank, batch_size=64, lpips=model)
        dist, z_star, key, trace = gl.pair_pbb_attack(both, view, z_init, rounds=3, population=6, sigma=0.25, seed=9, history=True, lpips=model)
    finally:
        lpips.set_default_model(None)
    loss = np.concatenate([np.load(d / "pos_loss.npy"), np.load(d / "neg_loss.npy")])
    assert loss.dtype == np.float64 and loss.shape == (8, 1) and np.array_equal(loss[:, 0], dist.astype(np.float64))
    saved_key = np.concatenate([np.load(d / "pos_key.npy"), np.load(d / "neg_key.npy")])
    assert saved_key.dtype == np.int64 and saved_key.shape == (8, 1) and np.array_equal(saved_key[:, 0], key)
    assert np.array_equal(np.concatenate([np.load(d / "pos_z.npy"), np.load(d / "neg_z.npy")]), z_star)
    init_loss = np.concatenate([np.load(d / "pos_init_loss.npy"), np.load(d / "neg_init_loss.npy")])
    assert np.array_equal(init_loss[:, 0], trace[0].astype(np.uint32).view(np.float32).astype(np.float64)) and (loss <= init_loss).all()
    assert np.array_equal(np.concatenate([np.load(d / "pos_trace.npy"), np.load(d / "neg_trace.npy")], axis=1), trace)
    assert np.load(d / "pos_trace.npy").shape == (4, 4)
    assert "pair_distance:l2-lpips" in open(d / "params.txt").read().splitlines()
    auc, ap, precision = eval_roc.main(eval_roc.parse_arguments(["--attack_type", "pbb", "-ldir", str(d)]))
    assert auc == eval_roc.plot_roc(-np.load(d / "pos_loss.npy")[:, 0], -np.load(d / "neg_loss.npy")[:, 0])[3] and 0.0 <= auc <= 1.0
