"""GPU: optimizer='powell' on the other generators and the other distance -- one sweep each on pggan's Generator.at(steps, alpha), vaegan's
Generator.frozen(1) and medgan's table_generator (the smallest models the other view tests build): a trace that never rises, the exact
S identity and independence of block_images; and one pair_pbb_attack run on the setup of tests/test_gpu_pair_pbb.py's search test: the key
is the pattern of the float attack(distance='l2-lpips') reports for (x, G(z*)), and never above the start."""
import numpy as np
import pytest

import gpu_common  # noqa: F401
import medgan_pbb_common as mc
import vaegan_wb_common as vw
import wb_common as wc
import wb_lpips_common as wl

pytestmark = pytest.mark.gpu
LADDER = 4


@pytest.fixture(scope="module")
def gl():
    import ganleaks_amd
    return ganleaks_amd


def _check_l2(gl, view, queries, z_init, count, d, kind, **generate_kwargs):
    """count(images u8, queries) -> the exact S of every pair"""
    from ganleaks_amd.attack import _dist32
    kw = dict(optimizer="powell", sweeps=1, ladder=LADDER, history=True, **generate_kwargs)
    dist, z_star, S, trace = gl.pbb_attack(queries, view, z_init, **kw)
    print("start", trace[0].tolist(), "final", S.tolist())
    n = len(queries)
    assert trace.shape == (2, n) and trace.dtype == np.int64 and z_star.shape == z_init.shape and z_star.dtype == np.float32
    assert (np.diff(trace, axis=0) <= 0).all() and np.array_equal(trace[-1], S)
    assert np.array_equal(trace[0], count(view.generate_u8(z_init, **generate_kwargs).numpy(), queries))
    assert np.array_equal(S, count(view.generate_u8(z_star, **generate_kwargs).numpy(), queries))
    assert np.array_equal(dist, _dist32(S, d, kind))
    assert (S < trace[0]).any()
    for a, b in zip(gl.pbb_attack(queries, view, z_init, block_images=LADDER * max(2, n // 2 - 1), **kw), (dist, z_star, S, trace)):
        assert np.array_equal(a, b)


def test_pggan_view(gl):
    from ganleaks_amd.gan_models.pggan.model_torch import Generator
    gen = Generator(64, 64, 3)
    gen.load_state_dict(gl.synth.pggan_state_dict(100, 64, 64))
    view = gen.at(2, 0.4)
    z_init, z_image = wc.search_latents(64)
    _check_l2(gl, view, view.generate_u8(z_image).numpy(), z_init, wc.ssd, 3 * 16 * 16, "u8")


def test_vaegan_view(gl):
    from ganleaks_amd.gan_models.vaegan.train import Generator
    d, nz = vw.SMALL
    parent = Generator(nz, d=d)
    parent.load_state_dict(gl.synth.vaegan_state_dict(z_dim=nz, d=d))
    view = parent.frozen(1)
    z_bank, z_query = vw.attack_latents()
    queries = view.generate_u8(z_query).numpy()
    z_init, _ = gl.pbb_init_from_bank(queries, view, z_bank, batch_size=64)
    _check_l2(gl, view, queries, z_init, wc.ssd, 12288, "u8")


def test_medgan_table(gl):
    from ganleaks_amd.gan_models.medgan.model import Autoencoder, Generator, generate_synthetic, table_generator
    F, Q = 65, 7
    gsd, asd = gl.synth.medgan_state_dicts(mc.weights_seed(F), F)
    gen, ae = Generator(128, 128), Autoencoder(F, 128, binary=True)
    gen.load_state_dict(gsd)
    ae.load_state_dict(asd)
    view = table_generator(gen, ae)
    z_true = np.random.default_rng(911).standard_normal((Q, 128)).astype(np.float32)
    z0 = (z_true + np.float32(0.3) * np.random.default_rng(912).standard_normal((Q, 128))).astype(np.float32)
    q = generate_synthetic(gen, ae, z_true)
    _check_l2(gl, view, q, z0, lambda rows, queries: mc.hamming(rows.astype(np.float32), queries), F, "int")      # S counts differing columns
    with pytest.raises(NotImplementedError, match="LPIPS"):
        gl.pair_pbb_attack(q, view, z0, optimizer="powell")


def _pattern(dist):
    return np.ascontiguousarray(dist, np.float32).view(np.uint32).astype(np.int64)


def test_pair_pbb_attack(gl, synth):
    from ganleaks_amd.gan_models.pggan.model_torch import Generator
    from ganleaks_amd.lpips import LpipsModel
    model = LpipsModel().load_state_dicts(synth.vgg16_state_dict(7), wl.lin_weights())
    gen = Generator(wl.PGGAN_SD[1], wl.PGGAN_SD[2], 3)
    gen.load_state_dict(synth.pggan_state_dict(*wl.PGGAN_SD))
    view = gen.at(wl.SEARCH_PG_STEPS, wl.SEARCH_ALPHA)
    z_init, z_image = wc.search_latents(wl.SEARCH_NZ)
    queries = view.generate_u8(z_image).numpy()
    kw = dict(optimizer="powell", sweeps=1, ladder=LADDER, history=True, lpips=model)
    dist, z_star, key, trace = gl.pair_pbb_attack(queries, view, z_init, **kw)
    start = trace[0].astype(np.uint32).view(np.float32)
    print("start", start.tolist(), "final", dist.tolist())
    assert trace.dtype == np.int64 and trace.shape == (2, 12) and key.dtype == np.int64 and dist.dtype == np.float32
    assert (np.diff(trace, axis=0) <= 0).all() and np.array_equal(trace[-1], key) and (key <= trace[0]).all() and (key < trace[0]).any()
    assert np.array_equal(_pattern(dist), key)
    images = view.generate_u8(z_star).numpy()
    recount = np.array([gl.attack(queries[q:q + 1], images[q:q + 1], distance="l2-lpips", batch_size=1, lpips=model)[0][0] for q in range(12)],
                       np.float32)
    assert np.array_equal(_pattern(recount), key)
    first = np.array([gl.attack(queries[q:q + 1], view.generate_u8(z_init[q:q + 1]).numpy(), distance="l2-lpips", batch_size=1, lpips=model)[0][0]
                      for q in range(12)], np.float32)
    assert np.array_equal(_pattern(first), trace[0])
    for a, b in zip(gl.pair_pbb_attack(queries, view, z_init, block_images=5 * LADDER, **kw), (dist, z_star, key, trace)):
        assert np.array_equal(a, b)
    # the evolution strategy is what it was with the new keywords named
    es = dict(rounds=2, population=5, sigma=0.0625, seed=7, history=True, lpips=model)
    for a, b in zip(gl.pair_pbb_attack(queries, view, z_init, **es), gl.pair_pbb_attack(queries, view, z_init, optimizer="es", **es)):
        assert np.array_equal(a, b)
