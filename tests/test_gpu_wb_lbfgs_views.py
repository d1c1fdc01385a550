"""GPU: optimizer='lbfgs' on the other generators and the other distance -- one short run each on pggan's Generator.at(steps, alpha) and
vaegan's Generator.frozen(1) (the smallest models tests/test_gpu_wb_pggan.py and tests/test_gpu_wb_vaegan.py build): a monotone trace, the
exact S identity and independence of block_images; and one pair_wb_attack run on the setup of tests/test_gpu_wb_lpips.py's search test: the
key is the pattern of the float attack(distance='l2-lpips') reports for (x, G(z*)), and never above the start."""
import numpy as np
import pytest

import gpu_common  # noqa: F401
import vaegan_wb_common as vw
import wb_common as wc
import wb_lpips_common as wl

pytestmark = pytest.mark.gpu
STEPS = 4


@pytest.fixture(scope="module")
def gl():
    import ganleaks_amd
    return ganleaks_amd


def _check_l2(gl, view, queries, z_init, d):
    from ganleaks_amd.attack import _dist32
    kw = dict(steps=STEPS, optimizer="lbfgs", history=True)
    dist, z_star, S, trace = gl.wb_attack(queries, view, z_init, **kw)
    print("start", trace[0].tolist(), "final", S.tolist())
    n = len(queries)
    assert trace.shape == (STEPS + 1, n) and trace.dtype == np.int64 and z_star.shape == z_init.shape and z_star.dtype == np.float32
    assert (np.diff(trace, axis=0) <= 0).all() and np.array_equal(trace[-1], S)
    assert np.array_equal(trace[0], wc.ssd(view.generate_u8(z_init).numpy(), queries))
    assert np.array_equal(S, wc.ssd(view.generate_u8(z_star).numpy(), queries))
    assert np.array_equal(dist, _dist32(S, d, "u8"))
    assert (S < trace[0]).any()
    for blocks in (max(2, n // 2 - 1), 4096):
        for a, b in zip(gl.wb_attack(queries, view, z_init, block_images=blocks, **kw), (dist, z_star, S, trace)):
            assert np.array_equal(a, b)


def test_pggan_view(gl):
    from ganleaks_amd.gan_models.pggan.model_torch import Generator
    gen = Generator(64, 64, 3)
    gen.load_state_dict(gl.synth.pggan_state_dict(100, 64, 64))
    view = gen.at(2, 0.4)
    z_init, z_image = wc.search_latents(64)
    _check_l2(gl, view, view.generate_u8(z_image).numpy(), z_init, 3 * 16 * 16)
    assert gen._precision == 1


def test_vaegan_view(gl):
    from ganleaks_amd.gan_models.vaegan.train import Generator
    d, nz = vw.SMALL
    parent = Generator(nz, d=d)
    parent.load_state_dict(gl.synth.vaegan_state_dict(z_dim=nz, d=d))
    view = parent.frozen(1)
    z_bank, z_query = vw.attack_latents()
    queries = view.generate_u8(z_query).numpy()
    z_init, _ = gl.pbb_init_from_bank(queries, view, z_bank, batch_size=64)
    _check_l2(gl, view, queries, z_init, 12288)
    assert view._precision == 1


def _pattern(dist):
    return np.ascontiguousarray(dist, np.float32).view(np.uint32).astype(np.int64)


def test_pair_wb_attack(gl, synth):
    from ganleaks_amd.gan_models.pggan.model_torch import Generator
    from ganleaks_amd.lpips import LpipsModel
    model = LpipsModel().load_state_dicts(synth.vgg16_state_dict(7), wl.lin_weights())
    gen = Generator(wl.PGGAN_SD[1], wl.PGGAN_SD[2], 3)
    gen.load_state_dict(synth.pggan_state_dict(*wl.PGGAN_SD))
    view = gen.at(wl.SEARCH_PG_STEPS, wl.SEARCH_ALPHA)
    z_init, z_image = wc.search_latents(wl.SEARCH_NZ)
    queries = view.generate_u8(z_image).numpy()
    kw = dict(steps=STEPS, optimizer="lbfgs", history=True, lpips=model)
    dist, z_star, key, trace = gl.pair_wb_attack(queries, view, z_init, **kw)
    start = trace[0].astype(np.uint32).view(np.float32)
    print("start", start.tolist(), "final", dist.tolist())
    assert trace.dtype == np.int64 and trace.shape == (STEPS + 1, 12) and key.dtype == np.int64 and dist.dtype == np.float32
    assert (np.diff(trace, axis=0) <= 0).all() and np.array_equal(trace[-1], key) and (key <= trace[0]).all() and (key < trace[0]).any()
    assert np.array_equal(_pattern(dist), key)
    images = view.generate_u8(z_star).numpy()
    recount = np.array([gl.attack(queries[q:q + 1], images[q:q + 1], distance="l2-lpips", batch_size=1, lpips=model)[0][0] for q in range(12)],
                       np.float32)
    assert np.array_equal(_pattern(recount), key)
    first = np.array([gl.attack(queries[q:q + 1], view.generate_u8(z_init[q:q + 1]).numpy(), distance="l2-lpips", batch_size=1, lpips=model)[0][0]
                      for q in range(12)], np.float32)
    assert np.array_equal(_pattern(first), trace[0])
    for a, b in zip(gl.pair_wb_attack(queries, view, z_init, block_images=5, **kw), (dist, z_star, key, trace)):
        assert np.array_equal(a, b)
    # Adam is what it was with the new keywords named
    adam = dict(steps=2, lr=wl.SEARCH_LR, history=True, lpips=model)
    for a, b in zip(gl.pair_wb_attack(queries, view, z_init, **adam), gl.pair_wb_attack(queries, view, z_init, optimizer="adam", **adam)):
        assert np.array_equal(a, b)
