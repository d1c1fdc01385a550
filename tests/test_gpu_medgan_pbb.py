"""GPU: the partial-black-box attack on medGAN tables (tests/test_medgan_pbb_cpu.py holds the host side) -- gl_medgan_codes against the forward's own thresholded rows bit for bit, and pbb_attack /
pbb_init_from_bank / GeneratedBank on a table_generator, scored by the exact number of differing columns."""
import ctypes
import functools

import numpy as np
import pytest

import gpu_common  # noqa: F401
import medgan_pbb_common as mc

pytestmark = pytest.mark.gpu
_p = ctypes.c_void_p
GUARD = 4096                     # bytes of sentinel on each side of a guarded device buffer
SENT8 = 0xA5


@pytest.fixture(scope="module")
def gl():
    import ganleaks_amd
    return ganleaks_amd


@functools.lru_cache(maxsize=None)
def _models(F, binary):
    """(generator, autoencoder, table_generator) for a table of F columns"""
    import ganleaks_amd as gl
    from ganleaks_amd.gan_models.medgan.model import Autoencoder, Generator, table_generator
    gsd, asd = gl.synth.medgan_state_dicts(mc.weights_seed(F), F)
    gen, ae = Generator(128, 128), Autoencoder(F, 128, binary=binary)
    gen.load_state_dict(gsd)
    ae.load_state_dict(asd)
    return gen, ae, table_generator(gen, ae)


def _synthetic(models, z):
    from ganleaks_amd.gan_models.medgan.model import generate_synthetic
    return generate_synthetic(models[0], models[1], z)


def _guarded(ctx, count):
    """a device buffer of `count` bytes between two sentinel guards -> (buffer, pointer to the payload)"""
    buf = ctx.to_device(np.full(2 * GUARD + count, SENT8, np.uint8))
    return buf, buf.ptr + GUARD


def _payload(buf, count):
    """(payload, guards untouched)"""
    host = buf.numpy()
    clean = (host[:GUARD] == SENT8).all() and (host[GUARD + count:] == SENT8).all() and len(host[GUARD + count:]) == GUARD
    return host[GUARD:GUARD + count], bool(clean)


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("n,F", mc.SHAPES)
def test_codes_are_the_generate_branch_rows(gl, n, F, binary):
    from ganleaks_amd._lib import check
    models = _models(F, binary)
    gen, ae, view = models[:3]
    z = mc.latents(n, F)
    want = _synthetic(models, z)
    assert want.dtype == np.float32 and set(np.unique(want)) <= {0.0, 1.0}
    zd = view.ctx.to_device(z)
    buf, ptr = _guarded(view.ctx, n * F)
    check(view.ctx.lib.gl_medgan_codes(gen._handle, ae._handle, _p(zd.ptr), n, _p(ptr)))
    got, clean = _payload(buf, n * F)
    assert clean, "gl_medgan_codes wrote outside [n][F]"
    assert np.array_equal(got.reshape(n, F), want.astype(np.uint8))
    u8 = view.generate_u8(z)
    assert u8.dtype == np.uint8 and u8.shape == (n, F) and np.array_equal(u8.numpy(), want.astype(np.uint8))
    rows = view.generate_rows(z)
    assert rows.dtype == np.float32 and rows.shape == (n, F) and np.array_equal(rows.numpy(), want)
    assert np.array_equal(view.forward(z).numpy(), ae.decode(gen(z)))
    assert (view.ctx, view.z_dim, view.image_shape, view.row_kind) == (gen.ctx, 128, (F,), "int")
    check(view.ctx.lib.gl_medgan_codes(gen._handle, ae._handle, _p(0), 0, _p(0)))                 # n == 0: nothing to do


def test_pbb_attack_on_a_small_table(gl):
    F, Q = 65, 7
    models = _models(F, True)
    view = models[2]
    z_true = np.random.default_rng(911).standard_normal((Q, 128)).astype(np.float32)
    z0 = (z_true + np.float32(0.3) * np.random.default_rng(912).standard_normal((Q, 128))).astype(np.float32)
    q = _synthetic(models, z_true)
    kw = dict(rounds=6, population=16, seed=5)
    dist, z_star, S, trace = gl.pbb.pbb_attack(q, view, z0, history=True, **kw)
    print("pbb: start", trace[0].tolist(), "end", trace[-1].tolist())
    assert trace.shape == (7, Q) and (np.diff(trace, axis=0) <= 0).all()
    assert np.array_equal(trace[0], mc.hamming(_synthetic(models, z0), q)) and np.array_equal(trace[-1], S)
    assert np.array_equal(S, mc.hamming(_synthetic(models, z_star), q))
    assert np.array_equal(dist, (S.astype(np.float64) / F).astype(np.float32))
    blocked = gl.pbb.pbb_attack(q, view, z0, block_images=48, **kw)      # three queries per block
    assert np.array_equal(blocked[1].view(np.uint32), z_star.view(np.uint32)) and np.array_equal(blocked[2], S)
    parts = [gl.pbb.pbb_attack(q[:3], view, z0[:3], **kw), gl.pbb.pbb_attack(q[3:], view, z0[3:], query_base=3, **kw)]
    assert np.array_equal(np.concatenate([p[1] for p in parts]).view(np.uint32), z_star.view(np.uint32))
    assert np.array_equal(np.concatenate([p[2] for p in parts]), S)
    assert np.array_equal(gl.pbb.pbb_attack(q.astype(np.uint8), view, z0, **kw)[2], S)


def test_generated_bank_and_the_start_are_the_full_black_box_answer(gl):
    models = _models(1071, True)
    view = models[2]
    z_bank = np.random.default_rng(921).standard_normal((700, 128)).astype(np.float32)
    bank = _synthetic(models, z_bank)
    rng = np.random.default_rng(922)
    q = bank[rng.integers(0, 700, 12)].copy()
    flip = rng.random(q.shape) < 0.02
    q[flip] = 1.0 - q[flip]
    want_d, want_i = gl.attack(q, bank, batch_size=64)
    got_d, got_i = gl.attack(q, gl.GeneratedBank(view, z_bank), distance="l2", batch_size=64)
    assert np.array_equal(got_d.view(np.uint32), want_d.view(np.uint32)) and np.array_equal(got_i, want_i)
    z_init, idx = gl.pbb.pbb_init_from_bank(q, view, z_bank, batch_size=64)
    assert np.array_equal(idx, want_i) and np.array_equal(z_init, z_bank[want_i]) and idx.max() < 640
    # a streamed bank: chunks of 100 rows (a table row holds 10 F + 1024 bytes while its chunk is prepared)
    got_d, got_i = gl.attack(q, gl.GeneratedBank(view, z_bank), distance="l2", batch_size=64, chunk_bytes=100 * (10 * 1071 + 1024))
    assert np.array_equal(got_d.view(np.uint32), want_d.view(np.uint32)) and np.array_equal(got_i, want_i)
    # a uint8 table holds the values themselves, for the start as for pbb_attack
    z_u8, idx_u8 = gl.pbb.pbb_init_from_bank(q.astype(np.uint8), view, z_bank, batch_size=64)
    assert np.array_equal(idx_u8, want_i) and np.array_equal(z_u8, z_init)


def test_refusals_on_the_device_path(gl):
    from ganleaks_amd._lib import check
    from ganleaks_amd.gan_models.medgan.model import Autoencoder, table_generator
    models = _models(65, True)
    gen, ae, view = models[:3]
    z = np.zeros((2, 128), np.float32)
    q = _synthetic(models, z)
    off = q.copy()
    off[1, 7] = 0.5
    attack = lambda rows: gl.pbb.pbb_attack(rows, view, z, rounds=1, population=2)      # noqa: E731
    with pytest.raises(ValueError, match="integer lattice"):
        attack(off)
    with pytest.raises(ValueError):
        attack(np.zeros((2, 64), np.float32))                              # a table of another width
    with pytest.raises(ValueError):
        attack(np.zeros((2, 5, 13), np.float32))                           # not a table
    with pytest.raises(ValueError):
        view.generate_u8(np.zeros((2, 100), np.float32))
    empty = Autoencoder(65, 128, binary=True)
    with pytest.raises(RuntimeError, match="load_state_dict"):
        table_generator(gen, empty)
    zd, out = view.ctx.to_device(z), view.ctx.empty((2, 65), np.uint8)
    with pytest.raises(gl.GanLeaksError, match="decoder not loaded"):
        check(view.ctx.lib.gl_medgan_codes(gen._handle, empty._ensure(), _p(zd.ptr), 2, _p(out.ptr)))
    with pytest.raises(gl.GanLeaksError, match="generator blocks not loaded"):
        check(view.ctx.lib.gl_medgan_codes(empty._ensure(), ae._handle, _p(zd.ptr), 2, _p(out.ptr)))
    with pytest.raises(gl.GanLeaksError, match="decoder not loaded"):
        check(view.ctx.lib.gl_medgan_codes(gen._handle, gen._handle, _p(zd.ptr), 2, _p(out.ptr)))


def test_handles_that_carry_both_parts_take_either_role(gl):
    """a handle may hold the generator blocks AND a decoder (the C ABI allows it).  Two such handles used as (A, B) and then as (B, A), and
    one as both: the hidden rows [n][128] and the decoded rows [n][F] have a workspace each, so a buffer sized for one role is never
    written in the other's shape.  Every call goes into a guarded destination and must give the rows of the plain forward."""
    from ganleaks_amd._lib import check
    from ganleaks_amd.gan_models.medgan.model import Autoencoder
    F, n = 1071, 100
    gen, ae, view = _models(F, True)
    ctx = view.ctx
    gsd, asd = gl.synth.medgan_state_dicts(mc.weights_seed(F), F)
    both = []
    for _ in range(2):
        h = Autoencoder(F, 128, binary=True)
        h.load_state_dict(asd)
        for blk, name in enumerate(("gen_block1", "gen_block2")):
            a = [np.ascontiguousarray(gsd[name + k], np.float32) for k in (".0.weight", ".0.bias", ".1.weight", ".1.bias", ".1.running_mean", ".1.running_var")]
            check(ctx.lib.gl_medgan_set_gen_block(h._handle, blk, *[x.ctypes.data_as(_p) for x in a], ctypes.c_float(0.001)))
        both.append(h)
    z = mc.latents(n, F)
    want = _synthetic((gen, ae), z).astype(np.uint8)
    zd = ctx.to_device(z)
    A, B = both
    for g_role, d_role in ((A, B), (B, A), (A, A), (B, A)):
        buf, ptr = _guarded(ctx, n * F)
        check(ctx.lib.gl_medgan_codes(g_role._handle, d_role._handle, _p(zd.ptr), n, _p(ptr)))
        got, clean = _payload(buf, n * F)
        assert clean and np.array_equal(got.reshape(n, F), want)
