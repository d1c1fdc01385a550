"""GPU: the VAEGAN encoder (csrc/gl_vaegan_enc.hip, gan_models/vaegan/train.py Encoder) against the reference's Encoder.encode run in float64
(tests/golden/vaegan_enc.npz, written by tests/golden/make_golden_vaegan_enc.py), for both kinds of input and both head widths; the u8 path
against the f32 path bit for bit; independence of the pass size and of the images that share a call; state-dict errors; GL_ERR_STATE."""
import ctypes
import os

import numpy as np
import pytest

import gpu_common  # noqa: F401
import recon_common as rc

pytestmark = pytest.mark.gpu
# the project's generator tolerance (ATOL of test_gpu_pggan.py / test_gpu_vaegan.py), scaled by the size of the outputs, which are not
# confined to (-1, 1)
RTOL = 5e-5
_p = ctypes.c_void_p


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "vaegan_enc.npz")))


@pytest.fixture(scope="module")
def encoders(synth, golden):
    from ganleaks_amd.gan_models.vaegan.train import Encoder
    out = {}
    for z in (100, 3):
        e = Encoder(z)
        assert e.load_state_dict(synth.vaegan_encoder_state_dict(int(golden["seed"]), z)) == "<All keys matched successfully>"
        out[z] = e
    return out


@pytest.mark.parametrize("z", [100, 3])
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_encode_matches_reference_float64(encoders, golden, z, kind):
    u8 = golden["images_u8"]
    x = u8 if kind == "u8" else rc.lattice(u8)
    mu, logvar = encoders[z].eval().encode(x)
    assert mu.shape == (8, z) and mu.dtype == np.float32 and logvar.shape == (8, z)
    for name, got in (("mu", mu), ("logvar", logvar)):
        ref = golden["%s64_z%d" % (name, z)]
        err, bound = float(np.abs(got - ref).max()), RTOL * max(1.0, float(np.abs(ref).max()))
        print("%s z_dim %d %s: max err %.3e (bound %.3e, max |ref| %.3f)" % (name, z, kind, err, bound, np.abs(ref).max()))
        assert err <= bound


@pytest.mark.parametrize("z", [100, 3])
def test_u8_path_equals_f32_path_on_the_lattice(encoders, golden, z):
    u8 = golden["images_u8"]
    a = encoders[z].encode(u8)
    b = encoders[z].encode(rc.lattice(u8))
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_passes_and_batch_do_not_change_a_row(encoders, synth):
    e = encoders[100]
    x = synth.lowpass_u8_images(91, 21, 64)
    one = e.encode(x)
    try:
        e.set_chunk(8)
        parts = e.encode(x)
    finally:
        e.set_chunk(0)
    single = e.encode(x[3:4])
    dev = e.encode_device(e.ctx.to_device(x))
    for i in range(2):
        assert np.array_equal(one[i].view(np.uint32), parts[i].view(np.uint32))
        assert np.array_equal(single[i][0].view(np.uint32), one[i][3].view(np.uint32))
        assert np.array_equal(dev[i].numpy().view(np.uint32), one[i].view(np.uint32))
    assert e.encode(x[:0])[0].shape == (0, 100)
    assert e.to("cuda").cuda().train(False) is e


def test_forward_is_draw_one(encoders, golden):
    import ganleaks_amd as gl
    e = encoders[3]
    u8 = golden["images_u8"]
    mu, logvar = e.encode(u8)
    z = e(u8, seed=5, query_base=40)
    want = rc.recon_latents(mu, np.exp(logvar), 2, 5, 40, 4.0).reshape(8, 2, 3)[:, 1]
    assert z.shape == (8, 3) and np.array_equal(z.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(gl.recon_latents(mu, logvar, 1, seed=5, query_base=40).numpy().reshape(8, 2, 3)[:, 1], z)


def test_state_dict_errors(synth):
    from ganleaks_amd.gan_models.vaegan.train import Encoder
    sd = synth.vaegan_encoder_state_dict(3, 3)
    e = Encoder(3)
    for key in ("cv2.bias", "bn6.running_var", "fc2_1.weight", "bn1.num_batches_tracked"):
        with pytest.raises(KeyError, match=key.replace(".", "\\.")):
            e.load_state_dict({k: v for k, v in sd.items() if k != key})
    with pytest.raises(ValueError, match="cv3\\.weight"):
        e.load_state_dict(dict(sd, **{"cv3.weight": sd["cv3.weight"][:, :, :3]}))
    with pytest.raises(ValueError, match="fc1\\.weight"):
        e.load_state_dict(synth.vaegan_encoder_state_dict(3, 4))
    with pytest.raises(KeyError, match="unexpected"):
        e.load_state_dict(dict(sd, extra=np.zeros(1, np.float32)))
    e.load_state_dict(dict(sd, extra=np.zeros(1, np.float32)), strict=False)
    with pytest.raises(ValueError, match="3,64,64"):
        e.encode(np.zeros((1, 3, 32, 32), np.uint8))


def test_second_state_dict_changes_the_output(synth, golden):
    from ganleaks_amd.gan_models.vaegan.train import Encoder
    e = Encoder(3)
    u8 = golden["images_u8"][:2]
    e.load_state_dict(synth.vaegan_encoder_state_dict(3, 3))
    a = e.encode(u8)
    e.load_state_dict(synth.vaegan_encoder_state_dict(int(golden["seed"]), 3))
    b = e.encode(u8)
    assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])
    assert np.abs(b[0] - golden["mu64_z3"][:2]).max() <= RTOL * max(1.0, np.abs(golden["mu64_z3"]).max())


def test_state_error_before_everything_is_loaded(synth):
    import ganleaks_amd as gl
    from ganleaks_amd._lib import check
    from ganleaks_amd.gan_models.vaegan.train import ENCODER_BN, Encoder
    ctx = gl.Context.get()
    lib = ctx.lib
    h = _p()
    for d in (32, 128):
        assert lib.gl_vaegan_enc_create(ctx.handle, 3, d, ctypes.byref(h)) == -1 and b"512 * 4 * 4" in lib.gl_last_error()
    for z in (0, 4097):
        assert lib.gl_vaegan_enc_create(ctx.handle, z, 64, ctypes.byref(h)) == -1
    e = Encoder(3)
    x = np.zeros((1, 3, 64, 64), np.uint8)
    with pytest.raises(gl.GanLeaksError, match="cv1") as err:
        e.encode(x)
    assert err.value.code == -4
    sd = {k: np.ascontiguousarray(v, np.float32) for k, v in synth.vaegan_encoder_state_dict(3, 3).items()}
    ptr = lambda k: sd[k].ctypes.data_as(_p)   # noqa: E731
    handle = e._ensure()
    for l in (0, 1, 3):
        check(lib.gl_vaegan_enc_set_conv(handle, l, ptr("cv%d.weight" % (l + 1)), ptr("cv%d.bias" % (l + 1)), *[ptr("bn%d.%s" % (l + 1, k)) for k in ENCODER_BN]))
    check(lib.gl_vaegan_enc_set_head(handle, 0, ptr("fc1.weight"), ptr("fc1.bias"), *[ptr("bn6.%s" % k) for k in ENCODER_BN], ptr("fc1_1.weight"), ptr("fc1_1.bias")))
    with pytest.raises(gl.GanLeaksError, match="cv3"):
        e.encode(x)
    check(lib.gl_vaegan_enc_set_conv(handle, 2, ptr("cv3.weight"), ptr("cv3.bias"), *[ptr("bn3.%s" % k) for k in ENCODER_BN]))
    with pytest.raises(gl.GanLeaksError, match="fc2") as err:
        e.encode(x)
    assert err.value.code == -4
    check(lib.gl_vaegan_enc_set_head(handle, 1, ptr("fc2.weight"), ptr("fc2.bias"), *[ptr("bn7.%s" % k) for k in ENCODER_BN], ptr("fc2_1.weight"), ptr("fc2_1.bias")))
    full = Encoder(3)
    full.load_state_dict(sd)
    assert np.array_equal(e.encode(x)[0], full.encode(x)[0])
    # exactly one image pointer; n == 0 touches nothing
    xd = ctx.to_device(x)
    out = ctx.empty((1, 3), np.float32)
    assert lib.gl_vaegan_enc_encode(handle, _p(xd.ptr), _p(xd.ptr), 1, _p(out.ptr), _p(out.ptr)) == -1
    assert lib.gl_vaegan_enc_encode(handle, _p(0), _p(0), 1, _p(out.ptr), _p(out.ptr)) == -1
    assert lib.gl_vaegan_enc_encode(handle, _p(0), _p(0), 0, _p(0), _p(0)) == 0
