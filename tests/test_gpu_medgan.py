"""GPU parity of the medGAN generator + decoder against outputs of the reference's own modules
(tests/golden/medgan_gen.npz).  Tolerance 2e-5 (fp32, different summation order).

The layers at the edges of the column padding (F = 1 ... 1071), the `>= 0.5` threshold and the workspace regrowth are compared with a float64 numpy
reference written from the state dicts; measured on an MI355X: hidden within 1.8e-6, decoded within 3.3e-6."""
import os

import numpy as np
import pytest

import gpu_common  # noqa: F401

pytestmark = pytest.mark.gpu

GUARD = 4096                     # 4-byte words of sentinel on each side of a guarded device buffer
SENT = 0xA5A5A5A5


def medgan_reference(gsd, asd, z, binary):
    """float64 Generator.forward and Autoencoder.decode from the state dicts (BatchNorm1d eval, eps 1e-3) -> (hidden, decoded)"""
    f = lambda a: np.asarray(a, np.float64)

    def block(x, name, act):
        h = x @ f(gsd[name + ".0.weight"]).T + f(gsd[name + ".0.bias"])
        h = (h - f(gsd[name + ".1.running_mean"])) / np.sqrt(f(gsd[name + ".1.running_var"]) + 1e-3) * f(gsd[name + ".1.weight"]) + f(gsd[name + ".1.bias"])
        return x + act(h)

    hidden = block(block(f(z), "gen_block1", lambda h: np.maximum(h, 0.0)), "gen_block2", np.tanh)
    lin = hidden @ f(asd["decoder.0.weight"]).T + f(asd["decoder.0.bias"])
    return hidden, (1.0 / (1.0 + np.exp(-lin)) if binary else np.maximum(lin, 0.0))


def guarded_decode(ae, hidden, n, F):
    """gl_medgan_decode with decoded_dev and binary_dev pointing INTO larger sentinel-filled device buffers -> (decoded, binary, guards untouched)"""
    import ctypes
    from ganleaks_amd._lib import as_device, check
    ctx = ae.ctx
    h = as_device(ctx, hidden, np.float32)
    bufs = [ctx.to_device(np.full(2 * GUARD + n * F, SENT, np.uint32)) for _ in range(2)]
    check(ctx.lib.gl_medgan_decode(ae._handle, ctypes.c_void_p(h.ptr), n, ctypes.c_void_p(bufs[0].ptr + 4 * GUARD), ctypes.c_void_p(bufs[1].ptr + 4 * GUARD)))
    host = [b.numpy() for b in bufs]
    clean = all((a[:GUARD] == SENT).all() and (a[GUARD + n * F:] == SENT).all() and len(a[GUARD + n * F:]) == GUARD for a in host)
    dec, binr = (a[GUARD:GUARD + n * F].view(np.float32).reshape(n, F) for a in host)
    return dec, binr, clean


def test_medgan_generator_and_decoder(synth, golden_dir):
    import ganleaks_amd as gl
    from ganleaks_amd.gan_models.medgan.model import Autoencoder, Generator, generate_synthetic
    g = np.load(os.path.join(golden_dir, "medgan_gen.npz"))
    gsd, asd = synth.medgan_state_dicts(555, 1071)
    z = np.random.default_rng(8).standard_normal((37, 128)).astype(np.float32)
    gen = Generator(128, 128)
    gen.load_state_dict(gsd)
    h = gen.eval()(z)
    assert h.shape == (37, 128) and np.abs(h - g["hidden"]).max() < 2e-5
    for binary in (True, False):
        ae = Autoencoder(1071, 128, binary=binary)
        ae.load_state_dict(asd)
        dec = ae.decode(h)
        assert dec.shape == (37, 1071)
        assert np.abs(dec - g["decoded_binary%d" % int(binary)]).max() < 2e-5
        assert np.array_equal(ae.decoder(h), dec)
    ae = Autoencoder(1071, 128, binary=True)
    ae.load_state_dict(asd)
    rows = generate_synthetic(gen, ae, z)
    ref = (g["decoded_binary1"] >= 0.5).astype(np.float32)
    far = np.abs(g["decoded_binary1"] - 0.5) > 1e-4            # away from the threshold the bits must agree
    assert rows.dtype == np.float32 and set(np.unique(rows)) <= {0.0, 1.0}
    assert np.array_equal(rows[far], ref[far]) and far.mean() > 0.999
    # tabular rows go through the exact integer search (whole numbers 0..255, no image lattice)
    d, i = gl.attack(rows[:5], rows, batch_size=1)
    assert i.tolist() == [0, 1, 2, 3, 4] and np.all(d == 0)
    with pytest.raises(gl.GanLeaksError):
        Generator(100, 128)._ensure()


def test_medgan_bank_attack_against_c_oracle(synth):
    """the tabular half of BASELINE configs[4]: medGAN rows (F = 1071 binary columns) as the bank, perturbed rows and fresh rows as
    queries, against the C oracle: indices bit-exact, dist = fl32(S / F).  S = number of differing columns for 0/1 data, so the byte
    oracle (which squares differences of codes) applies with codes 0 / 1."""
    import c_oracle
    import ganleaks_amd as gl
    from ganleaks_amd.attack_models.utils import Loss
    from ganleaks_amd.gan_models.medgan.model import Autoencoder, Generator, generate_synthetic
    gsd, asd = synth.medgan_state_dicts(555, 1071)
    gen = Generator(128, 128)
    gen.load_state_dict(gsd)
    ae = Autoencoder(1071, 128, binary=True)
    ae.load_state_dict(asd)
    rng = np.random.default_rng(17)
    bank = generate_synthetic(gen.eval(), ae, rng.standard_normal((700, 128)).astype(np.float32))
    assert bank.shape == (700, 1071) and set(np.unique(bank)) <= {0.0, 1.0}
    q = bank[[5, 77, 650, 699]].copy()
    flip = rng.random(q.shape) < 0.03
    q = np.where(flip, 1.0 - q, q).astype(np.float32)
    fresh = generate_synthetic(gen, ae, rng.standard_normal((6, 128)).astype(np.float32))
    q = np.concatenate([q, fresh])
    d, i = gl.attack(q, bank, batch_size=64)                   # 700 -> 640 rows used (fbb.py:77)
    _, oi, ssd = c_oracle.knn_l2_u8(bank.astype(np.uint8), q.astype(np.uint8), 64)
    assert np.array_equal(i, oi) and i.max() < 640
    assert np.array_equal(d, (ssd.astype(np.float64) / 1071.0).astype(np.float32))
    assert i[0] == 5 and i[1] == 77 and i[2] != 650            # 650, 699 sit in the truncated tail
    # Loss('l2').forward on whole-number float rows (0/1 tables): mean((y - x)^2) = S / F
    loss = Loss("l2")
    v = loss(bank[:64], q[:1])
    want = (c_oracle.ssd_row_u8(bank[:64].astype(np.uint8), q[0].astype(np.uint8)).astype(np.float64) / 1071.0).astype(np.float32)
    assert v.shape == (64,) and np.array_equal(v, want)
    z0 = np.zeros((3, 1071), np.float32)
    assert np.array_equal(loss(z0, z0[:1]), np.zeros(3, np.float32))
    raw = rng.integers(0, 256, (5, 3, 8, 8)).astype(np.float32)   # raw 0..255 floats: also whole numbers, not image codes
    want = ((raw[:, None] - raw[None, :1]) ** 2).reshape(5, -1).mean(axis=1).astype(np.float32)
    assert np.allclose(loss(raw, raw[:1]), want[:, ] if want.ndim == 1 else want, rtol=1e-6)


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("n,F", [(1, 1), (1, 64), (5, 65), (257, 128), (3, 129), (70, 192), (33, 1071)])
def test_medgan_layers_at_the_edges_of_the_column_padding(n, F, binary, synth):
    """mg_cols_pad changes branch at F = 64 / 65 / 128 / 129 / 192 and the packed decoder weight is cols_pad * 128: hidden and decoded values
    against float64, nothing written outside [n][F], and the 0 / 1 rows the threshold of the device's own decoded values"""
    from ganleaks_amd.gan_models.medgan.model import Autoencoder, Generator
    gsd, asd = synth.medgan_state_dicts(600 + F, F)
    z = np.random.default_rng(1000 + n).standard_normal((n, 128)).astype(np.float32)
    ref_h, ref_d = medgan_reference(gsd, asd, z, binary)
    gen = Generator(128, 128)
    gen.load_state_dict(gsd)
    h = gen.eval()(z)
    eh = np.abs(h - ref_h).max()
    ae = Autoencoder(F, 128, binary=binary)
    ae.load_state_dict(asd)
    dec, binr, clean = guarded_decode(ae, h, n, F)
    ed = np.abs(dec - ref_d).max()
    print("n=%d F=%d binary=%d: hidden error %.3e, decoded error %.3e" % (n, F, binary, eh, ed))
    assert h.shape == (n, 128) and eh < 2e-5
    assert clean, "gl_medgan_decode wrote outside [n][F]"
    assert np.isfinite(dec).all() and ed < 2e-5
    assert np.array_equal(binr.view(np.uint32), (dec >= 0.5).astype(np.float32).view(np.uint32))
    assert np.array_equal(ae.decode(h), dec)             # the unguarded call gives the same values
    assert 0 < (dec >= 0.5).mean() < 1 or n * F < 8


@pytest.mark.parametrize("binary,bias,want", [(True, 0.0, 1.0), (False, 0.5, 1.0), (False, float(np.nextafter(np.float32(0.5), np.float32(0))), 0.0)])
def test_medgan_threshold_edge(binary, bias, want, synth):
    """the reference's `>= 0.5` (gan_models/medgan/train.py:311-312), exactly: decoder weights all zero, so decoded = act(bias)"""
    from ganleaks_amd.gan_models.medgan.model import Autoencoder
    n, F = 5, 65
    ae = Autoencoder(F, 128, binary=binary)
    ae.load_state_dict({"decoder.0.weight": np.zeros((F, 128), np.float32), "decoder.0.bias": np.full(F, bias, np.float32)})
    hidden = np.random.default_rng(3).standard_normal((n, 128)).astype(np.float32)
    dec, binr, clean = guarded_decode(ae, hidden, n, F)
    assert clean
    assert np.array_equal(dec, np.full((n, F), np.float32(0.5) if binary else np.float32(bias), np.float32))
    assert np.array_equal(binr, np.full((n, F), want, np.float32))


def test_medgan_workspace_regrowth(synth):
    """one handle, n = 5, then 300 (the workspace regrows), then 2 (it stays): each result bit for bit what a fresh handle gives"""
    from ganleaks_amd.gan_models.medgan.model import Autoencoder, Generator
    F = 129
    gsd, asd = synth.medgan_state_dicts(640, F)
    rng = np.random.default_rng(9)
    gen = Generator(128, 128)
    gen.load_state_dict(gsd)
    ae = Autoencoder(F, 128, binary=True)
    ae.load_state_dict(asd)
    for n in (5, 300, 2):
        z = rng.standard_normal((n, 128)).astype(np.float32)
        fresh_g = Generator(128, 128)
        fresh_g.load_state_dict(gsd)
        fresh_a = Autoencoder(F, 128, binary=True)
        fresh_a.load_state_dict(asd)
        h, hf = gen(z), fresh_g(z)
        assert h.shape == (n, 128) and np.array_equal(h.view(np.uint32), hf.view(np.uint32)), n
        assert np.abs(h - medgan_reference(gsd, asd, z, True)[0]).max() < 2e-5
        assert np.array_equal(ae.decode(h).view(np.uint32), fresh_a.decode(hf).view(np.uint32)), n
