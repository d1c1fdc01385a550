"""GPU parity of the VAEGAN generator (spectral-norm ConvTranspose stack + self-attention) against two consecutive
forwards of the reference's own Generator (tests/golden/vaegan_gen.npz).  Tolerance 5e-5 on outputs in (-1,1).

The spectral-norm kernels are pinned through the public ABI: after each of two forwards all eight weight_u / weight_v of state_dict() against
VaeganOracle in float64, bound 4 x the error of the same oracle in float32 (floor: one float32 ulp of the vector's largest element), for
(z_dim, d) = (100, 64), (64, 32) and, with d = 32, z_dim = 300 (H > 256) and 3.  Measured on an MI355X over all 96 vectors: device 5.4e-9 - 6.4e-8,
float32 oracle 7.8e-9 - 1.3e-7, device / bound 0.02 - 0.36."""
import os

import numpy as np
import pytest

import gpu_common  # noqa: F401

pytestmark = pytest.mark.gpu

SN_KEYS = ["deconv%d.module.weight_%s" % (l, w) for l in (1, 2, 3, 4) for w in "uv"]
_steps = {}


def oracle_steps(synth, seed, z_dim, d, z, steps=2):
    """`steps` consecutive forwards of VaeganOracle in float64 and, on the same state dict, in float32: per forward the float64 output and, for each
    of the eight power-iteration vectors, (float64 vector, largest error of the float32 evaluation against it).  Computed once per generator."""
    key = (seed, z_dim, d, steps)
    if key not in _steps:
        import torch
        import vaegan_oracle
        sd = synth.vaegan_state_dict(seed, z_dim, d)
        o64, o32 = vaegan_oracle.VaeganOracle(sd), vaegan_oracle.VaeganOracle(sd, torch.float32)
        res = []
        for _ in range(steps):
            out = o64.forward(z)
            o32.forward(z)
            res.append((out, {k: (o64.sd[k].numpy().copy(), float(np.abs(o32.sd[k].double().numpy() - o64.sd[k].numpy()).max())) for k in SN_KEYS}))
        _steps[key] = res
    return _steps[key]


def check_spectral_state(got, want, tag):
    """every weight_u / weight_v within 4 x the float32 oracle's own error (tests/test_gpu_wb.py's margin), with a floor of one float32 ulp of the
    vector's largest element"""
    late = []
    for k in SN_KEYS:
        w64, e32 = want[k]
        ulp = float(np.spacing(np.float32(np.abs(w64).max())))
        err = float(np.abs(got[k].astype(np.float64) - w64).max())
        bound = max(4.0 * e32, ulp)
        print("%s %s [%d]: device %.3e  float32 oracle %.3e  bound %.3e  device / bound %.2f" % (tag, k, w64.size, err, e32, bound, err / bound))
        assert got[k].shape == w64.shape
        if not err <= bound:
            late.append((k, err, e32, bound))
    assert not late, (tag, late)


@pytest.mark.parametrize("precision", [1, 0])
def test_vaegan_generator_two_forwards(precision, synth, golden_dir):
    """precision 1 (default): split-fp16 convolutions; 0: fp32 MFMA.  The attention block (one q|k|v GEMM + the fp32-MFMA
    attention kernel) is shared."""
    from ganleaks_amd.gan_models.vaegan.train import Generator
    g = np.load(os.path.join(golden_dir, "vaegan_gen.npz"))
    gen = Generator(100, 64)
    assert "matched" in gen.load_state_dict(synth.vaegan_state_dict(777, 100, 64))
    gen.set_precision(precision)
    z = synth.latent(4, 6)
    out1 = gen.eval()(z)
    assert out1.shape == (6, 3, 64, 64)
    e1 = np.abs(out1 - g["out1"]).max()
    assert e1 < 5e-5, e1
    out2 = gen(z)                                       # the spectral-norm state advanced, like the reference's
    e2 = np.abs(out2 - g["out2"]).max()
    assert e2 < 5e-5, e2
    assert np.abs(gen.state_dict()["deconv1.module.weight_u"] - g["u1"]).max() < 1e-5
    assert np.abs(gen.state_dict()["deconv4.module.weight_v"] - g["v4"]).max() < 1e-5
    assert gen._precision == precision                  # no saturation fallback happened


def test_vaegan_oracle_and_chunks(synth):
    import vaegan_oracle
    from ganleaks_amd._lib import check
    from ganleaks_amd.gan_models.vaegan.train import Generator
    sd = synth.vaegan_state_dict(778, 64, 32)            # d = 32: attention width 64
    z = synth.latent(6, 70, 64)
    ref = vaegan_oracle.VaeganOracle(sd).forward(z[:4])
    gen = Generator(64, 32)
    gen.load_state_dict(sd)
    check(gen.ctx.lib.gl_dcgan_set_chunk(gen._ensure(), 32))    # 70 = 32 + 32 + 6
    out = gen(z)
    assert np.abs(out[:4] - ref).max() < 5e-5
    gen2 = Generator(64, 32)
    gen2.load_state_dict(sd)
    assert np.array_equal(gen2(z), out)
    gen3 = Generator(64, 32)
    gen3.load_state_dict(sd)
    gen3.set_precision(0)
    assert np.abs(gen3(z) - out).max() < 2e-5


def test_sample_script(tmp_path, synth):
    """vaegan/sample.py: seed 1000, batches of 100, one forward (and one spectral-norm step) per batch; generated.npz + samples.png"""
    import torch
    from ganleaks_amd.gan_models.vaegan import sample
    from ganleaks_amd.gan_models.vaegan.train import Generator
    sd = synth.vaegan_state_dict(779, 64, 32)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, tmp_path / "netG.pt")
    out = sample.main(sample.parse_args(["--model_dir", str(tmp_path), "--num_samples", "150"]))
    g = np.load(out)
    assert g["noise"].shape == (150, 64) and g["img_r01"].shape == (150, 64, 64, 3) and g["img_r01"].dtype == np.float32
    assert (tmp_path / "samples.png").stat().st_size > 1000
    # the same schedule by hand: two forwards of 100 latents each
    torch.manual_seed(1000)
    ref = Generator(64, 32)
    ref.load_state_dict(sd)
    z1, z2 = torch.randn(100, 64, 1, 1), torch.randn(100, 64, 1, 1)
    a, b = ref(z1.numpy()), ref(z2.numpy())
    assert np.array_equal(g["noise"][:100], z1.numpy().reshape(100, 64))
    want = (np.concatenate([a, b])[:150] + np.float32(1)) / np.float32(2)
    assert np.array_equal(g["img_r01"], want.transpose(0, 2, 3, 1))
    torch.save(torch.nn.Linear(2, 2), tmp_path / "netG.pt")       # a pickled module is refused, not executed
    with pytest.raises(ValueError):
        sample.main(sample.parse_args(["--model_dir", str(tmp_path)]))


def test_vaegan_bank_attack_against_c_oracle(synth):
    """the image half of BASELINE configs[4]: VAEGAN generate_u8 -> 8-bit bank -> exact L2 1-NN, against the C oracle
    (mirror of the DCGAN / PGGAN bank tests)"""
    import c_oracle
    import ganleaks_amd as gl
    import oracle
    from ganleaks_amd.gan_models.vaegan.train import Generator
    gen = Generator(100, 64)
    gen.load_state_dict(synth.vaegan_state_dict(777, 100, 64))
    z = synth.latent(14, 200)
    bank = gen.eval().generate_u8(z)
    hb = bank.numpy()
    assert hb.shape == (200, 3, 64, 64) and hb.dtype == np.uint8
    q = np.concatenate([synth.perturb_u8(3, hb[[7, 150, 199]], 5.0), synth.lowpass_u8_images(5, 3, 64)])
    d, i = gl.attack(q, bank, batch_size=64)
    od, oi, _ = c_oracle.knn_l2_u8(hb, q, 64)
    assert np.array_equal(i, oi) and np.array_equal(d, od) and i[0] == 7 and i[1] == 150 and i[2] != 199
    # and the codes are the quantisation of what forward() returns for the same spectral-norm state
    gen2 = Generator(100, 64)
    gen2.load_state_dict(synth.vaegan_state_dict(777, 100, 64))
    f = gen2.eval()(z)
    diff = hb.astype(np.int32) - oracle.quantize_to_u8(f).astype(np.int32)
    assert np.abs(diff).max() <= 1 and (diff != 0).mean() < 1e-3          # forward() and generate_u8 are separate launches of the same arithmetic


@pytest.mark.parametrize("z_dim,d,seed", [(100, 64, 777), (64, 32, 778)])
def test_spectral_state_of_all_layers_after_each_of_two_forwards(z_dim, d, seed, synth):
    """all eight power-iteration vectors through the public state_dict() (gl_dcgan_get_spectral_state), after the first and after the second forward"""
    from ganleaks_amd.gan_models.vaegan.train import Generator
    z = synth.latent(21, 2, z_dim)
    steps = oracle_steps(synth, seed, z_dim, d, z)
    gen = Generator(z_dim, d)
    gen.load_state_dict(synth.vaegan_state_dict(seed, z_dim, d))
    for s, (out64, want) in enumerate(steps):
        out = gen(z)
        assert np.abs(out - out64).max() < 5e-5
        check_spectral_state(gen.state_dict(), want, "z_dim=%d d=%d forward %d" % (z_dim, d, s + 1))


@pytest.mark.parametrize("precision", [1, 0])
@pytest.mark.parametrize("z_dim", [300, 3])
def test_vaegan_latent_wider_than_one_stride_and_tiny(z_dim, precision, synth):
    """z_dim = 300: H > 256, the second trip of every 256-stride loop of the spectral-norm kernels and a z_pad above 256; z_dim = 3: one partial
    32-wide K slice.  d = 32, n = 2, two forwards, outputs and all eight vectors against VaeganOracle"""
    from ganleaks_amd.gan_models.vaegan.train import Generator
    seed = 780 + z_dim
    z = synth.latent(22, 2, z_dim)
    steps = oracle_steps(synth, seed, z_dim, 32, z)
    gen = Generator(z_dim, 32)
    gen.load_state_dict(synth.vaegan_state_dict(seed, z_dim, 32))
    gen.set_precision(precision)
    for s, (out64, want) in enumerate(steps):
        out = gen(z)
        assert out.shape == (2, 3, 64, 64)
        e = np.abs(out - out64).max()
        print("z_dim=%d precision=%d forward %d: output error %.3e" % (z_dim, precision, s + 1, e))
        assert e < 5e-5, e
        check_spectral_state(gen.state_dict(), want, "z_dim=%d precision=%d forward %d" % (z_dim, precision, s + 1))
    assert gen._precision == precision                  # no saturation fallback happened
