"""CPU-only: the host restatement behind the PGGAN white-box tests (tests/wb_pggan_common.py) against the pinned forward and against central
differences, the preconditions of the GPU cases (no LeakyReLU unit close enough to zero for float32 to flip its slope; descent on the host
works at the search test's inputs), the refusals that need no GPU, and the exports in the cross-compiled library."""
import os
import subprocess

import numpy as np
import pytest
import torch

import wb_common as wc
import wb_pggan_common as wp

SEARCH_NZ, SEARCH_PG_STEPS, SEARCH_ALPHA = 64, 2, 0.4


@pytest.fixture(scope="module")
def net64(synth):
    return wp.PgganNet(synth.pggan_state_dict(100, 64, 64))


def test_host_module_is_the_pinned_generator(synth, golden_dir):
    """tests/golden/pggan_gen.npz holds outputs of the reference's own Generator (tests/test_oracle_pggan.py)"""
    g = np.load(os.path.join(golden_dir, "pggan_gen.npz"))
    assert len(g["cases"]) > 0
    for ci, (z_dim, C, steps, alpha) in enumerate(g["cases"]):
        z_dim, C, steps = int(z_dim), int(C), int(steps)
        net = wp.PgganNet(synth.pggan_state_dict(4321 + C, z_dim, C))
        out = wp.forward(net, synth.latent(3, 4, z_dim).reshape(4, z_dim), steps, float(alpha))
        assert out.shape == g["case%d" % ci].shape and np.abs(out - g["case%d" % ci]).max() < 2e-5, ci
    net = wp.PgganNet(synth.pggan_state_dict(101, 64, 64, prefix="gen.1."), prefix="gen.1.")
    assert np.abs(wp.forward(net, synth.latent(3, 4, 64).reshape(4, 64), 2, 1.0) - g["stack_g1"]).max() < 2e-5


@pytest.mark.parametrize("steps,alpha", [(0, 1.0), (1, 0.4), (2, 1.0), (2, 0.4)])
def test_host_gradients_against_differences(net64, steps, alpha):
    """autograd's vjp against central differences of the float64 module along one direction per row, and the radial direction: PixelNorm on the
    latent makes G constant along z, so z . dz = 0"""
    rng = np.random.default_rng(2)
    R = 4 * 2 ** steps
    z = rng.standard_normal((2, 64)).astype(np.float32)
    cot = rng.standard_normal((2, 3, R, R)).astype(np.float32)
    u = rng.standard_normal((2, 64))
    g, _ = wp.vjp_z(net64, z, cot, steps, alpha)
    h = 1e-6
    zt = torch.from_numpy(z.astype(np.float64))
    with torch.no_grad():
        yp = net64.run((zt + h * torch.from_numpy(u)).reshape(2, 64, 1, 1), steps, alpha).numpy()
        ym = net64.run((zt - h * torch.from_numpy(u)).reshape(2, 64, 1, 1), steps, alpha).numpy()
    fd = ((yp - ym) / (2 * h) * cot).reshape(2, -1).sum(axis=1)
    assert np.allclose((g * u).sum(axis=1), fd, rtol=1e-5, atol=0)
    assert (np.abs((g * z).sum(axis=1)) <= 1e-4 * np.linalg.norm(z, axis=1) * np.linalg.norm(g, axis=1)).all()


@pytest.mark.parametrize("name", sorted(wp.CASES))
def test_gpu_cases_flip_no_slope(synth, name):
    """the precondition of every GPU gradient case: a unit that flips its LeakyReLU slope moves a gradient row by about 1e-3, a thousand
    times the bound of tests/test_gpu_wb_pggan.py, and float32 torch itself flips on some seeds"""
    seed, nz, C, steps, n, _, _ = wp.CASES[name]
    sd = synth.pggan_state_dict(seed, nz, C)
    ok, near = wp.flip_margin_ok(wp.PgganNet(sd), wp.PgganNet(sd, torch.float32), wp.case_latents(name), steps, 1.0)
    print(name, "near-zero units:", near)
    assert ok


def test_search_precondition(net64):
    """the inputs of the GPU search test: on the host, every query whose start lies SEARCH_DELTA away from its latent ends at a quarter of its
    starting S or less; the queries that are their own start stay at S = 0 and z_init; the trace never rises"""
    z_init, z_image = wc.search_latents(SEARCH_NZ)
    queries = wp.quantize_u8(wp.forward(net64, z_image, SEARCH_PG_STEPS, SEARCH_ALPHA))
    z_best, S, trace = wp.search(queries, net64, z_init, SEARCH_PG_STEPS, SEARCH_ALPHA, wc.SEARCH_STEPS, wc.SEARCH_LR)
    print("start", trace[0].tolist(), "final", S.tolist())
    assert trace.shape == (wc.SEARCH_STEPS + 1, wc.SEARCH_Q) and (np.diff(trace, axis=0) <= 0).all() and np.array_equal(trace[-1], S)
    assert (trace[:, 0::3] == 0).all() and np.array_equal(z_best[0::3], z_init[0::3])
    assert (trace[0, 2::3] > 0).all() and (4 * S[2::3] <= trace[0, 2::3]).all(), (trace[0], S)
    assert np.array_equal(S, wc.ssd(wp.quantize_u8(wp.forward(net64, z_best, SEARCH_PG_STEPS, SEARCH_ALPHA)), queries))


class _View:
    """enough of a generator at a fixed depth for the checks that come before any GPU work"""
    image_shape = (3, 16, 16)

    def generate_u8(self, z):
        raise AssertionError("the argument checks must come first")

    l2_grad_z = generate_u8

    @property
    def ctx(self):
        raise AssertionError("the argument checks must come first")


def test_refusals_without_gpu(tmp_path, monkeypatch):
    import ganleaks_amd as gl
    from ganleaks_amd.attack_models import wb
    from ganleaks_amd.gan_models.pggan.model_torch import Generator
    gen = Generator(64, 64, 3)
    for bad in (-1, 9, 1.5, 5):                                    # 5: block 4 has 32 -> 16 channels at in_channels = 64
        with pytest.raises(ValueError, match="steps"):
            gen.at(bad)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            gen.at(2, bad)
    view = gen.at(2, 0.4)
    assert view.image_shape == (3, 16, 16) and view.z_dim == 64 and view.steps == 2 and view.alpha == 0.4
    assert gen.at(0).image_shape == (3, 4, 4) and gen.at(4).image_shape == (3, 64, 64)
    with pytest.raises(NotImplementedError, match=r"at\(steps, alpha\)"):
        gl.wb_attack(np.zeros((2, 3, 16, 16), np.uint8), gen, np.zeros((2, 64), np.float32))
    with pytest.raises(ValueError, match="shape"):
        gl.wb_attack(np.zeros((2, 3, 64, 64), np.uint8), _View(), np.zeros((2, 64), np.float32))
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit, match="PGGAN.*--pg_steps|--pg_steps.*PGGAN"):
        wb.main(wb.parse_arguments(["--gan", "pggan", "--generator_path", str(tmp_path / "nowhere.pth"), "--num_init", "64"]))
    with pytest.raises(SystemExit, match="pggan"):
        wb._request(wb.parse_arguments(["--gan", "dcgan", "--pg_steps", "2", "--generator_path", "x.pth", "--num_init", "64"]))
    with pytest.raises(SystemExit, match="resolution"):
        wb._request(wb.parse_arguments(["--gan", "pggan", "--pg_steps", "2", "--generator_path", "x.pth", "--num_init", "64"]))
    wb._request(wb.parse_arguments(["--gan", "pggan", "--pg_steps", "2", "--resolution", "16", "--generator_path", "x.pth", "--num_init", "64"]))
    assert not (tmp_path / "wb_attack").exists()


def test_exports_and_signatures():
    from ganleaks_amd import _lib
    from ganleaks_amd.gan_models.pggan.model_torch import Generator
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    sym = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, stdout=subprocess.PIPE).stdout.decode()
    exported = {line.split()[-1] for line in sym.splitlines() if line.strip()}
    for name in ("gl_pggan_vjp_z", "gl_pggan_l2_grad_z"):
        assert name in exported, name
        assert len(_lib.SIGNATURES[name][1]) == 8, name
    assert hasattr(Generator, "at") and not hasattr(Generator, "l2_grad_z") and not hasattr(Generator, "vjp_z")
