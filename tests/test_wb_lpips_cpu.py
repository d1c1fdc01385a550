"""CPU-only: the host restatement behind the white-box tests under 0.2 * LPIPS + L2 (tests/wb_lpips_common.py) against the float64 oracle and
against central differences; the preconditions of every GPU case of tests/test_gpu_wb_lpips.py (no ReLU unit close enough to zero for float32
to move it across, no tap position with all channels zero, no max-pool cell with tied positive maxima); descent on the host at the search
test's inputs; the refusals that need no GPU; and the exports in the cross-compiled library."""
import os
import subprocess

import numpy as np
import pytest
import torch

import wb_common as wc
import wb_lpips_common as wl
import wb_pggan_common as wp


@pytest.fixture(scope="module")
def vgg(synth):
    return wl.vgg_nets(synth)


def test_host_loss_is_the_oracle_distance(synth, vgg):
    """the torch graph gives the distance oracle/lpips_oracle.py pins to the reference's PNetLin"""
    targets, y = wl.image_case(synth, "16x16")
    _, loss = wl.grad_image(vgg[0], y, targets)
    x = (2.0 * (targets.astype(np.float64) / 255.0) - 1.0).astype(np.float32)
    tot, _, _ = wl.lo.l2_lpips_matrix(synth.vgg16_state_dict(7), [wl.lin_weights()["lin%d" % i] for i in range(5)], y, x)
    assert np.allclose(loss, np.diag(tot), rtol=1e-6, atol=0)


@pytest.mark.parametrize("name", sorted(wl.IMAGE_CASES))
def test_image_cases_meet_the_preconditions(synth, vgg, name):
    _, y = wl.image_case(synth, name)
    ok, near, zero, tied = wl.preconditions(vgg[0], vgg[1], y)
    print(name, "near-zero units:", near)
    assert ok and zero == 0 and tied == 0


def _relu_inputs(net, z):
    """the input of every ReLU of wb_common's DCGAN nn.Sequential"""
    seen = []
    hooks = [m.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().numpy())) for m in net if isinstance(m, torch.nn.ReLU)]
    wc.forward(net, z)
    for h in hooks:
        h.remove()
    return seen


@pytest.mark.parametrize("name", sorted(wl.COMPOSED_CASES))
def test_composed_cases_meet_the_preconditions(synth, name):
    c64, c32 = wl.composed_nets(synth, name)
    z, targets = wl.composed_case(c64, name)
    assert targets.dtype == np.uint8 and targets.shape[1] == 3
    ok, near, zero, tied = wl.preconditions(c64.vgg, c32.vgg, c64.forward(z))
    assert ok and zero == 0 and tied == 0
    if c64.steps is None:
        for h64, h32 in zip(_relu_inputs(c64.gen, z), _relu_inputs(c32.gen, z)):
            small = np.abs(h64) < 1e-3 * np.sqrt(np.mean(h64 ** 2))
            assert (np.abs(h32.astype(np.float64) - h64)[small] <= np.abs(h64)[small] / 8).all()
    else:
        assert wp.flip_margin_ok(c64.gen, c32.gen, z, c64.steps, c64.alpha)[0]


def test_host_gradients_against_differences(synth, vgg):
    """autograd of the float64 loss against its central differences along one direction per row: the image gradient, and the composed one"""
    targets, y = wl.image_case(synth, "16x16")
    g, _ = wl.grad_image(vgg[0], y, targets)
    u = np.random.default_rng(2).standard_normal(y.shape)
    h = 1e-6
    yt, x = torch.from_numpy(y.astype(np.float64)), vgg[0].target(targets)
    with torch.no_grad():
        fd = (vgg[0].loss(yt + h * torch.from_numpy(u), x) - vgg[0].loss(yt - h * torch.from_numpy(u), x)).numpy() / (2 * h)
    assert np.allclose((g * u).reshape(len(y), -1).sum(axis=1), fd, rtol=1e-5, atol=0)
    c64, _ = wl.composed_nets(synth, "pggan_a0.4")
    z, t = wl.composed_case(c64, "pggan_a0.4")
    gz, _ = c64.grad_z(z, t)
    uz = np.random.default_rng(3).standard_normal(z.shape)
    with torch.no_grad():
        lp = c64.vgg.loss(c64.image((torch.from_numpy(z.astype(np.float64)) + h * torch.from_numpy(uz)).reshape(len(z), -1, 1, 1)), c64.vgg.target(t))
        lm = c64.vgg.loss(c64.image((torch.from_numpy(z.astype(np.float64)) - h * torch.from_numpy(uz)).reshape(len(z), -1, 1, 1)), c64.vgg.target(t))
    assert np.allclose((gz * uz).sum(axis=1), (lp - lm).numpy() / (2 * h), rtol=1e-5, atol=0)


def test_search_precondition(synth):
    """the inputs of the GPU search test: on the host (float64 gradients, float32 Adam, 8-bit images, float64 distance) every query whose start
    lies SEARCH_DELTA away from its latent ends at a quarter of its starting distance or less -- measured: 0.062 to 0.085 of it after 16 steps
    at lr 0.05 -- and the trace never rises.  The GPU test asserts a half."""
    c64, _ = wl.composed_nets(synth, "pggan_a1.0")
    z_init, z_image = wc.search_latents(wl.SEARCH_NZ)
    queries = c64.quantize(c64.forward(z_image))
    z_best, S, trace = wl.search(queries, c64, z_init, wl.SEARCH_STEPS, wl.SEARCH_LR)
    print("start", trace[0].tolist(), "final", S.tolist(), "factor", (S[2::3] / trace[0, 2::3]).tolist())
    assert trace.shape == (wl.SEARCH_STEPS + 1, wc.SEARCH_Q) and (np.diff(trace, axis=0) <= 0).all() and np.array_equal(trace[-1], S)
    assert (trace[:, 0::3] == 0).all() and np.array_equal(z_best[0::3], z_init[0::3])
    assert (trace[0, 2::3] > 0).all() and (4 * S[2::3] <= trace[0, 2::3]).all(), (trace[0], S)


class _NoGrad:
    def generate_u8(self, z):
        raise AssertionError("the argument checks must come first")


class _Gen(_NoGrad):
    """enough of a generator for the checks that come before any GPU work"""
    def vjp_z(self, z, cot):
        raise AssertionError("the argument checks must come first")

    l2_grad_z = vjp_z

    @property
    def ctx(self):
        raise AssertionError("the argument checks must come first")


def test_refusals_without_gpu(tmp_path, monkeypatch):
    import ganleaks_amd as gl
    from ganleaks_amd.attack_models import wb
    from ganleaks_amd.gan_models.pggan.model_torch import Generator as PgganGenerator
    from ganleaks_amd.gan_models.vaegan.train import Generator as VaeganGenerator
    q = np.zeros((2, 3, 64, 64), np.uint8)
    z = np.zeros((2, 100), np.float32)
    with pytest.raises(NotImplementedError, match="LPIPS"):                      # wb_attack itself stays on exact l2
        gl.wb_attack(q, _Gen(), z, distance="l2-lpips")
    with pytest.raises(ValueError, match="wb_attack"):
        gl.pair_wb_attack(q, _Gen(), z, distance="l2")
    with pytest.raises(ValueError, match="l2-lpips"):
        gl.pair_wb_attack(q, _Gen(), z, distance="l1")
    with pytest.raises(NotImplementedError, match="VAEGAN"):
        gl.pair_wb_attack(q, VaeganGenerator(100), z)
    with pytest.raises(NotImplementedError, match="vjp_z"):
        gl.pair_wb_attack(q, _NoGrad(), z)
    with pytest.raises(NotImplementedError, match=r"at\(steps, alpha\)"):
        gl.pair_wb_attack(np.zeros((2, 3, 16, 16), np.uint8), PgganGenerator(64, 64, 3), np.zeros((2, 64), np.float32))
    with pytest.raises(NotImplementedError, match="vjp_z"):
        gl.pair_grad_z(_NoGrad(), z, q)
    for kw in (dict(steps=-1), dict(steps=1.5), dict(lr=0.0), dict(lr=float("nan")), dict(beta1=1.0), dict(beta2=-0.1), dict(eps=0.0),
               dict(z_max=float("inf")), dict(block_images=0)):
        with pytest.raises(ValueError):
            gl.pair_wb_attack(q, _Gen(), z, **kw)
    with pytest.raises(ValueError, match="z_init"):
        gl.pair_wb_attack(q, _Gen(), np.zeros((2, 100, 2, 2), np.float32))
    with pytest.raises(ValueError, match="queries"):
        gl.pair_wb_attack(q, _Gen(), np.zeros((3, 100), np.float32))
    with pytest.raises(ValueError, match="multiples of 16"):
        gl.pair_wb_attack(np.zeros((2, 3, 24, 24), np.uint8), _Gen(), z)
    with pytest.raises(ValueError, match="multiples of 16"):
        gl.pair_wb_attack(np.zeros((2, 3, 8, 8), np.uint8), PgganGenerator(64, 64, 3).at(1), np.zeros((2, 64), np.float32))
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit, match="multiple of 16"):
        wb._request(wb.parse_arguments(["--pair_distance", "l2-lpips", "--resolution", "24", "--generator_path", "x.pth", "--num_init", "64"]))
    with pytest.raises(SystemExit):
        wb.parse_arguments(["--pair_distance", "l2", "--generator_path", "x.pth", "--num_init", "64"])
    wb._request(wb.parse_arguments(["--pair_distance", "l2-lpips", "--generator_path", "x.pth", "--num_init", "64"]))
    assert wb.parse_arguments(["--generator_path", "x.pth"]).pair_distance is None
    assert not (tmp_path / "wb_attack").exists()


def test_exports_and_signatures():
    import ganleaks_amd as gl
    from ganleaks_amd import _lib
    from ganleaks_amd.lpips import LpipsModel
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    sym = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, stdout=subprocess.PIPE).stdout.decode()
    exported = {line.split()[-1] for line in sym.splitlines() if line.strip()}
    for name, nargs in (("gl_lpips_ref_dim", 2), ("gl_lpips_ref_rows_u8", 6), ("gl_lpips_grad_image", 9), ("gl_wb_diag_keys", 5)):
        assert name in exported, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    lib = _lib.load()
    assert lib.gl_lpips_ref_dim(64, 64) == lib.gl_lpips_feature_dim(64, 64) - 3 * 64 * 64 == 499712
    assert lib.gl_lpips_ref_dim(32, 16) == lib.gl_lpips_feature_dim(32, 16) - 3 * 32 * 16
    assert lib.gl_lpips_ref_dim(24, 16) == -1 and lib.gl_lpips_ref_dim(16, 8) == -1
    assert callable(gl.pair_wb_attack) and callable(gl.pair_grad_z)
    assert hasattr(LpipsModel, "grad_image") and hasattr(LpipsModel, "reference_rows")
