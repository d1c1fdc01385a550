"""CPU: the host side of tests/test_gpu_wb_vaegan.py and what of the VAEGAN attacks can be checked without a GPU -- the held-sigma restatement of
tests/vaegan_wb_common.py against the stateful float64 oracle, descent on the attack test's own queries, the refusals, the command lines and the
new C entry."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import vaegan_wb_common as vw
import wb_common as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


@pytest.fixture(scope="module")
def sd_small(synth):
    return synth.vaegan_state_dict(z_dim=vw.SMALL[1], d=vw.SMALL[0])


@pytest.mark.parametrize("d,nz", [vw.SMALL, vw.WIDE])
def test_held_restatement_is_the_oracles_kth_forward(synth, d, nz):
    import vaegan_oracle
    sd = synth.vaegan_state_dict(z_dim=nz, d=d)
    z = synth.latent(31, 3).reshape(3, -1)[:, :nz].copy()
    oracle = vaegan_oracle.VaeganOracle(sd)
    for k in (1, 2):
        want = oracle.forward(z)                                   # the oracle's k-th forward: it advances its own state
        net = vw.HeldVaegan(sd, k)
        got = vw.forward(net, z)
        assert got.shape == (3, 3, 64, 64) and np.abs(got - want.astype(np.float64)).max() <= 2.0 ** -23
        assert np.array_equal(vw.forward(net, z), got)             # held: the same function again
        for key, v in net.state.items():
            assert np.abs(v - oracle.sd[key].numpy()).max() <= 1e-12, key
    assert np.abs(vw.forward(vw.HeldVaegan(sd, 1), z) - vw.forward(vw.HeldVaegan(sd, 2), z)).max() > 0


def test_float32_restatement_is_in_float32s_class(sd_small, synth):
    z = synth.latent(32, 2).reshape(2, 100)
    y64, y32 = vw.forward(vw.HeldVaegan(sd_small, 1), z), vw.forward(vw.HeldVaegan(sd_small, 1, torch.float32), z)
    assert y32.dtype == np.float32 and np.abs(y32 - y64).max() < 1e-4
    cot = np.random.default_rng(1).standard_normal((2, 3, 64, 64)).astype(np.float32)
    g64, g32 = vw.vjp_z(vw.HeldVaegan(sd_small, 1), z, cot)[0], vw.vjp_z(vw.HeldVaegan(sd_small, 1, torch.float32), z, cot)[0]
    err = wc.row_errors(g32, g64)
    assert (err > 0).all() and (err < 1e-4).all(), err


@pytest.mark.parametrize("which,d,nz", [("small",) + vw.SMALL, ("wide",) + vw.WIDE])
def test_gradient_cases_keep_every_relu_input_away_from_zero(synth, which, d, nz):
    """the precondition of tests/test_gpu_wb_vaegan.py's gradient cases, and what it excludes: seed 605 of the d = 32 generator has a unit of the last
    hidden layer at -4.7e-8 of an rms of 1.1"""
    sd = synth.vaegan_state_dict(z_dim=nz, d=d)
    net64, net32 = vw.HeldVaegan(sd, 1), vw.HeldVaegan(sd, 1, torch.float32)
    cases = [(k, seed) for k, seed in vw.GRADIENT_CASES.items() if k[0] == which]
    assert sorted((n, chunk) for (_, n, chunk), _ in cases) == [(1, 0), (3, 0), (5, 2)]
    assert len(set(vw.GRADIENT_CASES.values())) == len(vw.GRADIENT_CASES)          # no two cases share their latents
    for (_, n, chunk), seed in cases:
        z, cot, targets = vw.gradient_inputs(net64, nz, n, seed)
        ok, near, smallest = vw.flip_margin_ok(net64, net32, z)
        print(which, n, chunk, seed, ok, near, smallest)
        assert ok and near > 0 and z.shape == (n, nz) and cot.shape == (n, 3, 64, 64) and targets.dtype == np.uint8
    if which == "small":
        z = np.random.default_rng(605).standard_normal((5, nz)).astype(np.float32)
        ok, _, smallest = vw.flip_margin_ok(net64, net32, z)
        assert not ok and smallest < 1e-7


def test_descent_lowers_every_query_of_the_attack_test(sd_small):
    """the precondition of tests/test_gpu_wb_vaegan.py::test_wb_attack: from the bank latent nearest to each query, float32 Adam on float32
    gradients lowers S within the test's steps, for every query; and the nearest bank latent is the one the query was made from, by a margin"""
    net64, net32 = vw.HeldVaegan(sd_small, 1), vw.HeldVaegan(sd_small, 1, torch.float32)
    z_bank, z_query = vw.attack_latents()
    queries = wc.quantize_u8(vw.forward(net64, z_query))
    bank = wc.quantize_u8(vw.forward(net64, z_bank))
    S = ((bank.reshape(len(bank), 1, -1).astype(np.int64) - queries.reshape(1, len(queries), -1).astype(np.int64)) ** 2).sum(axis=2)     # [bank][query]
    order = np.sort(S, axis=0)
    assert np.array_equal(S.argmin(axis=0), np.array(vw.ATTACK_PICK))
    assert (order[1] >= 1.5 * order[0]).all(), (order[0], order[1])         # 8-bit rounding of another arithmetic cannot change the nearest
    z_init = z_bank[list(vw.ATTACK_PICK)]
    _, S32, trace = vw.search(queries, net32, z_init, vw.ATTACK_STEPS, vw.ATTACK_LR)
    print("start", trace[0].tolist(), "final", S32.tolist())
    assert (np.diff(trace, axis=0) <= 0).all()
    assert (4 * trace[-1] <= 3 * trace[0]).all()                            # not by a hair: to three quarters or less


def test_refusals_without_gpu():
    import ganleaks_amd as gl
    from ganleaks_amd.gan_models.vaegan.train import FrozenGenerator, Generator
    q, z = np.zeros((2, 3, 64, 64), np.uint8), np.zeros((2, 100), np.float32)
    g = Generator(100, d=32)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="forwards"):
            g.frozen(bad)
    with pytest.raises(RuntimeError, match="load_state_dict"):
        g.frozen(1)
    # the plain generator is refused as before, with the messages it had
    with pytest.raises(NotImplementedError, match="VAEGAN"):
        gl.wb_attack(q, g, z)
    with pytest.raises(NotImplementedError, match="spectral-norm"):
        gl.pbb_attack(q, g, z)
    assert hasattr(g, "power_iterations") and not hasattr(FrozenGenerator, "power_iterations")
    for name in ("z_dim", "ctx", "image_shape", "forward", "__call__", "forward_device", "generate_u8", "set_precision", "set_chunk", "state_dict",
                 "vjp_z", "l2_grad_z"):
        assert hasattr(FrozenGenerator, name) or name == "z_dim", name
    assert FrozenGenerator.image_shape == (3, 64, 64)


@pytest.mark.parametrize("cli", ["wb", "pbb"])
def test_cli_needs_sn_forwards(cli, tmp_path, monkeypatch):
    import importlib
    mod = importlib.import_module("ganleaks_amd.attack_models." + cli)
    monkeypatch.chdir(tmp_path)
    base = ["--gan", "vaegan", "--generator_path", "x.pth", "--num_init", "64"]
    with pytest.raises(SystemExit, match=r"vaegan.*--sn_forwards"):
        mod._request(mod.parse_arguments(base))
    with pytest.raises(SystemExit, match=r"vaegan.*--sn_forwards"):
        mod.main(mod.parse_arguments(base))
    assert not (tmp_path / (cli + "_attack")).exists()              # refused before anything is written
    mod._request(mod.parse_arguments(base + ["--sn_forwards", "1"]))
    mod._request(mod.parse_arguments(base + ["--sn_forwards", "3", "--pair_distance", "l2-lpips"]))
    with pytest.raises(SystemExit, match="at least 1"):
        mod._request(mod.parse_arguments(base + ["--sn_forwards", "0"]))
    with pytest.raises(SystemExit, match="64"):
        mod._request(mod.parse_arguments(base + ["--sn_forwards", "1", "--resolution", "32"]))
    with pytest.raises(SystemExit, match="vaegan"):
        mod._request(mod.parse_arguments(["--gan", "dcgan", "--generator_path", "x.pth", "--num_init", "64", "--sn_forwards", "1"]))
    assert mod.parse_arguments([]).sn_forwards is None              # no default
    doc = mod.__doc__
    assert "--sn_forwards" in doc and "vaegan" in doc


def test_new_symbol_is_declared_exported_and_bound():
    from ganleaks_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    proto = re.search(r"int\s+gl_dcgan_advance_spectral\s*\(([^)]*)\)\s*;", header)
    assert proto, "gl_dcgan_advance_spectral is not declared in ganleaks.h"
    args = [a.strip() for a in proto.group(1).split(",")]
    assert args == ["gl_dcgan *g", "int times"]
    assert len(_lib.SIGNATURES["gl_dcgan_advance_spectral"][1]) == len(args)
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    assert hasattr(lib, "gl_dcgan_advance_spectral")
