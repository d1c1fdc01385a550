"""CPU-only: the partial-black-box attack under 0.2 * LPIPS + L2 -- the export of gl_pbb_group_min_keys in the cross-compiled library, the
ctypes table and the header; the refusals of pair_pbb_attack and of the command line that need no GPU; the host restatement of the grouped
minimum (tests/pair_pbb_common.py) against two plain loops; and the precondition of the GPU search test."""
import os
import re
import subprocess

import numpy as np
import pytest

import pair_pbb_common as pp
import wb_common as wc
import wb_lpips_common as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_and_signatures():
    import ganleaks_amd as gl
    from ganleaks_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    sym = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, stdout=subprocess.PIPE).stdout.decode()
    exported = {line.split()[-1] for line in sym.splitlines() if line.strip()}
    assert "gl_pbb_group_min_keys" in exported
    assert len(_lib.SIGNATURES["gl_pbb_group_min_keys"][1]) == 7
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"\bint\s+gl_pbb_group_min_keys\s*\(\s*gl_ctx\s*\*ctx,\s*const\s+float\s*\*M_dev,\s*int64_t\s+nq,\s*int64_t\s+lambda,\s*int64_t\s+ld,"
                     r"\s*uint64_t\s*\*keys_dev,\s*int32_t\s*\*j_dev\s*\)\s*;", header)
    assert int(re.search(r"#define\s+GL_ABI_VERSION\s+(\d+)", header).group(1)) == 1
    assert callable(gl.pair_pbb_attack) and callable(gl.pair_pbb_init_from_bank)
    from ganleaks_amd import pbb
    assert gl.pair_pbb_attack is pbb.pair_pbb_attack and gl.pair_pbb_init_from_bank is pbb.pair_pbb_init_from_bank


class _NoGenerate:
    pass


class _Gen:
    """enough of a generator for the checks that come before any GPU work"""
    def generate_u8(self, z):
        raise AssertionError("the argument checks must come first")

    @property
    def ctx(self):
        raise AssertionError("the argument checks must come first")


def test_pair_pbb_attack_refusals_without_gpu():
    import ganleaks_amd as gl
    from ganleaks_amd.gan_models.vaegan.train import Generator as VaeganGenerator
    q = np.zeros((2, 3, 64, 64), np.uint8)
    z = np.zeros((2, 100), np.float32)
    with pytest.raises(ValueError, match="pbb_attack"):
        gl.pair_pbb_attack(q, _Gen(), z, distance="l2")
    with pytest.raises(ValueError, match="l2-lpips"):
        gl.pair_pbb_attack(q, _Gen(), z, distance="l1")
    with pytest.raises(TypeError, match="generate_u8"):
        gl.pair_pbb_attack(q, _NoGenerate(), z)
    with pytest.raises(NotImplementedError, match="spectral-norm"):
        gl.pair_pbb_attack(q, VaeganGenerator(100), z)
    for shape in ((2, 3, 24, 64), (2, 3, 64, 40), (2, 1, 64, 64), (2, 3, 8, 8), (2, 3 * 64 * 64)):
        with pytest.raises(ValueError, match="multiples of 16"):
            gl.pair_pbb_attack(np.zeros(shape, np.uint8), _Gen(), z)
    for kw in (dict(rounds=-1), dict(rounds=1.5), dict(population=0), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")),
               dict(sigma=float("inf")), dict(query_base=(1 << 32) - 1), dict(query_base=-1), dict(sigma_min=5.0), dict(z_max=0.0), dict(up=0.0),
               dict(down=float("nan")), dict(block_images=0)):
        with pytest.raises(ValueError):
            gl.pair_pbb_attack(q, _Gen(), z, **kw)
    with pytest.raises(ValueError, match="z_init"):
        gl.pair_pbb_attack(q, _Gen(), np.zeros((2, 100, 2, 2), np.float32))
    with pytest.raises(ValueError, match="queries"):
        gl.pair_pbb_attack(q, _Gen(), np.zeros((3, 100), np.float32))
    # pbb_attack keeps refusing the distance, and says where it lives
    with pytest.raises(NotImplementedError, match="LPIPS.*pair_pbb_attack"):
        gl.pbb_attack(q, _Gen(), z, distance="l2-lpips")


def test_cli_refusals_without_gpu(tmp_path, monkeypatch):
    from ganleaks_amd.attack_models import pbb
    monkeypatch.chdir(tmp_path)
    assert pbb.parse_arguments([]).pair_distance is None
    base = ["--generator_path", str(tmp_path / "nowhere.pth"), "--num_init", "64"]
    with pytest.raises(SystemExit):
        pbb.main(pbb.parse_arguments(base + ["--pair_distance", "l2"]))
    with pytest.raises(SystemExit, match="multiple of 16"):
        pbb.main(pbb.parse_arguments(base + ["--resolution", "24", "--pair_distance", "l2-lpips"]))
    # a value that did not come through the parser (the YAML overlay)
    args = pbb.parse_arguments(base)
    args.pair_distance = "l2"
    with pytest.raises(SystemExit, match="l2-lpips"):
        pbb.main(args)
    assert not (tmp_path / "pbb_attack").exists()
    assert pbb.LATER_OPTIONS == ("pair_distance",)


def test_group_min_keys_restated():
    f32, inf = np.float32, np.float32(np.inf)
    # ties: the smallest j wins; +inf is the largest pattern of a distance; columns past nq * lam are not read
    M = np.full((3, 13), 9.0, f32)
    M[0, 0:4] = [2.0, 1.0, 1.0, 3.0]                       # a tie at j = 1, 2
    M[1, 4:8] = [inf, 5.0, 7.0, 5.0]                       # +inf next to a tie at j = 1, 3
    M[2, 8:12] = [inf, inf, inf, inf]                      # nothing but +inf: j = 0
    M[:, 12] = 0.0                                         # the padding column holds the smallest value of all
    M[0, 4:12] = 0.0                                       # so do other queries' columns
    keys, j = pp.group_min_keys(M, 4)
    assert keys.dtype == np.int64 and j.dtype == np.int32
    assert j.tolist() == [1, 1, 0] and keys.tolist() == [int(f32(1.0).view(np.uint32)), int(f32(5.0).view(np.uint32)), 0x7F800000]
    for got, want in zip((keys, j), pp.group_min_keys_brute(M, 4)):
        assert np.array_equal(got, want)
    # random matrices with many ties (values from a set of 4), ld > nq * lam, lam no power of two
    rng = np.random.default_rng(5)
    for nq, lam, ld in ((1, 1, 1), (7, 3, 25), (5, 64, 320), (9, 70, 650)):
        R = rng.choice(np.array([0.0, 0.5, 2.0, np.inf], f32), size=(nq, ld))
        for got, want in zip(pp.group_min_keys(R, lam), pp.group_min_keys_brute(R, lam)):
            assert np.array_equal(got, want)
    # the order of the patterns is the order of the non-negative floats, denormals and +0 included
    v = np.array([0.0, 1e-45, 1e-38, 1.0, 3e38, np.inf], f32)
    assert (np.diff(pp.bits32(v)) > 0).all()
    # lambda = 1 is the diagonal
    D = rng.random((6, 9)).astype(f32)
    keys, j = pp.group_min_keys(D, 1)
    assert np.array_equal(keys, pp.bits32(np.diag(D[:, :6]))) and (j == 0).all()


def test_search_precondition(synth):
    """the inputs of the GPU search test: on the host (pbb_common's candidates and accept rule, 8-bit images, the float64 distance) 16 rounds
    of 5 candidates from sigma = 1 / 16 do not halve the distance of the queries whose start lies SEARCH_DELTA away from their latent -- a
    gradient-free search in 64 dimensions gains about a percent of |z - z*| per round -- they end at 0.675 to 0.689 of it (measured; at
    lambda = 16 and sigma = 0.06 it is 0.57 to 0.70): the factor asserted is three quarters.  Queries that are their own start stay at 0 and at z_init, and the trace
    never rises.  The GPU test asserts a strict improvement."""
    c64, _ = wl.composed_nets(synth, "pggan_a1.0")
    z_init, z_image = wc.search_latents(wl.SEARCH_NZ)
    queries = c64.quantize(c64.forward(z_image))
    z_star, S, trace = pp.host_search(queries, c64, z_init, pp.SEARCH_ROUNDS, pp.SEARCH_LAMBDA, pp.SEARCH_SIGMA, pp.SEARCH_SEED)
    print("start", trace[0].tolist(), "final", S.tolist(), "factor", (S[2::3] / trace[0, 2::3]).tolist())
    assert pp.SEARCH_ROUNDS <= 16 and pp.SEARCH_LAMBDA <= 16
    assert trace.shape == (pp.SEARCH_ROUNDS + 1, wc.SEARCH_Q) and (np.diff(trace, axis=0) <= 0).all() and np.array_equal(trace[-1], S)
    assert (trace[:, 0::3] == 0).all() and np.array_equal(z_star[0::3], z_init[0::3])
    assert (trace[0, 2::3] > 0).all() and (S[2::3] <= 0.75 * trace[0, 2::3]).all(), (trace[0], S)
    assert (S[1::3] < trace[0, 1::3]).all()
