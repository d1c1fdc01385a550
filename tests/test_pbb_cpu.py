"""CPU-only: the host restatements behind the partial-black-box tests (tests/pbb_common.py) against published and derived facts, the
argument refusals of pbb_attack that need no GPU, and the three exports in the cross-compiled library and the ctypes table."""
import os
import re
import subprocess

import numpy as np
import pytest

import pbb_common as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


def test_philox_known_answers():
    """the Philox4x32-10 known-answer vectors of the Random123 distribution (kat_vectors)"""
    ones = 0xFFFFFFFF
    assert _hex(pc.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(pc.philox4x32_10((ones, ones, ones, ones), (ones, ones))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    # lanes are independent: the same two answers from one vector call
    w = pc.philox4x32_10(tuple(np.array([0, ones], np.uint64) for _ in range(4)), (np.array([0, ones], np.uint64),) * 2)
    assert _hex(x[0] for x in w) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8" and _hex(x[1] for x in w) == "408f276d 41c83b0e a20bc7c6 6d5451fd"


def test_noise_moments_and_scale():
    header = open(os.path.join(ROOT, "include", "ganleaks.h")).read()
    bits = int(re.search(r"#define\s+GL_PBB_NOISE_SCALE_BITS\s+(0x[0-9A-Fa-f]+)u", header).group(1), 16)
    assert pc.C.dtype == np.float32 and int(pc.C.view(np.uint32)) == bits
    assert pc.C == np.float32(1.0 / (65536.0 * np.sqrt(8.0 / 3.0)))
    t = pc.noise_t(0x123456789ABCDEF0, 3, np.arange(100, dtype=np.uint64)[:, None, None], np.arange(100, dtype=np.uint64)[None, :, None],
                   np.arange(100, dtype=np.uint64)[None, None, :])
    assert t.dtype == np.int32 and t.size == 10 ** 6 and np.abs(t).max() <= 524280 and (t % 2 == 0).all()
    eps = pc.noise(0x123456789ABCDEF0, 3, np.arange(100, dtype=np.uint64)[:, None, None], np.arange(100, dtype=np.uint64)[None, :, None],
                   np.arange(100, dtype=np.uint64)[None, None, :])
    assert eps.dtype == np.float32 and np.array_equal(eps, t.astype(np.float32) * pc.C)
    e = eps.astype(np.float64)
    assert abs(e.mean()) < 0.01 and abs(e.var() - 1.0) < 0.01, (e.mean(), e.var())
    assert np.abs(e).max() <= 524280 * float(pc.C) < 4.9
    # a function of the five indices: another seed, round or query gives other values; the query index counts modulo 2^32
    base = pc.noise(7, 1, 5, np.arange(8), np.arange(16)[:, None])
    for other in (pc.noise(8, 1, 5, np.arange(8), np.arange(16)[:, None]), pc.noise(7, 2, 5, np.arange(8), np.arange(16)[:, None]),
                  pc.noise(7, 1, 6, np.arange(8), np.arange(16)[:, None]), pc.noise(7 + (1 << 32), 1, 5, np.arange(8), np.arange(16)[:, None])):
        assert not np.array_equal(base, other)
    assert np.array_equal(base, pc.noise(7, 1, 5 + (1 << 32), np.arange(8), np.arange(16)[:, None]))


def test_candidates_restated():
    z = np.random.default_rng(1).standard_normal((3, 10)).astype(np.float32)
    sigma = np.array([0.5, 1e-4, 50.0], np.float32)
    c = pc.candidates(z, sigma, 7, 11, 2, 5, 4.0)
    assert c.shape == (21, 10) and c.dtype == np.float32 and np.abs(c).max() <= 4.0 and (np.abs(c[14:]) == 4.0).any()
    eps = pc.noise(11, 2, 6, 3, np.arange(10))
    want = np.float32(z[1] + np.float32(sigma[1] * eps))
    assert np.array_equal(c[7 + 3], np.clip(want, -4.0, 4.0))
    # the rows of a query do not depend on which other queries are submitted with it
    assert np.array_equal(pc.candidates(z[1:], sigma[1:], 7, 11, 2, 6, 4.0), c[7:])


def test_host_accept_rule():
    f32 = np.float32
    z = np.zeros((4, 2), f32)
    cand = np.arange(4 * 3 * 2, dtype=f32).reshape(12, 2)
    sigma = np.array([0.5, 0.5, 3.9, 1.1e-4], f32)
    S_cur = np.array([10, 10, 10, 10], np.int64)
    S_new = np.array([9, 10, 0, 11], np.int64)             # closer / tie (strict <: not taken) / closer / farther
    j_new = np.array([2, 1, 0, 1], np.int32)
    up, down = 1.5, 1.5 ** -0.25
    z2, s2, S2, take = pc.accept(z, sigma, S_cur, cand, S_new, j_new, 3, up, down, 1e-4, 4.0)
    assert take.tolist() == [True, False, True, False] and S2.tolist() == [9, 10, 0, 10] and s2.dtype == f32 and z2.dtype == f32
    assert np.array_equal(z2, np.stack([cand[2], z[1], cand[6], z[3]]))
    assert s2[0] == f32(f32(0.5) * f32(up)) and s2[1] == f32(f32(0.5) * f32(down))
    assert s2[2] == f32(4.0) and f32(f32(3.9) * f32(up)) > 4.0                     # clamped from above
    assert s2[3] == f32(1e-4) and f32(f32(1.1e-4) * f32(down)) < f32(1e-4)         # and from below
    assert z[0, 0] == 0 and S_cur[0] == 10 and sigma[0] == 0.5                     # the inputs are left alone
    # group_min: the first minimum on a tie
    q = np.array([[1, 2, 3], [0, 0, 0]], np.uint8)
    c = np.array([[1, 2, 4], [1, 2, 3], [1, 2, 3], [255, 255, 255], [255, 255, 255], [255, 255, 254]], np.uint8)
    S, j, allS = pc.group_min(q, c, 3)
    assert S.tolist() == [0, 2 * 65025 + 254 * 254] and j.tolist() == [1, 2] and allS.shape == (2, 3)


class _NoGenerate:
    pass


class _Gen:
    """enough of a generator for the checks that come before any GPU work"""
    def generate_u8(self, z):
        raise AssertionError("the argument checks must come first")

    @property
    def ctx(self):
        raise AssertionError("the argument checks must come first")


def test_pbb_attack_refusals_without_gpu():
    import ganleaks_amd as gl
    from ganleaks_amd.gan_models.vaegan.train import Generator as VaeganGenerator
    q = np.zeros((2, 3, 64, 64), np.uint8)
    z = np.zeros((2, 100), np.float32)
    with pytest.raises(TypeError, match="generate_u8"):
        gl.pbb_attack(q, _NoGenerate(), z)
    with pytest.raises(NotImplementedError, match="spectral-norm"):
        gl.pbb_attack(q, VaeganGenerator(100), z)
    with pytest.raises(NotImplementedError, match="LPIPS"):
        gl.pbb_attack(q, _Gen(), z, distance="l2-lpips")
    with pytest.raises(ValueError):
        gl.pbb_attack(q, _Gen(), z, distance="l1")
    for kw in (dict(rounds=-1), dict(population=0), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")),
               dict(query_base=(1 << 32) - 1), dict(sigma_min=5.0), dict(z_max=0.0)):
        with pytest.raises(ValueError):
            gl.pbb_attack(q, _Gen(), z, **kw)
    with pytest.raises(ValueError, match="z_init"):
        gl.pbb_attack(q, _Gen(), np.zeros((2, 100, 2, 2), np.float32))
    with pytest.raises(ValueError, match="queries"):
        gl.pbb_attack(q, _Gen(), np.zeros((3, 100), np.float32))


def test_cli_refusals_without_gpu(tmp_path):
    from ganleaks_amd.attack_models import pbb
    with pytest.raises(SystemExit, match="generator_path"):
        pbb.main(pbb.parse_arguments(["--num_init", "64"]))
    for extra in ([], ["--noise_path", "x.npz", "--num_init", "64"], ["--num_init", "0"], ["--num_init", "64", "--population", "0"],
                  ["--num_init", "64", "--sigma", "0"]):
        with pytest.raises(SystemExit):
            pbb.main(pbb.parse_arguments(["--generator_path", str(tmp_path / "nowhere.pth")] + extra))
    assert not (tmp_path / "pbb_attack").exists()


def test_exports_and_signatures():
    from ganleaks_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    names = ("gl_pbb_candidates", "gl_pbb_group_min", "gl_pbb_accept")
    sym = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, stdout=subprocess.PIPE).stdout.decode()
    exported = {line.split()[-1] for line in sym.splitlines() if line.strip()}
    for name in names:
        assert name in exported, name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["gl_pbb_candidates"][1]) == 11 and len(_lib.SIGNATURES["gl_pbb_group_min"][1]) == 9
    assert len(_lib.SIGNATURES["gl_pbb_accept"][1]) == 15
    from ganleaks_amd import pbb
    header = open(_lib.HEADER_PATH).read()
    assert int(re.search(r"#define\s+GL_PBB_GROUP\s+(\d+)", header).group(1)) == pbb.GL_PBB_GROUP
    assert int(re.search(r"#define\s+GL_PBB_PARTIAL_BYTES\s+(\d+)", header).group(1)) == pbb.GL_PBB_PARTIAL_BYTES
