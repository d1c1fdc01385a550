"""CPU-only: Powell's method in the partial-black-box attacks -- the restatement of tests/pbb_powell_common.py on problems whose answers are
worked out by hand (a separable quadratic it must solve exactly in one sweep, Numerical Recipes' test on hand-computed quadruples, a rotated
valley whose new direction and widths are written out), the key never rising, the refusals of pbb_attack, pair_pbb_attack and the command
line that need no GPU, params.txt, and the exports of the cross-compiled library."""
import os
import re
import subprocess

import numpy as np
import pytest

import pbb_powell_common as pc

f32 = np.float32


def _exact(fn):
    """generate = the identity; score = 64 * fn(z) per candidate, an exact integer for latents on the 1/8 lattice"""
    def score(queries, images, lam):
        keys = np.array([64.0 * fn(z, queries[i // lam]) for i, z in enumerate(images)])
        assert (keys == np.round(keys)).all() and (keys >= 0).all()
        return pc.group_min(keys.astype(np.uint64), lam)
    return score


def test_separable_quadratic_in_one_sweep():
    """f = sum a_c (z_c - m_c)^2 from z = 0 with every m_c in {+-1, +-1/2, +-1/4, +-1/8}, step0 = 1, ladder = 8: the ladder of line c is
    exactly that set, so line c lands on m_c and one sweep ends at f = 0.  Then z_e = 2 m has f_E = f_0: the displacement is not taken"""
    m = np.array([[1, -1, .5, -.5, .25, -.25, .125, -.125], [-.125, .25, 1, -1, -.5, .125, .5, -.25]], f32)
    a = np.arange(1, 9, dtype=np.float64)
    score = _exact(lambda z, target: float((a * (z.astype(np.float64) - target) ** 2).sum()))
    seen = []
    z, keys, trace, st = pc.search(m, lambda lat: lat, score, np.zeros((2, 8), f32), sweeps=1, ladder=8, step0=1.0, z_max=4.0,
                                   on_line=lambda s, i: seen.append(s.S_cur.copy()))
    assert np.array_equal(z, m) and keys.tolist() == [0, 0] and trace.shape == (2, 2)
    assert trace[0].tolist() == [int(64 * (a * m[q].astype(np.float64) ** 2).sum()) for q in range(2)]
    assert st.flag.tolist() == [0, 0] and np.array_equal(st.t[:, 8], np.full(2, pc.T_MIN, f32))      # rejected from a width of 0: max(t_min, 0)
    U0, _ = pc.init(2, 8, 1.0)
    assert np.array_equal(st.U[:, :8], U0[:, :8]) and np.array_equal(st.U[:, 8], m)
    # accepted at rung r: t = 2 * 2^-(r >> 1), and |m_c| = 2^-(r >> 1)
    assert np.array_equal(st.t[:, :8], 2 * np.abs(m))
    assert (np.diff(np.stack(seen).astype(np.int64), axis=0) <= 0).all()


def test_decide_on_hand_computed_quadruples():
    # (f0, fN, fE, delta): A = f0 - 2 fN + fE, B = f0 - fN - delta, C = f0 - fE; held iff fE < f0 and 2 A B^2 < delta C^2
    assert pc.decide_test(16, 4, 0, 9)                   # A = 8, B = 3, C = 16: 144 < 2304
    assert not pc.decide_test(16, 4, 0, 1)               # A = 8, B = 11: 1936 >= 256
    assert not pc.decide_test(16, 4, 16, 9)              # fE == f0: the first clause is strict
    assert not pc.decide_test(10, 12, 10, 1)             # fE == f0 where the second clause holds: A = -4, B = -3, C = 0: -72 < 0
    assert not pc.decide_test(16, 4, 17, 12)             # fE > f0 alone: B = 0, so the second clause would hold (0 < 12)
    assert not pc.decide_test(10, 4, 6, 4)               # A = 8, B = 2, C = 4: 64 == 64, the second clause is strict
    assert pc.decide_test(10, 4, 6, 5)                   # B = 1: 16 < 80
    assert not pc.decide_test(10, 4, 6, 3)               # B = 3: 144 >= 48
    assert not pc.decide_test(10, 10, 10, 0)             # nothing moved: fE == f0
    # the second clause alone decides where the first holds: fE just below f0
    assert pc.decide_test(16, 4, 15, 12) and not pc.decide_test(16, 4, 15, 0)      # A = 23, B = 0 -> 0 < 12; delta = 0 -> rhs = 0
    # through decide(): keys of both kinds, and a displacement of zero clears the flag whatever the keys say
    for kind, enc in ((0, lambda v: np.uint64(v)), (1, lambda v: np.uint64(np.array([v], f32).view(np.uint32)[0]))):
        st = pc.State(np.zeros((3, 2), f32))
        st.f0[:], st.S_cur[:], st.S_e[:] = enc(16), enc(4), enc(0)
        st.S_e[1] = enc(16)
        st.drop_best[:] = 9.0
        st.U[0, 2], st.U[1, 2] = (1, 1), (1, 1)          # query 2: dz = 0
        pc.decide(st, kind)
        assert st.flag.tolist() == [1, 0, 0] and st.t[:, 2].tolist() == [2.0, 0.0, 0.0]
    assert pc.key_value(np.uint64(np.array([0.375], f32).view(np.uint32)[0]), 1) == 0.375 and pc.key_value(np.uint64((1 << 53) - 1), 0) == 2.0 ** 53 - 1


def test_rotated_valley_new_direction():
    """f = 4 (x - y)^2 + (x + y - 4)^2, a valley along x = y towards (2, 2), from (0, 1) with step0 = 1, ladder = 8; keys are 64 f.
    line 0 from (0, 1), f = 13: x = 1 gives f = 4 (rung 0), drop 9, t[0] = 2.
    line 1 from (1, 1): y = 1 + a has f = 4 a^2 + (a - 2)^2: a = 1/2 gives 3.25 (a = 1: 5, a = 1/4: 3.3125), rung 2, drop 0.75, t[1] = 2 * 1/2 = 1.
    The coordinate lines crawl: f is still 3.25.  dz = (1, 1/2), z_e = (2, 2), fE = 0 < 13; A = 13 - 6.5 + 0 = 6.5, B = 13 - 3.25 - 9 = 0.75,
    2 A B^2 = 7.3125 < 9 * 169: the displacement is taken, t[2] = 2.  line 2 along (1, 1/2) at widths +-2, +-1, ...: +1 is (2, 2), f = 0,
    rung 2, t[2] = 2 * 2 * 1/2 = 2.  replace: i_best = 0, so row 0 <- row 1 = (0, 1) with t = 1, row 1 <- row 2 = (1, 1/2) with t = 2."""
    fn = lambda z, target: float(4 * (float(z[0]) - float(z[1])) ** 2 + (float(z[0]) + float(z[1]) - 4) ** 2)      # noqa: E731
    seen = []
    z, keys, trace, st = pc.search(np.zeros((1, 2), f32), lambda lat: lat, _exact(fn), np.array([[0, 1]], f32), sweeps=1, ladder=8, step0=1.0,
                                   z_max=4.0, on_line=lambda s, i: seen.append((i, int(s.S_cur[0]), s.t[0].tolist(), int(s.i_best[0]), float(s.drop_best[0]))))
    assert seen[0] == (0, 256, [2.0, 1.0, 0.0], 0, 576.0)
    assert seen[1] == (1, 208, [2.0, 1.0, 0.0], 0, 576.0)
    assert seen[2] == (2, 0, [2.0, 1.0, 2.0], 0, 576.0)
    assert trace[:, 0].tolist() == [832, 0] and z.tolist() == [[2.0, 2.0]] and keys.tolist() == [0]
    assert st.flag.tolist() == [1] and st.i_best.tolist() == [0]
    assert st.U[0].tolist() == [[0.0, 1.0], [1.0, 0.5], [1.0, 0.5]]
    assert st.t[0].tolist() == [1.0, 2.0, 2.0]


def _toy_generator(seed, nz, d):
    """a small fixed map from latents to 8-bit 'images', and exact sums of squared differences as the score"""
    W = np.random.default_rng(seed).standard_normal((d, nz))

    def generate(lat):
        return np.clip(np.rint(128.0 + 40.0 * np.tanh(np.asarray(lat, np.float64) @ W.T)), 0, 255).astype(np.int64)

    def score(queries, images, lam):
        S = ((images - np.repeat(queries, lam, axis=0)) ** 2).sum(axis=1)
        return pc.group_min(S.astype(np.uint64), lam)

    return generate, score


def test_key_never_rises():
    rng = np.random.default_rng(5)
    nq, nz = 6, 5
    generate, score = _toy_generator(1, nz, 48)
    queries = generate(rng.standard_normal((nq, nz)))
    seen = []
    z, keys, trace, st = pc.search(queries, generate, score, rng.standard_normal((nq, nz)).astype(f32), sweeps=3, ladder=4,
                                   on_line=lambda s, i: seen.append(s.S_cur.astype(np.int64)))
    seen = np.stack(seen)
    assert len(seen) == 3 * (nz + 1) and (np.diff(seen, axis=0) <= 0).all() and (seen[0] <= trace[0]).all()
    assert (np.diff(trace, axis=0) <= 0).all() and (trace[-1] < trace[0]).all() and np.array_equal(trace[-1], keys)
    assert np.array_equal(keys, ((generate(z) - queries) ** 2).sum(axis=1)) and np.abs(z).max() <= pc.Z_MAX
    assert st.flag.dtype == np.uint8 and (st.t[:, :nz] >= f32(pc.T_MIN)).all() and (st.t <= f32(pc.T_MAX)).all()


class _Reached(Exception):
    pass


class _Gen:
    """enough of a generator for the checks that come before any GPU work"""
    def generate_u8(self, z, **kw):
        raise AssertionError("the argument checks must come first")

    @property
    def ctx(self):
        raise _Reached()


BAD = (dict(optimizer="sgd"), dict(optimizer=None), dict(optimizer="Powell"), dict(optimizer="lbfgs"),
       dict(optimizer="powell", sweeps=-1), dict(optimizer="powell", sweeps=1.5), dict(optimizer="powell", sweeps=float("nan")),
       dict(optimizer="powell", ladder=0), dict(optimizer="powell", ladder=1), dict(optimizer="powell", ladder=7), dict(optimizer="powell", ladder=34),
       dict(optimizer="powell", ladder=4.5), dict(optimizer="powell", step0=0.0), dict(optimizer="powell", step0=-1.0),
       dict(optimizer="powell", step0=float("nan")), dict(optimizer="powell", step0=float("inf")),
       # Powell's keywords belong to it
       dict(sweeps=3), dict(optimizer="es", ladder=4), dict(step0=0.5),
       # and the evolution strategy's are refused where they were changed
       dict(optimizer="powell", population=32), dict(optimizer="powell", sigma=0.25), dict(optimizer="powell", up=2.0), dict(optimizer="powell", down=0.5),
       # what both optimisers check stays
       dict(optimizer="powell", z_max=0.0), dict(optimizer="powell", block_images=0), dict(optimizer="powell", sigma_min=8.0))


def test_refusals_without_gpu():
    import ganleaks_amd as gl
    q = np.zeros((2, 3, 64, 64), np.uint8)
    z = np.zeros((2, 100), np.float32)
    for kw in BAD:
        with pytest.raises(ValueError):
            gl.pbb_attack(q, _Gen(), z, **kw)
        with pytest.raises(ValueError):
            gl.pair_pbb_attack(q, _Gen(), z, **kw)
    for fn in (gl.pbb_attack, gl.pair_pbb_attack):
        with pytest.raises(ValueError, match="optimizer"):
            fn(q, _Gen(), z, optimizer="nelder-mead")
        with pytest.raises(ValueError, match="sweeps"):
            fn(q, _Gen(), z, optimizer="powell", sweeps=-1)
        with pytest.raises(ValueError, match="ladder"):
            fn(q, _Gen(), z, optimizer="powell", ladder=7)
        with pytest.raises(ValueError, match="step0"):
            fn(q, _Gen(), z, optimizer="powell", step0=0.0)
        with pytest.raises(ValueError, match="ladder"):
            fn(q, _Gen(), z, ladder=4)
        with pytest.raises(ValueError, match="population"):
            fn(q, _Gen(), z, optimizer="powell", population=32)
        # at their defaults the other optimiser's keywords pass, and so do seed and query_base: the checks end and the GPU is asked for
        for kw in (dict(optimizer="powell"), dict(optimizer="powell", sweeps=0, ladder=32, step0=0.5, seed=7, query_base=11, population=64, sigma=0.5),
                   dict(optimizer="es", sweeps=2, ladder=8, step0=1.0), dict()):
            with pytest.raises(_Reached):
                fn(q, _Gen(), z, **kw)
    # the refusals the two entries had come first and stay
    with pytest.raises(NotImplementedError, match="pair_pbb_attack"):
        gl.pbb_attack(q, _Gen(), z, optimizer="powell", distance="l2-lpips")
    with pytest.raises(ValueError, match="queries"):
        gl.pbb_attack(q, _Gen(), np.zeros((3, 100), np.float32), optimizer="powell")


def test_cli_refusals_and_params_without_gpu(tmp_path, monkeypatch):
    from ganleaks_amd.attack_models import pbb
    monkeypatch.chdir(tmp_path)
    base = ["--generator_path", str(tmp_path / "nowhere.pth"), "--num_init", "64"]
    for extra in (["--sweeps", "1"], ["--ladder", "4"], ["--step0", "1.0"], ["--optimizer", "es", "--sweeps", "1"], ["--optimizer", "powell", "--sweeps", "-1"],
                  ["--optimizer", "powell", "--ladder", "7"], ["--optimizer", "powell", "--ladder", "0"], ["--optimizer", "powell", "--ladder", "34"],
                  ["--optimizer", "powell", "--step0", "0"], ["--optimizer", "powell", "--step0", "nan"], ["--optimizer", "lbfgs"]):
        with pytest.raises(SystemExit):
            pbb.main(pbb.parse_arguments(base + extra))
    for flag in ("sweeps", "ladder", "step0"):
        with pytest.raises(SystemExit, match="--%s belongs to --optimizer powell" % flag):
            pbb._request(pbb.parse_arguments(base + ["--%s" % flag, "2"]))
        with pytest.raises(SystemExit, match=flag):
            pbb._request(pbb.parse_arguments(base + ["--optimizer", "es", "--%s" % flag, "2"]))
    with pytest.raises(SystemExit, match="ladder"):
        pbb._request(pbb.parse_arguments(base + ["--optimizer", "powell", "--ladder", "7"]))
    pbb._request(pbb.parse_arguments(base))
    pbb._request(pbb.parse_arguments(base + ["--optimizer", "es"]))
    pbb._request(pbb.parse_arguments(base + ["--optimizer", "powell"]))
    pbb._request(pbb.parse_arguments(base + ["--optimizer", "powell", "--sweeps", "0", "--ladder", "32", "--step0", "0.5"]))
    assert pbb._optimizer_keywords(pbb.parse_arguments(base)) == {}
    assert pbb._optimizer_keywords(pbb.parse_arguments(base + ["--optimizer", "es"])) == {}
    assert pbb._optimizer_keywords(pbb.parse_arguments(base + ["--optimizer", "powell", "--ladder", "4"])) == dict(optimizer="powell", sweeps=2, ladder=4,
                                                                                                                  step0=1.0)
    # params.txt of a run without the new flags: the lines it had, no new one
    keys = [line.split(":", 1)[0] for line in pbb._params_lines(pbb.parse_arguments(base))]
    assert keys == ["exp_name", "pos_data_dir", "neg_data_dir", "resolution", "BATCH_SIZE", "local_config", "gan", "generator_path", "nz", "ngf", "nc",
                    "in_channels", "steps", "alpha", "noise_path", "num_init", "init_seed", "rounds", "population", "sigma", "seed"]
    lines = pbb._params_lines(pbb.parse_arguments(base + ["--optimizer", "powell", "--sweeps", "1"]))
    assert lines[-2:] == ["optimizer:powell", "sweeps:1"] and len(lines) == len(keys) + 2
    assert not (tmp_path / "pbb_attack").exists()
    # the white-box command line keeps refusing it
    from ganleaks_amd.attack_models import wb
    with pytest.raises(SystemExit):
        wb.parse_arguments(base + ["--optimizer", "powell"])


NARGS = dict(init=6, begin=10, candidates=10, advance=15, extrapolate=8, decide=11, replace=7)


def test_exports_and_signatures():
    import inspect
    import ganleaks_amd as gl
    from ganleaks_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    sym = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, stdout=subprocess.PIPE).stdout.decode()
    exported = {line.split()[-1] for line in sym.splitlines() if line.strip()}
    with open(_lib.HEADER_PATH) as handle:
        header = re.sub(r"/\*.*?\*/", "", handle.read(), flags=re.S)
    for short, nargs in NARGS.items():
        name = "gl_pbb_powell_" + short
        assert name in exported, name
        declared = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert declared is not None and len(declared.group(1).split(",")) == nargs, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    for fn in (gl.pbb_attack, gl.pair_pbb_attack):
        par = inspect.signature(fn).parameters
        assert [par[k].default for k in ("optimizer", "sweeps", "ladder", "step0")] == ["es", 2, 8, 1.0]
        names = list(par)
        assert names.index("optimizer") < names.index("generate_kwargs") and par["generate_kwargs"].kind is inspect.Parameter.VAR_KEYWORD
