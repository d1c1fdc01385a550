"""CPU-only: L-BFGS in the white-box attack -- the refusals of wb_attack, pair_wb_attack and the command line that need no GPU, the exports
in the cross-compiled library, the float32 restatement of tests/wb_lbfgs_common.py against a textbook float64 two-loop recursion, and the
preconditions of the two GPU tests that do not rest on the restatement: on the host, L-BFGS under the quadratic test's protocol terminates,
and at the inputs wb_common fixes the search works."""
import math
import os
import subprocess

import numpy as np
import pytest

import wb_common as wc
import wb_lbfgs_common as lc

f32 = np.float32


class _Gen:
    """enough of a generator for the checks that come before any GPU work"""
    def generate_u8(self, z):
        raise AssertionError("the argument checks must come first")

    def l2_grad_z(self, z, t):
        raise AssertionError("the argument checks must come first")

    def vjp_z(self, z, cot):
        raise AssertionError("the argument checks must come first")

    @property
    def ctx(self):
        raise AssertionError("the argument checks must come first")


BAD = (dict(optimizer="sgd"), dict(optimizer=None), dict(optimizer="LBFGS"), dict(optimizer="lbfgs", memory=0), dict(optimizer="lbfgs", memory=17),
       dict(optimizer="lbfgs", memory=2.5), dict(optimizer="lbfgs", ladder=0), dict(optimizer="lbfgs", ladder=33), dict(optimizer="lbfgs", ladder=1.5),
       dict(optimizer="lbfgs", step0=0.0), dict(optimizer="lbfgs", step0=-1.0), dict(optimizer="lbfgs", step0=float("nan")),
       dict(optimizer="lbfgs", step0=float("inf")), dict(optimizer="lbfgs", steps=-1), dict(optimizer="lbfgs", z_max=0.0),
       dict(optimizer="lbfgs", block_images=0))


def test_refusals_without_gpu():
    import ganleaks_amd as gl
    q = np.zeros((2, 3, 64, 64), np.uint8)
    z = np.zeros((2, 100), np.float32)
    for kw in BAD:
        with pytest.raises(ValueError):
            gl.wb_attack(q, _Gen(), z, **kw)
        with pytest.raises(ValueError):
            gl.pair_wb_attack(q, _Gen(), z, **kw)
    with pytest.raises(ValueError, match="optimizer"):
        gl.wb_attack(q, _Gen(), z, optimizer="powell")
    with pytest.raises(ValueError, match="memory"):
        gl.wb_attack(q, _Gen(), z, optimizer="lbfgs", memory=17)
    with pytest.raises(ValueError, match="ladder"):
        gl.pair_wb_attack(q, _Gen(), z, optimizer="lbfgs", ladder=33)
    with pytest.raises(ValueError, match="step0"):
        gl.wb_attack(q, _Gen(), z, optimizer="lbfgs", step0=0.0)
    # the refusals wb_attack had come first and stay
    with pytest.raises(NotImplementedError, match="LPIPS"):
        gl.wb_attack(q, _Gen(), z, optimizer="lbfgs", distance="l2-lpips")
    with pytest.raises(ValueError, match="queries"):
        gl.wb_attack(q, _Gen(), np.zeros((3, 100), np.float32), optimizer="lbfgs")


def test_cli_refusals_without_gpu(tmp_path, monkeypatch):
    from ganleaks_amd.attack_models import wb
    monkeypatch.chdir(tmp_path)
    base = ["--generator_path", str(tmp_path / "nowhere.pth"), "--num_init", "64"]
    for extra in (["--optimizer", "powell"], ["--optimizer", "lbfgs", "--memory", "0"], ["--optimizer", "lbfgs", "--memory", "17"],
                  ["--optimizer", "lbfgs", "--ladder", "33"], ["--optimizer", "lbfgs", "--ladder", "0"], ["--optimizer", "lbfgs", "--step0", "0"],
                  ["--optimizer", "lbfgs", "--step0", "nan"], ["--memory", "4"], ["--optimizer", "adam", "--ladder", "4"], ["--step0", "1.0"]):
        with pytest.raises(SystemExit):
            wb.main(wb.parse_arguments(base + extra))
    with pytest.raises(SystemExit, match="lbfgs"):
        wb._request(wb.parse_arguments(base + ["--memory", "4"]))
    with pytest.raises(SystemExit, match="memory"):
        wb._request(wb.parse_arguments(base + ["--optimizer", "lbfgs", "--memory", "17"]))
    wb._request(wb.parse_arguments(base + ["--optimizer", "lbfgs"]))
    wb._request(wb.parse_arguments(base + ["--optimizer", "lbfgs", "--memory", "16", "--ladder", "32", "--step0", "0.5"]))
    wb._request(wb.parse_arguments(base + ["--optimizer", "adam"]))
    assert wb._optimizer_keywords(wb.parse_arguments(base)) == {}
    assert wb._optimizer_keywords(wb.parse_arguments(base + ["--optimizer", "lbfgs", "--ladder", "4"])) == dict(optimizer="lbfgs", memory=8, ladder=4,
                                                                                                                  step0=1.0)
    assert not (tmp_path / "wb_attack").exists()


def test_exports_and_signatures():
    import inspect
    import ganleaks_amd as gl
    from ganleaks_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    sym = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, stdout=subprocess.PIPE).stdout.decode()
    exported = {line.split()[-1] for line in sym.splitlines() if line.strip()}
    for name, nargs in (("gl_wb_lbfgs_push", 13), ("gl_wb_lbfgs_direction", 13), ("gl_wb_lbfgs_candidates", 9), ("gl_wb_lbfgs_advance", 9)):
        assert name in exported, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    for fn in (gl.wb_attack, gl.pair_wb_attack):
        par = inspect.signature(fn).parameters
        assert [par[k].default for k in ("optimizer", "memory", "ladder", "step0")] == ["adam", 8, 8, 1.0]


def test_dot_order():
    """the restated dot product is the sum it says it is: 64 ascending lane sums, then the butterfly"""
    rng = np.random.default_rng(0)
    for n in (1, 3, 64, 100, 130):
        a, b = rng.standard_normal(n).astype(f32), rng.standard_normal(n).astype(f32)
        lanes = []
        for lane in range(64):
            acc = f32(0.0)
            for c in range(lane, n, 64):
                acc = f32(acc + f32(a[c] * b[c]))
            lanes.append(acc)
        for o in (32, 16, 8, 4, 2, 1):
            lanes = [f32(lanes[i] + lanes[i ^ o]) for i in range(64)]
        assert len({v.tobytes() for v in lanes}) == 1                     # every lane ends with the same bits
        got = lc.dot32(a, b)
        assert got.tobytes() == lanes[0].tobytes()
        assert abs(float(got) - float(a.astype(np.float64) @ b.astype(np.float64))) <= (n / 64 + 7) * 2.0 ** -24 * float(np.abs(a) @ np.abs(b))


@pytest.mark.parametrize("nz,m", [(3, 1), (64, 3), (100, 8), (130, 8), (100, 16)])
def test_restatement_against_float64(nz, m):
    """the float32 two-loop against the textbook one in float64, on rings whose pairs come from a quadratic of condition 10 (y = A s).
    Tolerance: the recursion is 2 k <= 2 m passes and two scalings; each pass is a dot product, whose rounding error relative to |a| |b| is
    at most (ceil(nz / 64) + 6) u in the device's order (the lane sum and six butterfly stages) plus one u for the product, and an axpy of
    2 u; the passes compose through H, which can amplify a relative perturbation by its condition, at most kappa = 10 here.  So
    |p32 - p64| / |p64| <= 4 (2 m + 2) (ceil(nz / 64) + 9) kappa u with u = 2^-24 and 4 for the growth of intermediate vectors over the
    result (alpha y against q).  A wrong recursion is off by O(1)."""
    rng = np.random.default_rng(100 * nz + m)
    tol = 4.0 * (2 * m + 2) * (math.ceil(nz / 64) + 9) * 10.0 * 2.0 ** -24
    worst = 0.0
    for fill in (1, max(1, m // 2), m, m + 3):                           # partly filled, full, and wrapped past m
        A, _, _ = lc.quadratic(int(rng.integers(1 << 30)), nz, 1)
        st = lc.State(rng.standard_normal((1, nz)).astype(f32), m)
        g = (A[0] @ st.z[0].astype(np.float64)).astype(f32)[None]
        lc.push(st, g, np.zeros(1, np.uint8))
        for _ in range(fill):
            st.z = (st.z + f32(0.3) * rng.standard_normal((1, nz)).astype(f32)).astype(f32)
            g = (A[0] @ st.z[0].astype(np.float64)).astype(f32)[None]
            lc.push(st, g, np.ones(1, np.uint8))
        assert st.count[0] == min(fill, m) and st.head[0] == fill % m
        S, Y = lc.ring_rows(st, 0)
        want = lc.two_loop64(S, Y, g[0])
        p = lc.direction(st, g, 1.0)
        assert p.dtype == f32 and st.flag[0] == 0 and st.t[0] == 1.0 and st.count[0] == min(fill, m)
        err = np.linalg.norm(p[0] - want) / np.linalg.norm(want)
        worst = max(worst, err)
        assert err <= tol, (fill, err, tol)
        assert float(g[0].astype(np.float64) @ want) < 0
    print("nz=%d m=%d: worst relative error %.3e, tolerance %.3e" % (nz, m, worst, tol))


def test_restatement_cases():
    """what the recursion does at its edges: an empty ring, a rejected pair, a direction that is no descent direction, the ladder, the clamp,
    the width rule and a finished query"""
    nz, m, L = 5, 2, 4
    z = np.arange(10, dtype=f32).reshape(2, nz) / f32(10)
    st = lc.State(z, m)
    g = np.array([[3, 0, 4, 0, 0], [0, 0, 0, 0, 0]], f32)
    lc.push(st, g, np.zeros(2, np.uint8))
    p = lc.direction(st, g, 0.5)
    assert np.array_equal(p, -g) and st.flag.tolist() == [1, 1] and st.t[0] == f32(0.1) and np.isinf(st.t[1])     # |g| = 5; a zero gradient finishes
    cand = lc.candidates(st.z, p, st.t, L, 0.25).reshape(2, L, nz)
    assert np.array_equal(cand[1], np.repeat(z[1:2], L, axis=0))                                                # finished: the iterate itself
    assert np.allclose(cand[0, :, 0], np.maximum(-0.25, 0.0 - 0.3 * 2.0 ** -np.arange(L)), atol=1e-7) and cand[0, 0, 0] == f32(-0.25)
    assert np.array_equal(cand[0, :, 1], np.full(L, z[0, 1]))                                                   # a column without gradient
    lc.advance(st, np.array([1, 0], np.uint8), np.array([2, 0], np.int32), L)
    assert st.t[0] == f32(0.1) * f32(2.0) * f32(0.25) and np.isinf(st.t[1])
    lc.advance(st, np.array([0, 0], np.uint8), np.array([0, 0], np.int32), L)
    assert st.t[0] == f32(0.1) * f32(0.5) * f32(2.0 ** -L)
    # a pair with s.y <= 0 leaves the ring as it is; one with s.y > 0 goes in
    st.z[0] = st.z[0] + f32(1.0)
    lc.push(st, g + f32(-1.0), np.array([1, 1], np.uint8))
    assert st.count.tolist() == [0, 0] and np.array_equal(st.g_prev[0], g[0] - 1)
    st.z[0] = st.z[0] + f32(1.0)
    lc.push(st, g, np.array([1, 0], np.uint8))
    assert st.count.tolist() == [1, 0] and st.head.tolist() == [1, 0]
    # -H g with this pair is a descent direction for g, and none for a gradient H maps to the other side: the ring is dropped
    assert lc.direction(st.copy(), g, 0.5)[0] @ g[0] < 0
    st2 = st.copy()
    st2.S[0, 0] = -st2.S[0, 0]                                                                                  # s.y < 0: H is not positive
    bad = st2.Y[0, 0].copy()
    p = lc.direction(st2, bad[None].repeat(2, axis=0), 0.5)
    assert st2.flag[0] == lc.STEEPEST | lc.DROPPED and st2.count[0] == 0 and np.array_equal(p[0], -bad)
    # a rejected quasi-Newton step drops the ring
    st3 = st.copy()
    lc.direction(st3, g, 0.5)
    assert st3.flag[0] == 0 and st3.t[0] == 1
    lc.advance(st3, np.zeros(2, np.uint8), np.zeros(2, np.int32), L)
    assert st3.count[0] == 0 and st3.t[0] == 1


@pytest.mark.parametrize("nz,steps", [(8, 8), (100, 24)])
def test_quadratic_precondition(nz, steps):
    """the protocol of the GPU test's finite-termination case on the restatement: |g_steps| <= 1e-6 |g_0| on five seeds, two orders below the
    gate of 1e-4 the device is held to; steepest descent with exact steps cannot get below ((kappa - 1) / (kappa + 1))^steps"""
    worst = 0.0
    for seed in range(5):
        A, b, z0 = lc.quadratic(seed, nz)
        worst = max(worst, lc.quadratic_host(A, b, z0, 8, steps).max())
    print("nz=%d: worst |g_%d| / |g_0| = %.3e" % (nz, steps, worst))
    assert worst <= 1e-6
    assert (9.0 / 11.0) ** 8 > 0.2 > 1e-4


def test_search_precondition():
    """the inputs of the GPU search test: on the host, every query whose start lies SEARCH_DELTA away from its latent ends at a quarter of
    its starting S or less within SEARCH_STEPS gradient evaluations; the queries that are their own start stay at S = 0 and z_init; the
    trace never rises"""
    import ganleaks_amd as gl
    net = wc.dcgan_module(gl.synth.dcgan_state_dict(1234, features_g=16))
    z_init, z_image = wc.search_latents()
    queries = wc.quantize_u8(wc.forward(net, z_image))
    z, S, trace = lc.search(queries, net, z_init, lc.SEARCH_STEPS)
    print("start", trace[0].tolist(), "final", S.tolist())
    assert trace.shape == (lc.SEARCH_STEPS + 1, wc.SEARCH_Q) and (np.diff(trace, axis=0) <= 0).all() and np.array_equal(trace[-1], S)
    assert (trace[:, 0::3] == 0).all() and np.array_equal(z[0::3], z_init[0::3])
    assert (trace[0, 2::3] > 100000).all() and (4 * S[2::3] <= trace[0, 2::3]).all(), (trace[0], S)
    assert (S[1::3] < trace[0, 1::3]).all()
    assert np.array_equal(S, wc.ssd(wc.quantize_u8(wc.forward(net, z)), queries))
