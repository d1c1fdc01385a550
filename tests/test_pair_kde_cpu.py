"""CPU-only checks of the kernel-density arithmetic on the float paths (gan-leaks_amd/csrc/gl_kde_epi.h: gl_kde_weight_x,
gl_kde_weight_f32, gl_kde_cut_bits): the header, compiled for the host, against the numpy restatement of tests/pair_kde_common.py bit for
bit on more than 10^6 (D, D0, c) triples; the split of gl_kde_weight at x; the cut-off never excludes a weighted pair and the library's
array export equals the scalar; the measured error against float64 2^(-(D - D0) c); the host side of pair_kde_scores (refusals that must
come before a GPU is touched); the inputs of the GPU tests do not pass vacuously; no spills inside the K loops of the new kernels."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import kde_common as kc
import pair_kde_common as pk
from test_kde_cpu import sample_coefs, sample_deltas

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "gan-leaks_amd", "csrc", "gl_kde_epi.h")
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")

WRAPPER = r'''
#define GL_KDE_HOST_ONLY
#include "%s"
extern "C" void weights_f32(const float *D, const float *D0, const float *c, long long n, unsigned long long *out)
{
    for (long long i = 0; i < n; ++i) out[i] = gl_kde_weight_f32(D[i], D0[i], c[i]);
}
extern "C" void weights_x(const float *x, long long n, unsigned long long *out)
{
    for (long long i = 0; i < n; ++i) out[i] = gl_kde_weight_x(x[i]);
}
extern "C" void weights_int(const long long *delta, const float *c, long long n, unsigned long long *out)
{
    for (long long i = 0; i < n; ++i) out[i] = gl_kde_weight(delta[i], c[i]);
}
extern "C" unsigned cut_bits(float D0, float c) { return gl_kde_cut_bits(D0, c); }
'''


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "needs a host C++ compiler"
    d = tmp_path_factory.mktemp("pair_kde")
    src, lib = str(d / "pair_kde_host.cpp"), str(d / "libpair_kde_host.so")
    open(src, "w").write(WRAPPER % HEADER)
    # -O3 with contraction allowed: the header itself must keep every difference and product apart
    subprocess.run([cxx, "-O3", "-march=native", "-ffp-contract=fast", "-std=c++17", "-shared", "-fPIC", src, "-o", lib], check=True)
    h = ctypes.CDLL(lib)
    for name in ("weights_f32", "weights_x", "weights_int"):
        getattr(h, name).restype = None
    h.weights_f32.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_longlong, ctypes.c_void_p]
    h.weights_x.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]
    h.weights_int.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]
    h.cut_bits.argtypes = [ctypes.c_float, ctypes.c_float]
    h.cut_bits.restype = ctypes.c_uint32
    return h


def header_weights(h, D, D0, c):
    D = np.ascontiguousarray(D, np.float32)
    D0 = np.ascontiguousarray(np.broadcast_to(np.asarray(D0, np.float32), D.shape))
    c = np.ascontiguousarray(np.broadcast_to(np.asarray(c, np.float32), D.shape))
    out = np.empty(D.shape, np.uint64)
    h.weights_f32(D.ctypes.data, D0.ctypes.data, c.ctypes.data, D.size, out.ctypes.data)
    return out


def f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


D0_VALUES = np.float32([0.0, 1e-45, 3e-42, 1e-40, 1.1754944e-38, 1e-20, 1e-6, 1e-3, 0.0371, 0.37, 1.0, 17.5, 1e4, 1e30, 3.0e38])


def sample_D(D0, c, rng, per=4096):
    """D >= D0: D0 itself and the patterns right above it, around every integer value of x = (D - D0) c, D <= 2 D0, subnormals, +inf, and
    patterns spread over all magnitudes"""
    b0 = int(np.float32(D0).view(np.uint32))
    parts = [f32(np.minimum(b0 + np.arange(0, 64, dtype=np.int64), pk.INF_BITS)), f32([pk.INF_BITS, pk.INF_BITS - 1]),
             f32(np.arange(0, 48, dtype=np.int64))]                               # (subnormal D: kept where D >= D0)
    c64, d64 = float(c), float(D0)
    if D0 > 0:
        parts.append(np.float32(np.minimum(rng.uniform(d64, 2.0 * d64, size=per // 8), 3.4e38)))      # D <= 2 D0: the subtraction is exact
    if c64 > 0:
        with np.errstate(over="ignore"):
            for k in range(0, 43):
                centre = np.float32(min(d64 + k / c64, 3.0e38))
                around = centre.view(np.uint32).astype(np.int64) + np.arange(-6, 7)
                parts.append(f32(np.clip(around, b0, pk.INF_BITS)))
            parts.append(np.float32(np.minimum(d64 + rng.uniform(0, 42, size=per // 2) / c64, 3.0e38)))
    parts.append(f32(rng.integers(b0, pk.INF_BITS + 1, size=per // 4)))
    cut = pk.cut_bits(D0, c)
    parts.append(f32(np.clip(cut + np.arange(-40, 41, dtype=np.int64), b0, pk.INF_BITS)))
    D = np.concatenate([np.asarray(x, np.float32).reshape(-1) for x in parts])
    return D[D.view(np.uint32) >= b0]


def test_header_equals_the_numpy_restatement_bit_for_bit(host_lib):
    rng = np.random.default_rng(4301)
    total, worst, worst8, seen = 0, 0.0, 0.0, set()
    coefs = np.float32([0.0, 1e-38, 1e-30, 1e-12, 1e-6, 1e-3, 0.01, 0.37, 1.0, 3.0, 40.0, 41.0, 41.5, 1e3, 1e8, 1e20, 1e30, 3.4e38])
    for D0 in D0_VALUES:
        for c in coefs:
            D = sample_D(D0, c, rng)
            got = header_weights(host_lib, D, D0, c)
            want = pk.weight_f32(D, D0, c)
            assert np.array_equal(got, want), (float(D0), float(c), D[got != want][:5], got[got != want][:5], want[got != want][:5])
            total += len(D)
            assert got.max() <= kc.ONE
            assert np.all(got[D == D0] == kc.ONE)                      # D = D0: x = +0 (or 0 c)
            assert np.all(got[np.isinf(D)] == 0)                       # D = +inf: x = inf, or NaN for c = 0
            if c == 0:
                assert np.all(got[np.isfinite(D)] == kc.ONE)
            # the cut-off: header and restatement agree; x(cut - 1) < 41 <= x(cut); from it on every weight is 0
            cut = host_lib.cut_bits(float(D0), float(c))
            assert cut == pk.cut_bits(D0, c)
            b0 = int(np.float32(D0).view(np.uint32))
            assert b0 < cut <= pk.INF_BITS
            with np.errstate(invalid="ignore"):
                assert pk.x_of(f32([cut - 1]), D0, c)[0] < pk.X_CUT and not (pk.x_of(f32([cut]), D0, c)[0] < pk.X_CUT)
            assert np.all(got[D.view(np.uint32) >= cut] == 0), (float(D0), float(c))
            if c > 0 and float(D0) + 41.5 / float(c) < 3.0e38:
                assert cut < pk.INF_BITS
            # which integer parts of x the sample reached on both sides
            x = pk.x_of(D, D0, c)
            seen.update(np.unique(np.floor(x[np.isfinite(x) & (x < 43)])).astype(int).tolist())
            # relative error against float64 where the true weight is at least 2^-30 (D - D0 and the product exact in float64)
            fin = np.isfinite(D)
            xt = (D[fin].astype(np.float64) - float(D0)) * float(c)
            true = np.exp2(-xt)
            rel = np.abs(got[fin].astype(np.float64) / kc.ONE - true) / np.maximum(true, 1e-300)
            big = true >= 2.0 ** -30
            if big.any():
                worst = max(worst, float(rel[big].max()))
            if (xt <= 8).any():
                worst8 = max(worst8, float(rel[xt <= 8].max()))
    print("kde_weight_f32: %d triples, largest relative error where the weight is >= 2^-30: %.3e; for x <= 8: %.3e" % (total, worst, worst8))
    assert total >= 10 ** 6
    assert set(range(0, 42)) <= seen                                   # x on both sides of every integer 0..41
    assert worst <= pk.E_F32 / 2 * 1.001, worst                        # E_F32 is twice what this sample measures
    assert worst >= pk.E_F32 / 2 * 0.5, worst                          # ... and not a guess far above it
    # x <= 8: the truncation is below 2^-32 of the weight; what is left is the rounding of D - D0 and of the product (each at most
    # 2^-24 of x <= 8, times ln 2 on the weight) and twice the polynomial's 1.9e-7
    assert worst8 <= 2 * 8 * 2.0 ** -24 * np.log(2.0) + 2 * 1.9e-7 + 2.0 ** -31, worst8


def test_integer_weight_is_the_weight_of_its_x(host_lib):
    """gl_kde_weight(delta, c) == gl_kde_weight_x(fl32(delta) c) on the pairs of the integer test, and equals the integer restatement"""
    rng = np.random.default_rng(4102)
    total = 0
    for c in sample_coefs():
        delta = np.ascontiguousarray(sample_deltas(c, rng, per=4096), np.int64)
        cc = np.full(delta.shape, c, np.float32)
        a, b = np.empty(delta.shape, np.uint64), np.empty(delta.shape, np.uint64)
        host_lib.weights_int(delta.ctypes.data, cc.ctypes.data, delta.size, a.ctypes.data)
        with np.errstate(over="ignore"):
            x = np.ascontiguousarray(delta.astype(np.float32) * c)
        host_lib.weights_x(x.ctypes.data, x.size, b.ctypes.data)
        assert np.array_equal(a, b) and np.array_equal(a, kc.kde_weight(delta, c)) and np.array_equal(b, pk.weight_x(x))
        total += len(delta)
    assert total >= 10 ** 5
    nan = np.float32([np.nan, np.inf, 41.0, 40.999996, 0.0])
    out = np.empty(5, np.uint64)
    host_lib.weights_x(nan.ctypes.data, 5, out.ctypes.data)
    assert out[:3].tolist() == [0, 0, 0] and out[3] == 0 and out[4] == kc.ONE


def test_cut_bits_array_export_equals_the_scalar(host_lib):
    import ganleaks_amd as gl
    rng = np.random.default_rng(4302)
    D0 = np.concatenate([D0_VALUES, np.float32(np.exp(rng.uniform(np.log(1e-30), np.log(1e30), size=300)))])
    for c in np.float32([0.0, 1e-20, 0.003, 1.0, 123.0, 1e25]):
        got = gl.kde_cut_bits_rows(D0, c)
        assert got.dtype == np.uint32 and got.shape == D0.shape
        want = np.array([host_lib.cut_bits(float(v), float(c)) for v in D0], np.uint32)
        assert np.array_equal(got, want)
        assert np.array_equal(got[:40], np.array([pk.cut_bits(v, c) for v in D0[:40]], np.uint32))
        # no sampled pattern at or beyond the cut has a weight
        beyond = np.minimum(got.astype(np.int64)[:, None] + rng.integers(0, 1 << 20, size=(len(D0), 8)), pk.INF_BITS)
        assert np.all(pk.weight_f32(f32(beyond), D0[:, None], c) == 0)
    for bad_D0, bad_c in (([-1.0], 1.0), ([np.inf], 1.0), ([np.nan], 1.0), ([1.0], -1.0), ([1.0], np.inf)):
        with pytest.raises(gl.GanLeaksError):
            gl.kde_cut_bits_rows(np.float32(bad_D0), bad_c)
    assert gl.kde_cut_bits_rows(np.empty(0, np.float32), 1.0).shape == (0,)


def test_kde_coef_and_loss_float_form():
    from ganleaks_amd.attack import kde_coef, kde_loss, kde_units
    for kind in ("f32", "feat"):
        assert kde_units(12345, kind) == 1.0
        c32, h_eff = kde_coef([0.01, 0.5, 3.0], 777, kind)
        assert c32.dtype == np.float32 and np.array_equal(c32, (np.log2(np.e) / np.float64([0.01, 0.5, 3.0])).astype(np.float32))
        assert np.array_equal(h_eff, np.log2(np.e) / c32.astype(np.float64))
        D0 = np.float32([0.0, 0.123])
        W1 = np.full((2, 3), kc.ONE, np.uint64)
        assert np.allclose(kde_loss(W1, D0, h_eff, 64, 777, kind), D0.astype(np.float64)[:, None] + h_eff[None, :] * np.log(64.0), rtol=1e-15, atol=0)
        assert np.array_equal(kde_loss(W1 * np.uint64(64), D0, h_eff, 64, 777, kind), np.broadcast_to(D0.astype(np.float64)[:, None], (2, 3)) + 0.0)


class _Rows:
    """a bank of a given length that owns no memory"""
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def test_pair_kde_scores_argument_checks_need_no_gpu(monkeypatch):
    import ganleaks_amd as gl
    from ganleaks_amd import _lib
    from ganleaks_amd.shard import pair_kde_scores_on_devices

    def no_gpu(*a, **k):
        raise AssertionError("a refusal must come before any GPU work")
    monkeypatch.setattr(_lib.Context, "get", staticmethod(no_gpu))
    monkeypatch.setattr(_lib.Context, "__init__", no_gpu)
    q, bank = np.zeros((2, 3, 8, 8), np.uint8), np.zeros((64, 3, 8, 8), np.uint8)
    for distance in ("l2", "l2-lpips"):
        for bad in ([], [0.1] * 17, [0.1, float("nan")], 0.0, -1.0, [0.2, float("inf")], [[0.1, 0.2]]):
            with pytest.raises(ValueError):
                gl.pair_kde_scores(q, bank, bad, distance=distance)
            with pytest.raises(ValueError):
                pair_kde_scores_on_devices(q, bank=bank, bandwidths=bad, devices=[0], distance=distance)
        with pytest.raises(NotImplementedError, match="mfma"):
            gl.pair_kde_scores(q, bank, 0.1, distance=distance, float_path="mfma")
        with pytest.raises(NotImplementedError, match="mfma"):
            pair_kde_scores_on_devices(q, bank=bank, bandwidths=0.1, devices=[0], distance=distance, float_path="mfma")
        with pytest.raises(ValueError, match="float_path"):
            gl.pair_kde_scores(q, bank, 0.1, distance=distance, float_path="fast")
    with pytest.raises(ValueError, match="distance"):
        gl.pair_kde_scores(q, bank, 0.1, distance="cosine")
    with pytest.raises(ValueError, match="distance"):
        pair_kde_scores_on_devices(q, bank=bank, bandwidths=0.1, devices=[0], distance="cosine")
    with pytest.raises(ValueError, match="needs bandwidths"):
        pair_kde_scores_on_devices(q, bank=bank, devices=[0])
    # kde_scores' refusal propagates without float_path='exact'
    off = np.full((2, 3, 8, 8), 0.123, np.float32)
    with pytest.raises(NotImplementedError, match="off both lattices"):
        gl.pair_kde_scores(off, bank, 0.1, distance="l2")
    with pytest.raises(NotImplementedError, match="off both lattices"):
        gl.pair_kde_scores(q, np.full((64, 3, 8, 8), 0.123, np.float32), 0.1, distance="l2")
    for distance, fp in (("l2-lpips", None), ("l2", "exact")):
        with pytest.raises(ValueError, match="2\\^23"):
            gl.pair_kde_scores(off, _Rows(1 << 23), 0.1, distance=distance, float_path=fp, _layout="f32" if fp else None)
    # kde_scores itself keeps every refusal
    with pytest.raises(NotImplementedError, match="rounded floats"):
        gl.kde_scores(q, bank, 0.1, distance="l2-lpips")


def test_gpu_inputs_do_not_pass_vacuously():
    """the inputs of tests/test_gpu_pair_kde.py on host data alone: pick_coef's assertions hold for every T the GPU tests use"""
    import float_rows_common as frc
    for name, (seed, nq, nb, d) in pk.F32_CASES.items():
        q, bank = pk.f32_case(seed, nq, nb, d)
        M = frc.chain_matrix(q, bank)
        D0 = M.min(axis=1)
        assert (D0 == 0).sum() >= 5 and (D0 > 0).sum() >= 40
        for T in (1, 3, 16):
            coef = pk.pick_coef(M, D0, T)
            assert len(coef) == T and coef.dtype == np.float32
            S = pk.want_sums(M, D0, coef)
            assert np.all(S[:, 0] >= kc.ONE) and np.all(S[:, 0] < S[:, -1] + (T == 1))
    for kind, params in (("fp16", pk.FP16_CASE), ("split", pk.SPLIT_CASE)):
        seed, nq, nb, K = params
        case = pk.fp16_case(seed, nq, nb, K) if kind == "fp16" else pk.split_case(seed, nq, nb, K)
        M, _, _ = pk.int_case_matrix(kind, case)
        D0 = M.min(axis=1)
        for T in (1, 16):
            pk.pick_coef(M, D0, T)
        # the bound under the smallest coefficient excludes pairs, and none of them weighs anything
        coef = pk.pick_coef(M, D0, 16)
        cut = np.array([pk.cut_bits(v, coef[-1]) for v in D0], np.uint32)
        out = pk.bits_of(M) >= cut[:, None]
        assert out.any() and np.all(pk.weight_f32(M, D0[:, None], coef[-1])[out] == 0)


def test_blocked_rows_case_does_not_pass_vacuously():
    seed, nq, nb, K = pk.BLOCKED_CASE
    case = pk.fp16_case(seed, nq, nb, K, long=True, copies=1)
    M, _, _ = pk.int_case_matrix("fp16", case)
    pk.pick_coef(M, M.min(axis=1), 3)


@pytest.mark.skipif(not HIPCC, reason="needs hipcc")
def test_no_spills_inside_the_k_loops_of_the_pair_kde_kernels():
    feat = ["feat_pairs_h1_kernelILi5ELb1E", "feat_pairs_h1_kernelILi5ELb0E", "feat_pairs_split_kernelILi5E"]
    # the fp32 kernel is a VALU kernel: its K loop is bracketed by its fused multiply-adds (the division behind the loop expands to some
    # as well, which only widens the range that must be free of scratch instructions)
    names = ["gl_feat_count.hip:" + k for k in feat] + ["gl_l2f32.hip:l2_pairs_f32_kernelILi5E@v_fma"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_loop_spills.py"), "--kernels", ",".join(names),
                        "--pipelined", ",".join("gl_feat_count.hip:" + k for k in feat[:2])], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("0 scratch instructions inside the K loop") == 4, r.stdout
    assert r.stdout.count(", 0 instructions touch a fragment register still in flight") == 2, r.stdout
    assert "not found" not in r.stdout
