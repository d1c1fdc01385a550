"""CPU-only checks of the per-query radii and k-th neighbour distances on the float paths (pair_ball_counts_rows, pair_kth_distances,
eps_rows_to_bits, density_ratio_loss_f32, attack_models/density.py --pair_distance): every refusal that must come before a GPU is
touched, the threshold mapping against the float compare, the host search on patterns against np.sort, the three exports in header /
ctypes table / library, and the K loops of the new kernel instantiations by their assembly."""
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("gl_feat_count_rows_h1_scaled", "gl_feat_count_rows", "gl_l2_count_rows_f32")
INF_BITS = 0x7F800000

NO_GPU_CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
import numpy as np
import ganleaks_amd as gl
from ganleaks_amd import _lib, shard
def no_context(*a, **k):
    raise AssertionError("a Context was asked for")
_lib.Context.get = staticmethod(no_context)
_lib.Context.__init__ = no_context
q = np.zeros((4, 3, 8, 8), np.uint8)
bank = np.zeros((64, 3, 8, 8), np.uint8)
qf = np.full((4, 5), 0.3, np.float32)
bf = np.full((64, 5), 0.7, np.float32)
def raises(exc, fn, *a, **k):
    try:
        fn(*a, **k)
    except exc:
        return
    raise SystemExit("no %%s from %%s%%r" %% (exc.__name__, fn.__name__, (a[2:], k)))
for distance in ("l2-lpips", "l2"):
    for bad in (0, -3, 1.5, "3", [1, 0], [[1, 2]], list(range(1, 18)), [], True, None):
        raises(ValueError, gl.pair_kth_distances, q, bank, bad, distance=distance)
        raises(ValueError, shard.pair_kth_distances_on_devices, q, bank=bank, k=bad, devices=[0], distance=distance)
    for bad in (1.0, [1.0, 2.0], np.zeros((4, 17)), np.zeros((4, 0)), np.zeros((3, 2)), np.full((4, 2), np.nan), np.zeros((2, 2, 2))):
        raises(ValueError, gl.pair_ball_counts_rows, q, bank, bad, distance=distance)
        raises(ValueError, shard.pair_ball_counts_rows_on_devices, q, bank=bank, eps=bad, devices=[0], distance=distance)
    raises(ValueError, gl.pair_kth_distances, qf, bf, 1, distance=distance, float_path="fast")
    raises(ValueError, gl.pair_ball_counts_rows, qf, bf, np.zeros((4, 2)), distance=distance, float_path="fast")
    raises(NotImplementedError, gl.pair_kth_distances, qf, bf, 1, distance=distance, float_path="mfma")
    raises(NotImplementedError, gl.pair_ball_counts_rows, qf, bf, np.zeros((4, 2)), distance=distance, float_path="mfma")
    raises(ValueError, shard.pair_kth_distances_on_devices, qf, bank=bf, k=1, devices=[0], distance=distance, float_path="fast")
    raises(NotImplementedError, shard.pair_ball_counts_rows_on_devices, qf, bank=bf, eps=np.zeros((4, 2)), devices=[0], distance=distance,
           float_path="mfma")
raises(ValueError, gl.pair_kth_distances, q, bank, 1, distance="cosine")
raises(ValueError, gl.pair_ball_counts_rows, q, bank, np.zeros((4, 2)), distance="cosine")
raises(ValueError, shard.pair_kth_distances_on_devices, q, bank=bank, k=1, devices=[0], distance="cosine")
raises(ValueError, shard.pair_ball_counts_rows_on_devices, q, bank=bank, eps=np.zeros((4, 2)), devices=[0], distance="cosine")
# the old spellings still refuse
raises(NotImplementedError, gl.kth_distances, q, bank, 1, distance="l2-lpips")
raises(NotImplementedError, gl.ball_counts_rows, q, bank, np.zeros((4, 2)), distance="l2-lpips")
print("refused")
'''


def test_argument_errors_come_before_any_context():
    r = subprocess.run([sys.executable, "-c", NO_GPU_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("refused"), r.stdout + r.stderr


def test_eps_rows_to_bits_is_the_float_compare():
    from ganleaks_amd import eps_rows_to_bits
    fmax = float(np.finfo(np.float32).max)
    got = eps_rows_to_bits([[-np.inf, -1.0, -0.0, 0.0, 2.0 ** -149, 1.0, fmax, 1e40, np.inf]])
    assert got.dtype == np.int64 and got.shape == (1, 9)
    assert got.tolist() == [[-1, -1, 0, 0, 1, 0x3F800000, INF_BITS - 1, INF_BITS, INF_BITS]]
    rng = np.random.default_rng(11)
    # distances >= +0 of every magnitude (random patterns up to +inf), zeros, subnormals and +inf among them
    d = rng.integers(0, INF_BITS + 1, size=4000, dtype=np.int64).astype(np.uint32).view(np.float32)
    d[:8] = [0.0, 2.0 ** -149, 2.0 ** -126, 1.0, fmax, np.inf, 0.0, 3.5]
    bits = d.view(np.uint32).astype(np.int64)
    # radii: the distances themselves, their float32 neighbours, negative values, doubles that round, infinities
    with np.errstate(over="ignore"):
        up = np.nextafter(d[d < np.inf], np.float32(np.inf)).astype(np.float64)
    e = np.concatenate([d.astype(np.float64), np.nextafter(d, np.float32(-np.inf)).astype(np.float64), up, rng.standard_normal(500) * 1e-3,
                        [-np.inf, np.inf, -0.0, 1e40, -1e40, 1e-50, 0.1, 1.0 + 2.0 ** -25]])
    e = e[:(len(e) // 16) * 16].reshape(-1, 16)
    thr = eps_rows_to_bits(e)
    assert thr.shape == e.shape and thr.min() == -1 and thr.max() == INF_BITS
    with np.errstate(over="ignore"):
        e32 = e.astype(np.float32)
    for row_thr, row_e in zip(thr[::7], e32[::7]):
        assert np.array_equal(bits[:, None] <= row_thr[None, :], d[:, None] <= row_e[None, :])
    for bad in ([1.0, 2.0], np.zeros((3, 17)), np.zeros((3, 0)), [[np.nan]], np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            eps_rows_to_bits(bad)
    assert eps_rows_to_bits(np.zeros((0, 3))).shape == (0, 3)


def test_select_kth_rows_on_patterns():
    from ganleaks_amd.attack import kth_pass_bound, select_kth_rows
    assert kth_pass_bound(INF_BITS) == 8
    rng = np.random.default_rng(12)
    nq, n = 9, 60
    d = np.abs(rng.standard_normal((nq, n))).astype(np.float32)
    d[0, :5] = 0.0                                       # zeros
    d[1] = np.repeat(d[1, :n // 3], 3)                   # every value three times: the k-th and (k+1)-th tie
    d[2] = np.float32(2.5)                               # a row of equal values
    d[3, -4:] = np.inf                                   # +inf is a value like any other
    d[4] = np.inf
    d[5, :] = np.float32(2.0 ** -149)                    # the smallest pattern above zero
    d[6] = rng.integers(0, INF_BITS + 1, size=n).astype(np.uint32).view(np.float32)      # spread over every exponent
    rows = np.sort(d.view(np.uint32).astype(np.int64), axis=1)
    log = []

    def count_fn(thr):
        assert thr.dtype == np.int64 and thr.shape == (nq, 16) and np.all(thr[:, 1:] >= thr[:, :-1])
        log.append(thr.copy())
        return np.stack([np.searchsorted(rows[q], thr[q], side="right") for q in range(nq)]).astype(np.int64)

    for k in (1, 2, 22, n):
        del log[:]
        key, passes = select_kth_rows(count_fn, k, nq, INF_BITS)
        assert np.array_equal(key, rows[:, k - 1]), k
        assert 1 <= passes == len(log) <= 8
        assert np.all(log[0][:, -1] == INF_BITS), "the first pass carries +inf: the per-query total"
        assert np.array_equal(key.astype(np.uint32).view(np.float32), np.sort(d, axis=1)[:, k - 1])
    with pytest.raises(ValueError):
        select_kth_rows(count_fn, n + 1, nq, INF_BITS)


def test_density_ratio_loss_f32_and_its_clamp():
    from ganleaks_amd import density_ratio_loss_f32
    tiny = 2.0 ** -149
    a = np.asarray([0.0, tiny, 1.0, 0.25, 3.0e38, 0.0], np.float32)
    b = np.asarray([0.0, 0.0, 0.5, 4.0, tiny, 3.0e38], np.float32)
    got = density_ratio_loss_f32(a, b)
    assert got.dtype == np.float64 and np.all(np.isfinite(got))
    f = lambda x: math.log(max(float(np.float32(x)), tiny))          # noqa: E731
    want = [0.5 * (f(x) - f(y)) for x, y in zip(a, b)]
    assert np.array_equal(got, np.asarray(want, np.float64))
    assert got[0] == 0.0 and got[1] == 0.0 and got[2] == 0.5 * math.log(2.0)
    # exact duplicates (distance 0) score as the smallest non-zero pattern does
    assert np.array_equal(density_ratio_loss_f32([0.0], [0.7]), density_ratio_loss_f32([tiny], [0.7]))
    # monotone: closer under the bank, or farther under the reference set, is more member-like (smaller)
    x, y = np.float32(0.1), np.float32(0.5)
    assert density_ratio_loss_f32([x], [y]) < density_ratio_loss_f32([np.nextafter(x, np.float32(1))], [y])
    assert density_ratio_loss_f32([x], [np.nextafter(y, np.float32(1))]) < density_ratio_loss_f32([x], [y])


def test_density_pair_distance_refusals(tmp_path, monkeypatch):
    from ganleaks_amd.attack_models import density
    monkeypatch.chdir(tmp_path)
    os.makedirs(tmp_path / "syn")
    nowhere = str(tmp_path / "nowhere")
    base = ["--syn_data_path", str(tmp_path / "syn"), "--pos_data_dir", nowhere, "--neg_data_dir", nowhere]
    table = ["--syn_data_path", str(tmp_path / "t.npy"), "--pos_data_dir", nowhere, "--neg_data_dir", nowhere]
    # the folders are empty or missing: refused before anything is read
    for argv, needle in ((base + ["--pair_distance", "l2-lpips", "--distance", "l2-lpips"], "--pair_distance takes the place of --distance"),
                         (base + ["--pair_distance", "l2", "--distance", "cosine"], "--pair_distance takes the place of --distance"),
                         (table + ["--pair_distance", "l2-lpips"], "needs images"),
                         (base + ["--pair_distance", "l2-lpips", "--ref_data_dir", str(tmp_path / "r.npy")], "needs images"),
                         (base + ["--pair_distance", "l2-lpips", "--K", "0"], "--K must be"),
                         (base + ["--pair_distance", "l2", "--K", "0"], "--K must be"),
                         (base + ["--pair_distance", "l2", "--K_ref", "3"], "--K_ref needs --ref_data_dir")):
        with pytest.raises(SystemExit) as e:
            density.main(density.parse_arguments(argv))
        assert needle in str(e.value), (argv, str(e.value))
    with pytest.raises(SystemExit):
        density.parse_arguments(base + ["--pair_distance", "cosine"])
    args = density.parse_arguments(base)
    args.pair_distance = "cosine"                        # as a YAML overlay could set it
    with pytest.raises(SystemExit) as e:
        density.main(args)
    assert "--pair_distance must be" in str(e.value)
    assert not (tmp_path / "density_attack").exists()
    # the flag is absent by default, and --distance keeps its refusal
    assert density.parse_arguments(base).pair_distance is None
    assert density.parse_arguments(base + ["--pair_distance", "l2-lpips"]).pair_distance == "l2-lpips"
    with pytest.raises(SystemExit) as e:
        density.main(density.parse_arguments(base + ["--distance", "l2-lpips"]))
    assert "l2-lpips is not built" in str(e.value)


def test_new_exports_in_header_table_and_library():
    import ganleaks_amd
    from ganleaks_amd import _lib, lpips, shard
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    raw = open(_lib.HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NEW_EXPORTS:
        proto = re.search(r"\bint %s\(gl_ctx \*ctx,([^)]*)\)" % name, text)
        assert proto, "%s is not declared in ganleaks.h" % name
        assert name in _lib.SIGNATURES, "%s has no ctypes signature" % name
        assert hasattr(lib, name), "%s is not exported" % name
        assert len(proto.group(1).split(",")) + 1 == len(_lib.SIGNATURES[name][1]), name
        assert "const int64_t *thr_dev" in proto.group(1) and "uint64_t *counts_dev" in proto.group(1), name
    assert re.search(r"#define\s+GL_ABI_VERSION\s+1\b", raw) and lib.gl_abi_version() == 1
    # the reference lines each export serves
    assert "fbb.py:148" in raw[raw.index("The same counts with thresholds PER QUERY"):raw.index("int gl_feat_count_rows_h1_scaled")]
    assert "utils.py:163" in raw[raw.index("gl_l2_count_f32 with thresholds PER QUERY"):raw.index("int gl_l2_count_rows_f32")]
    for name in ("pair_ball_counts_rows", "pair_kth_distances", "eps_rows_to_bits", "count_balls_rows_f32", "density_ratio_loss_f32"):
        assert callable(getattr(ganleaks_amd, name)), name
    assert callable(lpips.feat_count_rows)
    for name in ("pair_kth_distances", "pair_ball_counts_rows"):
        assert callable(getattr(shard.DeviceGroup, name)) and callable(getattr(shard, name + "_on_devices"))


def test_host_side_threshold_checks_need_no_gpu():
    """lpips.feat_count_rows refuses mismatched rows and unsorted thresholds on the host (these FeatureBanks own no device memory)"""
    from ganleaks_amd import lpips

    class Rows:
        kind, ctx, role, fmt, K, n = "feat", None, "bank", "lattice", 64, 3

    bank, queries = Rows(), Rows()
    queries.role = "query"
    with pytest.raises(ValueError, match="ascending"):
        lpips.feat_count_rows(bank, queries, [[2, 1], [0, 1], [0, 1]])
    with pytest.raises(ValueError):
        lpips.feat_count_rows(bank, queries, [1, 2, 3])
    other = Rows()
    other.role, other.fmt = "query", "hilo"
    with pytest.raises(ValueError, match="different row layouts"):
        lpips.feat_count_rows(bank, other, [[0, 1]] * 3)


NEW_KERNELS = ("feat_pairs_h1_kernelILi4ELb1E", "feat_pairs_h1_kernelILi4ELb0E", "feat_pairs_split_kernelILi4E")
needs_hipcc = pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")


@needs_hipcc
def test_no_spills_inside_the_k_loops_of_the_per_query_counting_kernels():
    tool = os.path.join(ROOT, "tools", "check_loop_spills.py")
    kernels = ",".join("gl_feat_count.hip:" + k for k in NEW_KERNELS)
    pipelined = ",".join("gl_feat_count.hip:" + k for k in NEW_KERNELS[:2])
    r = subprocess.run([sys.executable, tool, "--kernels", kernels, "--pipelined", pipelined], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("0 scratch instructions inside the K loop") == 3, r.stdout
    assert r.stdout.count(", 0 instructions touch a fragment register still in flight") == 2, r.stdout
    assert "not found" not in r.stdout


@needs_hipcc
def test_no_spills_in_the_per_query_fp32_pair_kernel(tmp_path):
    """the check of test_no_spills_in_the_pair_kernels for l2_pairs_f32_kernel<4>: no scratch, and the accumulators do not travel through
    accumulator-register copies (no bound may stay live through the K loop)"""
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    src = os.path.join(ROOT, "gan-leaks_amd", "csrc", "gl_l2f32.hip")
    out = str(tmp_path / "gl_l2f32.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--cuda-device-only", "-S", src, "-o", out], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = open(out).read()
    m = re.search(r"^(_Z\S*l2_pairs_f32_kernelILi4E\S*):", asm, re.M)
    assert m
    body = asm[m.end():asm.index(".amdhsa_kernel " + m.group(1))]
    assert "v_fma_f32" in body or "v_fmac_f32" in body or "v_pk_fma_f32" in body
    assert body.count("scratch_") == 0, body.count("scratch_")
    assert body.count("v_accvgpr") <= 64, body.count("v_accvgpr")
    # two waves per SIMD, as the shared-threshold count (EPI 1) has: at most 256 registers, accumulator registers included
    regs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", asm[asm.index(".amdhsa_kernel " + m.group(1)):]).group(1))
    assert regs <= 256, regs
