"""CPU-only: the surface of the pair-distance quantiles on the float paths -- the host radix-select on float32 bit patterns, argument
checks that must run before any GPU context exists, the command line of attack_models/mc.py, the three new exports in header / ctypes
table / library, and the K loops of the new kernel instantiations (cross-compiled to gfx950 assembly: no spills, no use of a fragment
register still in flight)."""
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("gl_feat_hist_h1_scaled", "gl_feat_hist", "gl_l2_hist_f32")
INF_BITS = 0x7F800000


@pytest.fixture()
def no_context(monkeypatch):
    """any attempt to create or fetch a GPU context fails the test"""
    from ganleaks_amd import _lib

    def boom(*a, **k):
        raise AssertionError("a Context was asked for before the arguments were checked")
    monkeypatch.setattr(_lib.Context, "get", classmethod(boom))
    monkeypatch.setattr(_lib.Context, "__init__", boom)


def test_select_ranks_on_float_patterns_is_a_sort():
    """zeros, subnormals, +inf, heavy duplicates: the unsigned order of the patterns of floats >= +0 is the order of the floats, and
    select_ranks with s_max = the pattern of +inf finds every order statistic in levels of 11, 11 and 9 bits"""
    from ganleaks_amd.attack import F32_BITS_MAX, select_ranks
    assert F32_BITS_MAX == INF_BITS
    rng = np.random.default_rng(11)
    tiny = np.float32(1e-45)                               # the smallest subnormal
    values = np.concatenate([np.zeros(50, np.float32), tiny * rng.integers(1, 9, 60).astype(np.float32), np.full(7, np.inf, np.float32),
                             rng.uniform(0.044, 0.080, 3000).astype(np.float32), np.full(400, 0.0625, np.float32),
                             np.float32(10.0) ** rng.uniform(-38, 38, 500).astype(np.float32), np.full(3, np.finfo(np.float32).max, np.float32)])
    assert np.all(values >= 0) and not np.any(np.signbit(values))
    B = values.view(np.uint32).astype(np.int64)
    order = np.sort(B)
    assert np.array_equal(np.sort(values).view(np.uint32).astype(np.int64), order)      # the claim itself
    calls = []

    def hist_fn(lo, shift, n_bins):
        calls.append((lo, shift, n_bins))
        x = B[(B >= lo) & (B <= INF_BITS)]
        b = (x - lo) >> shift
        return np.bincount(b[b < n_bins], minlength=n_bins)

    ranks = list(range(0, B.size, 37)) + [B.size - 1, 0, 49, 50, 109, 110]
    got, passes = select_ranks(hist_fn, ranks, INF_BITS)
    assert np.array_equal(got, order[ranks]) and passes == len(calls)
    assert calls[0] == (0, 20, 2048) and {(s, n) for _, s, n in calls} == {(20, 2048), (9, 2048), (0, 512)}
    # one rank: 3 passes; and the ranks may come from the first level's total
    calls.clear()
    got, passes = select_ranks(hist_fn, lambda total: [total // 2], INF_BITS)
    assert passes == 3 and got[0] == order[B.size // 2]
    assert got.astype(np.uint32).view(np.float32)[0] == np.sort(values)[B.size // 2]


def test_entry_point_checks_run_before_any_context(no_context):
    import ganleaks_amd as gl
    from ganleaks_amd import shard
    q = np.zeros((2, 3, 16, 16), np.uint8)
    bank = np.zeros((64, 3, 16, 16), np.uint8)
    for bad in ([], [0.1] * 17, [0.1, float("nan")], [[0.1, 0.2]], -0.1, 1.5):
        for distance in ("l2", "l2-lpips"):
            with pytest.raises(ValueError):
                gl.pair_distance_quantiles(q, bank, bad, distance=distance)
    with pytest.raises(ValueError, match="distance must be 'l2' or 'l2-lpips'"):
        gl.pair_distance_quantiles(q, bank, 0.5, distance="bogus")
    for distance in ("l2", "l2-lpips"):
        with pytest.raises(ValueError, match="float_path"):
            gl.pair_distance_quantiles(q, bank, 0.5, distance=distance, float_path="bogus")
        with pytest.raises(NotImplementedError, match="mfma"):
            gl.pair_distance_quantiles(q, bank, 0.5, distance=distance, float_path="mfma")
    with pytest.raises(ValueError):
        shard.pair_distance_quantiles_on_devices(q, bank=bank, devices=[0])                       # needs quantiles
    with pytest.raises(ValueError):
        shard.pair_distance_quantiles_on_devices(q, bank=bank, devices=[0], quantiles=[2.0])
    with pytest.raises(ValueError):
        shard.pair_distance_quantiles_on_devices(q, bank=bank, devices=[0], quantiles=0.5, distance="bogus")
    with pytest.raises(NotImplementedError):
        shard.pair_distance_quantiles_on_devices(q, bank=bank, devices=[0], quantiles=0.5, float_path="mfma")
    params = inspect.signature(gl.pair_distance_quantiles).parameters
    assert list(params)[:3] == ["queries", "bank", "quantiles"]
    assert params["distance"].default == "l2-lpips" and params["batch_size"].default == 64 and params["float_path"].default is None
    for name in ("ctx", "reduce_fn", "lpips", "chunk_bytes", "index_base"):
        assert name in params
    for fn in (shard.DeviceGroup.pair_distance_quantiles, shard.pair_distance_quantiles_on_devices):
        params = inspect.signature(fn).parameters
        assert params["distance"].default == "l2-lpips" and params["make_lpips"].default is None and params["float_path"].default is None
    # the older spelling keeps its refusals
    with pytest.raises(NotImplementedError, match="l2-lpips"):
        gl.distance_quantiles(q, bank, 0.5, distance="l2-lpips")


def test_histogram_window_checks_need_no_gpu():
    """lpips.feat_hist and attack.pair_histogram_f32 refuse bad windows and mismatched rows on the host (these rows own no device memory)"""
    from ganleaks_amd import lpips
    from ganleaks_amd.attack import pair_histogram_f32

    class Rows:
        kind, ctx, role, fmt, K, n, d = "feat", None, "bank", "lattice", 64, 3, 12

    bank, queries = Rows(), Rows()
    queries.role = "query"
    for lo, shift, n_bins in ((-1, 0, 8), (1 << 32, 0, 8), (0, -1, 8), (0, 32, 8), (0, 0, 0), (0, 0, 2049)):
        with pytest.raises(ValueError, match="n_bins"):
            lpips.feat_hist(bank, queries, lo, shift, n_bins)
    other = Rows()
    other.role, other.fmt = "query", "hilo"
    with pytest.raises(ValueError, match="different row layouts"):
        lpips.feat_hist(bank, other, 0, 20, 2048)
    f1, f2 = Rows(), Rows()
    f1.kind = f2.kind = "f32"
    for lo, shift, n_bins in ((-1, 0, 8), (0, 32, 8), (0, 0, 2049)):
        with pytest.raises(ValueError, match="n_bins"):
            pair_histogram_f32(f1, f2, lo, shift, n_bins)
    with pytest.raises(ValueError, match="'f32' Banks"):
        pair_histogram_f32(bank, f2, 0, 20, 2048)
    f2.d = 13
    with pytest.raises(ValueError, match="values"):
        pair_histogram_f32(f1, f2, 0, 20, 2048)


def test_mc_command_line_has_eps_percentile(capsys):
    from ganleaks_amd.attack_models import mc
    assert mc.parse_arguments([]).eps_percentile is None
    assert "eps_percentile" in mc.LATER_OPTIONS and "eps_pair_quantile" in mc.LATER_OPTIONS
    for distance in ("l2", "l2-lpips"):
        args = mc.parse_arguments(["--distance", distance, "--eps_percentile", "0.001,0.5"])
        assert mc.radii_request(args) == ("percentile", [0.001, 0.5])
    for other in (["--eps", "0.1"], ["--eps_quantile", "0.5"], ["--eps_pair_quantile", "0.01"]):
        with pytest.raises(SystemExit, match="exclude each other"):
            mc.radii_request(mc.parse_arguments(["--eps_percentile", "0.01"] + other))
    for bad in ("1.5", "-0.1", "nan", "abc", ",".join(["0.1"] * 17), ""):
        with pytest.raises(SystemExit):
            mc.radii_request(mc.parse_arguments(["--eps_percentile=" + bad]))
    # the older options keep their answers and their refusals
    assert mc.radii_request(mc.parse_arguments([])) == ("quantile", [0.5])
    assert mc.radii_request(mc.parse_arguments(["--eps_pair_quantile", "0.01"])) == ("pair_quantile", [0.01])
    with pytest.raises(SystemExit, match="exact-integer"):
        mc.radii_request(mc.parse_arguments(["--distance", "l2-lpips", "--eps_pair_quantile", "0.01"]))
    with pytest.raises(SystemExit):
        mc.parse_arguments(["--help"])
    text = capsys.readouterr().out
    assert "--eps_percentile" in text and "--eps_pair_quantile" in text
    assert "--eps_percentile" in mc.__doc__


def test_new_exports_in_header_table_and_library():
    """tests/test_abi.py's rule, spelled out for the three new entry points; the ABI version stays 1 and no profiling id is added"""
    import importlib
    import ganleaks_amd as gl
    from ganleaks_amd import _lib, lpips, shard
    attack = importlib.import_module("ganleaks_amd.attack")     # (the package's `attack` attribute is the function)
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    header = open(_lib.HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", text))
    for name in NEW_EXPORTS:
        assert name in declared, "%s is not declared in ganleaks.h" % name
        assert name in _lib.SIGNATURES, "%s has no ctypes signature" % name
        assert hasattr(lib, name), "%s is not exported" % name
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert "uint32_t lo" in proto and "int shift" in proto and "int n_bins" in proto and "uint64_t *hist_dev" in proto
    assert sorted(_lib.SIGNATURES) == sorted(declared)
    assert lib.gl_abi_version() == 1
    assert sorted(_lib.Context.PROF_TAGS.values()) == list(range(9)) and not re.search(r"#define\s+GL_PROF_\w+\s+9\b", header)
    assert "GL_PROF_FEAT_COUNT" in header[header.index("gl_feat_hist_h1_scaled") - 1500:header.index("gl_feat_hist_h1_scaled")]
    # the Python surface
    assert gl.pair_distance_quantiles is attack.pair_distance_quantiles
    for obj, name in ((lpips, "feat_hist"), (attack, "pair_histogram_f32"), (shard.DeviceGroup, "pair_distance_quantiles"),
                      (shard, "pair_distance_quantiles_on_devices")):
        assert callable(getattr(obj, name))
    assert list(inspect.signature(lpips.feat_hist).parameters) == ["bank", "queries", "lo", "shift", "n_bins", "n_rows", "hist"]
    assert list(inspect.signature(attack.pair_histogram_f32).parameters) == ["bank", "queries", "lo", "shift", "n_bins", "n_rows", "hist"]


NEW_KERNELS = ("feat_pairs_h1_kernelILi3ELb1E", "feat_pairs_h1_kernelILi3ELb0E", "feat_pairs_split_kernelILi3E")


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
def test_no_spills_inside_the_k_loops_of_the_binning_kernels():
    """the binning form on the cluster kernel, on its cluster-free sibling and on the split-row tile, through the tool's --kernels /
    --pipelined arguments (gl_l2f32.hip's kernel has no matrix-core loop for the tool to find; it uses no scratch at all)"""
    tool = os.path.join(ROOT, "tools", "check_loop_spills.py")
    kernels = ",".join("gl_feat_count.hip:" + k for k in NEW_KERNELS)
    pipelined = ",".join("gl_feat_count.hip:" + k for k in NEW_KERNELS[:2])
    r = subprocess.run([sys.executable, tool, "--kernels", kernels, "--pipelined", pipelined], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("0 scratch instructions inside the K loop") == 3, r.stdout
    assert r.stdout.count(", 0 instructions touch a fragment register still in flight") == 2, r.stdout
    assert "not found" not in r.stdout
