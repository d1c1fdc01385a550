"""CPU-only checks of the exact quantiles of all pair distances (distance_quantiles, select_ranks, gl_l2_hist_i8*): the host radix-select
against a numpy histogram over synthetic multisets (expected values from np.sort alone), the exact rank formula, header / binding
agreement, the argument checks that need no GPU, mc.py's radius options, and no register spills in the K loops of the new kernels
(hipcc cross-compiles to gfx950 assembly)."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")


def numpy_hist_fn(M, calls):
    """the histogram primitive of the definition over a host multiset, by np.bincount; every window asked for is appended to `calls`"""
    M = np.asarray(M, np.int64)

    def hist_fn(lo, shift, n_bins):
        calls.append((lo, shift, n_bins))
        assert lo >= 0 and 0 <= shift <= 40 and 1 <= n_bins <= 2048
        b = (M[M >= lo] - lo) >> shift
        return np.bincount(b[b < n_bins], minlength=n_bins).astype(np.int64)

    return hist_fn


def _multisets():
    rng = np.random.default_rng(191)
    d = 12288
    return {
        "random": (rng.integers(0, 1 << 32, size=100000), (1 << 32) - 1, 3),
        "one value": (np.full(100000, 123456789), (1 << 32) - 1, 3),
        "two values 1 apart": (np.repeat([786431, 786432], [60000, 40000]), 65025 * 768, 3),       # 786432 = 24 << 15: a bin edge at every level
        "ends": (np.repeat([0, 65025 * d], [5, 7]), 65025 * d, 3),
        "wide": (np.concatenate([rng.integers(0, 1 << 40, size=50000), [(1 << 40) - 1, 0]]), (1 << 40) - 1, 4),
        "small": (rng.integers(0, 200, size=1000), 200, 1),
    }


@pytest.mark.parametrize("name", list(_multisets()))
def test_select_ranks_is_exact(name):
    from ganleaks_amd.attack import select_ranks
    M, s_max, levels = _multisets()[name]
    n = len(M)
    want = np.sort(M)
    for ranks in ([0], [n - 1], [n // 2], [0, n - 1, n // 2, n // 3, n // 3 + 1, min(17, n - 1), min(17, n - 1), n - 2]):
        calls = []
        S, passes = select_ranks(numpy_hist_fn(M, calls), ranks, s_max)
        assert S.dtype == np.int64 and np.array_equal(S, want[ranks]), (name, ranks)
        assert passes == len(calls)
        assert passes <= levels * len(set(want[ranks].tolist())), (name, ranks, passes)     # distinct answers >= distinct bins per level
        assert len(set(calls)) == len(calls), "a window was visited twice"
        # the first level covers [0, 2^bitlen(s_max))
        lo, shift, n_bins = calls[0]
        assert lo == 0 and (n_bins << shift) == 1 << max(int(s_max).bit_length(), 1)


def test_select_ranks_several_ranks_in_one_bin_take_one_pass_per_level():
    from ganleaks_amd.attack import select_ranks
    M = np.arange(1000, dtype=np.int64) + (5 << 21)              # all inside one first-level bin of a 32-bit range
    calls = []
    S, passes = select_ranks(numpy_hist_fn(M, calls), [3, 4, 5, 6], (1 << 32) - 1)
    assert S.tolist() == [(5 << 21) + r for r in (3, 4, 5, 6)] and passes == 3
    assert [c[1] for c in calls] == [21, 10, 0] and [c[2] for c in calls] == [2048, 2048, 1024]
    # ranks as a callable of |M|, read from the first histogram
    seen = []
    S, _ = select_ranks(numpy_hist_fn(M, []), lambda total: (seen.append(total), [total - 1])[1], (1 << 32) - 1)
    assert seen == [1000] and S.tolist() == [(5 << 21) + 999]
    with pytest.raises(ValueError):
        select_ranks(numpy_hist_fn(M, []), [1000], (1 << 32) - 1)
    with pytest.raises(ValueError):
        select_ranks(numpy_hist_fn(M, []), [-1], (1 << 32) - 1)


def test_rank_formula_is_exact_where_float64_rounds():
    from fractions import Fraction
    from ganleaks_amd.attack import quantile_ranks
    pairs = 10 ** 10 + 1
    qs = [0.0, 1.0, 0.5, 0.001, 0.3, 1.0 - 2.0 ** -53, 2.0 ** -40]
    want = [(Fraction(v) * (pairs - 1)).__floor__() for v in qs]
    assert quantile_ranks(qs, pairs) == want
    assert want[0] == 0 and want[1] == pairs - 1 and want[2] == (pairs - 1) // 2
    # the float 0.3 lies below 3/10, so the exact rank is 2 999 999 999; the float64 product rounds up to 3e9
    assert want[4] == 2999999999 and int(np.floor(np.float64(0.3) * np.float64(pairs - 1))) == 3000000000
    assert quantile_ranks(0.25, 5) == [1] and quantile_ranks([1.0], 1) == [0]


def test_header_and_binding_declare_the_histogram_functions():
    from ganleaks_amd import _lib
    from ganleaks_amd.attack import GL_HIST_MAX_BINS
    text = open(_lib.HEADER_PATH).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in ("gl_hist_init", "gl_l2_hist_i8", "gl_l2_hist_i8_wide"):
        assert re.search(r"\bint %s\s*\(" % n, code), n
        assert n in _lib.SIGNATURES, n
        decl = re.search(r"\bint %s\s*\((.*?)\)\s*;" % n, code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[n][1]), n
    assert GL_HIST_MAX_BINS == 2048 and re.search(r"#define\s+GL_HIST_MAX_BINS\s+%d\b" % GL_HIST_MAX_BINS, code)
    assert re.search(r"#define\s+GL_ABI_VERSION\s+1\b", code)
    assert re.search(r"#define\s+GL_PROF_L2_HIST\s+8\b", code) and _lib.Context.PROF_TAGS["l2_hist"] == 8
    # existing ids keep their values
    assert re.search(r"#define\s+GL_PROF_L2_COUNT\s+6\b", code) and re.search(r"#define\s+GL_PROF_FEAT_COUNT\s+7\b", code)
    lib = _lib.load()
    for n in ("gl_hist_init", "gl_l2_hist_i8", "gl_l2_hist_i8_wide"):
        assert hasattr(lib, n), n


def test_radii_request_three_way():
    from ganleaks_amd.attack_models import mc
    base = ["--syn_data_path", "nowhere"]
    assert mc.radii_request(mc.parse_arguments(base + ["--eps_pair_quantile", "0.001,0.5"])) == ("pair_quantile", [0.001, 0.5])
    assert mc.radii_request(mc.parse_arguments(base + ["--eps_pair_quantile", "0.01", "--distance", "l2"])) == ("pair_quantile", [0.01])
    assert mc.radii_request(mc.parse_arguments(base)) == ("quantile", [0.5])
    assert mc.radii_request(mc.parse_arguments(base + ["--eps", "0.1"])) == ("eps", [0.1])
    assert mc.radii_request(mc.parse_arguments(base + ["--eps_quantile", "0.2", "--distance", "l2-lpips"])) == ("quantile", [0.2])
    for extra in (["--eps_pair_quantile", "0.1", "--eps", "0.1"], ["--eps_pair_quantile", "0.1", "--eps_quantile", "0.5"],
                  ["--eps_pair_quantile", "0.1", "--eps", "0.1", "--eps_quantile", "0.5"], ["--eps", "0.1", "--eps_quantile", "0.5"],
                  ["--eps_pair_quantile", "0.1", "--distance", "l2-lpips"], ["--eps_pair_quantile", "1.5"], ["--eps_pair_quantile", "-0.1"],
                  ["--eps_pair_quantile", "nan"], ["--eps_pair_quantile", "x"], ["--eps_pair_quantile", ",".join(["0.5"] * 17)],
                  ["--eps_pair_quantile", ""]):
        with pytest.raises(SystemExit):
            mc.radii_request(mc.parse_arguments(base + extra))


def test_mc_help_suggests_the_usual_percentile(capsys):
    from ganleaks_amd.attack_models import mc
    with pytest.raises(SystemExit):
        mc.parse_arguments(["--help"])
    text = capsys.readouterr().out
    assert "--eps_pair_quantile" in text and "0.001" in text


def test_mc_refuses_the_pair_quantile_before_reading(tmp_path, monkeypatch):
    from ganleaks_amd.attack_models import mc
    monkeypatch.chdir(tmp_path)
    os.makedirs(tmp_path / "syn")
    common = ["--syn_data_path", str(tmp_path / "syn"), "--pos_data_dir", str(tmp_path / "nowhere"), "--neg_data_dir", str(tmp_path / "nowhere")]
    for extra, needle in ((["--eps_pair_quantile", "0.1", "--eps", "0.1"], "exclude each other"),
                          (["--eps_pair_quantile", "0.1", "--distance", "l2-lpips"], "--distance l2"), (["--eps_pair_quantile", "2"], "[0, 1]")):
        args = mc.parse_arguments(common + extra)         # the option exists: argparse accepts it
        with pytest.raises(SystemExit) as e:
            mc.main(args)
        assert needle in str(e.value), (extra, e.value)   # radii_request's own refusal
    assert not (tmp_path / "mc_attack").exists()


def test_distance_quantiles_argument_checks_need_no_gpu(monkeypatch):
    import ganleaks_amd as gl
    from ganleaks_amd import _lib, shard

    def no_context(*a, **kw):
        raise AssertionError("a Context was asked for")

    monkeypatch.setattr(_lib.Context, "get", classmethod(no_context))
    monkeypatch.setattr(_lib.Context, "__init__", no_context)
    q, bank = np.zeros((2, 3, 8, 8), np.uint8), np.zeros((64, 3, 8, 8), np.uint8)
    for bad in (float("nan"), [0.5, float("nan")], -0.001, 1.0000001, [0.5, 2.0], [0.5] * 17, [], [[0.1, 0.2]]):
        with pytest.raises(ValueError):
            gl.distance_quantiles(q, bank, bad)
        with pytest.raises(ValueError):
            shard.distance_quantiles_on_devices(q, bank=bank, quantiles=bad, devices=[0])
    with pytest.raises(ValueError):
        shard.distance_quantiles_on_devices(q, bank=bank, devices=[0])
    with pytest.raises(NotImplementedError) as e:
        gl.distance_quantiles(q, bank, 0.5, distance="l2-lpips")
    assert "l2-lpips" in str(e.value)
    with pytest.raises(ValueError):
        gl.distance_quantiles(q, bank, 0.5, distance="cosine")


@pytest.mark.skipif(HIPCC is None, reason="needs hipcc")
def test_no_spills_in_the_k_loops_of_the_histogram_kernels():
    # 128 x 128 tile: 32-bit S, 64-bit totals with int32 norms, wide (int64 norms); 256 x 256 tile on gl_pair256::mainloop
    kernels = ["l2_hist_i8_kernelILb0EiE", "l2_hist_i8_kernelILb1EiE", "l2_hist_i8_kernelILb1ElE", "l2_hist_i8_256p_kernel"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_loop_spills.py"), "--kernels", ",".join("gl_hist.hip:" + k for k in kernels),
                        "--pipelined", "gl_hist.hip:l2_hist_i8_256p_kernel"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(" 0 scratch instructions inside the K loop") == 4, r.stdout
    assert r.stdout.count(", 0 instructions touch a fragment register still in flight") == 1, r.stdout


@pytest.mark.skipif(HIPCC is None, reason="needs hipcc")
def test_no_scratch_in_the_histogram_kernels(tmp_path):
    """forming a bin per pair before the table is filled once cost 100 - 108 bytes of scratch per lane next to the 128 accumulator registers"""
    out = str(tmp_path / "gl_hist.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "gan-leaks_amd", "csrc", "gl_hist.hip"), "-o", out], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = open(out).read()
    sizes = re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", asm)
    assert len(sizes) == 4 and all(int(v) == 0 for v in sizes), sizes
    assert "scratch_" not in asm
