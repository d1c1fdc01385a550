"""CPU-only: the surface of the epsilon-ball counts under 'l2-lpips' -- argument checks that must run before any GPU context exists,
the command line of attack_models/mc.py, the four new exports in header / ctypes table / library, and the K loops of the new kernels
(cross-compiled to gfx950 assembly: no spills, no use of a fragment register still in flight)."""
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("gl_feat_count_h1_scaled", "gl_feat_count", "gl_feat_pair_dist_h1_scaled", "gl_feat_pair_dist")


@pytest.fixture()
def no_context(monkeypatch):
    """any attempt to create or fetch a GPU context fails the test"""
    from ganleaks_amd import _lib

    def boom(*a, **k):
        raise AssertionError("a Context was asked for before the arguments were checked")
    monkeypatch.setattr(_lib.Context, "get", classmethod(boom))
    monkeypatch.setattr(_lib.Context, "__init__", boom)


def test_distance_and_eps_are_checked_before_any_context(no_context):
    import ganleaks_amd as gl
    from ganleaks_amd import shard
    q = np.zeros((2, 3, 16, 16), np.uint8)
    bank = np.zeros((64, 3, 16, 16), np.uint8)
    with pytest.raises(ValueError, match="distance must be 'l2' or 'l2-lpips'"):
        gl.ball_counts(q, bank, 0.1, distance="bogus")
    for bad in ([], [0.1] * 17, [0.1, float("nan")], [[0.1, 0.2]]):
        for distance in ("l2", "l2-lpips"):
            with pytest.raises(ValueError):
                gl.ball_counts(q, bank, bad, distance=distance)
    with pytest.raises(ValueError, match="l2-lpips"):
        gl.pair_distances(q, bank, distance="l2")
    # the signatures the device groups pass through
    for fn in (shard.DeviceGroup.ball_counts, shard.ball_counts_on_devices):
        params = inspect.signature(fn).parameters
        assert params["distance"].default == "l2" and params["make_lpips"].default is None
    params = inspect.signature(gl.ball_counts).parameters
    assert params["distance"].default == "l2" and params["lpips"].default is None


def test_feat_count_threshold_checks_need_no_gpu():
    """lpips.feat_count refuses bad thresholds and mismatched rows on the host (the FeatureBanks here own no device memory)"""
    from ganleaks_amd import lpips

    class Rows:
        kind, ctx, role, fmt, K, n = "feat", None, "bank", "lattice", 64, 3

    bank, queries = Rows(), Rows()
    queries.role = "query"
    for thr in ([0.2, 0.1], [0.1, float("nan")], [], [0.1] * 17):
        with pytest.raises(ValueError):
            lpips.feat_count(bank, queries, thr)
    other = Rows()
    other.role, other.fmt = "query", "hilo"
    for fn in (lambda: lpips.feat_count(bank, other, [0.1]), lambda: lpips.feat_pair_dist(bank, other), lambda: lpips.feat_knn_keys(bank, other)):
        with pytest.raises(ValueError, match="different row layouts"):
            fn()
    big = Rows()
    big.role, big.n = "query", 1 << 20
    bank.n = 1 << 10
    with pytest.raises(ValueError, match="1 GiB"):
        lpips.feat_pair_dist(bank, big)


def test_mc_command_line_has_distance():
    from ganleaks_amd.attack_models import mc
    assert mc.parse_arguments([]).distance == "l2"
    assert mc.parse_arguments(["--distance", "l2-lpips"]).distance == "l2-lpips"
    assert mc.parse_arguments(["--distance", "l2"]).distance == "l2"
    with pytest.raises(SystemExit):
        mc.parse_arguments(["--distance", "cosine"])


def test_new_exports_in_header_table_and_library():
    """tests/test_abi.py's rule, spelled out for the four new entry points"""
    from ganleaks_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    declared = set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", text))
    for name in NEW_EXPORTS:
        assert name in declared, "%s is not declared in ganleaks.h" % name
        assert name in _lib.SIGNATURES, "%s has no ctypes signature" % name
        assert hasattr(lib, name), "%s is not exported" % name
        # the header's argument count is the table's
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert sorted(_lib.SIGNATURES) == sorted(declared)
    assert "#define GL_PROF_FEAT_COUNT 7" in open(_lib.HEADER_PATH).read() and _lib.Context.PROF_TAGS["feat_count"] == 7
    assert lib.gl_abi_version() == 1


NEW_KERNELS = ("feat_pairs_h1_kernelILi0ELb1E", "feat_pairs_h1_kernelILi0ELb0E", "feat_pairs_h1_kernelILi1ELb1E", "feat_pairs_h1_kernelILi1ELb0E",
               "feat_pairs_split_kernelILi0E", "feat_pairs_split_kernelILi1E")


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
def test_no_spills_inside_the_k_loops_of_the_counting_kernels():
    """count and store forms on the cluster kernel, on its cluster-free sibling and on the split-row tile, through the tool's --kernels /
    --pipelined arguments (its default run, pinned by tests/test_loop_spills.py, is unchanged)"""
    tool = os.path.join(ROOT, "tools", "check_loop_spills.py")
    kernels = ",".join("gl_feat_count.hip:" + k for k in NEW_KERNELS)
    pipelined = ",".join("gl_feat_count.hip:" + k for k in NEW_KERNELS[:4])
    r = subprocess.run([sys.executable, tool, "--kernels", kernels, "--pipelined", pipelined], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("0 scratch instructions inside the K loop") == 6, r.stdout
    assert r.stdout.count(", 0 instructions touch a fragment register still in flight") == 4, r.stdout
    assert "not found" not in r.stdout
    # a kernel that does not exist is an error, not a silent pass
    r = subprocess.run([sys.executable, tool, "--kernels", "gl_feat_count.hip:no_such_kernel"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "not found" in r.stdout
