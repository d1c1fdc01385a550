"""CPU-only: the surface of the K nearest samples under 'l2-lpips' -- argument checks that must run before any GPU context exists, the
command line of attack_models/knn.py, the three new exports in header / ctypes table / library, and the K loops of the new kernel
instantiations (cross-compiled to gfx950 assembly: no spills, no use of a fragment register still in flight)."""
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("gl_feat_topk_h1_scaled", "gl_feat_topk", "gl_topk_unpack_f32")


@pytest.fixture()
def no_context(monkeypatch):
    """any attempt to create or fetch a GPU context fails the test"""
    from ganleaks_amd import _lib

    def boom(*a, **k):
        raise AssertionError("a Context was asked for before the arguments were checked")
    monkeypatch.setattr(_lib.Context, "get", classmethod(boom))
    monkeypatch.setattr(_lib.Context, "__init__", boom)


def test_k_and_distance_are_checked_before_any_context(no_context):
    import ganleaks_amd as gl
    from ganleaks_amd import shard
    q = np.zeros((2, 3, 16, 16), np.uint8)
    bank = np.zeros((64, 3, 16, 16), np.uint8)
    with pytest.raises(ValueError, match="distance must be 'l2' or 'l2-lpips'"):
        gl.nearest_neighbours(q, bank, 3, distance="bogus")
    for distance in ("l2", "l2-lpips"):
        for bad in (0, 33, -1):
            with pytest.raises(ValueError, match="k must be in"):
                gl.nearest_neighbours(q, bank, bad, distance=distance)
        for bad in (2.0, True, None, "3"):
            with pytest.raises(TypeError):
                gl.nearest_neighbours(q, bank, bad, distance=distance)
    # the older spelling stays exact-integer only
    with pytest.raises(NotImplementedError, match="l2"):
        gl.attack(q, bank, distance="l2-lpips", k=3)
    params = inspect.signature(gl.nearest_neighbours).parameters
    assert list(params)[:3] == ["queries", "bank", "k"]
    assert params["distance"].default == "l2-lpips" and params["batch_size"].default == 64 and params["index_base"].default == 0
    for name in ("ctx", "reduce_fn", "lpips", "chunk_bytes"):
        assert params[name].default is None
    for fn in (shard.DeviceGroup.nearest_neighbours, shard.nearest_neighbours_on_devices):
        params = inspect.signature(fn).parameters
        assert params["distance"].default == "l2-lpips" and params["make_lpips"].default is None and params["k"].default is None


def test_feat_topk_keys_checks_need_no_gpu():
    """lpips.feat_topk_keys refuses a bad k and mismatched rows on the host (the FeatureBanks here own no device memory)"""
    from ganleaks_amd import lpips

    class Rows:
        kind, ctx, role, fmt, K, n = "feat", None, "bank", "lattice", 64, 3

    bank, queries = Rows(), Rows()
    queries.role = "query"
    for bad in (0, 33):
        with pytest.raises(ValueError, match="k must be in"):
            lpips.feat_topk_keys(bank, queries, bad)
    other = Rows()
    other.role, other.fmt = "query", "hilo"
    with pytest.raises(ValueError, match="different row layouts"):
        lpips.feat_topk_keys(bank, other, 3)
    longer = Rows()
    longer.role, longer.K = "query", 128
    with pytest.raises(ValueError, match="feature lengths differ"):
        lpips.feat_topk_keys(bank, longer, 3)
    split = Rows()
    split.role = None
    with pytest.raises(ValueError, match="lattice rows on one side"):
        lpips.feat_topk_keys(bank, split, 3)
    hilo_a, hilo_b = Rows(), Rows()
    hilo_a.fmt = hilo_b.fmt = "hilo"                      # two 'bank' rows: hi / lo layouts need roles ('bank', 'query')
    with pytest.raises(ValueError, match="roles"):
        lpips.feat_topk_keys(hilo_a, hilo_b, 3)


def test_knn_command_line():
    from ganleaks_amd.attack_models import knn
    args = knn.parse_arguments([])
    assert args.K == 5 and args.distance == "l2-lpips" and args.BATCH_SIZE == 30 and args.ngpu == 1 and args.devices is None
    args = knn.parse_arguments(["--K", "32", "--distance", "l2", "--devices", "0,1", "-name", "x"])
    assert args.K == 32 and args.distance == "l2" and args.devices == "0,1" and args.exp_name == "x"
    assert knn.knn_request(args) == (32, "l2")
    with pytest.raises(SystemExit):
        knn.parse_arguments(["--distance", "cosine"])
    with pytest.raises(SystemExit):
        knn.parse_arguments(["--K", "many"])
    # main() refuses before any file is read: the paths below do not exist
    for bad in (["--K", "0"], ["--K", "33"], ["--K", "-1"]):
        with pytest.raises(SystemExit, match="--K"):
            knn.main(knn.parse_arguments(["--syn_data_path", "/nonexistent/bank"] + bad))
    args = knn.parse_arguments(["--syn_data_path", "/nonexistent/bank"])
    args.distance = "cosine"                              # as a YAML overlay could set it
    with pytest.raises(SystemExit, match="--distance"):
        knn.main(args)
    args = knn.parse_arguments(["--syn_data_path", "/nonexistent/bank"])
    args.K = 2.5
    with pytest.raises(SystemExit, match="--K"):
        knn.main(args)


def test_new_exports_in_header_table_and_library():
    """tests/test_abi.py's rule, spelled out for the three new entry points"""
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
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert sorted(_lib.SIGNATURES) == sorted(declared)
    assert lib.gl_abi_version() == 1
    import ganleaks_amd as gl
    from ganleaks_amd import lpips, shard
    from ganleaks_amd.attack import nearest_neighbours, unpack_topk_f32
    assert gl.nearest_neighbours is nearest_neighbours
    assert callable(lpips.feat_topk_keys) and callable(unpack_topk_f32) and callable(shard.nearest_neighbours_on_devices)


NEW_KERNELS = ("feat_pairs_h1_kernelILi2ELb1E", "feat_pairs_h1_kernelILi2ELb0E", "feat_pairs_split_kernelILi2E")


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
def test_no_spills_inside_the_k_loops_of_the_storing_kernels():
    """the piece-storing form on the cluster kernel, on its cluster-free sibling and on the split-row tile, through the tool's --kernels /
    --pipelined arguments, as tests/test_count_lpips_cpu.py runs it for the counting and matrix forms"""
    tool = os.path.join(ROOT, "tools", "check_loop_spills.py")
    kernels = ",".join("gl_feat_count.hip:" + k for k in NEW_KERNELS)
    pipelined = ",".join("gl_feat_count.hip:" + k for k in NEW_KERNELS[:2])
    r = subprocess.run([sys.executable, tool, "--kernels", kernels, "--pipelined", pipelined], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("0 scratch instructions inside the K loop") == 3, r.stdout
    assert r.stdout.count(", 0 instructions touch a fragment register still in flight") == 2, r.stdout
    assert "not found" not in r.stdout
