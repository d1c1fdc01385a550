"""CPU-only checks of the top-K nearest-neighbour search (attack(k=), gl_l2_topk_i8*, gl_topk_*): the host statement of the list merge,
header / binding agreement, no register spills inside the K loops of the new pairwise kernels (hipcc cross-compiles to gfx950 assembly),
none of the scalar-store instructions anywhere in the source tree, and the golden file from the reference is self-consistent."""
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

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")


def _expected_merge(parts, k):
    allk = np.concatenate([np.asarray(a, np.uint64).reshape(len(a), -1) for a in parts], axis=1)
    out = np.full((len(allk), k), EMPTY, np.uint64)
    for q, row in enumerate(allk):
        s = np.sort(row)[:k]
        out[q, :len(s)] = s
    return out


def test_merge_topk_host_against_sort():
    from ganleaks_amd.shard import merge_topk_host
    rng = np.random.default_rng(5)
    nq, k = 9, 5
    # keys (S << 32 | index) with few distinct S values: every S is shared by several indices, across lists too
    lists = []
    for r in range(3):
        S = rng.integers(0, 4, size=(nq, k)).astype(np.uint64)
        idx = (np.arange(k, dtype=np.uint64)[None, :] + np.uint64(100 * r)) * np.ones((nq, 1), np.uint64)
        lists.append(np.sort((S << np.uint64(32)) | idx, axis=1))
    got = merge_topk_host(lists, k)
    assert got.dtype == np.uint64 and got.shape == (nq, k)
    assert np.array_equal(got, _expected_merge(lists, k))
    assert np.all(np.diff(got.astype(np.float64), axis=1) >= 0)
    # ties in S resolve to the smaller index: for equal S the list of rank 0 (indices 0..4) comes before rank 1 (100..)
    for q in range(nq):
        s, i = got[q] >> np.uint64(32), got[q] & np.uint64(0xFFFFFFFF)
        for a in range(k - 1):
            assert s[a] < s[a + 1] or i[a] < i[a + 1]


def test_merge_topk_host_empty_slots_and_short_lists():
    from ganleaks_amd.shard import merge_topk_host
    k = 4
    a = np.array([[3, 9, EMPTY, EMPTY], [EMPTY] * 4], np.uint64)          # a shard with two rows; a shard with none
    b = np.array([[1, 2], [7, EMPTY]], np.uint64)                         # lists shorter than k
    got = merge_topk_host([a, b], k)
    assert got.tolist() == [[1, 2, 3, 9], [7, int(EMPTY), int(EMPTY), int(EMPTY)]]
    # fewer than k keys altogether: the rest stays empty; one list alone is returned sorted and padded
    assert merge_topk_host([b], k).tolist() == [[1, 2, int(EMPTY), int(EMPTY)], [7, int(EMPTY), int(EMPTY), int(EMPTY)]]
    assert np.array_equal(merge_topk_host([a, b, a], 2), _expected_merge([a, b, a], 2))
    # k = 1 is the element-wise minimum of the top-1 keys
    from ganleaks_amd.shard import merge_keys_host
    x, y = np.array([5, 1, 8], np.uint64), np.array([4, 2, 9], np.uint64)
    assert np.array_equal(merge_topk_host([x, y], 1)[:, 0], merge_keys_host([x, y]))


def test_header_and_binding_declare_the_topk_functions():
    from ganleaks_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = ["gl_topk_init", "gl_l2_topk_i8", "gl_l2_topk_i8_wide", "gl_topk_merge", "gl_topk_unpack", "gl_topk_set_workspace"]
    for n in names:
        assert re.search(r"\bint %s\s*\(" % n, code), n
        assert n in _lib.SIGNATURES, n
    assert re.search(r"#define\s+GL_TOPK_MAX\s+32\b", code)
    assert re.search(r"#define\s+GL_ABI_VERSION\s+1\b", code)
    assert re.search(r"#define\s+GL_PROF_TOPK_SELECT\s+5\b", code)
    # argument counts of the binding follow the header
    for n in names:
        decl = re.search(r"\bint %s\s*\((.*?)\)\s*;" % n, code, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[n][1]) == decl.count(",") + 1, n
    from ganleaks_amd.attack import GL_TOPK_MAX
    assert GL_TOPK_MAX == 32
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.gl_abi_version() == 1
        for n in names:
            assert hasattr(lib, n), n


def test_python_argument_checks_need_no_gpu():
    from ganleaks_amd.attack import _check_k
    assert _check_k(1) == 1 and _check_k(np.int64(32)) == 32
    for bad in (0, 33, -1):
        with pytest.raises(ValueError):
            _check_k(bad)
    with pytest.raises(TypeError):
        _check_k(2.0)
    import ganleaks_amd as gl
    with pytest.raises(NotImplementedError) as e:
        gl.attack(np.zeros((2, 3, 8, 8), np.uint8), np.zeros((64, 3, 8, 8), np.uint8), distance="l2-lpips", k=3)
    assert "l2" in str(e.value)


def _assembly(tmp, src):
    out = os.path.join(tmp, src + ".s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "gan-leaks_amd", "csrc", src), "-o", out], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return open(out).read()


@pytest.mark.skipif(not HIPCC, reason="needs hipcc")
def test_no_spills_inside_the_k_loops_of_the_topk_kernels(tmp_path):
    from check_loop_spills import inflight_hazards, loop_spills
    topk = _assembly(str(tmp_path), "gl_topk.hip")
    # 128 x 128 tile: 32-bit S, 64-bit totals with int32 norms, wide (int64 norms); 256 x 256 tile on gl_pair256::mainloop
    for needle in ("l2_topk_i8_kernelILb0EiE", "l2_topk_i8_kernelILb1EiE", "l2_topk_i8_kernelILb1ElE", "l2_topk_i8_256p_kernel"):
        assert loop_spills(topk, needle) == 0, needle
    reads, hazards = inflight_hazards(topk, "l2_topk_i8_256p_kernel")
    assert reads > 0 and hazards == [], hazards[:5]
    for m in re.finditer(r"\.amdhsa_kernel (\S*l2_topk_i8\S*)(.*?)\.end_amdhsa_kernel", topk, re.S):
        assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", m.group(2)), "%s uses scratch memory" % m.group(1)
    # the top-1 kernels are as free of spills as before
    knn = _assembly(str(tmp_path), "gl_l2knn.hip")
    for needle in ("l2_knn_i8_wide_kernel", "l2_knn_i8_kernelILb0E", "l2_knn_i8_kernelILb1E", "l2_knn_i8_256p_kernelILi0ELi8E"):
        assert loop_spills(knn, needle) == 0, needle


def test_source_tree_holds_no_scalar_store_instruction():
    pre = "s" + "_"
    words = [pre + w for w in ("store" + "_dword", "buffer" + "_store_", "scratch" + "_store_", "atomic" + "_", "buffer" + "_atomic_",
                               "dcache" + "_wb", "dcache" + "_discard")]
    pat = re.compile("(?<![a-z0-9_])(" + "|".join(re.escape(w) for w in words) + ")", re.I)
    hits = []
    for top in ("gan-leaks_amd", "include", "tools", "tests", "oracle"):
        for d, dirs, files in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [x for x in dirs if x not in ("__pycache__", "_build", "_ref")]
            for f in files:
                if f.endswith((".hip", ".h", ".c", ".cpp", ".py", ".sh", ".s", ".S")) or f == "Makefile":
                    if pat.search(open(os.path.join(d, f), errors="replace").read()):
                        hits.append(os.path.join(d, f))
    assert not hits, hits


def test_golden_topk_is_self_consistent(synth):
    import c_oracle
    g = np.load(os.path.join(ROOT, "tests", "golden", "knn_topk.npz"))
    keep = int(g["keep"])
    assert int(g["n_cases"]) == 3 and keep == 8
    expected = [(21, 700, 8, 8, 16, 64), (22, 330, 6, 6, 64, 30), (23, 1100, 8, 8, 32, 64)]
    for c in range(3):
        seed, nb, npos, nneg, res, bs = (int(v) for v in g["case%d" % c])
        assert (seed, nb, npos, nneg, res, bs) == expected[c]
        case = synth.attack_case(seed, nb, npos, nneg, res)
        q = np.concatenate([case["pos"], case["neg"]])
        n_eff, d = (nb // bs) * bs, 3 * res * res
        assert g["idx%d" % c].shape == (len(q), keep)
        for qi in range(len(q)):                          # every query: none is left out
            S = c_oracle.ssd_row_u8(case["bank"][:n_eff], q[qi])
            order = np.argsort(S, kind="stable")[:keep]
            assert np.array_equal(order, g["idx%d" % c][qi]), (c, qi)
            dist = (S[order].astype(np.float64) * (4.0 / (65025.0 * d))).astype(np.float32)
            assert np.max(np.abs(dist.astype(np.float64) - g["dist%d" % c][qi].astype(np.float64))) <= 1e-6, (c, qi)
