"""CPU-only checks of the epsilon-ball counts (ball_counts, eps_to_ssd, gl_l2_count_i8*, gl_counts_*): the threshold on the exact S equals
the float32 comparison of the definition for every pair, the host statement of the cross-shard sum, argument checks that need no GPU,
header / binding agreement, no register spills and no scratch memory in the new kernels (hipcc cross-compiles to gfx950 assembly), and
the definition against the reference's own distances in tests/golden/knn_topk.npz."""
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


def _dist32(S, d, kind):
    S = np.asarray(S).astype(np.float64)
    return (S / float(d) if kind == "int" else S * (4.0 / (65025.0 * d))).astype(np.float32)


@pytest.mark.parametrize("kind", ["u8", "int"])
@pytest.mark.parametrize("res", [16, 32])
def test_eps_to_ssd_equals_the_float32_comparison(synth, kind, res):
    import c_oracle
    import ganleaks_amd as gl
    case = synth.attack_case(171 + res, 80, 13, 12, res)
    bank, q = case["bank"], np.concatenate([case["pos"], case["neg"]])
    if kind == "int":
        # an integer table is any rows of bytes read as the values themselves; small values keep some distances inside the float32 grid
        bank, q = bank // 32, q // 32
    d = 3 * res * res
    S = np.stack([c_oracle.ssd_row_u8(bank, x) for x in q])           # every pair: 25 x 80
    dist = _dist32(S, d, kind)
    top1 = dist.min(axis=1)
    eps = [float(np.quantile(top1, v, method="lower")) for v in (0.1, 0.5, 0.9)] + [float(np.quantile(top1, 0.37)), 0.0, -0.5, np.inf,
                                                                                    float(dist.max()), float(dist.min()), 1e-12, 1e30]
    # an eps that several distinct S round to: the largest S of the table has neighbours S +- 1 ... with the same float32 when S > 2^24 d / 65025
    big = int(S.max())
    same = [s for s in range(big - 40, big + 40) if _dist32(s, d, kind) == _dist32(big, d, kind)]
    eps.append(float(_dist32(big, d, kind)))
    thr = gl.eps_to_ssd(eps, d, kind)
    assert thr.dtype == np.int64 and thr.shape == (len(eps),)
    for e, t in zip(eps, thr):
        assert np.array_equal(S <= t, dist <= np.float32(e)), e
        # the threshold is the LARGEST qualifying S (or -1, or the largest S there is)
        assert -1 <= t <= 65025 * d
        if t >= 0:
            assert _dist32(t, d, kind) <= np.float32(e)
        if t < 65025 * d:
            assert not _dist32(t + 1, d, kind) <= np.float32(e)
    assert thr[5] == -1 and not np.any(S <= thr[5])                    # a negative eps: nothing counts
    assert thr[6] == 65025 * d and np.all(S <= thr[6])                 # inf: everything counts
    assert thr[-1] == max(same) and thr[-1] >= big
    # order and repeats of eps do not matter to the values
    assert np.array_equal(gl.eps_to_ssd(eps[::-1] + eps[:2], d, kind), np.concatenate([thr[::-1], thr[:2]]))
    assert gl.eps_to_ssd(0.25, d, kind).shape == (1,)


def test_eps_to_ssd_where_many_s_share_one_float32():
    import ganleaks_amd as gl
    d = 3 * 1024 * 1024                                                # S up to 2^37.6: up to 2^14 consecutive S per float32 value
    for e in (0.7, 1.9, 3.99):
        t = int(gl.eps_to_ssd(e, d)[0])
        s = np.arange(t - 40000, t + 40000, dtype=np.int64)
        inside = _dist32(s, d, "u8") <= np.float32(e)
        assert inside[:40001].all() and not inside[40001:].any(), e


def test_merge_counts_host_is_the_sum():
    from ganleaks_amd.shard import HostMerge, merge_counts_host
    rng = np.random.default_rng(172)
    parts = [rng.integers(0, 1 << 40, size=(7, 5)).astype(np.uint64) for _ in range(3)]
    got = merge_counts_host(parts)
    assert got.dtype == np.uint64 and np.array_equal(got, parts[0] + parts[1] + parts[2])
    assert np.array_equal(merge_counts_host(parts[:1]), parts[0]) and merge_counts_host(parts[:1]) is not parts[0]
    # the rendezvous of DeviceGroup's host route in its sum mode, and its older modes untouched
    assert np.array_equal(HostMerge(1).merge(0, parts[0], op="sum"), parts[0])
    assert np.array_equal(HostMerge(1).merge(0, parts[0][:, 0]), parts[0][:, 0])


def test_ball_counts_argument_checks_need_no_gpu():
    import ganleaks_amd as gl
    q, bank = np.zeros((2, 3, 8, 8), np.uint8), np.zeros((64, 3, 8, 8), np.uint8)
    for bad in ([], [0.1] * 17, [0.1, float("nan")], float("nan"), [[0.1, 0.2]]):
        with pytest.raises(ValueError):
            gl.ball_counts(q, bank, bad)
        with pytest.raises(ValueError):
            gl.eps_to_ssd(bad, 192)
    with pytest.raises(ValueError):
        gl.eps_to_ssd(0.1, 192, kind="f32")
    from ganleaks_amd.attack import GL_COUNT_MAX_T
    assert GL_COUNT_MAX_T == 16
    from ganleaks_amd.attack_models import mc
    with pytest.raises(SystemExit):
        mc.radii_request(mc.parse_arguments(["--eps", "0.1", "--eps_quantile", "0.5"]))
    with pytest.raises(SystemExit):
        mc.radii_request(mc.parse_arguments(["--eps_quantile", "1.5"]))
    with pytest.raises(SystemExit):
        mc.radii_request(mc.parse_arguments(["--eps", ",".join(["0.1"] * 17)]))
    assert mc.radii_request(mc.parse_arguments([])) == ("quantile", [0.5])
    assert mc.radii_request(mc.parse_arguments(["--eps", "0.3,0.1"])) == ("eps", [0.3, 0.1])


def test_header_and_binding_declare_the_count_functions():
    from ganleaks_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = ["gl_counts_init", "gl_l2_count_i8", "gl_l2_count_i8_wide", "gl_counts_add"]
    for n in names:
        assert re.search(r"\bint %s\s*\(" % n, code), n
        assert n in _lib.SIGNATURES, n
        decl = re.search(r"\bint %s\s*\((.*?)\)\s*;" % n, code, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[n][1]) == decl.count(",") + 1, n
    assert re.search(r"#define\s+GL_COUNT_MAX_T\s+16\b", code)
    assert re.search(r"#define\s+GL_ABI_VERSION\s+1\b", code)
    assert re.search(r"#define\s+GL_PROF_L2_COUNT\s+6\b", code)
    assert _lib.Context.PROF_TAGS["l2_count"] == 6
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.gl_abi_version() == 1
        for n in names:
            assert hasattr(lib, n), n


@pytest.mark.skipif(not HIPCC, reason="needs hipcc")
def test_no_spills_and_no_scratch_in_the_count_kernels(tmp_path):
    from check_loop_spills import inflight_hazards, loop_spills
    out = str(tmp_path / "gl_count.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "gan-leaks_amd", "csrc", "gl_count.hip"), "-o", out], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = open(out).read()
    # 128 x 128 tile: 32-bit S, 64-bit totals with int32 norms, wide (int64 norms); 256 x 256 tile on gl_pair256::mainloop
    for needle in ("l2_count_i8_kernelILb0EiE", "l2_count_i8_kernelILb1EiE", "l2_count_i8_kernelILb1ElE", "l2_count_i8_256p_kernel"):
        assert loop_spills(asm, needle) == 0, needle
    reads, hazards = inflight_hazards(asm, "l2_count_i8_256p_kernel")
    assert reads > 0 and hazards == [], hazards[:5]
    kernels = re.findall(r"\.amdhsa_kernel (\S*l2_count_i8\S*)(.*?)\.end_amdhsa_kernel", asm, re.S)
    assert len(kernels) == 4
    for name, body in kernels:
        assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", body), "%s uses scratch memory" % name
    # the counters are added with vector atomics on 64-bit integers, one instruction per kernel
    assert len(re.findall(r"\bglobal_atomic_add_x2\b", asm)) == 4


def test_definition_against_the_golden_distances_of_the_reference(synth):
    """tests/golden/knn_topk.npz holds the reference's own custom_knn distances (torch fp32) of the 8 nearest samples.  They lie within
    1e-6 of the exact ones (test_golden_topk_is_self_consistent), so at eps = float32(float64(dist[q, j]) + 1e-6) at least j + 1 samples lie
    inside the ball, for every query and every j < 8.  Without the 1e-6, 11 of the 352 cases fail (the reference's fp32 sum lands below the
    exact value)."""
    import c_oracle
    import ganleaks_amd as gl
    g = np.load(os.path.join(ROOT, "tests", "golden", "knn_topk.npz"))
    cases = fails_without = 0
    for c in range(int(g["n_cases"])):
        seed, nb, npos, nneg, res, bs = (int(v) for v in g["case%d" % c])
        case = synth.attack_case(seed, nb, npos, nneg, res)
        q = np.concatenate([case["pos"], case["neg"]])
        n_eff, d = (nb // bs) * bs, 3 * res * res
        for qi in range(len(q)):
            S = c_oracle.ssd_row_u8(case["bank"][:n_eff], q[qi])
            dist = _dist32(S, d, "u8")
            for j in range(8):
                gd = g["dist%d" % c][qi, j]
                eps = np.float32(np.float64(gd) + 1e-6)
                count = int((dist <= eps).sum())
                assert count >= j + 1, (c, qi, j)
                assert count == int((S <= gl.eps_to_ssd(eps, d)[0]).sum())
                cases += 1
                fails_without += int((dist <= np.float32(gd)).sum()) < j + 1
    print("without the 1e-6: %d of %d cases fail" % (fails_without, cases))
    assert cases == 352
    assert fails_without == 11                            # the margin is needed: the check discriminates
