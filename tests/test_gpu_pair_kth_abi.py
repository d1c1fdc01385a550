"""GPU: the three counting exports with thresholds per query on the float paths (gl_feat_count_rows_h1_scaled, gl_feat_count_rows,
gl_l2_count_rows_f32) against exact host oracles: integer rows under condition C for the LPIPS pair kernels (tests/pair_rows_common.py: D32
of every pair is known bit for bit from int64 arithmetic), the CPU chain for the fp32 rows (float_rows_common.chain_matrix).  Every query
gets its own row of 16 thresholds, taken from its own distance row, so the thresholds differ across the 16 columns of a fragment.
Expected everywhere: (bits(M[q])[None, :] <= thr[q][:, None]).sum(1), compared with array_equal."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_common  # noqa: F401
import float_rows_common as frc
import pair_rows_common as pr
import test_gpu_pair_rows_exact as ex

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
p = ctypes.c_void_p
INF_BITS = 0x7F800000


def bits64(M):
    return pr.bits_of(M).astype(np.int64)


def threshold_rows(B, tie_col):
    """int64 [nq, 16], every row ascending, from each query's own row of patterns B[q] (NaN patterns ignored): -1, a value above +inf's
    pattern, repeated values, attained values and their predecessors, and the tie planted at column `tie_col` (a value at least two pairs
    of the query share) straddled by thr and thr - 1.  Query 1 (if any): sixteen times -1; query 2: a first threshold that already counts
    every pair."""
    nq = len(B)
    thr = np.empty((nq, 16), np.int64)
    for q in range(nq):
        sb = np.sort(B[q][B[q] <= INF_BITS])
        n = len(sb)
        tie = int(B[q, tie_col])
        assert (B[q] == tie).sum() >= 2
        row = [-1, sb[0] - 1, sb[0], sb[0], sb[n // 10], sb[n // 4] - 1, sb[n // 4], sb[n // 2], sb[n // 2] + 1, tie - 1, tie,
               sb[(3 * n) // 4], sb[-1] - 1, sb[-1], INF_BITS, INF_BITS + 5]
        thr[q] = np.sort(np.asarray(row, np.int64))
    if nq > 1:
        thr[1] = -1
    if nq > 2:
        top = int(np.max(B[2][B[2] <= INF_BITS]))
        thr[2] = np.sort(np.asarray([top] * 6 + [top + 1] * 4 + [INF_BITS] * 3 + [INF_BITS + 5] * 3, np.int64))
    assert np.all(thr[:, 1:] >= thr[:, :-1])
    return thr


def expected(B, thr):
    want = np.stack([(B[q][None, :] <= thr[q][:, None]).sum(axis=1) for q in range(len(B))]).astype(np.uint64)
    # a threshold above +inf's pattern counts every pair that is not NaN, as the clamped one does
    assert np.array_equal(want, np.stack([(B[q][None, :] <= np.minimum(thr[q], INF_BITS)[:, None]).sum(axis=1) for q in range(len(B))]))
    return want


def feat_count_rows(pair, thr, counts=None, row0=0, n_rows=None):
    """thr int64 [nq, T] through the raw ABI; returns the counters DeviceArray"""
    from ganleaks_amd.attack import new_counts
    ctx = pair.ctx
    b, q = pair._ops(row0, n_rows)
    thr = np.ascontiguousarray(thr, np.int64)
    thr_dev = ctx.to_device(thr)
    if counts is None:
        counts = new_counts(ctx, pair.Q.n, thr.shape[1])
    if pair.h1:
        pair.check(pair.lib.gl_feat_count_rows_h1_scaled(pair.h, *b, *q, pair.B.K, pair.scale, p(thr_dev.ptr), thr.shape[1], p(counts.ptr)))
    else:
        pair.check(pair.lib.gl_feat_count_rows(pair.h, *b, *q, pair.B.K, p(thr_dev.ptr), thr.shape[1], p(counts.ptr)))
    ctx.sync()
    return counts


def check_case(c, half):
    """one prepared case: the full table, a table of 3 columns, and two calls over two parts of the bank (cut at row `half`)"""
    B = bits64(c.M)
    thr = threshold_rows(B, 7)
    assert np.all(thr[1] == -1) and thr.max() > INF_BITS and (thr == -1).sum() >= c.nq
    want = expected(B, thr)
    assert not want[1].any() and np.all(want[2] == c.nb) and np.all(np.delete(want[:, -1], 1) == c.nb)
    assert all(int(B[q, 7]) in thr[q] and int(B[q, 7]) - 1 in thr[q] for q in range(3, c.nq)), "thr and thr - 1 straddle the planted tie"
    got = feat_count_rows(c.pair, thr).numpy()[:c.nq]
    assert np.array_equal(got, want), "counts: " + ex._where(got, want, c.tile)
    cols = [1, 9, 15]
    got = feat_count_rows(c.pair, thr[:, cols]).numpy()[:c.nq]
    assert np.array_equal(got, want[:, cols]), "three columns: " + ex._where(got, want[:, cols], c.tile)
    counts = feat_count_rows(c.pair, thr, row0=half)
    assert np.array_equal(counts.numpy()[:c.nq], expected(B[:, half:], thr))
    counts = feat_count_rows(c.pair, thr, counts=counts, row0=0, n_rows=half)
    assert np.array_equal(counts.numpy()[:c.nq], want), "two calls over two parts of the bank accumulate"


class Case:
    """a case on the device with its oracle, as ex.Prepared holds one"""


def _prepared(ctx, kind, case):
    c = Case()
    c.kind, c.name, c.tile = kind, "here", 256 if kind == "fp16" else 128
    q, b = case["q"], case["b"]
    if kind == "split":
        c.Nq, c.Nb = (pr.row_sq_sums(h.astype(np.int16) + l) for h, l in (q, b))
        c.acc = pr.split_dot(q[0], q[1], b[0], b[1])
    else:
        c.Nq, c.Nb = pr.require_c(q), pr.require_c(b)
        c.acc = pr.dot_exact(q, b)
    c.M = pr.d32_exact(c.acc, c.Nq, c.Nb)
    c.B, c.Q = ex.Rows(ctx, kind, b, c.Nb), ex.Rows(ctx, kind, q, c.Nq)
    c.pair = ex.Pair(ctx, c.B, c.Q)
    c.nq, c.nb = case["nq"], case["nb"]
    return c


def row_major_case():
    """K1 = 192, 257 queries x 513 bank rows: ragged second and third tiles, the smallest shape that crosses a tile edge on both sides"""
    return ex._short(112, 513, 257, 192)


@pytest.fixture(scope="module")
def ctx():
    import ganleaks_amd
    ctx = ganleaks_amd.Context.get()
    yield ctx
    ctx.trim()


def test_fp16_rows_row_major(ctx):
    c = _prepared(ctx, "fp16", row_major_case())
    assert not c.B.blocked
    check_case(c, 264)                                               # (a row-major operand starts at a multiple of 16 bytes)


def test_fp16_rows_k_blocked(ctx):
    """K1 = 2^20 halves: K-blocked rows, 8 segments, two 256-row blocks of the bank, the second ragged"""
    K, nb, nq = 1 << 20, 300, 20
    q, b = pr.long_rows(131, nq, K), pr.long_rows(130, nb, K)
    b[nb - 3] = b[7]                                                 # the tie: every query is as far from row 7 as from row nb - 3
    pr.plant(q, b, [(0, nb - 1), (5, 7)], [(6, nb - 2, K - 1, 1)])
    c = _prepared(ctx, "fp16", dict(q=q, b=b, nq=nq, nb=nb, K=K))
    assert c.B.blocked
    check_case(c, 256)                                               # (a K-blocked operand starts on a block boundary)
    del c
    ctx.trim()


def test_split_rows(ctx):
    c = _prepared(ctx, "split", ex._split(172, 300, 130, 96))
    check_case(c, 152)


CHILD = r'''
import os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import ganleaks_amd as gl
from ganleaks_amd import _lib
import test_gpu_pair_kth_abi as t
assert _lib.LIB_PATH.endswith("libganleaks_hip_tuning.so")
os.environ["GL_PAIR_VARIANT"] = "5"
ctx = gl.Context.get()
t.check_case(t._prepared(ctx, "fp16", t.row_major_case()), 264)
print("RESULT ok")
'''


def test_fp16_rows_on_the_cluster_free_schedule():
    """the row-major case through feat_pairs_h1_kernel<4, false> (what a device with fewer than 256 CUs runs), forced in the tuning build
    by GL_PAIR_VARIANT=5 (K-blocked rows always take the clustered schedule)"""
    tuning = os.path.join(ROOT, "gan-leaks_amd", "libganleaks_hip_tuning.so")
    if not os.path.exists(tuning):
        subprocess.run(["make", "-C", os.path.join(ROOT, "gan-leaks_amd", "csrc"), "-j8", "tuning"], check=True)
    env = dict(os.environ, GANLEAKS_LIB=tuning)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert "RESULT ok" in r.stdout.decode()


def f32_count_rows(ctx, bank_dev, n_rows, q_dev, nq, d, thr, counts=None):
    from ganleaks_amd import _lib
    from ganleaks_amd.attack import new_counts
    thr = np.ascontiguousarray(thr, np.int64)
    thr_dev = ctx.to_device(thr)
    if counts is None:
        counts = new_counts(ctx, nq, thr.shape[1])
    _lib.check(ctx.lib.gl_l2_count_rows_f32(ctx.handle, p(bank_dev), n_rows, p(q_dev), nq, d, p(thr_dev.ptr), thr.shape[1], p(counts.ptr)))
    ctx.sync()
    return counts


@pytest.mark.parametrize("d", [75, 3072])
def test_fp32_rows(ctx, d):
    """70 queries x 130 rows (two query tiles, three bank tiles, both ragged); d = 75 takes the scalar loads, d = 3072 the 16-byte ones.
    Bank row 40 is so far away that its distance overflows to +inf for every query, bank row 90 holds a NaN."""
    rng = np.random.default_rng(d)
    nq, nb = 70, 130
    bank = rng.normal(0.0, 1.5, (nb, d)).astype(np.float32)
    q = rng.normal(0.0, 1.5, (nq, d)).astype(np.float32)
    q[0], q[69] = bank[129], bank[3]
    bank[nb - 3] = bank[7]
    bank[40, 1] = np.float32(3.0e38)
    bank[90, d - 1] = np.float32(np.nan)
    M = frc.chain_matrix(q, bank)
    assert np.all(np.isinf(M[:, 40])) and np.all(np.isnan(M[:, 90])) and M[0, 129] == 0 and np.isfinite(np.delete(M, [40, 90], axis=1)).all()
    B = bits64(M)
    thr = threshold_rows(B, 7)
    want = expected(B, thr)
    # a pair at +inf is counted at 0x7F800000 and not below; the NaN pair is never counted
    at = np.argmax(thr[0] == INF_BITS)
    assert thr[0, at - 1] == INF_BITS - 1 and want[0, at] == nb - 1 and want[0, at - 1] == nb - 2 and np.all(np.delete(want[:, -1], 1) == nb - 1)
    bd, qd = ctx.to_device(bank), ctx.to_device(q)
    got = f32_count_rows(ctx, bd.ptr, nb, qd.ptr, nq, d, thr).numpy()[:nq]
    assert np.array_equal(got, want), np.argwhere(got != want)[:6].tolist()
    cols = [1, 9, 15]
    assert np.array_equal(f32_count_rows(ctx, bd.ptr, nb, qd.ptr, nq, d, thr[:, cols]).numpy()[:nq], want[:, cols])
    half = 68
    counts = f32_count_rows(ctx, bd.ptr + half * d * 4, nb - half, qd.ptr, nq, d, thr)
    assert np.array_equal(counts.numpy()[:nq], expected(B[:, half:], thr))
    counts = f32_count_rows(ctx, bd.ptr, half, qd.ptr, nq, d, thr, counts=counts)
    assert np.array_equal(counts.numpy()[:nq], want), "two calls over two parts of the bank accumulate"
    # the Python wrapper on 'f32' Banks (finite rows)
    from ganleaks_amd.attack import Bank, count_balls_rows_f32
    keep = [n for n in range(nb) if n not in (40, 90)]
    fb, fq = Bank.from_images(bank[keep], ctx, force_kind="f32"), Bank.from_images(q, ctx, force_kind="f32")
    got = count_balls_rows_f32(fb, fq, thr).numpy()[:nq]
    assert np.array_equal(got, expected(B[:, keep], thr))


def _fails(lib, rc, needle):
    assert rc != 0, rc
    msg = lib.gl_last_error().decode()
    assert msg and needle in msg, msg


def test_bad_arguments_return_an_error_and_launch_nothing(ctx):
    from ganleaks_amd.attack import new_counts
    lib, h = ctx.lib, ctx.handle
    rows = ctx.zeros((256, 256), np.float32)
    norms = ctx.zeros((256,), np.float32)
    thr = ctx.to_device(np.full((256, 16), INF_BITS, np.int64))      # would count every pair
    counts = new_counts(ctx, 256, 16)
    r, n, t, c = p(rows.ptr), p(norms.ptr), p(thr.ptr), p(counts.ptr)
    calls = {
        "gl_feat_count_rows_h1_scaled": lambda K, t, T, c: lib.gl_feat_count_rows_h1_scaled(h, r, n, 256, r, n, 256, K, 16384.0, t, T, c),
        "gl_feat_count_rows": lambda K, t, T, c: lib.gl_feat_count_rows(h, r, n, 256, r, n, 256, K // 2, t, T, c),
        "gl_l2_count_rows_f32": lambda K, t, T, c: lib.gl_l2_count_rows_f32(h, r, 256, r, 256, K, t, T, c),
    }
    for name, call in calls.items():
        _fails(lib, call(128, t, 0, c), "n_thr=0 outside [1, 16]")
        _fails(lib, call(128, t, 17, c), "n_thr=17 outside [1, 16]")
        _fails(lib, call(128, p(0), 16, c), "NULL")
        _fails(lib, call(128, p(thr.ptr + 4), 16, c), "thresholds must be 8-byte aligned")
        _fails(lib, call(128, t, 16, p(counts.ptr + 4)), "counters must be 8-byte aligned")
        _fails(lib, call(128, t, 16, p(0)), "NULL")
        assert name in lib.gl_last_error().decode()
    _fails(lib, calls["gl_feat_count_rows_h1_scaled"](96, t, 16, c), "multiple of 64")
    _fails(lib, calls["gl_feat_count_rows"](96, t, 16, c), "multiple of 32")
    _fails(lib, lib.gl_l2_count_rows_f32(h, r, 256, r, 256, 0, t, 16, c), "bad sizes")
    _fails(lib, lib.gl_feat_count_rows_h1_scaled(h, r, n, 256, r, n, 256, 128, 0.0, t, 16, c), "row scale")
    # an empty problem is GL_OK and touches nothing
    assert lib.gl_feat_count_rows_h1_scaled(h, p(0), p(0), 0, r, n, 256, 128, 16384.0, p(0), 16, p(0)) == 0
    assert lib.gl_feat_count_rows(h, r, n, 256, p(0), p(0), 0, 64, p(0), 16, p(0)) == 0
    assert lib.gl_l2_count_rows_f32(h, p(0), 0, r, 256, 128, p(0), 16, p(0)) == 0
    ctx.sync()
    assert not counts.numpy().any(), "a refused call launched"
