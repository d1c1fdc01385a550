"""GPU: the LPIPS pair kernels against an exact host oracle on integer rows (tests/pair_rows_common.py: condition C makes every fp32
accumulation exact, so D32 of every pair is known bit for bit from int64 arithmetic -- no VGG16, no tolerance).  The rows go straight into
the C ABI: fp16 search rows through gl_feat_*_h1_scaled (feat_knn_h1c / h1s and feat_pairs_h1_kernel, all on gl_pair256::mainloop), split
rows through gl_feat_* (feat_knn_kernel, feat_pairs_split_kernel).  Every comparison is np.array_equal, except the one case with a row scale
that is no power of two, whose bound of one float32 ulp is derived in pair_rows_common.

fp16 shapes and the path each reaches on a whole MI355X (256 CUs: the clustered kernels; super-tiles of 4 x 8 tiles dealt to 8 clusters):
  a  K1 = 64 at 1 x 1; K1 = 192 at bank 257 x 255 queries and 513 x 300: 2 and 3 ragged tiles, one segment, one super-tile
  b  K1 = 64 * 2048, 64 * 2049, 64 * (2 * 2048 + 100) at bank 300 x 260: 1, 2 and 3 segments (totals in HBM scratch from 2), 2 x 2 tiles
  c  K1 = 16384 at 300 x 260: a row stride of exactly 32 KiB
  d  bank 8193 x 48 queries at K1 = 64 * 2049: 9 bank super-tiles, cluster 0 takes a second one (bank row 8192) with segment totals in use;
     queries 2049 x bank 1025 at K1 = 192: two query super-tiles
  e  K1 = 2^20 and 2^20 + 64 * 37 at bank 300 x 258: K-blocked, 8 and 9 segments, block 1 ragged on both sides, its unused rows poisoned,
     one call from the second block of the bank buffer; K1 = 2^20 - 64: the longest row-major row
  f  two shards ending at global index 2^32 - 2, folded in reverse order
Split rows (tile 128, kSplitSeg = 2048 slices of 32 values): a, b and f.  A child process runs b through the cluster-free kernels
(tuning build, GL_PAIR_VARIANT=5)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_common  # noqa: F401
import pair_rows_common as pr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
p = ctypes.c_void_p
SEG = 64 * 2048                  # halves of K per accumulation segment of the fp16 kernels (split rows: 32 * 2048 values)


# ---- the cases (host data only: tests/test_pair_rows_oracle_cpu.py builds every one and checks condition C)

def _planted(q, b, K):
    """exact duplicates and near-duplicates across tiles and blocks, and a tie inside the bank; sizes permitting"""
    nq, nb = len(q), len(b)
    if nq < 30 or nb < 30:
        return q, b
    b[nb - 3] = b[7]                                                 # tie: rows 7 and nb - 3 are one row, the smaller index wins
    pairs = [(0, nb - 1), (nq - 1, 3), (20, 7)]
    # (queries nq - 1 and nq - 2 and bank rows from nb - 5 on lie in the second tile / block wherever there is one)
    near = [(5, nb - 2, K - 1, 1), (nq - 2, nb - 5, 0, -1), (6, 11, min(SEG, K - 64), 2), (7, 255 % nb, K // 2, -1)]
    pr.plant(q, b, pairs, near)
    return q, b


def _short(seed, nb, nq, K):
    q, b = _planted(pr.short_rows(seed + 1, nq, K), pr.short_rows(seed, nb, K), K)
    return dict(q=q, b=b, nq=nq, nb=nb, K=K)


def _long(seed, nb, nq, K):
    q, b = _planted(pr.long_rows(seed + 1, nq, K), pr.long_rows(seed, nb, K), K)
    return dict(q=q, b=b, nq=nq, nb=nb, K=K)


def _edge_1x1(K):
    return dict(q=pr.edge_row(1, K), b=pr.edge_row(2, K), nq=1, nb=1, K=K)


def _second_supertile():
    """8193 bank rows drawn from a pool of 1031 distinct rows (row r = pool[r % 1031]; 1031 is prime, so the rows of a tile never repeat at
    the same place of another tile) plus one row of its own at 8192, the only row of the second super-tile of cluster 0"""
    K, nb, nq = 64 * 2049, 8193, 48
    pool = pr.long_rows(40, 1032, K)
    idx = np.arange(nb) % 1031
    idx[8192] = 1031
    q = pr.long_rows(41, nq, K)
    pr.plant(q, pool, [(3, 1031), (4, 975), (47, 0)], [(5, 1031, K - 1, 1), (6, 1031, SEG, -1), (7, 1030, 5, 1)])
    return dict(q=q, b=pool[idx], nq=nq, nb=nb, K=K, pool=pool, idx=idx)


FP16_CASES = {
    "a_1x1_k64": lambda: _edge_1x1(64),
    "a_257x255_k192": lambda: _short(10, 257, 255, 192),
    "a_513x300_k192": lambda: _short(12, 513, 300, 192),
    "b_seg1": lambda: _long(20, 300, 260, SEG),
    "b_seg1_plus": lambda: _long(22, 300, 260, SEG + 64),
    "b_seg2_ragged": lambda: _long(24, 300, 260, 2 * SEG + 64 * 100),
    "c_stride_32k": lambda: _long(30, 300, 260, 16384),
    "d_second_supertile": _second_supertile,
    "d_two_query_supertiles": lambda: _short(44, 1025, 2049, 192),
    "e_blocked_threshold": lambda: _long(50, 300, 258, 1 << 20),
    "e_blocked_ragged": lambda: _long(52, 300, 258, (1 << 20) + 64 * 37),
    "e_longest_row_major": lambda: _long(54, 300, 258, (1 << 20) - 64),
    "f_shards": lambda: _short(60, 557, 70, 192),
}
ALL_FIVE = ["b_seg1", "b_seg1_plus", "b_seg2_ragged", "e_blocked_threshold", "e_blocked_ragged", "e_longest_row_major"]
TOP1_AND_COUNTS = ["a_1x1_k64", "a_257x255_k192", "a_513x300_k192", "c_stride_32k", "d_second_supertile", "d_two_query_supertiles"]


def _split(seed, nb, nq, K, long=False):
    bh, bl = pr.split_rows(seed, nb, K, long)
    qh, ql = pr.split_rows(seed + 1, nq, K, long)
    if nq >= 30 and nb >= 30:
        for x, y in ((qh, bh), (ql, bl)):                            # the same plants in both halves: whole-row duplicates
            y[nb - 3] = y[7]
            x[0], x[nq - 1], x[20], x[5] = y[nb - 1], y[3], y[7], y[nb - 2]
        qh[5, K - 1] += 1
        pr.require_c_split(qh, ql)
    return dict(q=(qh, ql), b=(bh, bl), nq=nq, nb=nb, K=K)


SPLIT_CASES = {
    "a_1x1_k32": lambda: _split(70, 1, 1, 32),
    "a_129x127_k96": lambda: _split(72, 129, 127, 96),
    "a_257x150_k96": lambda: _split(74, 257, 150, 96),
    "b_seg1": lambda: _split(80, 150, 130, SEG // 2, True),
    "b_seg1_plus": lambda: _split(82, 150, 130, SEG // 2 + 32, True),
    "b_seg2_ragged": lambda: _split(84, 150, 130, SEG + 32 * 100, True),
    "f_shards": lambda: _split(90, 280, 40, 96),
}


# ---- device side

class Rows:
    """one operand on the device: the rows as the kernels read them, and norms float32 [capacity]"""

    def __init__(self, ctx, kind, rows, N):
        self.kind, self.N = kind, np.asarray(N, np.int64)
        if kind == "split":
            hi, lo = rows
            self.n, self.K = hi.shape
            self.row_bytes, self.blocked, self.cap = 4 * self.K, False, self.n
            host = pr.pack_split(hi, lo)
        else:
            self.n, self.K = rows.shape
            self.row_bytes, self.blocked = 2 * self.K, self.K >= pr.BLOCKED_FROM
            self.cap = int(ctx.lib.gl_lpips_search_rows_capacity(self.n, self.K))
            assert self.cap == pr.blocked_capacity(self.n, self.K)
            host = pr.pack_blocked(rows, self.cap) if self.blocked else pr.half_bits(rows)
        assert host.size * 2 == self.cap * self.row_bytes
        self.V = ctx.to_device(host.reshape(-1))
        self.norms = self.norm_array(ctx, pr.norm_inputs(self.N))

    def norm_array(self, ctx, values):
        """float32 [capacity] on the device: `values` for the rows, NaN behind them (nothing may read those)"""
        host = np.full(self.cap, np.nan, np.float32)
        host[:self.n] = values
        return ctx.to_device(host)

    def at(self, row0):
        """pointer to the rows from row `row0` on; K-blocked rows only from a block boundary of a buffer of whole blocks"""
        if self.blocked:
            block = 256 * self.row_bytes
            assert self.V.nbytes % block == 0, "a K-blocked buffer holds whole blocks of 256 rows"
            assert (row0 * self.row_bytes) % block == 0, "a K-blocked operand starts on a block boundary"
        assert 0 <= row0 < self.cap and (row0 * self.row_bytes) % 16 == 0
        return p(self.V.ptr + row0 * self.row_bytes)


class Pair:
    """the five reductions over one (bank, queries) pair of operands through the C ABI; `row0`, `n_rows`: a sub-range of the bank"""

    def __init__(self, ctx, B, Q, scale=pr.SCALE, q_norms=None, b_norms=None):
        from ganleaks_amd import _lib
        assert B.kind == Q.kind and B.K == Q.K
        self.ctx, self.lib, self.h, self.B, self.Q, self.scale = ctx, ctx.lib, ctx.handle, B, Q, float(scale)
        self.check = _lib.check
        self.h1 = B.kind == "fp16"
        self.qn = Q.norms if q_norms is None else q_norms
        self.bn = B.norms if b_norms is None else b_norms
        assert self.qn.shape == (Q.cap,) and self.bn.shape == (B.cap,)

    def _ops(self, row0, n_rows):
        n = self.B.n - row0 if n_rows is None else n_rows
        assert 0 < n <= self.B.n - row0
        return (self.B.at(row0), p(self.bn.ptr + 4 * row0), n), (self.Q.at(0), p(self.qn.ptr), self.Q.n)

    def top1(self, index_base=0, keys=None, row0=0, n_rows=None):
        b, q = self._ops(row0, n_rows)
        if keys is None:
            keys = self.ctx.empty((self.Q.n,), np.uint64)
            self.check(self.lib.gl_keys_init(self.h, p(keys.ptr), self.Q.n))
        if self.h1:
            self.check(self.lib.gl_feat_knn_h1_scaled(self.h, *b, index_base, *q, self.B.K, p(keys.ptr), self.scale))
        else:
            self.check(self.lib.gl_feat_knn(self.h, *b, index_base, *q, self.B.K, p(keys.ptr)))
        return keys

    def matrix(self, ld, fill, row0=0, n_rows=None):
        b, q = self._ops(row0, n_rows)
        out = self.ctx.to_device(np.full((self.Q.n, ld), fill, np.uint32))
        if self.h1:
            self.check(self.lib.gl_feat_pair_dist_h1_scaled(self.h, *b, *q, self.B.K, self.scale, p(out.ptr), ld))
        else:
            self.check(self.lib.gl_feat_pair_dist(self.h, *b, *q, self.B.K, p(out.ptr), ld))
        return out.numpy()

    def counts(self, thr, col0=0, pitch=None, counts=None, row0=0, n_rows=None):
        from ganleaks_amd.attack import new_counts
        b, q = self._ops(row0, n_rows)
        thr = np.ascontiguousarray(thr, np.float32)
        pitch = len(thr) if pitch is None else pitch
        if counts is None:
            counts = new_counts(self.ctx, self.Q.n, pitch)
        if self.h1:
            self.check(self.lib.gl_feat_count_h1_scaled(self.h, *b, *q, self.B.K, self.scale, thr.ctypes.data_as(p), len(thr), col0, pitch, p(counts.ptr)))
        else:
            self.check(self.lib.gl_feat_count(self.h, *b, *q, self.B.K, thr.ctypes.data_as(p), len(thr), col0, pitch, p(counts.ptr)))
        return counts

    def hist(self, lo, shift, n_bins, hist=None, row0=0, n_rows=None):
        from ganleaks_amd.attack import new_hist
        b, q = self._ops(row0, n_rows)
        if hist is None:
            hist = new_hist(self.ctx, n_bins)
        if self.h1:
            self.check(self.lib.gl_feat_hist_h1_scaled(self.h, *b, *q, self.B.K, self.scale, int(lo), shift, n_bins, p(hist.ptr)))
        else:
            self.check(self.lib.gl_feat_hist(self.h, *b, *q, self.B.K, int(lo), shift, n_bins, p(hist.ptr)))
        return hist

    def topk(self, k, index_base=0, keys=None, row0=0, n_rows=None):
        b, q = self._ops(row0, n_rows)
        if keys is None:
            keys = self.ctx.empty((self.Q.n, k), np.uint64)
            self.check(self.lib.gl_topk_init(self.h, p(keys.ptr), self.Q.n, k))
        if self.h1:
            self.check(self.lib.gl_feat_topk_h1_scaled(self.h, *b, index_base, *q, self.B.K, self.scale, k, p(keys.ptr)))
        else:
            self.check(self.lib.gl_feat_topk(self.h, *b, index_base, *q, self.B.K, k, p(keys.ptr)))
        return keys


def _where(got, want, tile):
    """the pattern of wrong cells of a [nq, nb] comparison: how many, the first few, and the (query tile, bank tile) pairs they fall in"""
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    tiles = sorted(set((int(q) // tile, int(n) // tile) for q, n in bad[:100000])) if bad.ndim == 2 and bad.shape[1] == 2 else []
    return "%d wrong, first %s, (query tile, bank tile) %s" % (len(bad), bad[:6].tolist(), tiles[:12])


class Prepared:
    """a case on the device with its oracle: acc (the exact accumulator of every pair), M (D32 with the rows' own norms)"""

    def __init__(self, ctx, kind, name):
        case = (FP16_CASES if kind == "fp16" else SPLIT_CASES)[name]()
        self.kind, self.name, self.tile = kind, name, 256 if kind == "fp16" else 128
        q, b = case["q"], case["b"]
        if kind == "split":
            pr.require_c_split(*q), pr.require_c_split(*b)
            # the norms of the values the rows hold, sum((hi + lo)^2): D32 = (|q - n|^2 + 2 lo_q.lo_n) / s^2, the dropped lo.lo showing
            self.Nq, self.Nb = (pr.row_sq_sums(h.astype(np.int16) + l) for h, l in (q, b))
            self.acc = pr.split_dot(q[0], q[1], b[0], b[1])
        elif "pool" in case:
            self.Nq, self.Nb = pr.require_c(q), pr.require_c(case["pool"])[case["idx"]]
            self.acc = pr.dot_exact(q, case["pool"])[:, case["idx"]]
        else:
            self.Nq, self.Nb = pr.require_c(q), pr.require_c(b)
            self.acc = pr.dot_exact(q, b)
        self.M = pr.d32_exact(self.acc, self.Nq, self.Nb)
        self.B, self.Q = Rows(ctx, kind, b, self.Nb), Rows(ctx, kind, q, self.Nq)
        self.pair = Pair(ctx, self.B, self.Q)
        self.nq, self.nb = case["nq"], case["nb"]


_slot = {}


def prepared(ctx, kind, name):
    """one case at a time stays on the device (the K-blocked ones are 2 GiB); tests of one case follow each other"""
    if _slot.get("key") != (kind, name):
        _slot.clear()
        ctx.trim()
        _slot.update(key=(kind, name), value=Prepared(ctx, kind, name))
    return _slot["value"]


def check_top1_and_counts(c, M=None, pair=None):
    M, pair = c.M if M is None else M, pair or c.pair
    keys = pair.top1().numpy()
    want = pr.top1_keys(M)
    assert np.array_equal(keys, want), "top-1 keys: " + _where(keys[:, None], want[:, None], c.tile)
    thr = pr.thresholds16(M)
    got = pair.counts(thr).numpy()[:c.nq]
    want = pr.ball_counts(M, thr)
    assert np.array_equal(got, want), "counts: " + _where(got, want, c.tile)
    return keys


def check_matrix(c, M=None, pair=None):
    M, pair = c.M if M is None else M, pair or c.pair
    ld, fill = c.nb + 7, 0x7FC0BEEF                                  # a NaN pattern no kernel writes
    got = pair.matrix(ld, fill)
    assert np.all(got[:, c.nb:] == fill), "the tail of a matrix line was written"
    assert np.array_equal(got[:, :c.nb], pr.bits_of(M)), "matrix: " + _where(got[:, :c.nb], pr.bits_of(M), c.tile)


def check_counts_columns(c):
    """five radii into columns 3..7 of a table of 11: the other columns stay 0"""
    thr = pr.thresholds16(c.M)[[0, 3, 6, 9, 15]]
    got = c.pair.counts(thr, col0=3, pitch=11).numpy()[:c.nq]
    want = np.zeros((c.nq, 11), np.uint64)
    want[:, 3:8] = pr.ball_counts(c.M, thr)
    assert np.array_equal(got, want), "counts at col0 = 3: " + _where(got, want, c.tile)


def check_hist(c, M=None, pair=None):
    M, pair = c.M if M is None else M, pair or c.pair
    bits = np.sort(pr.bits_of(M).reshape(-1))
    lo = int(bits[len(bits) // 2]) - 700
    for window in ((0, 20, 2048), (max(lo, 0), 0, 2048)):
        got = pair.hist(*window).numpy().reshape(-1)
        want = pr.histogram(M, *window)
        assert np.array_equal(got, want), ("histogram %s: " % (window,)) + str(np.argwhere(got != want)[:6].tolist())
    assert pr.histogram(M, 0, 20, 2048).sum() == M.size and pr.histogram(M, max(lo, 0), 0, 2048).sum() > 0


def check_topk(c, ctx, one_tile_workspace_at=5):
    for k in (1, 5, 32):
        got = c.pair.topk(k).numpy()
        want = pr.topk_keys(c.M, k)
        assert np.array_equal(got, want), ("top-%d: " % k) + str(np.argwhere(got != want)[:6].tolist())
    from ganleaks_amd import _lib
    _lib.check(ctx.lib.gl_topk_set_workspace(ctx.handle, c.tile * c.tile * 4))          # slices of one tile: every slice boundary
    try:
        got = c.pair.topk(one_tile_workspace_at).numpy()
    finally:
        _lib.check(ctx.lib.gl_topk_set_workspace(ctx.handle, 0))
    assert np.array_equal(got, pr.topk_keys(c.M, one_tile_workspace_at)), "top-%d with a workspace of one tile" % one_tile_workspace_at


def check_small_norms(c, ctx):
    """norms are inputs: with some of them far too small qn + bn - 2 acc / s^2 is negative and D32 must be +0 (pattern 0, not -0)"""
    Nq, Nb = c.Nq.copy(), c.Nb.copy()
    Nq[::3] = 0
    Nb[1::2] = 0
    M = pr.d32_exact(c.acc, Nq, Nb)
    clamped = Nq[:, None] + Nb[None, :] - 2 * c.acc < 0
    assert clamped.sum() > 50 and (~clamped).sum() > 50
    pair = Pair(ctx, c.B, c.Q, q_norms=c.Q.norm_array(ctx, pr.norm_inputs(Nq)), b_norms=c.B.norm_array(ctx, pr.norm_inputs(Nb)))
    got = pair.matrix(c.nb, 0x7FC0BEEF)
    assert not np.any(got == 0x80000000), "a clamped distance came out as -0"
    assert np.array_equal(got, pr.bits_of(M)), "matrix with small norms: " + _where(got, pr.bits_of(M), c.tile)
    keys = pair.top1().numpy()
    assert np.array_equal(keys, pr.top1_keys(M))
    assert np.array_equal(pair.counts([0.0]).numpy()[:c.nq], pr.ball_counts(M, [0.0]))
    assert int(pair.hist(0, 0, 1).numpy()[0, 0]) == int((pr.bits_of(M) == 0).sum()) >= clamped.sum()
    assert np.array_equal(pair.topk(5).numpy(), pr.topk_keys(M, 5))


def check_lattice_scale(c, ctx):
    """a row scale that is no power of two (the one of 64 x 64 lattice rows): fmaf rounds a * acc + t once from exact operands, the
    double-precision restatement twice -- within one float32 ulp, indices compared where the two nearest reference values are further
    apart than the two roundings can move them"""
    s = float(ctx.lib.gl_lpips_lattice_scale(64, 64))
    assert np.log2(s) != int(np.log2(s))
    qn = (c.Nq / (np.float64(s) * s)).astype(np.float32)
    bn = (c.Nb / (np.float64(s) * s)).astype(np.float32)
    ref = pr.d32_rounded(c.acc, qn, bn, s)
    pair = Pair(ctx, c.B, c.Q, scale=s, q_norms=c.Q.norm_array(ctx, qn), b_norms=c.B.norm_array(ctx, bn))
    got = pair.matrix(c.nb, 0x7FC0BEEF).view(np.float32)
    off = np.abs(got.view(np.uint32).astype(np.int64) - pr.bits_of(ref).astype(np.int64))
    print("lattice scale %r: cells off by 0 / 1 / more ulp: %d / %d / %d" % (s, (off == 0).sum(), (off == 1).sum(), (off > 1).sum()))
    assert pr.same_within_one_ulp(got, ref), "matrix: " + _where(off > 1, off < 0, c.tile)
    keys = pair.top1().numpy()
    assert np.array_equal(keys, pr.top1_keys(got)), "the search and the stored matrix differ"
    sure = pr.separated_rows(ref)
    assert sure.sum() > c.nq // 2
    assert np.array_equal((keys & np.uint64(0xFFFFFFFF))[sure].astype(np.int64), pr.bits_of(ref).argmin(axis=1)[sure])
    assert pr.same_within_one_ulp((keys >> np.uint64(32)).astype(np.uint32).view(np.float32), ref.min(axis=1))


def check_second_block(c):
    """a bank operand that starts at row 256 of its K-blocked buffer, with norms + 256 and index_base 256"""
    assert c.B.blocked and c.nb > 256
    sub = c.M[:, 256:]
    keys = c.pair.top1(index_base=256, row0=256).numpy()
    assert np.array_equal(keys, pr.top1_keys(sub, 256)), "top-1 from the second block"
    assert np.array_equal(c.pair.topk(5, index_base=256, row0=256).numpy(), pr.topk_keys(sub, 5, 256))
    thr = pr.thresholds16(sub)
    assert np.array_equal(c.pair.counts(thr, row0=256).numpy()[:c.nq], pr.ball_counts(sub, thr))
    got = c.pair.matrix(c.nb - 256, 0, row0=256)
    assert np.array_equal(got, pr.bits_of(sub)), "matrix from the second block: " + _where(got, pr.bits_of(sub), 256)


def check_all_five(c, ctx):
    check_top1_and_counts(c)
    check_matrix(c)
    check_counts_columns(c)
    check_hist(c)
    check_topk(c, ctx)


def check_shards(c, ctx):
    """two shards whose global indices end at 2^32 - 2, folded into one set of keys, lists, counters and bins in reverse order"""
    split = c.nb - c.nb // 2 + 21                                     # shard 0 = rows [0, split), shard 1 the rest
    split -= split % 8                                               # (a row-major operand starts at a multiple of 16 bytes)
    base0 = (1 << 32) - 1 - c.nb
    assert base0 + c.nb == (1 << 32) - 1
    shards = [(split, c.nb - split, base0 + split), (0, split, base0)]
    keys = lists = counts = hist = None
    thr = pr.thresholds16(c.M)
    for row0, n, base in shards:
        keys = c.pair.top1(index_base=base, keys=keys, row0=row0, n_rows=n)
        lists = c.pair.topk(32, index_base=base, keys=lists, row0=row0, n_rows=n)
        counts = c.pair.counts(thr, counts=counts, row0=row0, n_rows=n)
        hist = c.pair.hist(0, 20, 2048, hist=hist, row0=row0, n_rows=n)
    want = pr.top1_keys(c.M, base0)
    assert np.array_equal(keys.numpy(), want), np.argwhere(keys.numpy() != want)[:6].tolist()
    assert int((want & np.uint64(0xFFFFFFFF)).max()) == (1 << 32) - 2   # query 0 is a copy of the last row
    assert np.array_equal(lists.numpy(), pr.topk_keys(c.M, 32, base0))
    assert np.array_equal(counts.numpy()[:c.nq], pr.ball_counts(c.M, thr))
    assert np.array_equal(hist.numpy().reshape(-1), pr.histogram(c.M, 0, 20, 2048))
    return split


# ---- the tests

@pytest.fixture(scope="module")
def ctx():
    import ganleaks_amd
    ctx = ganleaks_amd.Context.get()
    yield ctx
    _slot.clear()
    ctx.trim()


@pytest.mark.parametrize("name", TOP1_AND_COUNTS)
def test_fp16_rows_top1_and_counts(name, ctx):
    c = prepared(ctx, "fp16", name)
    keys = check_top1_and_counts(c)
    if name == "d_second_supertile":
        # the row of the second super-tile wins where it was planted, alone (query 3 is its copy, 5 and 6 one step away)
        assert (keys[[3, 5, 6]] & np.uint64(0xFFFFFFFF)).tolist() == [8192] * 3 and (keys[3] >> np.uint64(32)) == 0
        assert (keys[4] & np.uint64(0xFFFFFFFF)) == 975               # a copy of pool row 975 = bank rows 975, 2006, ..., 7161: the first wins
        check_matrix(c)
    if name == "a_1x1_k64":
        check_matrix(c)
        check_topk(c, ctx, one_tile_workspace_at=1)


@pytest.mark.parametrize("name", ALL_FIVE)
def test_fp16_rows_all_five_reductions(name, ctx):
    c = prepared(ctx, "fp16", name)
    assert c.B.blocked == name.startswith("e_blocked")
    check_all_five(c, ctx)
    if c.B.blocked:
        check_second_block(c)
    if name in ("b_seg1_plus", "e_blocked_ragged"):                  # one row-major and one K-blocked case (the rows are on the device already)
        check_small_norms(c, ctx)
        check_lattice_scale(c, ctx)


def test_fp16_rows_shards_up_to_the_last_index(ctx):
    c = prepared(ctx, "fp16", "f_shards")
    split = check_shards(c, ctx)
    assert 7 < split <= c.nb - 3                                     # the tied rows 7 and nb - 3 sit in different shards


@pytest.mark.parametrize("name", [n for n in SPLIT_CASES if n != "f_shards"])
def test_split_rows_all_five_reductions(name, ctx):
    c = prepared(ctx, "split", name)
    check_all_five(c, ctx)
    if name == "b_seg1_plus":
        check_small_norms(c, ctx)


def test_split_rows_shards_up_to_the_last_index(ctx):
    check_shards(prepared(ctx, "split", "f_shards"), ctx)


CHILD = r'''
import os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import ganleaks_amd as gl
from ganleaks_amd import _lib
import test_gpu_pair_rows_exact as t
assert _lib.LIB_PATH.endswith("libganleaks_hip_tuning.so")
os.environ["GL_PAIR_VARIANT"] = "5"
ctx = gl.Context.get()
for name in ("b_seg1", "b_seg1_plus", "b_seg2_ragged"):
    t.check_all_five(t.prepared(ctx, "fp16", name), ctx)
print("RESULT ok")
'''


def test_cluster_free_kernels_against_the_same_oracle():
    """shape b through feat_knn_h1s_kernel and feat_pairs_h1_kernel<EPI, false> (what a device with fewer than 256 CUs runs), forced in the
    tuning build by GL_PAIR_VARIANT=5"""
    tuning = os.path.join(ROOT, "gan-leaks_amd", "libganleaks_hip_tuning.so")
    if not os.path.exists(tuning):
        subprocess.run(["make", "-C", os.path.join(ROOT, "gan-leaks_amd", "csrc"), "-j8", "tuning"], check=True)
    env = dict(os.environ, GANLEAKS_LIB=tuning)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert "RESULT ok" in r.stdout.decode()
