"""The host side of tests/test_gpu_pair_rows_exact.py, checked without a GPU: the reference functions of tests/pair_rows_common.py against
Python-int brute force, the K-blocked packer against the inverse the package ships (FeatureBank.rows_numpy), and condition C for every
generator at the shapes the GPU file uses."""
import struct

import numpy as np
import pytest

import pair_rows_common as pr
import test_gpu_pair_rows_exact as g


def _f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _brute_matrix(q, b, Nq, Nb):
    """[[float]] from Python integers: max(Nq + Nb - 2 q.n, 0) * 2^-28 (an integer below 2^24 times a power of two: exact as a float)"""
    out = []
    for i, qr in enumerate(q.tolist()):
        out.append([max(int(Nq[i]) + int(Nb[j]) - 2 * sum(x * y for x, y in zip(qr, br)), 0) * 2.0 ** -28 for j, br in enumerate(b.tolist())])
    return out


@pytest.fixture(scope="module")
def tiny():
    b = pr.short_rows(3, 23, 64, amp=9)
    q = pr.plant(pr.short_rows(4, 7, 64, amp=9), b, [(0, 5), (2, 19)], [(1, 5, 7, 1), (3, 22, 63, -2)])
    b[11] = b[5]                                                    # a tie at distance 0 for query 0: the smaller index wins
    Nq, Nb = pr.row_sq_sums(q), pr.row_sq_sums(b)
    return q, b, Nq, Nb


def test_reference_matrix_is_python_integer_arithmetic(tiny):
    q, b, Nq, Nb = tiny
    assert Nq.tolist() == [sum(v * v for v in r) for r in q.tolist()]
    acc = pr.dot_exact(q, b)
    assert acc.tolist() == [[sum(x * y for x, y in zip(qr, br)) for br in b.tolist()] for qr in q.tolist()]
    M = pr.d32_exact(acc, Nq, Nb)
    assert M.dtype == np.float32
    brute = _brute_matrix(q, b, Nq, Nb)
    assert M.tolist() == brute
    # with the rows' own norms the matrix is |q - n|^2 / 2^28, the formula of the issue
    want = np.float32(((q.astype(np.int64)[:, None, :] - b.astype(np.int64)[None, :, :]) ** 2).sum(axis=2) * 2.0 ** -28)
    assert np.array_equal(M, want)
    assert M[0, 5] == 0 and M[0, 11] == 0 and M[1, 5] == np.float32(2.0 ** -28) and M[3, 22] == np.float32(4 * 2.0 ** -28)
    # norms as the ABI takes them: exact
    assert pr.norm_inputs(Nq).astype(np.float64).tolist() == [int(v) * 2.0 ** -28 for v in Nq]


def test_small_norms_clamp_to_plus_zero(tiny):
    q, b, Nq, Nb = tiny
    acc = pr.dot_exact(q, b)
    M = pr.d32_exact(acc, np.zeros_like(Nq), np.zeros_like(Nb))
    neg = acc > 0
    assert neg.any() and np.all(pr.bits_of(M)[neg] == 0)             # +0, never the pattern of -0
    assert np.array_equal(M[~neg], np.float32(-2 * acc[~neg] * 2.0 ** -28))


def test_keys_counts_histogram_against_brute_force(tiny):
    q, b, Nq, Nb = tiny
    M = pr.d32_exact(pr.dot_exact(q, b), Nq, Nb)
    brute = _brute_matrix(q, b, Nq, Nb)
    base = (1 << 32) - 1 - len(b)
    top1, k5 = pr.top1_keys(M, base), pr.topk_keys(M, 5, base)
    for i, row in enumerate(brute):
        keys = sorted((_f32_bits(d) << 32) | (base + j) for j, d in enumerate(row))
        assert int(top1[i]) == keys[0]
        assert [int(v) for v in k5[i]] == keys[:5]
    assert int(top1[0]) & 0xFFFFFFFF == base + 5                      # the tie of rows 5 and 11
    assert int(top1.max()) & 0xFFFFFFFF <= (1 << 32) - 2
    wide = pr.topk_keys(M, 32, 0)
    assert wide.shape == (7, 32) and np.all(wide[:, 23:] == ~np.uint64(0)) and np.array_equal(wide[:, :5], pr.topk_keys(M, 5, 0))
    assert np.array_equal(pr.merge_topk([pr.topk_keys(M[:, 9:], 5, 9), pr.topk_keys(M[:, :9], 5, 0)], 5), pr.topk_keys(M, 5, 0))
    thr = pr.thresholds16(M)
    assert thr[0] == 0 and np.isinf(thr[-1]) and np.all(np.diff(thr) >= 0) and np.isin(thr[1:10], M).sum() >= 8
    counts = pr.ball_counts(M, thr)
    assert counts.tolist() == [[sum(1 for d in row if d <= float(t)) for t in thr] for row in brute]
    assert counts[0, 0] == 2 and np.all(counts[:, -1] == len(b))
    allbits = [_f32_bits(d) for row in brute for d in row]
    lo = sorted(allbits)[len(allbits) // 2] - 100
    for window in ((0, 20, 2048), (lo, 0, 2048), (lo, 3, 17)):
        want = [0] * window[2]
        for v in allbits:
            if v >= window[0] and (v - window[0]) >> window[1] < window[2]:
                want[(v - window[0]) >> window[1]] += 1
        assert pr.histogram(M, *window).tolist() == want
    assert pr.histogram(M, 0, 20, 2048).sum() == M.size


def test_split_dot_drops_lo_lo():
    qh, ql = pr.split_rows(5, 6, 96)
    bh, bl = pr.split_rows(6, 9, 96)
    acc = pr.split_dot(qh, ql, bh, bl)
    want = [[sum(a * c + a * d + e * c for a, e, c, d in zip(qh[i].tolist(), ql[i].tolist(), bh[j].tolist(), bl[j].tolist())) for j in range(9)]
            for i in range(6)]
    assert acc.tolist() == want
    full = pr.dot_exact(qh + ql, bh + bl)
    assert np.array_equal(acc, full - pr.dot_exact(ql, bl))
    packed = pr.pack_split(qh, ql)
    assert packed.shape == (6, 192) and packed.dtype == np.uint16
    v = packed.view(np.float16).reshape(6, 3, 2, 32)
    assert np.array_equal(v[:, :, 0, :].reshape(6, 96), qh) and np.array_equal(v[:, :, 1, :].reshape(6, 96), ql)


def test_rounded_reference_and_ulp_comparison():
    rng = np.random.default_rng(9)
    acc = rng.integers(-(1 << 21), 1 << 21, size=(5, 8))
    qn, bn = rng.uniform(0, 0.02, 5).astype(np.float32), rng.uniform(0, 0.02, 8).astype(np.float32)
    s = np.float32(14133.53)
    ref = pr.d32_rounded(acc, qn, bn, s)
    a = np.float32(-2.0) * (np.float32(1.0) / (s * s))
    for i in range(5):
        for j in range(8):
            want = max(np.float32(float(a) * int(acc[i, j]) + float(np.float32(qn[i] + bn[j]))), np.float32(0))
            assert ref[i, j] == want
    # a power-of-two scale leaves nothing to round: the two statements agree bit for bit
    q, b = pr.short_rows(1, 4, 64), pr.short_rows(2, 6, 64)
    Nq, Nb = pr.row_sq_sums(q), pr.row_sq_sums(b)
    acc = pr.dot_exact(q, b)
    assert np.array_equal(pr.d32_rounded(acc, pr.norm_inputs(Nq), pr.norm_inputs(Nb), pr.SCALE), pr.d32_exact(acc, Nq, Nb))
    up = np.nextafter(ref, np.float32(np.inf))
    assert pr.same_within_one_ulp(up, ref) and not pr.same_within_one_ulp(np.nextafter(up, np.float32(np.inf)), ref)
    m = np.array([[1.0, 1.0000001, 3.0], [1.0, 2.0, 3.0]], np.float32)
    assert pr.separated_rows(m).tolist() == [False, True]


@pytest.mark.parametrize("n,K", [(1, 1 << 20), (300, 1 << 20), (258, (1 << 20) + 64 * 37)])
def test_blocked_packer_is_the_inverse_of_rows_numpy(n, K):
    """FeatureBank.rows_numpy undoes the K-blocked layout for tools; the packer must be its inverse, byte formula included"""
    from ganleaks_amd import _lib
    from ganleaks_amd.lpips import FeatureBank
    rows = pr.long_rows(n, n, K)
    cap = int(_lib.load().gl_lpips_search_rows_capacity(n, K))
    assert cap == pr.blocked_capacity(n, K) == -(-n // 256) * 256
    buf = pr.pack_blocked(rows, cap)
    assert buf.dtype == np.uint16 and buf.size == cap * K

    class Host:
        def numpy(self):
            return buf.view(np.float16)

    fb = FeatureBank(None, Host(), None, n, K, 0, role="bank", fmt="lattice")
    assert fb.blocked
    assert np.array_equal(fb.rows_numpy().view(np.uint16), pr.half_bits(rows))
    rng = np.random.default_rng(n)
    for r, k in zip(rng.integers(0, n, 50).tolist() + [n - 1], rng.integers(0, K, 50).tolist() + [K - 1]):
        byte = ((r // 256) * (K // 64) + k // 64) * 32768 + (r % 256) * 128 + (k % 64) * 2
        assert buf[byte // 2] == pr.half_bits(rows[r:r + 1, k:k + 1])[0, 0]
    if cap > n:                                                      # the unused rows of the last block hold poison, every K slice of them
        m = 256 - n % 256
        tail = buf.reshape(cap // 256, K // 64, 256, 64)[-1, :, n % 256:, :]
        assert np.array_equal(tail, np.broadcast_to(np.resize(pr.POISON, m * 64).reshape(m, 64), tail.shape))
        bad = pr.POISON.view(np.float16).astype(np.float32)
        assert np.all(np.isnan(bad) | (np.abs(bad) == 65504)) and np.isnan(bad).any() and (bad == 65504).any() and (bad == -65504).any()
    assert pr.blocked_capacity(300, (1 << 20) - 64) == 300          # the longest row-major row


def test_a_wrong_packer_does_not_pass():
    """what the device would read from a packer with the block index off by one, or with the last K slice zeroed, is not the reference: the
    oracle tells them apart on host data alone"""
    from ganleaks_amd.lpips import FeatureBank
    torch = pytest.importorskip("torch")
    K, n = 1 << 20, 260
    rows = pr.long_rows(77, n, K)
    q = pr.long_rows(78, 2, K)
    good = pr.pack_blocked(rows, poison=False).reshape(2, K // 64, 256, 64)

    def read_back(buf):
        class Host:
            def numpy(self):
                return np.ascontiguousarray(buf).reshape(-1).view(np.float16)
        back = FeatureBank(None, Host(), None, n, K, 0, role="bank", fmt="lattice").rows_numpy()
        return torch.from_numpy(np.ascontiguousarray(back)).to(torch.int8).numpy()

    M = pr.d32_exact(pr.dot_exact(q, rows), pr.row_sq_sums(q), pr.row_sq_sums(rows))
    swapped = good[::-1]                                             # block index off by one (modulo the two blocks)
    last_zeroed = good.copy()
    last_zeroed[:, -1] = 0
    for wrong in (swapped, last_zeroed):
        got = pr.d32_exact(pr.dot_exact(q, read_back(wrong)), pr.row_sq_sums(q), pr.row_sq_sums(rows))
        assert not np.array_equal(got, M)
        assert (got != M).mean() > 0.4


@pytest.mark.parametrize("name", sorted(g.FP16_CASES) + sorted(g.SPLIT_CASES))
def test_every_generated_row_set_of_the_gpu_file_satisfies_condition_c(name):
    if name in g.SPLIT_CASES:
        case = g.SPLIT_CASES[name]()
        for hi, lo in (case["q"], case["b"]):
            assert np.all(pr.require_c_split(hi, lo) < pr.C_BOUND)
    else:
        case = g.FP16_CASES[name]()
        for rows in (case["q"], case["b"]):
            assert np.all(pr.require_c(rows) < pr.C_BOUND)
    assert len(case["q"][0] if name in g.SPLIT_CASES else case["q"]) == case["nq"]


def test_the_gpu_file_has_the_shapes_of_its_edges():
    want = {"a_1x1_k64", "a_257x255_k192", "a_513x300_k192", "b_seg1", "b_seg1_plus", "b_seg2_ragged", "c_stride_32k", "d_second_supertile",
            "d_two_query_supertiles", "e_blocked_threshold", "e_blocked_ragged", "e_longest_row_major"}
    assert want <= set(g.FP16_CASES)
    assert {"a_1x1_k32", "a_129x127_k96", "a_257x150_k96", "b_seg1", "b_seg1_plus", "b_seg2_ragged"} <= set(g.SPLIT_CASES)


def test_rows_violating_condition_c_are_rejected():
    ok = pr.short_rows(1, 2, 64)
    bad = ok.copy()
    bad[1, 3] = 2049
    with pytest.raises(ValueError, match="2048"):
        pr.require_c(bad)
    heavy = np.full((1, 64 * 16), 64, np.int16)                      # 1024 * 64^2 = 2^22 exactly: one too many
    with pytest.raises(ValueError, match="2\\^22"):
        pr.require_c(heavy)
    heavy[0, 0] = 63
    assert pr.require_c(heavy)[0] == (1 << 22) - 127
    with pytest.raises(ValueError, match="integer"):
        pr.require_c(ok.astype(np.float32))
    hi = np.full((1, 64 * 16), 40, np.int16)
    lo = np.full((1, 64 * 16), 24, np.int16)                         # each half is fine, |hi| + |lo| = 64 is not
    pr.require_c(hi), pr.require_c(lo)
    with pytest.raises(ValueError, match="hi"):
        pr.require_c_split(hi, lo)
    with pytest.raises(ValueError):
        pr.require_c(np.full((2, 1 << 20), 2, np.int8))              # long rows of +-2 everywhere: 2^22
    full = np.full((2, 1820), 48, np.int16)                          # 1820 * 48^2 = 2^22 - 1024, and one value moved by 40 is too much
    pr.require_c(full)
    with pytest.raises(ValueError):
        pr.plant(full.copy(), full, [], [(0, 0, 5, 40)])
