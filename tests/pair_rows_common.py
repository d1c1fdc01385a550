"""Shared by tests/test_pair_rows_oracle_cpu.py and tests/test_gpu_pair_rows_exact.py: integer-valued rows for the LPIPS pair kernels and
the host statement of every reduction over them, bit for bit.

Condition C.  fp16 rows hold integers with |v| <= 2048 and sum(v^2) < 2^22 per row (split rows: sum((|hi| + |lo|)^2) < 2^22).  Then every
partial sum of products a kernel can form, in any order of slices, segments and tiles, is an integer of magnitude at most
(sum q^2 + sum n^2) / 2 < 2^22: the fp32 MFMA accumulators and the segment totals hold the exact dot product `acc`.  The norms are inputs of
the ABI; given as float32(N) / s^2 with integers N < 2^22 and a power-of-two row scale s, qn + bn = (Nq + Nb) / s^2 is exact and

    D32 = fmaxf(fmaf(-2 / s^2, acc, qn + bn), 0) = max(Nq + Nb - 2 acc, 0) / s^2          (|Nq + Nb - 2 acc| < 2^24: one exact fp32 value)

which is |q - n|^2 / s^2 when N is the row's own sum of squares.  The same epilogue ends the fp16 searches (feat_knn_h1c / h1s), the split-row
search (feat_knn_kernel with no per-row scales) and every feat_pairs_* kernel (finish_tile).  Split rows: the kernels form
acc = hi.hi + hi.lo + lo.hi and drop lo.lo, so acc = (hi + lo).(hi + lo) - lo.lo -- stated by split_dot below.

For a row scale that is no power of two, a = -2 * fl32(1 / fl32(s * s)) is what the launchers pass, t = fl32(qn + bn) what the epilogue adds,
and fmaf rounds a * acc + t once (acc exact); the double-precision restatement d32_rounded() rounds twice, so the device value lies within
one float32 ulp of it (same_within_one_ulp).

Rows live on the host as integer arrays (int8 for long rows, int16 for short ones): numpy converts those to float32 at memory speed, which
it does not for float16.  half_bits() gives the fp16 patterns the device reads; every integer up to 2048 is an exact fp16 value."""
import numpy as np

try:                             # the element-wise passes over ~10^9 values run threaded in torch; numpy does the same, slower
    import torch
except ImportError:              # pragma: no cover
    torch = None

SCALE = 16384.0                  # 2^14, the scale of hi / lo search rows and of split rows
C_BOUND = 1 << 22
BLOCK_ROWS = 256                 # K-blocked rows: [row / 256][K / 64][row % 256][64 halves]
BLOCKED_FROM = 1 << 20           # halves per row from which fp16 search rows are K-blocked (2 MiB)
POISON = np.array([0x7E00, 0x7BFF, 0xFBFF, 0xFE01, 0x7C01], np.uint16)      # NaN, +65504, -65504, -NaN, signalling NaN

def half_bits(rows):
    """integer rows -> the fp16 bit patterns of the same values, uint16 of the same shape"""
    rows = np.asarray(rows)
    assert rows.dtype.kind == "i" and (rows.dtype.itemsize == 1 or np.abs(rows).max(initial=0) <= 2048)
    if torch is not None:
        return torch.from_numpy(rows).to(torch.float16).numpy().view(np.uint16)
    return rows.astype(np.float16).view(np.uint16)


# ---- condition C

def row_sq_sums(rows):
    """sum(v^2) per row as int64"""
    rows = np.asarray(rows)
    out = np.zeros(len(rows), np.float64)
    step = max(1, (1 << 25) // max(len(rows), 1))
    for k in range(0, rows.shape[1], step):
        if torch is not None:
            c = torch.from_numpy(rows[:, k:k + step]).to(torch.float32)
            out += (c * c).sum(dim=1, dtype=torch.float64).numpy()
        else:
            c = rows[:, k:k + step].astype(np.float32)
            out += np.einsum("ij,ij->i", c, c, dtype=np.float64)
    return np.rint(out).astype(np.int64)


def require_c(rows):
    """raise ValueError unless `rows` (integers [n, K]) has |v| <= 2048 and sum(v^2) < 2^22 in every row; returns sum(v^2) [n] int64"""
    rows = np.asarray(rows)
    if rows.dtype.kind != "i" or rows.ndim != 2:
        raise ValueError("rows must be an integer array [n, K]")
    if rows.dtype.itemsize > 1 and np.abs(rows).max(initial=0) > 2048:
        raise ValueError("condition C: |v| <= 2048")
    s = row_sq_sums(rows)
    if np.any(s >= C_BOUND):
        raise ValueError("condition C: sum(v^2) = %d >= 2^22 in row %d" % (int(s.max()), int(s.argmax())))
    return s


def require_c_split(hi, lo):
    """the same for split rows: sum((|hi| + |lo|)^2) < 2^22; returns that sum [n] int64"""
    hi, lo = np.asarray(hi), np.asarray(lo)
    if hi.shape != lo.shape:
        raise ValueError("hi and lo differ in shape")
    require_c(hi)
    require_c(lo)
    both = np.abs(hi.astype(np.int16)) + np.abs(lo.astype(np.int16))
    if both.max(initial=0) > 2048:
        raise ValueError("condition C: |hi| + |lo| must stay <= 2048")
    s = row_sq_sums(both)
    if np.any(s >= C_BOUND):
        raise ValueError("condition C: sum((|hi| + |lo|)^2) = %d >= 2^22 in row %d" % (int(s.max()), int(s.argmax())))
    return s


# ---- seeded generators (every one asserts condition C on what it returns)

def long_rows(seed, n, K, wide=8, amp=40):
    """int8 [n, K], mostly -1 / 0 / +1, plus values in [-amp, amp] at `wide` random places per row, at both ends of the row and on both
    sides of every multiple of 64 * 2048 (the segment boundaries): a dropped or repeated slice moves almost every dot product"""
    rng = np.random.default_rng(seed)
    # two bits of a random byte give bit1 - bit0 = -1 / 0 / +1 with probabilities 1/4, 1/2, 1/4: four values per byte
    u = rng.integers(0, 256, size=(n, -(-K // 4)), dtype=np.uint8)
    if torch is not None:
        x = torch.from_numpy(u)[:, :, None] >> torch.tensor([0, 2, 4, 6], dtype=torch.uint8)
        rows = (((x >> 1) & 1).to(torch.int8) - (x & 1).to(torch.int8)).numpy()
    else:
        x = u[:, :, None] >> np.array([0, 2, 4, 6], np.uint8)
        rows = ((x >> 1) & 1).astype(np.int8) - (x & 1).astype(np.int8)
    rows = np.ascontiguousarray(rows.reshape(n, -1)[:, :K])
    spots = [0, K - 1] + [s + d for s in range(64 * 2048, K, 64 * 2048) for d in (-1, 0)]
    spots = np.array(sorted(set(p for p in spots if 0 <= p < K)), np.int64)
    rows[:, spots] = rng.integers(-amp, amp + 1, size=(n, len(spots)), dtype=np.int8)
    if wide:
        at = rng.integers(0, K, size=(n, wide))
        rows[np.arange(n)[:, None], at] = rng.integers(-amp, amp + 1, size=(n, wide), dtype=np.int8)
    require_c(rows)
    return rows


def short_rows(seed, n, K, amp=None):
    """int16 [n, K] uniform in [-amp, amp]; amp defaults to the widest range condition C allows for K (at most 100)"""
    if amp is None:
        amp = min(100, int(np.sqrt((C_BOUND - 1) / K)))
    rng = np.random.default_rng(seed)
    rows = rng.integers(-amp, amp + 1, size=(n, K), dtype=np.int16)
    require_c(rows)
    return rows


def edge_row(seed, K):
    """one int16 row at the edge of condition C: a single +-2047 and values within +-7 elsewhere (2047^2 + 49 (K - 1) < 2^22 needs K <= 84)"""
    rng = np.random.default_rng(seed)
    row = rng.integers(-7, 8, size=(1, K), dtype=np.int16)
    row[0, int(rng.integers(0, K))] = 2047 if seed % 2 else -2047
    require_c(row)
    return row


def plant(queries, bank, pairs, near=()):
    """queries[q] = bank[n] for (q, n) in pairs; for (q, n, k, delta) in near: queries[q] = bank[n] with value k moved by delta
    (an integer step: distance delta^2 / s^2).  In place; returns queries"""
    for q, n in pairs:
        queries[q] = bank[n]
    for q, n, k, delta in near:
        queries[q] = bank[n]
        queries[q, k] += delta
    require_c(queries)
    return queries


def split_rows(seed, n, K, long=False):
    """(hi, lo) integer arrays [n, K] with independent values in both halves (the kernels do not need lo to be a remainder)"""
    if long:
        hi, lo = long_rows(seed, n, K, amp=20), long_rows(seed + 7919, n, K, amp=20)
    else:
        amp = max(1, min(50, int(np.sqrt((C_BOUND - 1) / K)) // 2))
        hi, lo = short_rows(seed, n, K, amp), short_rows(seed + 7919, n, K, amp)
    require_c_split(hi, lo)
    return hi, lo


# ---- packers

def blocked_capacity(n, K):
    """rows a buffer for n fp16 search rows of K halves must hold (gl_lpips_search_rows_capacity)"""
    return -(-n // BLOCK_ROWS) * BLOCK_ROWS if K >= BLOCKED_FROM else n


def pack_blocked(rows, capacity=None, poison=True):
    """integer rows [n, K] -> the K-blocked buffer of fp16 patterns as a flat uint16 array of capacity * K halves: half k of row r at byte
    ((r / 256) * (K / 64) + k / 64) * 32768 + (r % 256) * 128 + (k % 64) * 2.  The rows of the last block past n hold POISON (or zeros)."""
    rows = np.asarray(rows)
    n, K = rows.shape
    if K % 64:
        raise ValueError("pack_blocked needs K a multiple of 64")
    cap = -(-n // BLOCK_ROWS) * BLOCK_ROWS if capacity is None else int(capacity)
    if cap % BLOCK_ROWS or cap < n:
        raise ValueError("a K-blocked buffer holds whole blocks of 256 rows, at least n")
    out = np.empty((cap // BLOCK_ROWS, K // 64, BLOCK_ROWS, 64), np.uint16)
    for b in range(cap // BLOCK_ROWS):
        m = min(max(n - b * BLOCK_ROWS, 0), BLOCK_ROWS)
        if m:
            src = half_bits(rows[b * BLOCK_ROWS:b * BLOCK_ROWS + m]).reshape(m, K // 64, 64).transpose(1, 0, 2)
            if torch is not None:
                torch.from_numpy(out[b, :, :m, :].view(np.int16)).copy_(torch.from_numpy(src.view(np.int16)))
            else:
                out[b, :, :m, :] = src
        if m < BLOCK_ROWS:
            out[b, :, m:, :] = np.resize(POISON, (BLOCK_ROWS - m) * 64).reshape(BLOCK_ROWS - m, 64) if poison else 0
    return out.reshape(-1)


def pack_split(hi, lo):
    """(hi, lo) integer rows [n, K] -> split rows as fp16 patterns, uint16 [n, 2 K]: every 32 values are 32 hi halves followed by 32 lo
    halves (K slices of 128 bytes, 4 K bytes per row)"""
    hi, lo = np.asarray(hi), np.asarray(lo)
    n, K = hi.shape
    if lo.shape != hi.shape or K % 32:
        raise ValueError("pack_split needs two arrays [n, K] with K a multiple of 32")
    out = np.empty((n, K // 32, 2, 32), np.uint16)
    out[:, :, 0, :] = half_bits(hi).reshape(n, K // 32, 32)
    out[:, :, 1, :] = half_bits(lo).reshape(n, K // 32, 32)
    return out.reshape(n, 2 * K)


# ---- the reference

def dot_exact(q, b):
    """q . b for integer rows under condition C as int64 [nq, nb]: a float32 BLAS matmul over chunks of K (every partial sum is
    an integer below 2^22, so float32 is exact in any order), summed in float64"""
    q, b = np.asarray(q), np.asarray(b)
    K = q.shape[1]
    assert b.shape[1] == K
    out = np.zeros((len(q), len(b)), np.float64)
    step = max(64, (1 << 25) // max(len(q) + len(b), 1))
    for k in range(0, K, step):
        if torch is not None:
            out += (torch.from_numpy(q[:, k:k + step]).to(torch.float32) @ torch.from_numpy(b[:, k:k + step]).to(torch.float32).T).numpy()
        else:
            out += q[:, k:k + step].astype(np.float32) @ b[:, k:k + step].astype(np.float32).T
    return np.rint(out).astype(np.int64)


def split_dot(q_hi, q_lo, b_hi, b_lo):
    """what the split-row kernels accumulate: hi.hi + hi.lo + lo.hi (lo.lo is dropped), int64 [nq, nb]"""
    return dot_exact(q_hi, b_hi) + dot_exact(q_hi, b_lo) + dot_exact(q_lo, b_hi)


def norm_inputs(N, scale=SCALE):
    """float32(N) / s^2 for integers N < 2^22 and a power-of-two s: the norms handed to the ABI (exact)"""
    e = np.log2(scale)
    assert e == int(e), "norm_inputs needs a power-of-two scale"
    N = np.asarray(N, np.int64)
    assert np.all(N >= 0) and np.all(N < C_BOUND)
    return (N.astype(np.float64) * 2.0 ** (-2 * int(e))).astype(np.float32)


def d32_exact(acc, Nq, Nb, scale=SCALE):
    """D32 [nq, nb] float32 = max(Nq + Nb - 2 acc, 0) / s^2 for a power-of-two s, from int64 arithmetic (a clamped cell is +0)"""
    e = np.log2(scale)
    assert e == int(e), "d32_exact needs a power-of-two scale"
    num = np.asarray(Nq, np.int64)[:, None] + np.asarray(Nb, np.int64)[None, :] - 2 * np.asarray(acc, np.int64)
    assert np.abs(num).max(initial=0) < 1 << 24
    return (np.maximum(num, 0).astype(np.float64) * 2.0 ** (-2 * int(e))).astype(np.float32)


def d32_rounded(acc, qn, bn, scale):
    """any row scale: float32(float64(a) acc + float64(fl32(qn + bn))) clamped at 0, a = -2 fl32(1 / fl32(s s)) as the launchers form it;
    a acc is exact in double (24 x 24 bits).  The device rounds a acc + t once, this twice: they differ by at most one float32 ulp."""
    s = np.float32(scale)
    a = np.float32(-2.0) * (np.float32(1.0) / np.float32(s * s))
    t = (np.asarray(qn, np.float32)[:, None] + np.asarray(bn, np.float32)[None, :]).astype(np.float32)
    d = (np.float64(a) * np.asarray(acc, np.int64).astype(np.float64) + t.astype(np.float64)).astype(np.float32)
    return np.maximum(d, np.float32(0.0))


def bits_of(M):
    return np.ascontiguousarray(M, np.float32).view(np.uint32)


def top1_keys(M, index_base=0):
    """bits(min) << 32 | (index_base + first argmin) per query, uint64 [nq]; M >= +0, where the order of the patterns is the order of the floats"""
    bits = bits_of(M)
    idx = bits.argmin(axis=1)                                   # numpy's argmin is the first one = the smallest index
    return (bits[np.arange(len(bits)), idx].astype(np.uint64) << np.uint64(32)) | (np.uint64(index_base) + idx.astype(np.uint64))


def topk_keys(M, k, index_base=0):
    """the k nearest per query by a stable argsort (ties to the smaller index), as keys uint64 [nq, k]; ~0 pads a list longer than the bank"""
    bits = bits_of(M)
    order = np.argsort(bits, axis=1, kind="stable")[:, :k]
    keys = (np.take_along_axis(bits, order, axis=1).astype(np.uint64) << np.uint64(32)) | (np.uint64(index_base) + order.astype(np.uint64))
    if keys.shape[1] < k:
        keys = np.concatenate([keys, np.full((len(keys), k - keys.shape[1]), ~np.uint64(0))], axis=1)
    return keys


def merge_topk(lists, k):
    """the k smallest keys of several [nq, *] key lists"""
    return np.sort(np.concatenate(lists, axis=1), axis=1)[:, :k]


def ball_counts(M, thr):
    """counts [nq, len(thr)] uint64 = (M <= thr[t]).sum over the bank"""
    return np.stack([(M <= np.float32(t)).sum(axis=1) for t in thr], axis=1).astype(np.uint64)


def histogram(M, lo, shift, n_bins):
    """hist [n_bins] uint64 over ALL pairs: bin (bits - lo) >> shift of the patterns inside the window"""
    bits = bits_of(M).astype(np.int64).reshape(-1)
    b = (bits - int(lo)) >> int(shift)
    keep = (bits >= int(lo)) & (b < int(n_bins)) & (bits <= 0x7F800000)
    return np.bincount(b[keep], minlength=int(n_bins)).astype(np.uint64)


def thresholds16(M):
    """16 ascending float32 radii: 0, attained values (quantiles of M picked as exact members, the smallest and the largest one), values
    between attained ones, +inf"""
    v = np.unique(M)
    pick = v[np.minimum((np.array([0.0, 0.001, 0.01, 0.05, 0.2, 0.5, 0.8, 0.99, 1.0]) * (len(v) - 1)).astype(np.int64), len(v) - 1)]
    mins = np.quantile(M.min(axis=1), [0.25, 0.5, 0.75], method="lower")
    between = np.float32(0.5) * (v[len(v) // 3] + v[min(len(v) // 3 + 1, len(v) - 1)])
    thr = np.sort(np.concatenate([[0.0], pick, mins, [between, v[-1] * np.float32(1.5), np.inf]]).astype(np.float32))
    assert len(thr) == 16
    return thr


def same_within_one_ulp(dev, ref):
    """non-negative float32 arrays whose patterns differ by at most 1 everywhere"""
    d = bits_of(dev).astype(np.int64) - bits_of(ref).astype(np.int64)
    return bool(np.all(np.abs(d) <= 1))


def separated_rows(ref, ulps=2):
    """bool [nq]: the two nearest reference values of the row differ by more than `ulps` float32 ulps (its argmin is then decided whatever
    way the device's single rounding falls)"""
    bits = np.sort(bits_of(ref).astype(np.int64), axis=1)
    if bits.shape[1] < 2:
        return np.ones(len(bits), bool)
    return (bits[:, 1] - bits[:, 0]) > ulps
