"""What the kernel-density tests of the float paths share: a numpy restatement of gl_kde_weight_x / gl_kde_weight_f32 / gl_kde_cut_bits
(gan-leaks_amd/csrc/gl_kde_epi.h), written from the contract and not from the header's code path -- float32 arrays whose every difference,
product and sum numpy rounds on its own --, the host sums over a float32 distance matrix, and inputs that do not pass vacuously (host
data only: tests/test_pair_kde_cpu.py builds every case and checks it without a GPU)."""
import numpy as np

import kde_common as kc
import pair_rows_common as pr

ONE = kc.ONE
X_CUT = kc.X_CUT
INF_BITS = 0x7F800000
# Twice the largest relative error of gl_kde_weight_f32 against float64 2^(-(D - D0) c) measured where the true weight is >= 2^-30
# (test_pair_kde_cpu.py, 1.1 x 10^6 triples: 9.71e-4, just below 2^-10, the truncation to units of 2^-40 at a weight of 2^-30, as on the
# integer path; for x <= 8, where the truncation does not matter, the same test measures 5.3e-7: the fp32 roundings of D - D0 and of the
# product and the polynomial's error).  Doubled because a sample is not a proof.
E_F32 = 2 * 9.71e-4


def weight_x(x):
    """uint64 array: gl_kde_weight_x of float32 x (>= 0, inf or NaN)"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        live = x < X_CUT                                   # NaN and inf: not live
    xs = np.where(live, x, np.float32(0))
    n = np.floor(xs)                                       # float32 holds 0..40 exactly
    f = xs - n                                             # exact
    q = np.full(f.shape, kc.COEF[5], np.float32)
    for k in (4, 3, 2, 1, 0):
        q *= f                                             # separate statements: every result is a rounded float32
        q += kc.COEF[k]
    q *= f
    p = np.float32(1.0) + q
    assert p.dtype == np.float32 and (p.size == 0 or (p.min() >= 0.5 and p.max() <= 1.0))
    bits = p.view(np.uint32)
    m = ((bits & np.uint32(0x7FFFFF)) | np.uint32(0x800000)).astype(np.uint64)
    down = (np.uint32(127) - (bits >> np.uint32(23))).astype(np.uint64) + n.astype(np.uint64)
    w = (m << np.uint64(17)) >> down
    return np.where(live, w, np.uint64(0))


def x_of(D, D0, c):
    """x = fl32(fl32(D - D0) c), broadcast: one rounded subtraction, one rounded product"""
    D, D0, c = np.broadcast_arrays(np.asarray(D, np.float32), np.asarray(D0, np.float32), np.asarray(c, np.float32))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        delta = D - D0
        assert delta.dtype == np.float32
        x = delta * c
    assert x.dtype == np.float32
    return x


def weight_f32(D, D0, c):
    """uint64 array: gl_kde_weight_f32 of every (D >= D0 >= 0, c >= 0 finite) triple, broadcast"""
    return weight_x(x_of(D, D0, c))


def cut_bits(D0, c):
    """the smallest pattern b in [bits(D0), +inf] with not (x(b) < 41): a bisection over the patterns, scalar"""
    D0, c = np.float32(D0), np.float32(c)

    def beyond(b):
        with np.errstate(invalid="ignore"):
            return not (x_of(np.uint32(b).view(np.float32), D0, c) < X_CUT)

    lo, hi = int(D0.view(np.uint32)), INF_BITS
    assert lo < hi and not beyond(lo)
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if beyond(mid):
            hi = mid
        else:
            lo = mid
    return hi


def bits_of(M):
    return np.ascontiguousarray(M, np.float32).view(np.uint32)


def want_sums(M, D0, coef):
    """uint64 [Q, T]: the host sums over all columns of the float32 matrix M (every M[q, n] >= D0[q]; +inf weighs nothing)"""
    D0 = np.asarray(D0, np.float32)
    assert np.all(bits_of(M) >= bits_of(D0)[:, None]) and not np.isnan(M).any()
    return np.stack([weight_f32(M, D0[:, None], c).sum(axis=1, dtype=np.uint64) for c in np.asarray(coef, np.float32)], axis=1)


def check_not_vacuous(M, D0, coef):
    """on the host data: under the smallest coefficient at least a quarter of the pairs weigh something; under the largest every query has
    a pair of weight 0 and a weighted pair besides its nearest"""
    coef = np.asarray(coef, np.float32)
    assert np.all(coef[1:] <= coef[:-1])
    D0 = np.asarray(D0, np.float32)[:, None]
    w = weight_f32(M, D0, coef[-1])
    assert (w != 0).sum() >= 0.25 * M.size, (w != 0).sum() / M.size
    weighted = (weight_f32(M, D0, coef[0]) != 0).sum(axis=1)
    assert np.all(weighted < M.shape[1]), "every query needs a pair of weight 0 under the largest coefficient"
    assert np.all(weighted >= 2), "every query needs a weighted pair besides its nearest"


def pick_coef(M, D0, T):
    """T descending float32 coefficients from the spread of M - D0, and the proof on the host weights that they do not pass vacuously: the
    smallest puts x = 40 at the 0.35 quantile of all finite pairs (the 0.5 quantile when it is the only one -- then the largest as well,
    and the second nearest of every query must lie below that quantile), the largest puts every query's second nearest pair at x <= 30"""
    delta = M.astype(np.float64) - np.asarray(D0, np.float64)[:, None]
    finite = delta[np.isfinite(delta)]
    near = np.partition(delta, 1, axis=1)[:, 1]
    hi = 30.0 / max(float(near.max()), 1e-30)
    lo = 40.0 / float(np.quantile(finite, 0.35))
    assert hi > lo, (hi, lo)
    coef = np.float32(np.geomspace(hi, lo, T)) if T > 1 else np.float32([40.0 / float(np.quantile(finite, 0.5))])
    coef = np.sort(coef)[::-1].copy()
    check_not_vacuous(M, D0, coef)
    return coef


def bandwidths_of(coef):
    """the bandwidths whose kde_coef is (up to its own rounding) `coef`: h = log2(e) / coef"""
    return np.log2(np.e) / np.asarray(coef, np.float64)


def host_loss(M, h_eff, n_eff):
    """float64 [Q, T]: -h ln(1/n_eff sum_n exp(-M / h)) by a log-sum-exp around the row minimum, M in float64"""
    M = np.asarray(M, np.float64)
    D0 = M.min(axis=1, keepdims=True)
    out = np.empty((len(M), len(h_eff)), np.float64)
    for t, h in enumerate(np.asarray(h_eff, np.float64)):
        out[:, t] = D0[:, 0] - h * np.log(np.exp(-(M - D0) / h).sum(axis=1) / float(n_eff))
    return out


# ---- fp32 rows: near-duplicate clusters inside the bank, queries that are copies and near-copies of bank rows

def f32_case(seed, nq, nb, d, copies=5):
    """(queries, bank) float32 [*, d]: N(0, 1) rows; bank rows 4 k + 1 .. 4 k + 3 are row 4 k plus noise of three sizes; every query is a bank
    row plus noise, the first `copies` queries exact copies (D0 = 0)"""
    rng = np.random.default_rng(seed)
    bank = rng.normal(0.0, 1.0, (nb, d)).astype(np.float32)
    for k, s in ((1, 0.02), (2, 0.05), (3, 0.1)):
        dst = np.arange(k, nb, 4)
        bank[dst] = bank[dst - k] + rng.normal(0.0, s, (len(dst), d)).astype(np.float32)
    src = rng.integers(0, nb, size=nq)
    sig = np.float32(0.03) * (1 + np.arange(nq) % 3).astype(np.float32)
    q = bank[src] + sig[:, None] * rng.normal(0.0, 1.0, (nq, d)).astype(np.float32)
    q[:copies] = bank[src[:copies]]
    return np.ascontiguousarray(q, np.float32), bank


# ---- condition-C integer rows for the LPIPS kernels (pair_rows_common): D32 = max(Nq + Nb - 2 acc, 0) / 2^28 exactly

def _cluster_int(rows, rng, changes, step):
    """rows 4 k + 1 .. 4 k + 3 become row 4 k with `changes` values moved by up to +-step * k"""
    n, K = rows.shape
    for k in (1, 2, 3):
        dst = np.arange(k, n, 4)
        rows[dst] = rows[dst - k]
        at = rng.integers(0, K, size=(len(dst), changes))
        rows[dst[:, None], at] += rng.integers(-step * k, step * k + 1, size=at.shape).astype(rows.dtype)
    return rows


def _near_queries(bank, nq, rng, changes, step, copies):
    n, K = bank.shape
    src = rng.integers(0, n, size=nq)
    q = bank[src].copy()
    at = rng.integers(0, K, size=(nq, changes))
    move = rng.integers(-step, step + 1, size=at.shape).astype(bank.dtype)
    move[:copies] = 0                                      # exact copies: D0 = 0
    q[np.arange(nq)[:, None], at] += move
    return q


def fp16_case(seed, nq, nb, K, long=False, copies=3):
    """dict(q, b, nq, nb, K) of integer rows under condition C with planted clusters: short rows (int16, |v| <= 60) or long ones (int8,
    mostly -1 / 0 / +1, for the K-blocked row lengths)"""
    rng = np.random.default_rng(seed)
    if long:
        b = pr.long_rows(seed, nb, K, amp=20)
        b = _cluster_int(b, rng, 40, 2)
        q = _near_queries(b, nq, rng, 30, 2, copies)
    else:
        b = pr.short_rows(seed, nb, K, amp=60)
        b = _cluster_int(b, rng, 8, 3)
        q = _near_queries(b, nq, rng, 6, 3, copies)
    pr.require_c(b), pr.require_c(q)
    return dict(q=q, b=b, nq=nq, nb=nb, K=K)


def split_case(seed, nq, nb, K, copies=3):
    """the same for split rows: hi in +-50, lo in +-2 (the kernels drop lo.lo, so a copy sits at 2 |lo|^2 / s^2, far below an unrelated row)"""
    rng = np.random.default_rng(seed)
    bh = _cluster_int(pr.short_rows(seed, nb, K, amp=50), rng, 6, 3)
    bl = pr.short_rows(seed + 7919, nb, K, amp=2)
    for k in (1, 2, 3):
        dst = np.arange(k, nb, 4)
        bl[dst] = bl[dst - k]
    src = rng.integers(0, nb, size=nq)
    qh, ql = bh[src].copy(), bl[src].copy()
    at = rng.integers(0, K, size=(nq, 5))
    move = rng.integers(-3, 4, size=at.shape).astype(qh.dtype)
    move[:copies] = 0
    qh[np.arange(nq)[:, None], at] += move
    pr.require_c_split(bh, bl), pr.require_c_split(qh, ql)
    return dict(q=(qh, ql), b=(bh, bl), nq=nq, nb=nb, K=K)


def int_case_matrix(kind, case):
    """(M float32 [nq, nb], Nq, Nb): the exact D32 of every pair of an fp16_case / split_case, with the rows' own norms"""
    q, b = case["q"], case["b"]
    if kind == "split":
        Nq, Nb = (pr.row_sq_sums(h.astype(np.int16) + l) for h, l in (q, b))
        acc = pr.split_dot(q[0], q[1], b[0], b[1])
    else:
        Nq, Nb = pr.require_c(q), pr.require_c(b)
        acc = pr.dot_exact(q, b)
    return pr.d32_exact(acc, Nq, Nb), Nq, Nb


# the kernel-level GPU cases (tests/test_gpu_pair_kde.py), built and proven non-vacuous on the CPU by tests/test_pair_kde_cpu.py
F32_CASES = {"d50_scalar_loads": (4201, 70, 150, 50), "d96_vector_loads": (4202, 70, 150, 96)}
FP16_CASE = (4210, 300, 520, 128)                         # two 256-tiles, ragged both ways
SPLIT_CASE = (4211, 130, 260, 64)                         # two 128-tiles queries, three bank
BLOCKED_CASE = (4212, 4, 20, pr.BLOCKED_FROM)             # the smallest K-blocked row length
