"""What the kernel-density tests share: a numpy restatement of gl_kde_weight / gl_kde_cut (gan-leaks_amd/csrc/gl_kde_epi.h), written from
the contract and not from the header's code path -- float32 arrays whose every product and sum numpy rounds on its own -- the exact host
S of every pair (a float64 matmul), and inputs that do not pass vacuously."""
import numpy as np

FRAC_BITS = 40
ONE = 1 << FRAC_BITS
X_CUT = np.float32(41.0)
# 2^-f = 1 + f q(f) on [0, 1): the coefficients of q, lowest first (GL_KDE_C1 .. GL_KDE_C6)
COEF = [np.float32(float.fromhex(h)) for h in ("-0x1.62e430p-1", "0x1.ebfba8p-3", "-0x1.c6a652p-5", "0x1.3a79c4p-7", "-0x1.529848p-10",
                                                "0x1.e2025cp-14")]
# twice the largest relative error of kde_weight against float64 2^(-delta c) measured where the true weight is >= 2^-30 (test_kde_cpu.py,
# 1.3 x 10^6 pairs: 9.77e-4 = 2^-10, the truncation to units of 2^-40 at a weight of 2^-30; for x = delta c <= 8, where the truncation
# does not matter, the same test measures 4.4e-7).  Doubled because a sample is not a proof.
E_W = 2 * 9.8e-4


def kde_weight(delta, c):
    """uint64 array: the weight of every (delta >= 0, c >= 0 finite) pair, broadcast"""
    delta, c = np.broadcast_arrays(np.asarray(delta, np.int64), np.asarray(c, np.float32))
    assert np.all(delta >= 0)
    with np.errstate(over="ignore"):
        x = delta.astype(np.float32) * c                   # one rounded product
    assert x.dtype == np.float32
    live = x < X_CUT
    xs = np.where(live, x, np.float32(0))
    n = np.floor(xs)                                       # float32 holds 0..40 exactly
    f = xs - n                                             # exact
    q = np.full(f.shape, COEF[5], np.float32)
    for k in (4, 3, 2, 1, 0):
        q *= f                                             # separate statements: every result is a rounded float32
        q += COEF[k]
    q *= f
    p = np.float32(1.0) + q
    assert p.dtype == np.float32 and p.min() >= 0.5 and p.max() <= 1.0
    bits = p.view(np.uint32)
    m = ((bits & np.uint32(0x7FFFFF)) | np.uint32(0x800000)).astype(np.uint64)
    # p = m 2^(e - 150): p 2^(40 - n) = m 2^sh, sh = e - 110 - n in [-24, 17]; truncated by shifting m 2^17 right by 17 - sh
    down = (np.uint32(127) - (bits >> np.uint32(23))).astype(np.uint64) + n.astype(np.uint64)
    w = (m << np.uint64(17)) >> down
    return np.where(live, w, np.uint64(0))


def kde_cut(c):
    """the smallest delta with fl32(fl32(delta) c) >= 41, or 2^62 when there is none below it"""
    c = np.float32(c)

    def x(v):
        with np.errstate(over="ignore"):
            return np.float32(np.int64(v)) * c

    lo, hi = 0, 1 << 62
    if x(hi) < X_CUT:
        return hi
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if x(mid) < X_CUT:
            lo = mid
        else:
            hi = mid
    return hi


def host_S(q, b, block=16384):
    """int64 [Q, N]: the exact sum of squared differences of every pair (float64 matmul, K in blocks to bound the memory)"""
    q = np.ascontiguousarray(q).reshape(len(q), -1)
    b = np.ascontiguousarray(b).reshape(len(b), -1)
    dot = np.zeros((len(q), len(b)), np.float64)
    qn, bn = np.zeros(len(q), np.float64), np.zeros(len(b), np.float64)
    for k0 in range(0, q.shape[1], block):
        qf, bf = q[:, k0:k0 + block].astype(np.float64), b[:, k0:k0 + block].astype(np.float64)
        dot += qf @ bf.T
        qn += (qf * qf).sum(axis=1)
        bn += (bf * bf).sum(axis=1)
    S = qn[:, None] + bn[None, :] - 2.0 * dot
    assert S.max() < 2.0 ** 53 and S.min() >= 0
    return S.astype(np.int64)


_last = {"delta": None, "weights": {}}                   # the weights of the case at hand: pick_coef and want_sums evaluate the same pairs


def sparse_weights(delta, c):
    """(pairs per query below kde_cut(c), their weights in row order); the other pairs weigh nothing (kde_cut's claim, checked pair by pair
    on the CPU), so a large case never evaluates them"""
    if _last["delta"] is None or _last["delta"].shape != delta.shape or not np.array_equal(_last["delta"], delta):
        _last["delta"], _last["weights"] = delta, {}
    key = float(np.float32(c))
    if key not in _last["weights"]:
        mask = delta < kde_cut(c)
        _last["weights"][key] = (mask.sum(axis=1), kde_weight(delta[mask], c))
    return _last["weights"][key]


def row_sums(counts, values):
    """sums of consecutive runs of `values`, counts[q] values for row q (uint64)"""
    ends = np.cumsum(counts)
    total = np.concatenate([[np.uint64(0)], np.cumsum(values, dtype=np.uint64)])
    return total[ends] - total[ends - counts]


def want_sums(S, S0, coef):
    """uint64 [Q, T]: the oracle's sums over all columns of S"""
    delta = S - np.asarray(S0, np.int64)[:, None]
    return np.stack([row_sums(*sparse_weights(delta, c)) for c in np.asarray(coef, np.float32)], axis=1)


def mixed_S0(S):
    """offsets per query: the row minimum for a third of the queries, 0 for a third, the minimum - 1000 (negative where the nearest is
    close) for the rest"""
    low = S.min(axis=1)
    style = np.arange(len(S)) % 3
    return np.where(style == 0, low, np.where(style == 1, 0, low - 1000)).astype(np.int64)


def pick_coef(S, S0, T):
    """T descending float32 coefficients derived from the spread of S - S0, and the proof on the oracle's weights that they do not pass
    vacuously (check_not_vacuous).  The smallest puts x = 40, the last weight that is not 0, at the 0.35 quantile of all pairs (the 0.5 quantile when it
    is the only one), the largest puts every query's second nearest pair at x <= 30."""
    delta = S - np.asarray(S0, np.int64)[:, None]
    sample = delta.ravel()[::max(1, delta.size // 200000)].astype(np.float64)
    near = np.partition(delta, 1, axis=1)[:, 1].astype(np.float64)     # the second nearest of every query
    hi = min(30.0 / max(float(near.max()), 1.0), 40.5)
    lo = 40.0 / float(np.quantile(sample, 0.35))
    assert hi > lo, (hi, lo)
    coef = np.float32(np.geomspace(hi, lo, T)) if T > 1 else np.float32([40.0 / float(np.quantile(sample, 0.5))])
    coef = np.sort(coef)[::-1].copy()
    check_not_vacuous(delta, coef)
    return coef


def check_not_vacuous(delta, coef, nearest_too=True):
    """under the smallest coefficient at least a quarter of the pairs weigh something; under the largest every query has a pair of weight 0
    and (nearest_too) a weighted pair besides its nearest"""
    counts, w = sparse_weights(delta, coef[-1])
    assert (w != 0).sum() >= 0.25 * delta.size, (w != 0).sum() / delta.size
    counts, w = sparse_weights(delta, coef[0])
    weighted = row_sums(counts, (w != 0).astype(np.uint64))
    assert np.all(weighted < delta.shape[1]), "every query needs a pair of weight 0 under the largest coefficient"
    if nearest_too:
        assert np.all(weighted >= 2), "every query needs a weighted pair besides its nearest"


def planted_case(synth, seed, n_bank, n_q, shape, sigmas=(2.0, 6.0, 20.0, 40.0)):
    """uniformly random u8 rows have concentrated distances, so most queries are near-duplicates of bank rows at several noise levels and
    the bank holds near-duplicates of its own rows: (bank, queries)"""
    rng = np.random.default_rng(seed)
    bank = rng.integers(0, 256, size=(n_bank,) + tuple(shape), dtype=np.uint8)
    # clusters inside the bank: with G noise levels, rows g + G k (k = 1, 2, 3) of every block of 4 G rows are perturbed copies of row g
    for g, s in enumerate(sigmas):
        idx = np.arange(g, n_bank - 3, 4 * len(sigmas))
        for k in (1, 2, 3):
            dst = idx + k * len(sigmas)
            dst = dst[dst < n_bank]
            bank[dst] = synth.perturb_u8(seed + 10 * g + k, bank[idx[:len(dst)]], s)
    q = np.empty((n_q,) + tuple(shape), np.uint8)
    src = rng.integers(0, n_bank, size=n_q)
    for g, s in enumerate(sigmas):
        sel = np.arange(g, n_q, len(sigmas))
        q[sel] = synth.perturb_u8(seed + 100 + g, bank[src[sel]], s)
    return bank, q
