"""GPU: the kernel-density (soft-min) sums on the exact-integer path (kde_sums, kde_scores, gl_l2_kde_rows_i8*, DeviceGroup.kde_scores).

The oracle is tests/kde_common.py: a numpy restatement of the weight on S from a float64 matmul on the host, so neither the kernels nor the
host code under test produce expected values; the integer sums are compared with array_equal.  Every comparison first asserts on the
oracle's weights that its coefficients do not pass vacuously (kde_common.check_not_vacuous)."""
import numpy as np
import pytest

import gpu_common  # noqa: F401
import kde_common as kc

pytestmark = pytest.mark.gpu
ONE = np.uint64(kc.ONE)


@pytest.fixture(scope="module")
def gl():
    import ganleaks_amd
    return ganleaks_amd


def sums(bank, queries, S0, coef, **kw):
    from ganleaks_amd.attack import kde_sums
    out, fq, _ = kde_sums(bank, queries, S0, coef, **kw)
    assert out.dtype == np.dtype(np.uint64)
    return out.numpy()[:fq.n]


@pytest.fixture(scope="module")
def small(gl):
    """300 rows x 130 queries of 3 x 8 x 8: both extents ragged in the 128 x 128 tile, three tiles of bank rows, two of queries"""
    bank, q = kc.planted_case(gl.synth, 4110, 300, 130, (3, 8, 8))
    bank[299] = bank[0]
    q[7], q[129] = bank[3], bank[299]                      # exact copies: S = 0; query 129 has two of them, a tie at its minimum
    return bank, q, kc.host_S(q, bank)


def test_tile128_ragged_both_ways(gl, small):
    from ganleaks_amd.attack import Bank, count_balls_rows
    ctx = gl.Context.get()
    bank, q, S = small
    b, f = Bank.from_images(bank, ctx), Bank.from_images(q, ctx)
    S0 = kc.mixed_S0(S)
    assert (S0 < 0).any() and (S0 == S.min(axis=1)).any() and (S[129] == 0).sum() == 2 and S0[129] == 0
    for T in (1, 5, 16):
        coef = kc.pick_coef(S, S0, T)
        got, want = sums(b, f, S0, coef), kc.want_sums(S, S0, coef)
        assert got.shape == (130, T) and np.array_equal(got, want), (T, np.argwhere(got != want)[:5])
    # a device array of offsets is taken as it is
    assert np.array_equal(sums(b, f, ctx.to_device(S0), coef), want)
    # coef = 0: every pair weighs 2^40
    assert np.array_equal(sums(b, f, S0, [0.0]), np.full((130, 1), 300 * kc.ONE, np.uint64))
    assert np.array_equal(sums(b, f, S0, [float(coef[0]), 0.0])[:, 1], np.full(130, 300 * kc.ONE, np.uint64))
    # a coefficient with coef * 1 >= 41: only pairs at S0 itself weigh, 2^40 each -- the count of the ball of radius S0
    at = count_balls_rows(b, f, S0[:, None])[0].numpy()[:130, 0]
    assert np.array_equal(at.astype(np.int64), (S == S0[:, None]).sum(axis=1)) and at.max() >= 2 and at.min() == 0
    for c in (41.0, 1e30):
        assert np.array_equal(sums(b, f, S0, [c])[:, 0], at * ONE), c
    with pytest.raises(ValueError):
        sums(b, f, S0, coef[::-1])                         # the coefficients must be descending
    with pytest.raises(ValueError):
        sums(b, f, S0[:100], coef)


def test_large_tile(gl):
    """enough tiles for the 256 x 256 kernel (9 x 130, both extents ragged), the shape of test_gpu_count_rows.py::test_large_tile"""
    from ganleaks_amd.attack import Bank
    ctx = gl.Context.get()
    bank, q = kc.planted_case(gl.synth, 4120, 33068, 2125, (3, 8, 8))
    bank[777] = bank[12]
    bank[33067] = bank[12]
    q[5] = bank[12]
    q[2124] = bank[33067]
    S = kc.host_S(q, bank)
    S0 = kc.mixed_S0(S)
    coef = kc.pick_coef(S, S0, 2)
    got = sums(Bank.from_images(bank, ctx), Bank.from_images(q, ctx), S0, coef)
    want = kc.want_sums(S, S0, coef)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert (S[5] == 0).sum() == 3 and S0[5] == -1000


def _big_case(gl, seed, shape, n, nq):
    """planted rows plus the extremes: a zero query against a row of 255 (S = s_max > 2^32, delta >= 2^32 from S0 = 0), against a zero row
    (S = 0) and against a nearly-zero row (its second nearest)"""
    rng = np.random.default_rng(seed)
    bank, q = kc.planted_case(gl.synth, seed, n, nq, shape)
    bank[3] = 0
    bank[4] = rng.integers(0, 4, size=shape, dtype=np.uint8)
    bank[5] = 255
    q[0] = 0
    q[1] = bank[9]
    bank[20] = bank[9]
    return bank, q, kc.host_S(q, bank)


def test_big_and_wide(gl):
    """64-bit totals (d > 66051) and int64 norms (d > 262143)"""
    from ganleaks_amd.attack import Bank
    ctx = gl.Context.get()
    for shape, n, nq in (((3, 150, 150), 300, 5), ((3, 300, 300), 200, 3)):
        d = int(np.prod(shape))
        s_max = 65025 * d
        bank, q, S = _big_case(gl, 4130 + shape[1], shape, n, nq)
        assert s_max > 2 ** 32 and S[0, 5] == s_max and S[0, 3] == 0 and S[1, 9] == 0
        b, f = Bank.from_images(bank, ctx, norms64="auto"), Bank.from_images(q, ctx, norms64="auto")
        assert b.wide == (shape[1] == 300)
        S0 = S.min(axis=1)
        assert S0[0] == 0 and (S - S0[:, None]).max() >= 2 ** 32
        for T in (1, 16):
            coef = kc.pick_coef(S, S0, T)
            got, want = sums(b, f, S0, coef), kc.want_sums(S, S0, coef)
            assert np.array_equal(got, want), (shape, T, np.argwhere(got != want)[:5])
        # a coefficient so small that the pair at delta = s_max >= 2^32 still weighs: a 32-bit delta would weigh it like a near pair
        tiny = np.float32([20.0 / s_max])
        want = kc.want_sums(S, S0, tiny)
        w_far = kc.kde_weight(np.int64(s_max), tiny[0])
        assert 0 < w_far < kc.kde_weight(np.int64(s_max - 2 ** 32), tiny[0])
        assert np.array_equal(sums(b, f, S0, tiny), want), shape
    # the wide form at a small d and at 3 x 150 x 150 gives what the int32-norm form gives, and what the oracle gives
    for shape, n, nq in (((768,), 300, 20), ((67500,), 40, 4)):
        bank, q = kc.planted_case(gl.synth, 4140 + shape[0], n, nq, shape)
        S = kc.host_S(q, bank)
        S0 = kc.mixed_S0(S)
        coef = kc.pick_coef(S, S0, 16)
        want = kc.want_sums(S, S0, coef)
        for wide in (False, True):
            b, f = Bank.from_images(bank, ctx, norms64=wide), Bank.from_images(q, ctx, norms64=wide)
            assert b.wide == wide
            assert np.array_equal(sums(b, f, S0, coef), want), (shape, wide)
        with pytest.raises(ValueError):
            sums(Bank.from_images(bank, ctx, norms64=True), Bank.from_images(q, ctx, norms64=False), S0, coef)


class _RowsGenerator:
    """stands in for a generator: `z` are bank row numbers"""

    def __init__(self, ctx, bank):
        self.ctx, self.bank, self.calls = ctx, bank, 0

    def generate_u8(self, z):
        self.calls += 1
        return self.ctx.to_device(self.bank[np.asarray(z)])


def test_order_independence(gl, small):
    from ganleaks_amd.attack import Bank, GeneratedBank
    ctx = gl.Context.get()
    bank, q, S = small
    f = Bank.from_images(q, ctx)
    S0 = S.min(axis=1)
    coef = kc.pick_coef(S, S0, 16)
    want = kc.want_sums(S, S0, coef)
    # the bank in two chunk calls accumulating into one table
    from ganleaks_amd.attack import kde_sums
    acc = kde_sums(Bank.from_images(bank[:170], ctx), f, S0, coef)[0]
    kde_sums(Bank.from_images(bank[170:], ctx), f, S0, coef, sums=acc)
    assert np.array_equal(acc.numpy()[:130], want)
    # n_rows: the first rows of a prepared bank only
    part = sums(Bank.from_images(bank, ctx), f, S0, coef, n_rows=170)
    assert np.array_equal(part, kc.want_sums(S[:, :170], S0, coef))
    # the bank rows permuted
    perm = np.random.default_rng(4150).permutation(300)
    assert np.array_equal(sums(Bank.from_images(bank[perm], ctx), f, S0, coef), want)
    # kde_scores over the forms of a bank: 300 rows, batch 64 -> 256 take part
    S256, unit = S[:, :256], 65025.0 * 192 / 4.0
    h = (np.log2(np.e) / (kc.pick_coef(S256, S256.min(axis=1), 3).astype(np.float64) * unit)).tolist()     # ascending bandwidths
    c32 = np.float32(np.log2(np.e) / (np.asarray(h) * unit))
    kc.check_not_vacuous(S256 - S256.min(axis=1)[:, None], np.sort(c32)[::-1])
    want_W = kc.want_sums(S256, S256.min(axis=1), c32)
    ref = gl.kde_scores(q, bank, h, batch_size=64)
    assert ref[1].dtype == np.uint64 and ref[2].dtype == np.int64 and ref[0].dtype == np.float64
    assert np.array_equal(ref[1], want_W) and np.array_equal(ref[2], S256.min(axis=1))
    gen = _RowsGenerator(ctx, bank)
    others = {
        "prepared": gl.kde_scores(f, Bank.from_images(bank[:256], ctx), h, batch_size=64),
        # streamed: 2 * 192 bytes per row -> 77 rows per chunk, 4 chunks, boundaries not multiples of the tile
        "streamed": gl.kde_scores(q, bank, h, batch_size=64, chunk_bytes=2 * 192 * 77),
        "device array": gl.kde_scores(ctx.to_device(q), ctx.to_device(bank), h, batch_size=64, chunk_bytes=2 * 192 * 77),
        "generated": gl.kde_scores(q, GeneratedBank(gen, np.arange(300)), h, batch_size=64, chunk_bytes=2 * 192 * 101),
        "order of h": tuple(x[:, ::-1] if x.ndim == 2 else x for x in gl.kde_scores(q, bank, h[::-1], batch_size=64)),
    }
    assert gen.calls == 6, "three chunks, generated twice"
    for name, other in others.items():
        for a, r in zip(other, ref):
            assert np.array_equal(a, r), name


def test_integer_table(gl):
    rng = np.random.default_rng(4160)
    F = 300
    bank = (rng.random((500, F)) < 0.3).astype(np.float32)             # 0 / 1 rows, as medGAN's thresholded samples
    for g in range(0, 480, 8):                                          # clusters inside the bank: row g + 1 is row g with a few entries flipped
        bank[g + 1] = np.abs(bank[g] - (rng.random(F) < 0.03))
    # every query is a cluster's first row with a few entries flipped: a nearest, a second nearest, and the rest of the bank far away
    q = np.abs(bank[8 * rng.integers(0, 60, size=21)] - (rng.random((21, F)) < 0.02)).astype(np.float32)
    q[0] = bank[17]
    bank[400] = bank[17]
    S = kc.host_S(q, bank)
    S0 = S.min(axis=1)
    assert (S[0] == 0).sum() == 2
    h = (np.log2(np.e) / (kc.pick_coef(S, S0, 3).astype(np.float64) * F)).tolist()        # distance = S / F
    c32 = np.float32(np.log2(np.e) / (np.asarray(h) * float(F)))
    loss, W, got_S0 = gl.kde_scores(q, bank, h, batch_size=100)
    assert np.array_equal(got_S0, S0) and np.array_equal(W, kc.want_sums(S, S0, c32))
    kc.check_not_vacuous(S - S0[:, None], np.sort(c32)[::-1])
    assert W.min(axis=1)[0] >= 2 * kc.ONE
    with pytest.raises(NotImplementedError, match="off both lattices"):
        gl.kde_scores(q / 3.0, bank, h, batch_size=100)
    with pytest.raises(NotImplementedError):
        gl.kde_scores(q, np.full((500, F), 7, np.uint8), h, batch_size=100)      # integer-table queries, 8-bit codes in the bank


def test_a_pair_below_its_offset_is_an_error(gl, small):
    from ganleaks_amd.attack import Bank
    ctx = gl.Context.get()
    bank, q, S = small
    b, f = Bank.from_images(bank, ctx), Bank.from_images(q, ctx)
    S0 = S.min(axis=1)
    coef = kc.pick_coef(S, S0, 5)
    bad = S0.copy()
    bad[77] += 1                                           # one above the true minimum of one query
    with pytest.raises(gl.GanLeaksError, match="below the offset"):
        sums(b, f, bad, coef)
    # the flag is cleared: the next valid call on the same context is correct
    assert np.array_equal(sums(b, f, S0, coef), kc.want_sums(S, S0, coef))


@pytest.fixture(scope="module")
def ties_case(gl):
    """37 queries x 1000 rows of 3 x 8 x 8, batch 64: 960 rows take part; every row is there three times, some queries equal a bank row"""
    synth = gl.synth
    base = synth.lowpass_u8_images(711, 320, 8)
    bank = base[np.arange(1000) % 320]
    q = np.concatenate([synth.perturb_u8(712, base[:20], 6.0), base[[5, 100, 319]], synth.lowpass_u8_images(713, 14, 8)])
    return bank, q, kc.host_S(q, bank[:960])


def test_kde_scores_against_float64_log_sum_exp(gl, ties_case):
    bank, q, S = ties_case
    n_eff, unit = 960, 65025.0 * 192 / 4.0
    D = S.astype(np.float64) / unit
    top1 = D.min(axis=1)
    h = [float(np.median(top1[top1 > 0])), 0.3 * float(np.median(top1[top1 > 0])), 5.0, 1e-7]
    c32 = np.float32(np.log2(np.e) / (np.asarray(h, np.float64) * unit))
    h_eff = np.log2(np.e) / (c32.astype(np.float64) * unit)            # the bandwidths the rounded coefficients stand for
    S0 = S.min(axis=1)
    kc.check_not_vacuous(S - S0[:, None], np.sort(c32[:3])[::-1])
    loss, W, got_S0 = gl.kde_scores(q, bank, h, batch_size=64)
    assert loss.shape == W.shape == (37, 4) and got_S0.shape == (37,)
    assert np.array_equal(got_S0, S0) and np.array_equal(got_S0, gl.kth_distances(q, bank, 1, batch_size=64)[1][:, 0])
    assert np.array_equal(W, kc.want_sums(S, S0, c32))
    D0 = S0.astype(np.float64) / unit
    for t in range(3):
        # -h ln(1/n sum exp(-D / h)) with the minimum taken out, in float64
        ref = D0 + h_eff[t] * (np.log(float(n_eff)) - np.log(np.exp(-(D - D0[:, None]) / h_eff[t]).sum(axis=1)))
        err = np.abs(loss[:, t] - ref)
        bound = h_eff[t] * (kc.E_W + n_eff * 2.0 ** -40) + 4 * np.spacing(np.abs(ref))
        print("h = %.3e: largest |loss - ref| = %.3e, bound %.3e" % (h[t], err.max(), bound.min()))
        assert np.all(err <= bound), (t, err.max(), bound.min())
    # a bandwidth so small that only the ties at the minimum contribute: W = m 2^40
    m = (S == S0[:, None]).sum(axis=1)
    assert m.min() == 3 and np.array_equal(W[:, 3], m.astype(np.uint64) * ONE)
    assert np.array_equal(loss[:, 3], D0 + h_eff[3] * np.log(float(n_eff) / (m * 1.0)))
    # soft-min: between the nearest distance and the mean distance, growing with h
    assert np.all(loss[:, 3] >= D0) and np.all(loss[:, 1] <= loss[:, 0] + 1e-12) and np.all(loss[:, 0] <= loss[:, 2] + 1e-12)
    assert np.all(loss[:, 2] <= D.mean(axis=1))


def test_two_contexts_on_one_device(gl, ties_case):
    """the --devices 0,0 route: RCCL refuses two ranks on one device, keys and sums are merged on the host"""
    from ganleaks_amd.shard import DeviceGroup, kde_scores_on_devices
    bank, q, S = ties_case
    unit = 65025.0 * 192 / 4.0
    coef = kc.pick_coef(S, S.min(axis=1), 3)               # (asserts that the weights do not pass vacuously)
    h = (np.log2(np.e) / (coef.astype(np.float64) * unit)).tolist()
    c32 = np.float32(np.log2(np.e) / (np.asarray(h) * unit))
    kc.check_not_vacuous(S - S.min(axis=1)[:, None], np.sort(c32)[::-1])
    single = gl.kde_scores(q, bank, h, batch_size=64)
    assert np.array_equal(single[2], S.min(axis=1)) and np.array_equal(single[1], kc.want_sums(S, single[2], c32))
    with DeviceGroup([0, 0]) as group:
        for weights in ([1.0, 2.0], None):
            got = group.kde_scores(q, bank=bank, bandwidths=h, batch_size=64, weights=weights)
            for a, r in zip(got, single):
                assert a.dtype == r.dtype and np.array_equal(a, r), weights
        with pytest.raises(ValueError):
            group.kde_scores(q, bank=bank, bandwidths=[0.1, -1.0], batch_size=64)
        with pytest.raises(NotImplementedError):
            group.kde_scores(q.astype(np.float32) / 3.0, bank=bank, bandwidths=h, batch_size=64)
        again = group.kde_scores(q, bank=bank, bandwidths=h[:1], batch_size=64, weights=[3.0, 1.0])
        assert np.array_equal(again[1][:, 0], single[1][:, 0])
    got = kde_scores_on_devices(q, bank=bank, devices=[0, 0, 0], bandwidths=h, batch_size=64)
    assert np.array_equal(got[1], single[1]) and np.array_equal(got[0], single[0])


class _Rows:
    """a bank of a given length that owns no memory"""
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def test_bad_arguments_leave_the_device_usable(gl, small):
    from ganleaks_amd.attack import kde_sums
    bank, q, S = small
    launches = []
    real = kde_sums

    def recording(*a, **k):
        launches.append(1)
        return real(*a, **k)
    scope = gl.kde_scores.__globals__                      # the module kde_scores looks kde_sums up in
    scope["kde_sums"] = recording
    try:
        for bad in ([], [0.1] * 17, [0.1, 0.0], [-0.5], [0.1, float("nan")]):
            with pytest.raises(ValueError):
                gl.kde_scores(q, bank, bad, batch_size=64)
        with pytest.raises(NotImplementedError, match="l2-lpips"):
            gl.kde_scores(q, bank, 0.1, batch_size=64, distance="l2-lpips")
        with pytest.raises(NotImplementedError, match="off both lattices"):
            gl.kde_scores(q.astype(np.float32) / 3.0, bank, 0.1, batch_size=64)
        with pytest.raises(NotImplementedError, match="off both lattices"):
            gl.kde_scores(q, bank.astype(np.float32) / 3.0, 0.1, batch_size=64)
        with pytest.raises(ValueError, match="2\\^23"):
            gl.kde_scores(q, _Rows(1 << 23), 0.1, batch_size=64)
        assert launches == []
        S256 = S[:, :256]
        h = (np.log2(np.e) / (kc.pick_coef(S256, S256.min(axis=1), 3).astype(np.float64) * 65025.0 * 192 / 4.0)).tolist()
        loss, W, S0 = gl.kde_scores(q, bank, h, batch_size=64)
        assert launches == [1]
    finally:
        scope["kde_sums"] = real
    c32 = np.float32(np.log2(np.e) / (np.asarray(h) * 65025.0 * 192 / 4.0))
    kc.check_not_vacuous(S256 - S256.min(axis=1)[:, None], np.sort(c32)[::-1])
    assert np.array_equal(S0, S[:, :256].min(axis=1)) and np.array_equal(W, kc.want_sums(S[:, :256], S0, c32))
