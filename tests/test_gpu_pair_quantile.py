"""GPU: the histogram of all pair distances (pair_histogram, gl_l2_hist_i8*) and the exact quantiles built on it (distance_quantiles,
DeviceGroup.distance_quantiles, mc.py --eps_pair_quantile).
The oracle everywhere is c_oracle.ssd_row_u8 followed by numpy on the exact S of every pair (np.bincount for the histograms,
np.partition for the values at the ranks, the float32 conversion of the definition for eps), so neither the kernels nor select_ranks take
part in the expected values.  Every comparison is array_equal."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

import gpu_common  # noqa: F401

pytestmark = pytest.mark.gpu
p = ctypes.c_void_p


@pytest.fixture(scope="module")
def gl():
    import ganleaks_amd
    return ganleaks_amd


@pytest.fixture(scope="module")
def coracle():
    import c_oracle
    return c_oracle


def oracle_S(coracle, bank, queries, n_eff):
    """int64 [Q, n_eff]: the exact sum of squared differences of every pair"""
    bank = np.ascontiguousarray(bank[:n_eff]).reshape(n_eff, -1)
    queries = np.ascontiguousarray(queries).reshape(len(queries), -1)
    return np.stack([coracle.ssd_row_u8(bank, q) for q in queries]).astype(np.int64)


def oracle_hist(S, lo, shift, n_bins):
    x = S.reshape(-1)
    b = (x[x >= lo] - lo) >> shift
    return np.bincount(b[b < n_bins], minlength=n_bins).astype(np.int64)


def oracle_ranks(quantiles, pairs):
    return [int(Fraction(float(v)) * (pairs - 1)) for v in quantiles]


def oracle_quantiles(S, quantiles, d, integers=False):
    """(eps float32 [T], S int64 [T], pairs) by the definition: sorted(M)[floor(v * (|M| - 1))]"""
    flat = S.reshape(-1)
    ranks = oracle_ranks(quantiles, flat.size)
    part = np.partition(flat, sorted(set(ranks)))
    s = np.asarray([part[r] for r in ranks], np.int64)
    f = s.astype(np.float64)
    eps = (f / float(d) if integers else f * (4.0 / (65025.0 * d))).astype(np.float32)
    return eps, s, flat.size


def full_window(d):
    """the first level of the radix-select: [0, 2^bitlen(65025 d)) in 2048 bins"""
    bits = int(65025 * d).bit_length()
    return 0, bits - 11, 2048


def host(hist):
    return hist.numpy().reshape(-1).astype(np.int64)


def gpu_hist(bank, queries, window, n_rows=None, hist=None):
    from ganleaks_amd.attack import pair_histogram
    lo, shift, n_bins = window
    out = pair_histogram(bank, queries, lo, shift, n_bins, n_rows, hist)[0]
    assert out.dtype == np.dtype(np.uint64) and tuple(out.shape) == (n_bins, 1)
    return out


def check_quantiles(got, want):
    eps, S, pairs = got
    assert eps.dtype == np.float32 and S.dtype == np.int64 and isinstance(pairs, int)
    assert np.array_equal(S, want[1]), (S, want[1])
    assert np.array_equal(eps, want[0]) and pairs == want[2]


def _case(synth, seed, n_bank, n_q, res):
    case = synth.attack_case(seed, n_bank, n_q - n_q // 2, n_q // 2, res)
    return case["bank"], np.concatenate([case["pos"], case["neg"]])


@pytest.fixture(scope="module")
def ragged(coracle, synth):
    """333 x 3x16x16 (batch 30: n_eff 330, no multiple of a tile) against 300 queries; S of every pair, computed once"""
    bank, q = _case(synth, 191, 333, 300, 16)
    S = oracle_S(coracle, bank, q, 330)
    S.setflags(write=False)
    return bank, q, S


@pytest.mark.parametrize("nq", [1, 130, 300])
def test_ragged_windows(gl, ragged, nq):
    from ganleaks_amd.attack import Bank
    ctx = gl.Context.get()
    bank, q, S = ragged
    q, S = q[:nq], S[:nq]
    b, f = Bank.from_images(bank, ctx), Bank.from_images(q, ctx)
    med = int(np.sort(S.reshape(-1))[S.size // 2])
    full = full_window(768)
    windows = [full,
               (max(med - 1000, 0), 0, 2048),             # zoomed: one S per bin, placed on the median
               (0, 26, 1), (med, 3, 1),                   # a single bin: everything / the 8 values from the median on
               (0, 15, 1000), (med - 3, 0, 1000),         # no power of two
               (int(S.max()) + 1, 0, 2048),               # entirely above the largest S
               (65025 * 768 + 1, 0, 2048), (1 << 39, 40, 2)]
    for w in windows:
        got = gpu_hist(b, f, w, 330)
        assert np.array_equal(host(got), oracle_hist(S, *w)), w
    assert host(gpu_hist(b, f, full, 330)).sum() == nq * 330
    assert not host(gpu_hist(b, f, windows[6], 330)).any()
    # a second call into the same bins doubles them; raw queries are prepared on the fly; n_rows defaults to the whole bank
    h = gpu_hist(b, f, windows[1], 330)
    assert gpu_hist(b, q, windows[1], 330, hist=h) is h
    assert np.array_equal(host(h), 2 * oracle_hist(S, *windows[1]))
    b330 = Bank.from_images(bank[:330], ctx)
    assert np.array_equal(host(gpu_hist(b330, f, full)), oracle_hist(S, *full))


def test_quantiles_and_what_follows_from_them(gl, ragged):
    bank, q, S = ragged
    qs = [0.5, 0, 1, 0.001, 0.5, 0.3]                     # unsorted, with repeats
    want = oracle_quantiles(S, qs, 768)
    got = gl.distance_quantiles(q, bank, qs, batch_size=30)
    check_quantiles(got, want)
    eps, s, pairs = got
    assert pairs == 300 * 330 and s[1] == S.min() and s[2] == S.max()
    # a scalar quantile gives one value
    check_quantiles(gl.distance_quantiles(q, bank, 0.25, batch_size=30), oracle_quantiles(S, [0.25], 768))
    # the two inequalities of the definition, by the ball counts
    ranks = oracle_ranks(qs, pairs)
    at = gl.ball_counts(q, bank, eps, batch_size=30).sum(axis=0)
    below = gl.ball_counts(q, bank, np.nextafter(eps, np.float32(-np.inf)), batch_size=30).sum(axis=0)
    for t, r in enumerate(ranks):
        assert at[t] >= r + 1 and below[t] <= r, (t, r, at[t], below[t])
    # v = 0 is attack()'s smallest distance
    d1, _ = gl.attack(q, bank, distance="l2", batch_size=30)
    assert eps[1] == d1.min()


@pytest.fixture(scope="module")
def large(coracle):
    """test_large_tile's shape (enough tiles for the 256 x 256 kernel: 9 x 130, both extents ragged) of uniform-random codes: the pairs
    crowd into a narrow band of the 2048 first-level bins, the worst case for bin contention"""
    rng = np.random.default_rng(154)
    bank = rng.integers(0, 256, size=(33068, 3, 8, 8), dtype=np.uint8)
    q = rng.integers(0, 256, size=(2125, 3, 8, 8), dtype=np.uint8)
    bank[777] = bank[12]
    bank[33067] = bank[12]
    q[5] = bank[12]
    q[2124] = bank[33067]
    S = oracle_S(coracle, bank, q, 33068)
    S.setflags(write=False)
    return bank, q, S


def test_large_tile(gl, large):
    from ganleaks_amd.attack import Bank
    ctx = gl.Context.get()
    bank, q, S = large
    b, f = Bank.from_images(bank, ctx), Bank.from_images(q, ctx)
    full = full_window(192)
    want = oracle_hist(S, *full)
    got = host(gpu_hist(b, f, full))
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    assert got.sum() == 2125 * 33068 and got[0] == 6
    qs = [0, 0.001, 0.5, 1]
    check_quantiles(gl.distance_quantiles(f, b, qs, batch_size=1), oracle_quantiles(S, qs, 192))


def test_big_and_wide(gl, coracle):
    from ganleaks_amd.attack import Bank
    ctx = gl.Context.get()
    rng = np.random.default_rng(192)
    for shape, n, nq in (((3, 150, 150), 150, 5), ((3, 300, 300), 40, 3)):       # 64-bit totals (d > 66051); int64 norms (d > 262143)
        d = int(np.prod(shape))
        bank = rng.integers(0, 256, size=(n,) + shape, dtype=np.uint8)
        q = rng.integers(0, 256, size=(nq,) + shape, dtype=np.uint8)
        bank[5] = 255                                     # the largest S = 65025 d against a zero query
        q[0] = 0
        q[1] = bank[9]
        S = oracle_S(coracle, bank, q, n)
        assert S.max() == 65025 * d and S.min() == 0
        b, f = Bank.from_images(bank, ctx, norms64="auto"), Bank.from_images(q, ctx, norms64="auto")
        assert b.wide == (shape[1] == 300)
        full = full_window(d)
        assert (1 << (full[1] + 11)) > 65025 * d >= (1 << (full[1] + 10))
        top = (65025 * d) >> full[1]
        for w in (full, (65025 * d - 2047, 0, 2048), (65025 * d, 0, 1), (int(np.median(S)), 12, 1000), (65025 * d + 1, 0, 8)):
            got = host(gpu_hist(b, f, w))
            assert np.array_equal(got, oracle_hist(S, *w)), (d, w)
        got = host(gpu_hist(b, f, full))
        assert got[top] >= 1 and not got[top + 1:].any()  # the largest S there is lands in the top bin in use
        qs = [1, 0, 0.5, 0.999]
        check_quantiles(gl.distance_quantiles(q, bank, qs, batch_size=1), oracle_quantiles(S, qs, d))
    # the wide form at a small d gives what the int32-norm form gives, and what the oracle gives
    bank = rng.integers(0, 256, size=(300, 768), dtype=np.uint8)
    q = rng.integers(0, 256, size=(20, 768), dtype=np.uint8)
    q[0] = bank[7]
    S = oracle_S(coracle, bank, q, 300)
    med = int(np.median(S))
    for w in (full_window(768), (med - 1024, 0, 2048), (0, 40, 1)):
        want = oracle_hist(S, *w)
        for wide in (False, True):
            b, f = Bank.from_images(bank, ctx, norms64=wide), Bank.from_images(q, ctx, norms64=wide)
            assert b.wide == wide
            assert np.array_equal(host(gpu_hist(b, f, w)), want), (w, wide)
    for wide in (False, True):
        b, f = Bank.from_images(bank, ctx, norms64=wide), Bank.from_images(q, ctx, norms64=wide)
        check_quantiles(gl.distance_quantiles(f, b, [0.5, 0.01], batch_size=1), oracle_quantiles(S, [0.5, 0.01], 768))
    with pytest.raises(ValueError):
        gpu_hist(Bank.from_images(bank, ctx, norms64=True), Bank.from_images(q, ctx, norms64=False), full_window(768))


def test_integer_table(gl, coracle):
    from ganleaks_amd.attack import Bank
    ctx = gl.Context.get()
    rng = np.random.default_rng(193)
    F = 37
    bank = rng.integers(0, 256, size=(300, F)).astype(np.float32)
    q = rng.integers(0, 256, size=(21, F)).astype(np.float32)
    q[0] = bank[17]
    S = oracle_S(coracle, bank.astype(np.uint8), q.astype(np.uint8), 300)
    b, f = Bank.from_images(bank, ctx), Bank.from_images(q, ctx)
    assert b.kind == "int" and f.kind == "int"
    for w in (full_window(F), (int(np.median(S)) - 500, 0, 1000)):
        assert np.array_equal(host(gpu_hist(b, f, w)), oracle_hist(S, *w)), w
    qs = [0.01, 0.5, 0, 1]
    want = oracle_quantiles(S, qs, F, integers=True)      # eps = fl32(S / F)
    check_quantiles(gl.distance_quantiles(q, bank, qs, batch_size=100), want)
    check_quantiles(gl.distance_quantiles(f, b, qs, batch_size=100), want)
    assert want[1][2] == 0


class _RowsGenerator:
    """stands in for a generator: `z` are bank row numbers"""

    def __init__(self, ctx, bank):
        self.ctx, self.bank = ctx, bank

    def generate_u8(self, z):
        return self.ctx.to_device(self.bank[np.asarray(z)])


@pytest.fixture(scope="module")
def thousand(coracle, synth):
    bank, q = _case(synth, 194, 1000, 45, 16)             # d = 768; batch 30: 990 rows take part
    S = oracle_S(coracle, bank, q, 990)
    S.setflags(write=False)
    return bank, q, S


QS = [0.001, 0.5, 0.9, 0.5, 0]


def test_resident_streamed_and_generated_agree(gl, synth, thousand):
    from ganleaks_amd.attack import Bank, GeneratedBank
    from ganleaks_amd.gan_models.dcgan.model_torch import Generator
    ctx = gl.Context.get()
    bank, q, S = thousand
    want = oracle_quantiles(S, QS, 768)
    check_quantiles(gl.distance_quantiles(q, Bank.from_images(bank[:990], ctx), QS, batch_size=30), want)
    # streamed: 2 * 768 bytes per row -> 400 rows per chunk: 3 chunks, the last one ragged (190 rows)
    check_quantiles(gl.distance_quantiles(q, bank, QS, batch_size=30, chunk_bytes=2 * 768 * 400), want)
    check_quantiles(gl.distance_quantiles(ctx.to_device(q), ctx.to_device(bank), QS, batch_size=30, chunk_bytes=2 * 768 * 400), want)
    check_quantiles(gl.distance_quantiles(q, GeneratedBank(_RowsGenerator(ctx, bank), np.arange(1000)), QS, batch_size=30,
                                          chunk_bytes=2 * 768 * 177), want)
    # the smallest DCGAN: the bank never materialised against its materialised rows
    gen = Generator(100, 3, 16)
    gen.load_state_dict(synth.dcgan_state_dict(1234, features_g=16))
    z = synth.latent(1, 200)
    rows = gen.generate_u8(z)
    gq = synth.perturb_u8(5, gen.generate_u8(synth.latent(2, 24)).numpy(), 6.0)
    resident = gl.distance_quantiles(gq, rows, QS, batch_size=64)
    check_quantiles(gl.distance_quantiles(gq, gl.GeneratedBank(gen, z), QS, batch_size=64, chunk_bytes=50 * 2 * 768), resident)
    assert resident[2] == 24 * 192
    with pytest.raises(ValueError):
        gl.distance_quantiles(q, bank[:20], QS, batch_size=30)     # no full batch


def test_shards_give_the_single_context_result(gl, monkeypatch, thousand):
    import importlib
    from ganleaks_amd import shard
    from ganleaks_amd.attack import Bank
    attack = importlib.import_module("ganleaks_amd.attack")     # (the package's `attack` attribute is the function)
    ctx = gl.Context.get()
    bank, q, S = thousand
    want = oracle_quantiles(S, QS, 768)
    one = gl.distance_quantiles(q, bank, QS, batch_size=30)
    check_quantiles(one, want)
    # two index_base shards, [0, 400) and [400, 990): the histogram of every level is the host sum of both (merge_counts_host).  The
    # reduction sees only the bins, so the window of the pass is taken from the launch that filled them.
    real = attack.pair_histogram
    windows = []

    def recording(bank_, queries_, lo, shift, n_bins, n_rows=None, hist=None):
        windows.append((lo, shift, n_bins))
        return real(bank_, queries_, lo, shift, n_bins, n_rows, hist)

    monkeypatch.setattr(attack, "pair_histogram", recording)
    fq = Bank.from_images(q, ctx)
    parts = {0: bank[:400], 400: bank[400:990]}
    for mine, other in ((0, 400), (400, 0)):
        rest = Bank.from_images(parts[other], ctx, index_base=other)
        levels = []

        def reduce_fn(hist):
            lo, shift, n_bins = windows[-1]
            levels.append(n_bins)
            assert hist.dtype == np.dtype(np.uint64) and tuple(hist.shape) == (n_bins, 1)
            theirs = real(rest, fq, lo, shift, n_bins)[0]
            return ctx.to_device(shard.merge_counts_host([hist.numpy(), theirs.numpy()]))

        got = gl.distance_quantiles(fq, parts[mine], QS, batch_size=30, index_base=mine, reduce_fn=reduce_fn)
        check_quantiles(got, want)
        assert len(levels) >= 3 and levels[0] == 2048
    monkeypatch.setattr(attack, "pair_histogram", real)
    # a world of one: the reduction returns its input; and the collective route itself (gl_allgather_rows + gl_counts_add over
    # nq = n_bins, n_thr = 1), as far as one rank can take it.  A shard is not truncated again.
    comm = gl._lib.Comm(ctx)
    check_quantiles(gl.distance_quantiles(q, bank[:990], QS, batch_size=30, reduce_fn=lambda h: shard.allreduce_sum_counts(h, comm=comm)), want)
    check_quantiles(gl.distance_quantiles(q, bank[:990], QS, batch_size=30,
                                          reduce_fn=lambda h: shard.allreduce_sum_counts(h, comm=comm, _even_alone=True)), want)
    comm.destroy()
    # an empty multiset
    with pytest.raises(ValueError):
        gl.distance_quantiles(q, bank[:0], QS, batch_size=30, reduce_fn=lambda h: h)
    # DeviceGroup on [0, 0]: two contexts on one device, the bins summed on the host (one rendezvous per level)
    with shard.DeviceGroup([0, 0]) as group:
        assert group.collective == "host-merge"
        check_quantiles(group.distance_quantiles(q, bank=bank, quantiles=QS, batch_size=30), want)
        check_quantiles(group.distance_quantiles(q, bank=bank, quantiles=QS, batch_size=30, weights=[1.0, 3.0]), want)
        check_quantiles(group.distance_quantiles(q, bank=bank, quantiles=QS, batch_size=30, weights=[1e-9, 1.0]), want)   # an empty shard
        rows = [id(entry[1]) for entry in group._queries]
        counts = group.ball_counts(q, bank=bank, eps=one[0], batch_size=30)       # shares the prepared queries
        assert [id(entry[1]) for entry in group._queries] == rows
        with pytest.raises(ValueError):
            group.distance_quantiles(q, bank=bank, quantiles=[1.5], batch_size=30)
        with pytest.raises(ValueError):
            group.distance_quantiles(q, bank=bank, batch_size=30)
        # rows off the lattices are refused on the host, and the group stays usable
        off = (2.0 * (q.astype(np.float64) / 255.0) - 1.0).astype(np.float32) * np.float32(0.7)
        with pytest.raises(NotImplementedError) as e:
            group.distance_quantiles(off, bank=bank, quantiles=QS, batch_size=30)
        assert "exact-integer" in str(e.value) and not group._broken
        with pytest.raises(NotImplementedError):
            group.distance_quantiles(q, bank=bank.astype(np.float32), quantiles=QS, batch_size=30)     # an integer table against 8-bit codes
        check_quantiles(group.distance_quantiles(q, bank=bank, quantiles=QS, batch_size=30), want)
    assert np.array_equal(counts, gl.ball_counts(q, bank, one[0], batch_size=30))
    check_quantiles(shard.distance_quantiles_on_devices(q, lambda c: _RowsGenerator(c, bank), np.arange(1000), devices=[0, 0, 0], quantiles=QS,
                                                        batch_size=30), want)
    check_quantiles(shard.distance_quantiles_on_devices(q, devices=[0], bank=bank, quantiles=QS, batch_size=30), want)


def test_bad_arguments_leave_the_device_usable(gl, coracle, synth):
    from ganleaks_amd.attack import Bank
    ctx = gl.Context.get()
    lib = ctx.lib
    bank, q = _case(synth, 195, 200, 10, 16)
    b, f = Bank.from_images(bank, ctx), Bank.from_images(q, ctx)
    hist = ctx.zeros((2048, 1), np.uint64)

    def fails(rc, needle):
        assert rc < 0, rc
        msg = lib.gl_last_error().decode()
        assert needle in msg, msg

    args = lambda **kw: [kw.get(n, v) for n, v in (("ctx", ctx.handle), ("bank", p(b.rows_i8.ptr)), ("bn", p(b.norms.ptr)), ("n", 200),   # noqa: E731
                                                   ("q", p(f.rows_i8.ptr)), ("qn", p(f.norms.ptr)), ("nq", 10), ("d", 768),
                                                   ("lo", 0), ("shift", 15), ("bins", 2048), ("hist", p(hist.ptr)))]
    fails(lib.gl_l2_hist_i8(*args(bins=0)), "n_bins=0")
    fails(lib.gl_l2_hist_i8(*args(bins=2049)), "n_bins=2049")
    fails(lib.gl_l2_hist_i8(*args(shift=-1)), "shift=-1")
    fails(lib.gl_l2_hist_i8(*args(shift=41)), "shift=41")
    fails(lib.gl_l2_hist_i8(*args(lo=-1)), "lo=-1")
    fails(lib.gl_l2_hist_i8(*args(ctx=None)), "NULL ctx")
    fails(lib.gl_l2_hist_i8(*args(hist=None)), "NULL device pointer")
    fails(lib.gl_l2_hist_i8(*args(bn=None)), "NULL device pointer")
    fails(lib.gl_l2_hist_i8(*args(q=None)), "NULL device pointer")
    fails(lib.gl_l2_hist_i8(*args(bank=p(b.rows_i8.ptr + 8))), "16-byte aligned")
    fails(lib.gl_l2_hist_i8(*args(hist=p(hist.ptr + 4))), "8-byte aligned")
    fails(lib.gl_l2_hist_i8(*args(d=int(lib.gl_l2_max_d(0)) + 1)), "bad sizes")
    fails(lib.gl_l2_hist_i8_wide(*args(d=int(lib.gl_l2_max_d(1)) + 1)), "bad sizes")
    fails(lib.gl_l2_hist_i8_wide(*args(bins=2049)), "n_bins=2049")
    fails(lib.gl_l2_hist_i8(*args(n=-1)), "bad sizes")
    fails(lib.gl_hist_init(ctx.handle, p(hist.ptr), 0), "n_bins=0")
    fails(lib.gl_hist_init(ctx.handle, p(hist.ptr), 2049), "n_bins=2049")
    fails(lib.gl_hist_init(ctx.handle, None, 8), "NULL")
    fails(lib.gl_hist_init(None, p(hist.ptr), 8), "NULL ctx")
    # no rows / no queries: nothing happens, nothing is dereferenced
    assert lib.gl_l2_hist_i8(*args(n=0, bank=None, bn=None)) == 0
    assert lib.gl_l2_hist_i8(*args(nq=0, q=None, qn=None, hist=None)) == 0
    assert not hist.numpy().any()
    # gl_l2_hist_i8 accumulates; gl_hist_init zeroes; gl_counts_add sums shards as [n_bins][1] counters
    S = oracle_S(coracle, bank, q, 200)
    want = oracle_hist(S, 0, 15, 2048).astype(np.uint64).reshape(2048, 1)
    assert lib.gl_l2_hist_i8(*args()) == 0
    assert np.array_equal(hist.numpy(), want)
    assert lib.gl_l2_hist_i8(*args()) == 0
    assert np.array_equal(hist.numpy(), 2 * want)
    lists = ctx.to_device(np.stack([want, 3 * want, 5 * want]))
    assert lib.gl_counts_add(ctx.handle, p(hist.ptr), p(lists.ptr), 2048, 1, 3) == 0
    assert np.array_equal(hist.numpy(), 11 * want)
    assert lib.gl_hist_init(ctx.handle, p(hist.ptr), 2048) == 0
    assert not hist.numpy().any()
    # one launch, no workspace, its own profiling id
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        gpu_hist(b, f, (0, 15, 2048))
        prof = ctx.prof_read()
        assert prof["l2_hist"][1] == 1 and prof["l2_count"][1] == 0 and prof["l2_knn"][1] == 0, prof
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()
    # and the next call works
    check_quantiles(gl.distance_quantiles(f, b, [0.5], batch_size=1), oracle_quantiles(S, [0.5], 768))


def test_python_refusals(gl, synth):
    from ganleaks_amd.attack import Bank, pair_histogram
    ctx = gl.Context.get()
    bank, q = _case(synth, 196, 100, 6, 16)
    off = (2.0 * (q.astype(np.float64) / 255.0) - 1.0).astype(np.float32) * np.float32(0.7)      # off both lattices
    for queries, samples in ((off, bank), (q, (2.0 * (bank.astype(np.float64) / 255.0) - 1.0).astype(np.float32) * np.float32(0.7)),
                             (Bank.from_images(off, ctx), bank), (q, Bank.from_images(off, ctx))):
        with pytest.raises(NotImplementedError) as e:
            gl.distance_quantiles(queries, samples, 0.5, batch_size=1)
        assert "exact-integer" in str(e.value) and "lattice" in str(e.value)
    with pytest.raises(NotImplementedError):
        pair_histogram(Bank.from_images(off, ctx), Bank.from_images(q, ctx), 0, 15, 2048)
    with pytest.raises(NotImplementedError):           # an integer table against 8-bit codes
        gl.distance_quantiles((q.reshape(6, -1) // 2).astype(np.float32), bank.reshape(100, -1), 0.5, batch_size=1)

    class Feat:
        kind = "feat"

    for queries, samples in ((Feat(), bank), (q, Feat())):
        with pytest.raises(NotImplementedError) as e:
            gl.distance_quantiles(queries, samples, 0.5)
        assert "feature rows" in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        gl.distance_quantiles(q, bank, 0.5, distance="l2-lpips")
    assert "l2-lpips" in str(e.value)


def test_mc_pair_quantile_end_to_end(gl, coracle, tmp_path, monkeypatch):
    """integer tables through the file route (.npy): --eps_pair_quantile against the oracle, alone and sharded; and a run without the
    option writes what the driver wrote before the option existed (expected arrays and params.txt stated here, from the oracle)"""
    from ganleaks_amd.attack_models import mc
    rng = np.random.default_rng(197)
    F, bs = 37, 64
    tables = {"syn": rng.integers(0, 256, size=(150, F)), "pos": rng.integers(0, 256, size=(13, F)), "neg": rng.integers(0, 256, size=(11, F))}
    tables["pos"][3] = tables["syn"][40]
    for name, t in tables.items():
        np.save(tmp_path / (name + ".npy"), t.astype(np.float32))
    monkeypatch.chdir(tmp_path)
    base = ["--syn_data_path", str(tmp_path / "syn.npy"), "--pos_data_dir", str(tmp_path / "pos.npy"), "--neg_data_dir", str(tmp_path / "neg.npy"),
            "--BATCH_SIZE", str(bs)]
    mc.main(mc.parse_arguments(base + ["--exp_name", "pair", "--eps_pair_quantile", "0.01"]))
    mc.main(mc.parse_arguments(base + ["--exp_name", "pair2", "--eps_pair_quantile", "0.01", "--devices", "0,0"]))
    mc.main(mc.parse_arguments(base + ["--exp_name", "pair3", "--eps_pair_quantile", "0.5,0.001,0.01"]))
    mc.main(mc.parse_arguments(base + ["--exp_name", "plain"]))
    n_eff = 128
    queries = np.concatenate([tables["pos"], tables["neg"]]).astype(np.uint8)
    S = oracle_S(coracle, tables["syn"].astype(np.uint8), queries, n_eff)
    dist = (S.astype(np.float64) / float(F)).astype(np.float32)
    files = ("eps.npy", "pos_count.npy", "neg_count.npy", "pos_mc.npy", "neg_mc.npy", "pos_loss.npy", "neg_loss.npy")

    def expected(eps):
        counts = np.stack([(dist <= e).sum(axis=1) for e in eps], axis=1).astype(np.int64)
        score = counts.astype(np.float64) / float(n_eff)
        return {"eps.npy": eps, "pos_count.npy": counts[:13], "neg_count.npy": counts[13:], "pos_mc.npy": score[:13], "neg_mc.npy": score[13:],
                "pos_loss.npy": -score[:13, :1], "neg_loss.npy": -score[13:, :1]}

    def check_dir(name, eps):
        out = tmp_path / "mc_attack" / name
        assert sorted(os.listdir(out)) == sorted(files + ("params.txt",))
        for fname, want in expected(eps).items():
            got = np.load(out / fname)
            assert got.dtype == want.dtype and np.array_equal(got, want), (name, fname)
        return out

    one = check_dir("pair", oracle_quantiles(S, [0.01], F, integers=True)[0])
    check_dir("pair3", oracle_quantiles(S, [0.5, 0.001, 0.01], F, integers=True)[0])
    two = tmp_path / "mc_attack" / "pair2"
    for fname in files:
        assert open(one / fname, "rb").read() == open(two / fname, "rb").read(), fname
    eps = np.load(one / "eps.npy")
    counts = np.concatenate([np.load(one / "pos_count.npy"), np.load(one / "neg_count.npy")])
    assert np.array_equal(counts, gl.ball_counts(queries.astype(np.float32), tables["syn"].astype(np.float32), eps, batch_size=bs))
    assert "eps_pair_quantile:0.01" in open(one / "params.txt").read().splitlines()
    # without the option: the median heuristic of the nearest-sample distances, and the params.txt of before
    top1 = dist.min(axis=1)
    plain = check_dir("plain", np.asarray([np.quantile(top1, 0.5, method="lower")], np.float32))
    for fname, want in expected(np.load(plain / "eps.npy")).items():
        import io
        buf = io.BytesIO()
        np.save(buf, want, allow_pickle=False)
        assert open(plain / fname, "rb").read() == buf.getvalue(), fname
    want_params = ["exp_name:plain", "syn_data_path:%s" % (tmp_path / "syn.npy"), "pos_data_dir:%s" % (tmp_path / "pos.npy"),
                   "neg_data_dir:%s" % (tmp_path / "neg.npy"), "resolution:64", "BATCH_SIZE:64", "local_config:None", "ngpu:1", "devices:None",
                   "eps:None", "distance:l2", "eps_quantile:None"]
    assert open(plain / "params.txt").read() == "".join(line + "\n" for line in want_params)
    # off-lattice rows surface the refusal's text
    np.save(tmp_path / "off.npy", tables["pos"].astype(np.float32) / 3.0)
    with pytest.raises(NotImplementedError) as e:
        mc.main(mc.parse_arguments(base[:2] + ["--pos_data_dir", str(tmp_path / "off.npy"), "--neg_data_dir", str(tmp_path / "neg.npy"),
                                              "--BATCH_SIZE", str(bs), "--exp_name", "off", "--eps_pair_quantile", "0.01"]))
    assert "exact-integer" in str(e.value)
