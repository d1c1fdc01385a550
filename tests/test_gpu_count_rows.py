"""GPU: counts with thresholds per query (count_balls_rows, ball_counts_rows, gl_l2_count_rows_i8*) and the exact k-th neighbour distance
for any k (kth_distances, DeviceGroup.kth_distances).

The oracle everywhere is S = |q|^2 + |b|^2 - 2 q b^T from a float64 matmul on the host -- exact, every sum stays below 2^53 -- so neither
the kernels nor the host search take part in the expected values.  Everything is compared with array_equal."""
import ctypes
import os

import numpy as np
import pytest

import gpu_common  # noqa: F401

pytestmark = pytest.mark.gpu
p = ctypes.c_void_p


@pytest.fixture(scope="module")
def gl():
    import ganleaks_amd
    return ganleaks_amd


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


def want_counts(S, thr):
    return np.stack([(S <= thr[:, t:t + 1]).sum(axis=1) for t in range(thr.shape[1])], axis=1).astype(np.int64)


def thr_rows(S, T, s_max, seed):
    """int64 [Q, T], rows ascending, different for every query: negatives, 0, attained S values and S - 1, s_max and its neighbours, values
    far beyond, repeats"""
    rng = np.random.default_rng(seed)
    nq, n = S.shape
    rows = np.arange(nq)
    srt = np.sort(S, axis=1)
    r1, r2 = rng.integers(0, n, size=nq), rng.integers(0, n, size=nq)
    pool = np.stack([-1 - (rows % 3), np.zeros(nq, np.int64), srt[:, 0], srt[:, 0] - 1, srt[rows, r1], srt[rows, r1] - 1, srt[rows, r2], srt[rows, r2],
                     srt[:, n // 2], srt[:, -1], srt[:, -1] - 1, np.full(nq, s_max), s_max + 1 + rows, np.full(nq, s_max - 1),
                     np.full(nq, 2 ** 62), rng.integers(0, s_max + 1, size=nq)], axis=1).astype(np.int64)
    pick = np.stack([rng.permutation(16)[:T] for _ in range(nq)])
    return np.sort(np.take_along_axis(pool, pick, axis=1), axis=1)


def rows_counts(bank, queries, thr):
    from ganleaks_amd.attack import count_balls_rows
    counts, fq, _ = count_balls_rows(bank, queries, thr)
    assert counts.dtype == np.dtype(np.uint64)
    return counts.numpy()[:fq.n].astype(np.int64)


def test_tile128_ragged_both_ways(gl):
    from ganleaks_amd.attack import Bank, count_balls
    ctx = gl.Context.get()
    rng = np.random.default_rng(701)
    bank = rng.integers(0, 256, size=(300, 3, 8, 8), dtype=np.uint8)
    q = rng.integers(0, 256, size=(130, 3, 8, 8), dtype=np.uint8)
    q[7], q[129], bank[299] = bank[3], bank[299], bank[0]
    S = host_S(q, bank)
    b, f = Bank.from_images(bank, ctx), Bank.from_images(q, ctx)
    for T in (1, 5, 16):
        thr = thr_rows(S, T, 65025 * 192, 702 + T)
        got = rows_counts(b, f, thr)
        want = want_counts(S, thr)
        assert got.shape == (130, T) and np.array_equal(got, want), (T, np.argwhere(got != want)[:5])
        # every row carrying the same thresholds: what count_balls gives
        same = np.repeat(thr[11:12], 130, axis=0)
        assert np.array_equal(rows_counts(b, f, same), count_balls(b, f, thr[11])[0].numpy()[:130].astype(np.int64)), T
        assert np.array_equal(rows_counts(b, f, same), want_counts(S, same)), T
    # rows that nothing meets next to rows that everything meets
    thr = np.where((np.arange(130) % 2 == 0)[:, None], np.int64(-1), np.int64(65025 * 192)) * np.ones((130, 3), np.int64)
    assert np.array_equal(rows_counts(b, f, thr), np.where((np.arange(130) % 2 == 0)[:, None], 0, 300) * np.ones((130, 3), np.int64))
    # counters accumulate across calls (chunks of a streamed bank), a device array of thresholds is taken as it is
    from ganleaks_amd.attack import count_balls_rows
    thr = thr_rows(S, 16, 65025 * 192, 731)
    thr_dev = ctx.to_device(thr)
    counts = count_balls_rows(Bank.from_images(bank[:170], ctx), f, thr_dev)[0]
    count_balls_rows(Bank.from_images(bank[170:], ctx), f, thr_dev, counts=counts)
    assert np.array_equal(counts.numpy()[:130].astype(np.int64), want_counts(S, thr))
    with pytest.raises(ValueError):
        count_balls_rows(b, f, thr[:, ::-1])               # rows must be ascending
    with pytest.raises(ValueError):
        count_balls_rows(b, f, thr[:100])


def test_large_tile(gl):
    """the shape of test_gpu_count.py::test_large_tile: enough tiles for the 256 x 256 kernel (9 x 130, both extents ragged)"""
    from ganleaks_amd.attack import Bank
    ctx = gl.Context.get()
    rng = np.random.default_rng(154)
    bank = rng.integers(0, 256, size=(33068, 3, 8, 8), dtype=np.uint8)
    q = rng.integers(0, 256, size=(2125, 3, 8, 8), dtype=np.uint8)
    bank[777] = bank[12]
    bank[33067] = bank[12]
    q[5] = bank[12]
    q[2124] = bank[33067]
    S = host_S(q, bank)
    thr = thr_rows(S, 16, 65025 * 192, 703)
    # the nearest hundred of every query too: thresholds the k-th neighbour search ends on
    thr[:, 5] = np.partition(S, 100, axis=1)[:, 100]
    thr = np.sort(thr, axis=1)
    got = rows_counts(Bank.from_images(bank, ctx), Bank.from_images(q, ctx), thr)
    want = want_counts(S, thr)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert (S[5] == 0).sum() == 3


TILE_CHILD = r'''
import json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
import ganleaks_amd as gl
from ganleaks_amd import _lib
from ganleaks_amd.attack import Bank, count_balls_rows
assert _lib.LIB_PATH.endswith("libganleaks_hip_tuning.so")
ctx = gl.Context.get()
rng = np.random.default_rng(167)
bank_u8 = rng.integers(0, 256, size=(2100, 3, 64, 64), dtype=np.uint8)      # ragged last tiles of either size
q_u8 = rng.integers(0, 256, size=(515, 3, 64, 64), dtype=np.uint8)
q_u8[:40] = gl.synth.perturb_u8(168, bank_u8[rng.integers(0, 2100, size=40)], 6.0)
qf, bf = q_u8.reshape(515, -1).astype(np.float64), bank_u8.reshape(2100, -1).astype(np.float64)
S = ((qf * qf).sum(1)[:, None] + (bf * bf).sum(1)[None, :] - 2.0 * (qf @ bf.T)).astype(np.int64)
srt = np.sort(S, axis=1)
rows = np.arange(515)
ranks = rng.integers(0, 2100, size=(515, 6))
thr = np.sort(np.concatenate([srt[rows[:, None], ranks], srt[rows[:, None], ranks[:, :3]] - 1, srt[:, :1], srt[:, :1] - 1,
                              np.full((515, 1), 65025 * 12288), np.full((515, 1), -1 - (rows[:, None] %% 2)), srt[:, -1:] + rows[:, None] %% 2], axis=1), axis=1)
assert thr.shape == (515, 14)
want = np.stack([(S <= thr[:, t:t + 1]).sum(axis=1) for t in range(14)], axis=1)
bank, q = Bank.from_images(bank_u8, ctx), Bank.from_images(q_u8, ctx)
counts = {}
for tile in (128, 256):
    os.environ["GL_L2_TILE"] = str(tile)
    counts[tile] = count_balls_rows(bank, q, thr)[0].numpy()[:515].astype(np.int64)
print(json.dumps({"tiles_equal": bool(np.array_equal(counts[128], counts[256])), "oracle": bool(np.array_equal(counts[256], want)),
                  "some_hits": bool(0 < want[:, 1:-1].sum() < 515 * 2100 * 12)}))
'''


def test_both_tiles_give_the_same_counts():
    """3 x 64 x 64, 515 x 2100: the 256 x 256 and the 128 x 128 kernels forced in turn (GL_L2_TILE, read by the tuning build only)"""
    import json
    import subprocess
    import sys
    from ganleaks_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.exists(_lib.TUNING_LIB_PATH), "build() makes libganleaks_hip_tuning.so"
    env = dict(os.environ, GANLEAKS_LIB=_lib.TUNING_LIB_PATH)
    r = subprocess.run([sys.executable, "-c", TILE_CHILD % {"root": root}], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out == {"tiles_equal": True, "oracle": True, "some_hits": True}, out


def test_big_and_wide(gl):
    """64-bit totals (d > 66051) and int64 norms (d > 262143); S = s_max > 2^32 separates a 32-bit compare from a 64-bit one"""
    from ganleaks_amd.attack import Bank
    ctx = gl.Context.get()
    rng = np.random.default_rng(155)
    for shape, n, nq in (((3, 150, 150), 300, 5), ((3, 300, 300), 200, 3)):
        d = int(np.prod(shape))
        s_max = 65025 * d
        assert s_max > 2 ** 32
        bank = rng.integers(0, 256, size=(n,) + shape, dtype=np.uint8)
        q = rng.integers(0, 256, size=(nq,) + shape, dtype=np.uint8)
        bank[3] = 0
        bank[5] = 255                                     # the largest S = 65025 d against a zero query
        bank[150] = 255
        q[0] = 0
        q[1] = bank[9]
        bank[20] = bank[9]
        S = host_S(q, bank)
        assert S[0, 5] == s_max and S[0, 3] == 0 and S[1, 9] == 0
        b, f = Bank.from_images(bank, ctx, norms64="auto"), Bank.from_images(q, ctx, norms64="auto")
        assert b.wide == (shape[1] == 300)
        thr = thr_rows(S, 16, s_max, 704)
        thr[0, :] = np.sort(np.concatenate([thr[0, :12], [s_max - 1, s_max, s_max - 2 ** 32, s_max - 2 ** 32 - 1]]))
        got, want = rows_counts(b, f, thr), want_counts(S, thr)
        assert np.array_equal(got, want), (shape, np.argwhere(got != want)[:5])
        two = np.repeat(np.asarray([[s_max - 1, s_max]], np.int64), nq, axis=0)
        got = rows_counts(b, f, two)
        assert np.array_equal(got, want_counts(S, two)) and got[0].tolist() == [n - 2, n]
    # the wide form at a small d and at 3 x 150 x 150 gives what the int32-norm form gives, and what the oracle gives
    for d, n, nq in ((768, 300, 20), (67500, 40, 4)):
        bank = rng.integers(0, 256, size=(n, d), dtype=np.uint8)
        q = rng.integers(0, 256, size=(nq, d), dtype=np.uint8)
        q[0] = bank[7]
        S = host_S(q, bank)
        thr = thr_rows(S, 16, 65025 * d, 705)
        want = want_counts(S, thr)
        for wide in (False, True):
            b, f = Bank.from_images(bank, ctx, norms64=wide), Bank.from_images(q, ctx, norms64=wide)
            assert b.wide == wide
            assert np.array_equal(rows_counts(b, f, thr), want), (d, wide)
            assert np.array_equal(rows_counts(b, q, thr), want), (d, wide)
        with pytest.raises(ValueError):
            rows_counts(Bank.from_images(bank, ctx, norms64=True), Bank.from_images(q, ctx, norms64=False), thr)


def _eps_rows(gl, S, d, kind, T, seed):
    """radii per query, any order: exact distances of attained S, their float32 neighbours, negatives, 0, inf, repeats"""
    from ganleaks_amd.attack import _dist32
    rng = np.random.default_rng(seed)
    nq, n = S.shape
    rows = np.arange(nq)
    at = _dist32(S[rows[:, None], rng.integers(0, n, size=(nq, 5))], d, kind).astype(np.float32)
    pool = np.concatenate([at, np.nextafter(at[:, :3], np.float32(-np.inf)), np.nextafter(at[:, :2], np.float32(np.inf)), at[:, :1],
                           np.full((nq, 1), -1.0, np.float32), np.zeros((nq, 1), np.float32), np.full((nq, 1), np.inf, np.float32),
                           _dist32(S.min(axis=1, keepdims=True), d, kind).astype(np.float32), np.full((nq, 1), 1e30, np.float32)], axis=1)
    assert pool.shape == (nq, 16)
    pick = np.stack([rng.permutation(16)[:T] for _ in range(nq)])
    return np.take_along_axis(pool, pick, axis=1)


def _want_eps_counts(S, eps, d, kind):
    from ganleaks_amd.attack import _dist32
    dist = _dist32(S, d, kind).astype(np.float32)
    e = np.asarray(eps, np.float64).astype(np.float32)
    return np.stack([(dist <= e[:, t:t + 1]).sum(axis=1) for t in range(e.shape[1])], axis=1).astype(np.int64)


def test_integer_table(gl):
    rng = np.random.default_rng(161)
    F = 300
    bank = (rng.random((500, F)) < 0.3).astype(np.float32)             # 0 / 1 rows, as medGAN's thresholded samples
    q = (rng.random((21, F)) < 0.3).astype(np.float32)
    q[0] = bank[17]
    bank[400] = bank[17]
    S = host_S(q, bank)
    assert (S[0] == 0).sum() == 2
    eps = _eps_rows(gl, S, F, "int", 16, 706)
    got = gl.ball_counts_rows(q, bank, eps, batch_size=100)
    assert got.dtype == np.int64 and np.array_equal(got, _want_eps_counts(S, eps, F, "int"))
    # row q is what ball_counts gives for that query with that row of radii
    for qi in (0, 1, 20):
        assert np.array_equal(got[qi], gl.ball_counts(q[qi:qi + 1], bank, eps[qi], batch_size=100)[0]), qi
    dist, Sk, passes = gl.kth_distances(q, bank, [1, 2, 40, 500], batch_size=100)
    srt = np.sort(S, axis=1)
    assert np.array_equal(Sk, srt[:, [0, 1, 39, 499]]) and Sk[0, 1] == 0
    assert np.array_equal(dist, (Sk.astype(np.float64) / np.float64(F)).astype(np.float32))
    with pytest.raises(NotImplementedError) as e:
        gl.ball_counts_rows(q / 3.0, bank, eps, batch_size=100)        # off both lattices
    assert "exact-integer" in str(e.value) and "float paths" in str(e.value)
    with pytest.raises(NotImplementedError):
        gl.kth_distances(q, bank / 3.0, 3, batch_size=100)
    with pytest.raises(NotImplementedError):
        gl.ball_counts_rows(q, np.full((500, F), 7, np.uint8), eps, batch_size=100)      # integer-table queries, 8-bit codes in the bank


class _RowsGenerator:
    """stands in for a generator: `z` are bank row numbers"""

    def __init__(self, ctx, bank):
        self.ctx, self.bank = ctx, bank

    def generate_u8(self, z):
        return self.ctx.to_device(self.bank[np.asarray(z)])


def test_bank_forms_agree(gl, synth):
    from ganleaks_amd.attack import Bank, GeneratedBank, new_counts
    ctx = gl.Context.get()
    case = synth.attack_case(162, 1000, 23, 22, 16)       # d = 768
    bank, q = case["bank"], np.concatenate([case["pos"], case["neg"]])
    bs = 30
    S = host_S(q, bank[:990])
    eps = _eps_rows(gl, S, 768, "u8", 16, 707)
    want = _want_eps_counts(S, eps, 768, "u8")
    res = gl.ball_counts_rows(q, bank, eps, batch_size=bs)
    assert res.dtype == np.int64 and res.shape == (45, 16) and np.array_equal(res, want)
    for qi in (0, 44):
        assert np.array_equal(res[qi], gl.ball_counts(q[qi:qi + 1], bank, eps[qi], batch_size=bs)[0]), qi
    f = Bank.from_images(q, ctx)
    seen = []

    def reduce_fn(counts):
        seen.append((counts.shape, counts.dtype))
        other = new_counts(ctx, 45, 16)
        gl.count_balls_rows(Bank.from_images(bank[:100], ctx), f, thr_sorted, counts=other)
        gl.count_balls_rows(Bank.from_images(bank[333:990], ctx), f, thr_sorted, counts=other)
        from ganleaks_amd._lib import check
        check(ctx.lib.gl_counts_add(ctx.handle, p(counts.ptr), p(other.ptr), 45, 16, 1))      # the sum over the "other shards"
        return counts

    thr_sorted = np.sort(gl.eps_to_ssd_rows(eps, 768, "u8"), axis=1)
    others = {
        "prepared": gl.ball_counts_rows(f, Bank.from_images(bank[:990], ctx), eps, batch_size=bs),
        # streamed: 2 * 768 bytes per row -> 301 rows per chunk, 4 chunks, boundaries not multiples of the tile
        "streamed": gl.ball_counts_rows(q, bank, eps, batch_size=bs, chunk_bytes=2 * 768 * 301),
        "device array": gl.ball_counts_rows(ctx.to_device(q), ctx.to_device(bank), eps, batch_size=bs, chunk_bytes=2 * 768 * 301),
        "generated": gl.ball_counts_rows(q, GeneratedBank(_RowsGenerator(ctx, bank), np.arange(1000)), eps, batch_size=bs, chunk_bytes=2 * 768 * 177),
        # a world of one that owns rows [100, 333): not truncated again; the summing reduce_fn adds the rest of the bank
        "shard": gl.ball_counts_rows(f, bank[100:333], eps, batch_size=bs, index_base=100, reduce_fn=reduce_fn),
    }
    assert seen == [((45, 16), np.dtype(np.uint64))]
    for name, other in others.items():
        assert np.array_equal(other, res), name
    # the k-th distance over the same forms
    k = [31, 1, 990]
    ref = gl.kth_distances(q, bank, k, batch_size=bs)
    assert np.array_equal(ref[1], np.sort(S, axis=1)[:, [30, 0, 989]])
    for name, other in {"prepared": gl.kth_distances(f, Bank.from_images(bank[:990], ctx), k, batch_size=bs),
                        "streamed": gl.kth_distances(q, bank, k, batch_size=bs, chunk_bytes=2 * 768 * 301),
                        "generated": gl.kth_distances(q, GeneratedBank(_RowsGenerator(ctx, bank), np.arange(1000)), k, batch_size=bs,
                                                      chunk_bytes=2 * 768 * 401)}.items():
        assert np.array_equal(other[0], ref[0]) and np.array_equal(other[1], ref[1]) and other[2] == ref[2], name
    with pytest.raises(ValueError):
        gl.ball_counts_rows(q, bank[:20], eps, batch_size=bs)          # no full batch
    with pytest.raises(ValueError):
        gl.ball_counts_rows(q, bank, eps[:40], batch_size=bs)          # a row of radii per query


@pytest.fixture(scope="module")
def kth_case(gl):
    """37 queries x 1000 rows of 3 x 8 x 8, batch 64: 960 rows take part.  Rows planted three times, so that the k-th and the (k+1)-th
    tie; some queries equal a bank row."""
    synth = gl.synth
    base = synth.lowpass_u8_images(711, 320, 8)
    bank = base[np.arange(1000) % 320]                     # every row three times among the 960 that take part
    q = np.concatenate([synth.perturb_u8(712, base[:20], 6.0), base[[5, 100, 319]], synth.lowpass_u8_images(713, 14, 8)])
    assert q.shape == (37, 3, 8, 8)
    S = np.sort(host_S(q, bank[:960]), axis=1)
    return bank, q, S


KS = [1, 2, 32, 33, 100, 960]


def test_kth_distances(gl, kth_case):
    from ganleaks_amd.attack import Bank, count_balls_rows, kth_pass_bound
    bank, q, srt = kth_case
    ctx = gl.Context.get()
    dist, S, passes = gl.kth_distances(q, bank, KS, batch_size=64)
    assert dist.dtype == np.float32 and S.dtype == np.int64 and dist.shape == S.shape == (37, 6)
    assert np.array_equal(S, srt[:, [k - 1 for k in KS]])
    assert np.all(S[20:23, 0] == 0) and np.all(srt[:, 31] == srt[:, 32]) and np.all(srt[:, 99] == srt[:, 100]), "the k-th and the (k+1)-th tie"
    assert np.array_equal(S[20:23, 1], np.zeros(3, np.int64)), "a planted row is there more than once"
    bound = kth_pass_bound(65025 * 192)
    assert bound == 6 and 1 <= passes <= len(KS) * bound
    assert np.array_equal(dist, (S.astype(np.float64) * (4.0 / (65025.0 * 192))).astype(np.float32))
    d32, _ = gl.attack(q, bank, distance="l2", batch_size=64, k=32)
    for i, k in enumerate(KS):
        if k <= 32:
            assert np.array_equal(dist[:, i], d32[:, k - 1]), k
    # at the distance itself at least k samples lie inside; at the next smaller S fewer than k do
    inside = gl.ball_counts_rows(q, bank, dist, batch_size=64)
    assert np.all(inside >= np.asarray(KS)[None, :])
    order = np.argsort(S, axis=1, kind="stable")
    below = count_balls_rows(Bank.from_images(bank[:960], ctx), q, np.take_along_axis(S - 1, order, axis=1))[0].numpy()[:37].astype(np.int64)
    assert np.all(below < np.take_along_axis(np.asarray(KS)[None, :].repeat(37, axis=0), order, axis=1))
    # one k, repeats and any order
    one = gl.kth_distances(q, bank, 100, batch_size=64)
    assert one[0].shape == (37, 1) and np.array_equal(one[1][:, 0], srt[:, 99]) and one[2] <= bound
    rep = gl.kth_distances(q, bank, [960, 1, 960], batch_size=64)
    assert np.array_equal(rep[1], srt[:, [959, 0, 959]]) and rep[2] <= 2 * bound
    with pytest.raises(ValueError) as e:
        gl.kth_distances(q, bank, 961, batch_size=64)
    assert "961" in str(e.value)


def test_two_contexts_on_one_device(gl, kth_case):
    """the --devices 0,0 route: RCCL refuses two ranks on one device, the counts of every pass are summed on the host"""
    from ganleaks_amd.shard import DeviceGroup, kth_distances_on_devices
    bank, q, srt = kth_case
    single = gl.kth_distances(q, bank, KS, batch_size=64)
    with DeviceGroup([0, 0]) as group:
        got = group.kth_distances(q, bank=bank, k=KS, batch_size=64)
        assert np.array_equal(got[0], single[0]) and np.array_equal(got[1], single[1]) and got[2] == single[2]
        with pytest.raises(ValueError):
            group.kth_distances(q, bank=bank, k=961, batch_size=64)    # checked against the global n_eff, before any rank starts
        with pytest.raises(NotImplementedError):
            group.kth_distances(q.astype(np.float32) / 3.0, bank=bank, k=3, batch_size=64)
        again = group.kth_distances(q, bank=bank, k=[33], batch_size=64, weights=[1.0, 2.0])
        assert np.array_equal(again[1][:, 0], srt[:, 32])
    got = kth_distances_on_devices(q, bank=bank, devices=[0, 0, 0], k=[100, 1], batch_size=64)
    assert np.array_equal(got[1], srt[:, [99, 0]])


def test_one_launch_per_pass_no_workspace(gl, kth_case):
    from ganleaks_amd.attack import Bank
    bank, q, srt = kth_case
    ctx = gl.Context.get()
    b, f = Bank.from_images(bank[:960], ctx), Bank.from_images(q, ctx)
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        _, S, passes = gl.kth_distances(f, b, 316, batch_size=64)
        prof = ctx.prof_read()
        assert prof["l2_count"][1] == passes and prof["l2_knn"][1] == 0 and prof["topk_select"][1] == 0 and prof["l2_hist"][1] == 0, prof
        assert np.array_equal(S[:, 0], srt[:, 315])
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()


def test_bad_arguments_leave_the_device_usable(gl, synth):
    from ganleaks_amd.attack import Bank
    ctx = gl.Context.get()
    lib = ctx.lib
    case = synth.attack_case(165, 200, 5, 5, 16)
    bank, q = case["bank"], np.concatenate([case["pos"], case["neg"]])
    b, f = Bank.from_images(bank, ctx), Bank.from_images(q, ctx)
    T = 3
    counts = ctx.zeros((10, T), np.uint64)
    S = host_S(q, bank)
    thr_host = np.sort(np.stack([S[:, 3], S[:, 50] - 1, S.min(axis=1)], axis=1), axis=1)
    thr = ctx.to_device(np.concatenate([thr_host, thr_host]))          # (room for the misaligned call)

    def fails(rc, needle):
        assert rc < 0, rc
        msg = lib.gl_last_error().decode()
        assert needle in msg, msg

    args = lambda **kw: [kw.get(n, v) for n, v in (("ctx", ctx.handle), ("bank", p(b.rows_i8.ptr)), ("bn", p(b.norms.ptr)), ("n", 200),   # noqa: E731
                                                   ("q", p(f.rows_i8.ptr)), ("qn", p(f.norms.ptr)), ("nq", 10), ("d", 768),
                                                   ("thr", p(thr.ptr)), ("T", T), ("counts", p(counts.ptr)))]
    fails(lib.gl_l2_count_rows_i8(*args(T=0)), "n_thr=0")
    fails(lib.gl_l2_count_rows_i8(*args(T=17)), "n_thr=17")
    fails(lib.gl_l2_count_rows_i8(*args(ctx=None)), "NULL ctx")
    fails(lib.gl_l2_count_rows_i8(*args(thr=None)), "NULL thresholds")
    fails(lib.gl_l2_count_rows_i8(*args(thr=p(thr.ptr + 4))), "8-byte aligned")
    fails(lib.gl_l2_count_rows_i8(*args(counts=None)), "NULL device pointer")
    fails(lib.gl_l2_count_rows_i8(*args(bn=None)), "NULL device pointer")
    fails(lib.gl_l2_count_rows_i8(*args(bank=p(b.rows_i8.ptr + 8))), "16-byte aligned")
    fails(lib.gl_l2_count_rows_i8(*args(counts=p(counts.ptr + 4))), "8-byte aligned")
    fails(lib.gl_l2_count_rows_i8(*args(d=int(lib.gl_l2_max_d(0)) + 1)), "bad sizes")
    fails(lib.gl_l2_count_rows_i8_wide(*args(d=int(lib.gl_l2_max_d(1)) + 1)), "bad sizes")
    fails(lib.gl_l2_count_rows_i8(*args(n=-1)), "bad sizes")
    # no rows / no queries: nothing happens, nothing is dereferenced
    assert lib.gl_l2_count_rows_i8(*args(n=0, bank=None, bn=None)) == 0
    assert lib.gl_l2_count_rows_i8(*args(nq=0, q=None, qn=None, counts=None, thr=None)) == 0
    assert np.all(counts.numpy() == 0)
    # accumulates
    want = want_counts(S, thr_host).astype(np.uint64)
    assert lib.gl_l2_count_rows_i8(*args()) == 0
    assert np.array_equal(counts.numpy(), want)
    assert lib.gl_l2_count_rows_i8(*args()) == 0
    assert np.array_equal(counts.numpy(), 2 * want)
    # and the next call works
    assert np.array_equal(gl.kth_distances(f, b, 4, batch_size=1)[1][:, 0], np.sort(S, axis=1)[:, 3])
