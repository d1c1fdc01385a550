"""GPU: epsilon-ball counts under the exact-integer L2 distance (ball_counts, gl_l2_count_i8*, gl_counts_*).
The oracle everywhere is c_oracle.ssd_row_u8 followed by the float32 comparison of the definition itself,
    counts[q, t] = #{ n < n_eff : float32(float64(S) * 4 / (65025 d)) <= float32(eps[t]) }        (S / d for integer tables),
so neither the kernels nor eps_to_ssd take part in the expected values.  Every query is checked; counts are compared with array_equal."""
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


@pytest.fixture(scope="module")
def coracle():
    import c_oracle
    return c_oracle


def oracle_dist(coracle, bank, queries, n_eff, integers=False):
    """float32 [Q, n_eff]: the distance of every pair as attack() would report it"""
    bank = np.ascontiguousarray(bank[:n_eff]).reshape(n_eff, -1)
    queries = np.ascontiguousarray(queries).reshape(len(queries), -1)
    d = bank.shape[1]
    out = np.empty((len(queries), n_eff), np.float32)
    for qi, q in enumerate(queries):
        S = coracle.ssd_row_u8(bank, q).astype(np.float64)
        out[qi] = (S / float(d) if integers else S * (4.0 / (65025.0 * d))).astype(np.float32)
    return out


def oracle_counts(dist, eps):
    e = np.atleast_1d(np.asarray(eps, np.float64)).astype(np.float32)
    return np.stack([(dist <= e[t]).sum(axis=1) for t in range(len(e))], axis=1).astype(np.int64)


def eps_sets(dist):
    """T = 1, 5 and 16: quantiles of the nearest-neighbour distances, values in between, 0, a negative one and inf; unsorted, with repeats"""
    top1 = dist.min(axis=1)
    qs = [float(np.quantile(top1, v, method="lower")) for v in (0.1, 0.5, 0.9)]
    mid = float(np.quantile(dist, 0.3))
    one = [qs[1]]
    five = [qs[2], qs[0], mid, qs[0], 0.0]
    sixteen = [np.inf, qs[1], -1.0, qs[0], mid, qs[2], 0.0, qs[1], float(dist.max()), float(dist.min()), float(np.quantile(dist, 0.01)),
               float(np.quantile(dist, 0.7)), 1e-9, qs[2] * 1.5, float(np.nextafter(np.float32(qs[1]), np.float32(0))), 1e30]
    return one, five, sixteen


def check_counts(gl, coracle, bank, queries, batch_size, integers=False, oracle_bank=None, oracle_queries=None, **kw):
    n_eff = (len(bank) // batch_size) * batch_size
    dist = oracle_dist(coracle, bank if oracle_bank is None else oracle_bank, queries if oracle_queries is None else oracle_queries, n_eff, integers)
    for eps in eps_sets(dist):
        got = gl.ball_counts(queries, bank, eps, batch_size=batch_size, **kw)
        assert got.dtype == np.int64 and got.shape == (len(queries), len(eps))
        want = oracle_counts(dist, eps)
        assert np.array_equal(got, want), (len(eps), np.argwhere(got != want)[:5])
    return dist


def _case(synth, seed, n_bank, n_q, res):
    case = synth.attack_case(seed, n_bank, n_q - n_q // 2, n_q // 2, res)
    return case["bank"], np.concatenate([case["pos"], case["neg"]])


@pytest.mark.parametrize("nq", [1, 63, 130, 300])
def test_resident_ragged(gl, coracle, synth, nq):
    bank, q = _case(synth, 151, 333, max(nq, 2), 16)      # d = 768; batch 30 truncates 333 -> 330: no multiple of a tile
    q = q[:nq]
    dist = check_counts(gl, coracle, bank, q, 30)
    # a scalar eps gives one column
    e = float(np.median(dist.min(axis=1)))
    got = gl.ball_counts(q, bank, e, batch_size=30)
    assert got.shape == (nq, 1) and np.array_equal(got, oracle_counts(dist, [e]))


def test_large_tile(gl, coracle):
    """enough tiles for the 256 x 256 kernel (the rule of gl_l2_knn_i8: at least 1024 of them): 9 x 130, both extents ragged"""
    rng = np.random.default_rng(154)
    bank = rng.integers(0, 256, size=(33068, 3, 8, 8), dtype=np.uint8)
    q = rng.integers(0, 256, size=(2125, 3, 8, 8), dtype=np.uint8)
    bank[777] = bank[12]
    bank[33067] = bank[12]
    q[5] = bank[12]
    q[2124] = bank[33067]
    dist = check_counts(gl, coracle, bank, q, 1)
    assert gl.ball_counts(q, bank, 0.0, batch_size=1)[[5, 2124], 0].tolist() == [3, 3]
    assert (dist[5] == 0).sum() == 3


def test_big_and_wide(gl, coracle):
    from ganleaks_amd.attack import Bank
    ctx = gl.Context.get()
    rng = np.random.default_rng(155)
    for shape, n, nq in (((3, 150, 150), 150, 5), ((3, 300, 300), 40, 3)):       # 64-bit totals (d > 66051); int64 norms (d > 262143)
        bank = rng.integers(0, 256, size=(n,) + shape, dtype=np.uint8)
        q = rng.integers(0, 256, size=(nq,) + shape, dtype=np.uint8)
        bank[3] = 0
        bank[5] = 255                                     # the largest S = 65025 d against a zero query
        q[0] = 0
        q[1] = bank[9]
        bank[20] = bank[9]
        check_counts(gl, coracle, bank, q, 1)
        assert Bank.from_images(bank[:2], ctx, norms64="auto").wide == (shape[1] == 300)
    # the wide form at a small d and at 3 x 150 x 150 gives what the int32-norm form gives, and what the oracle gives
    for d, n, nq in ((768, 300, 20), (67500, 40, 4)):
        bank = rng.integers(0, 256, size=(n, d), dtype=np.uint8)
        q = rng.integers(0, 256, size=(nq, d), dtype=np.uint8)
        q[0] = bank[7]
        dist = oracle_dist(coracle, bank, q, n)
        for eps in eps_sets(dist):
            want = oracle_counts(dist, eps)
            for wide in (False, True):
                b, f = Bank.from_images(bank, ctx, norms64=wide), Bank.from_images(q, ctx, norms64=wide)
                assert b.wide == wide
                assert np.array_equal(gl.ball_counts(f, b, eps, batch_size=1), want), (d, wide)
                assert np.array_equal(gl.ball_counts(q, b, eps, batch_size=1), want), (d, wide)
        with pytest.raises(ValueError):
            gl.ball_counts(Bank.from_images(q, ctx, norms64=False), Bank.from_images(bank, ctx, norms64=True), 1.0)


def test_integer_table(gl, coracle):
    rng = np.random.default_rng(161)
    F = 300
    bank = (rng.random((500, F)) < 0.3).astype(np.float32)             # 0 / 1 rows, as medGAN's thresholded samples
    q = (rng.random((21, F)) < 0.3).astype(np.float32)
    q[0] = bank[17]
    bank[400] = bank[17]
    check_counts(gl, coracle, bank, q, 100, integers=True, oracle_bank=bank.astype(np.uint8), oracle_queries=q.astype(np.uint8))
    assert gl.ball_counts(q, bank, 0.0, batch_size=100)[0, 0] == 2
    with pytest.raises(NotImplementedError) as e:
        gl.ball_counts(q / 3.0, bank, 0.5, batch_size=100)             # off both lattices
    assert "exact-integer" in str(e.value)
    with pytest.raises(NotImplementedError):
        gl.ball_counts(q, bank / 3.0, 0.5, batch_size=100)


class _RowsGenerator:
    """stands in for a generator: `z` are bank row numbers"""

    def __init__(self, ctx, bank):
        self.ctx, self.bank = ctx, bank

    def generate_u8(self, z):
        return self.ctx.to_device(self.bank[np.asarray(z)])


def test_resident_streamed_generated_device_and_torch_agree(gl, coracle, synth):
    import torch
    from ganleaks_amd.attack import Bank, GeneratedBank
    ctx = gl.Context.get()
    bank, q = _case(synth, 162, 1000, 45, 16)              # d = 768
    bs = 30
    dist = oracle_dist(coracle, bank, q, 990)
    eps = eps_sets(dist)[2]
    want = oracle_counts(dist, eps)
    res = gl.ball_counts(q, bank, eps, batch_size=bs)
    assert np.array_equal(res, want)
    # streamed: 2 * 768 bytes per row -> 301 rows per chunk, 4 chunks, boundaries not multiples of the tile
    others = {
        "streamed": gl.ball_counts(q, bank, eps, batch_size=bs, chunk_bytes=2 * 768 * 301),
        "device array": gl.ball_counts(ctx.to_device(q), ctx.to_device(bank), eps, batch_size=bs, chunk_bytes=2 * 768 * 301),
        "generated": gl.ball_counts(q, GeneratedBank(_RowsGenerator(ctx, bank), np.arange(1000)), eps, batch_size=bs, chunk_bytes=2 * 768 * 177),
        "torch": gl.ball_counts(torch.from_numpy(q), torch.from_numpy(bank), eps, batch_size=bs),
        "float images": gl.ball_counts(torch.from_numpy((2.0 * (q.astype(np.float64) / 255.0) - 1.0).astype(np.float32)), bank, eps, batch_size=bs),
    }
    for name, other in others.items():
        assert np.array_equal(other, res), name
    # a prepared Bank passed twice: fresh counters per call
    b, f = Bank.from_images(bank, ctx), Bank.from_images(q, ctx)
    first = gl.ball_counts(f, b, eps, batch_size=bs)
    second = gl.ball_counts(f, b, eps, batch_size=bs)
    assert np.array_equal(first, res) and np.array_equal(second, res)
    # a shard is not truncated again, and reduce_fn sees uint64 [Q, T] counters in the library's (sorted) column order
    seen = []

    def reduce_fn(counts):
        seen.append((counts.shape, counts.dtype))
        return counts

    part = gl.ball_counts(f, bank[100:333], eps, batch_size=bs, index_base=100, reduce_fn=reduce_fn)
    assert seen == [((45, 16), np.dtype(np.uint64))]
    assert np.array_equal(part, oracle_counts(oracle_dist(coracle, bank[100:333], q, 233), eps))
    with pytest.raises(ValueError):
        gl.ball_counts(q, bank[:20], eps, batch_size=bs)  # no full batch


def test_ties_count_in_multiples(gl, coracle, synth):
    base = synth.lowpass_u8_images(157, 12, 16)
    bank = base[np.arange(72) % 12]                       # every row 6 times
    q = np.concatenate([synth.perturb_u8(158, base[[0, 5, 11]], 5.0), synth.lowpass_u8_images(159, 4, 16)])
    dist = oracle_dist(coracle, bank, q, 72)
    for eps in eps_sets(dist):
        got = gl.ball_counts(q, bank, eps, batch_size=12)
        assert np.array_equal(got, oracle_counts(dist, eps))
        assert np.all(got % 6 == 0)
    assert np.all(gl.ball_counts(q, bank, dist.min(axis=1).max(), batch_size=12) >= 6)


def test_consequences_against_attack(gl, synth):
    bank, q = _case(synth, 163, 700, 90, 16)
    bs = 64
    d1, _ = gl.attack(q, bank, distance="l2", batch_size=bs)
    eps = [float(np.quantile(d1, v, method="lower")) for v in (0.5, 0.1, 0.9)] + [float(d1.min()), float(d1.max())]
    counts = gl.ball_counts(q, bank, eps, batch_size=bs)
    for t, e in enumerate(eps):
        assert np.array_equal(counts[:, t] >= 1, d1 <= np.float32(e)), t
    dk, _ = gl.attack(q, bank, distance="l2", batch_size=bs, k=8)
    for j in range(8):
        # eps = the j-th smallest distance of every query in turn: at least j + 1 samples lie within it
        for lo in range(0, len(q), 16):
            col = gl.ball_counts(q, bank, dk[lo:lo + 16, j], batch_size=bs)
            for i in range(col.shape[1]):
                assert col[lo + i, i] >= j + 1, (j, lo + i)


def test_golden_distances_from_the_reference(gl, synth, golden_dir):
    """tests/golden/knn_topk.npz holds the reference's own custom_knn distances (torch fp32), which lie within 1e-6 of the exact ones
    (test_golden_topk_is_self_consistent): at eps = float32(dist[q, j] + 1e-6) at least j + 1 samples lie within the ball"""
    g = np.load(os.path.join(golden_dir, "knn_topk.npz"))
    for c in range(int(g["n_cases"])):
        seed, nb, npos, nneg, res, bs = (int(v) for v in g["case%d" % c])
        case = synth.attack_case(seed, nb, npos, nneg, res)
        q = np.concatenate([case["pos"], case["neg"]])
        gd = g["dist%d" % c]
        for j in range(8):
            eps = (gd[:, j].astype(np.float64) + 1e-6).astype(np.float32)
            for lo in range(0, len(q), 16):
                col = gl.ball_counts(q, case["bank"], eps[lo:lo + 16], batch_size=bs)
                for i in range(col.shape[1]):
                    assert col[lo + i, i] >= j + 1, (c, j, lo + i)


def test_one_launch_no_workspace(gl, synth):
    from ganleaks_amd.attack import Bank, count_balls
    ctx = gl.Context.get()
    bank, q = _case(synth, 164, 700, 300, 16)
    b, f = Bank.from_images(bank, ctx), Bank.from_images(q, ctx)
    thr = gl.eps_to_ssd([0.01, 0.05], 768)
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        count_balls(b, f, thr)
        prof = ctx.prof_read()
        assert prof["l2_count"][1] == 1 and prof["l2_knn"][1] == 0 and prof["topk_select"][1] == 0, prof
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()


def test_bad_arguments_leave_the_device_usable(gl, coracle, synth):
    from ganleaks_amd.attack import Bank
    ctx = gl.Context.get()
    lib = ctx.lib
    bank, q = _case(synth, 165, 200, 10, 16)
    b, f = Bank.from_images(bank, ctx), Bank.from_images(q, ctx)
    T = 3
    counts = ctx.zeros((10, T), np.uint64)
    thr = (ctypes.c_int64 * 17)(*range(100000, 100017))
    down = (ctypes.c_int64 * 3)(5, 4, 6)

    def fails(rc, needle):
        assert rc < 0, rc
        msg = lib.gl_last_error().decode()
        assert needle in msg, msg

    args = lambda **kw: [kw.get(n, v) for n, v in (("ctx", ctx.handle), ("bank", p(b.rows_i8.ptr)), ("bn", p(b.norms.ptr)), ("n", 200),   # noqa: E731
                                                   ("q", p(f.rows_i8.ptr)), ("qn", p(f.norms.ptr)), ("nq", 10), ("d", 768),
                                                   ("thr", ctypes.cast(thr, p)), ("T", T), ("counts", p(counts.ptr)))]
    fails(lib.gl_l2_count_i8(*args(T=0)), "n_thr=0")
    fails(lib.gl_l2_count_i8(*args(T=17)), "n_thr=17")
    fails(lib.gl_l2_count_i8(*args(thr=ctypes.cast(down, p))), "ascending")
    fails(lib.gl_l2_count_i8(*args(ctx=None)), "NULL ctx")
    fails(lib.gl_l2_count_i8(*args(thr=None)), "NULL thresholds")
    fails(lib.gl_l2_count_i8(*args(counts=None)), "NULL device pointer")
    fails(lib.gl_l2_count_i8(*args(bn=None)), "NULL device pointer")
    fails(lib.gl_l2_count_i8(*args(bank=p(b.rows_i8.ptr + 8))), "16-byte aligned")
    fails(lib.gl_l2_count_i8(*args(counts=p(counts.ptr + 4))), "8-byte aligned")
    fails(lib.gl_l2_count_i8(*args(d=int(lib.gl_l2_max_d(0)) + 1)), "bad sizes")
    fails(lib.gl_l2_count_i8_wide(*args(d=int(lib.gl_l2_max_d(1)) + 1)), "bad sizes")
    fails(lib.gl_l2_count_i8(*args(n=-1)), "bad sizes")
    fails(lib.gl_counts_init(ctx.handle, p(counts.ptr), 10, 0), "n_thr=0")
    fails(lib.gl_counts_init(ctx.handle, None, 10, T), "NULL")
    fails(lib.gl_counts_add(ctx.handle, p(counts.ptr), None, 10, T, 2), "NULL")
    fails(lib.gl_counts_add(ctx.handle, p(counts.ptr), p(counts.ptr), 10, 17, 2), "n_thr=17")
    fails(lib.gl_counts_add(None, p(counts.ptr), p(counts.ptr), 10, T, 2), "bad ctx")
    # no rows / no queries / thresholds nothing meets: nothing happens, nothing is dereferenced
    neg = (ctypes.c_int64 * 3)(-3, -2, -1)
    assert lib.gl_l2_count_i8(*args(n=0, bank=None, bn=None)) == 0
    assert lib.gl_l2_count_i8(*args(nq=0, q=None, qn=None, counts=None)) == 0
    assert lib.gl_l2_count_i8(*args(thr=ctypes.cast(neg, p))) == 0
    assert np.all(counts.numpy() == 0)
    # gl_l2_count_i8 accumulates; gl_counts_init zeroes; gl_counts_add sums lists
    S = np.stack([coracle.ssd_row_u8(bank, x) for x in q])
    t3 = np.sort(np.quantile(S, [0.01, 0.2, 0.6]).astype(np.int64))
    want = np.stack([(S <= t).sum(axis=1) for t in t3], axis=1).astype(np.uint64)
    t3c = (ctypes.c_int64 * 3)(*[int(v) for v in t3])
    assert lib.gl_l2_count_i8(*args(thr=ctypes.cast(t3c, p))) == 0
    assert np.array_equal(counts.numpy(), want)
    assert lib.gl_l2_count_i8(*args(thr=ctypes.cast(t3c, p))) == 0
    assert np.array_equal(counts.numpy(), 2 * want)
    lists = ctx.to_device(np.stack([want, 3 * want, 5 * want]))
    assert lib.gl_counts_add(ctx.handle, p(counts.ptr), p(lists.ptr), 10, T, 3) == 0
    assert np.array_equal(counts.numpy(), 11 * want)
    assert lib.gl_counts_init(ctx.handle, p(counts.ptr), 10, T) == 0
    assert np.all(counts.numpy() == 0)
    # and the next call works
    d1, _ = gl.attack(f, b, distance="l2", batch_size=1)
    assert np.array_equal(gl.ball_counts(f, b, float(d1.max()), batch_size=1)[:, 0] >= 1, np.ones(10, bool))


TILE_CHILD = r'''
import json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
import ganleaks_amd as gl
from ganleaks_amd import _lib
from ganleaks_amd.attack import Bank, count_balls, knn_keys, unpack_keys
assert _lib.LIB_PATH.endswith("libganleaks_hip_tuning.so")
ctx = gl.Context.get()
rng = np.random.default_rng(167)
bank_u8 = rng.integers(0, 256, size=(2100, 3, 64, 64), dtype=np.uint8)      # ragged last tiles of either size
q_u8 = rng.integers(0, 256, size=(515, 3, 64, 64), dtype=np.uint8)
q_u8[:40] = gl.synth.perturb_u8(168, bank_u8[rng.integers(0, 2100, size=40)], 6.0)
bank, q = Bank.from_images(bank_u8, ctx), Bank.from_images(q_u8, ctx)
d1 = unpack_keys(ctx, knn_keys(bank, q)[0], 515, 12288)[0]
eps = [float(np.quantile(d1, v)) for v in (0.02, 0.05, 0.5)] + [float(d1.max()) * 1.01, 0.0, np.inf]
thr = np.sort(gl.eps_to_ssd(eps, 12288))
counts = {}
for tile in (128, 256):
    os.environ["GL_L2_TILE"] = str(tile)
    counts[tile] = count_balls(bank, q, thr)[0].numpy().copy()
top1_inside = (d1[:, None] <= np.sort(np.asarray(eps, np.float32))[None, :])
print(json.dumps({"tiles_equal": bool(np.array_equal(counts[128], counts[256])),
                  # sorted columns: eps = 0 (nothing inside), the three quantiles, beyond the largest top-1 distance, inf
                  "some_hits": bool(counts[256][:, 0].sum() == 0 and 0 < counts[256][:, 1].sum() <= counts[256][:, 3].sum() < 515 * 2100),
                  "everything_inside_inf": bool(np.all(counts[256][:, -1] == 2100)),
                  "agrees_with_top1": bool(np.array_equal(counts[256] >= 1, top1_inside))}))
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
    assert out == {"tiles_equal": True, "some_hits": True, "everything_inside_inf": True, "agrees_with_top1": True}, out
