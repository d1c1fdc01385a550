"""GPU: the K nearest bank samples of every query under the exact-integer L2 distance (attack(k=), gl_l2_topk_i8*, gl_topk_*).
The oracle everywhere is c_oracle.ssd_row_u8 + a stable argsort: exact, and independent of the code under test."""
import ctypes
import os

import numpy as np
import pytest

import gpu_common  # noqa: F401

pytestmark = pytest.mark.gpu
p = ctypes.c_void_p
KS = (1, 2, 5, 16, 32)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def gl():
    import ganleaks_amd
    return ganleaks_amd


@pytest.fixture(scope="module")
def coracle():
    import c_oracle
    return c_oracle


def oracle_topk(coracle, bank, queries, n_eff, k, integers=False):
    """(dist float32 [Q, k], idx int64 [Q, k]): the first k of the order (S, n) over rows [0, n_eff)"""
    bank = np.ascontiguousarray(bank[:n_eff]).reshape(n_eff, -1)
    queries = np.ascontiguousarray(queries).reshape(len(queries), -1)
    d = bank.shape[1]
    dist = np.empty((len(queries), k), np.float32)
    idx = np.empty((len(queries), k), np.int64)
    for qi, q in enumerate(queries):
        S = coracle.ssd_row_u8(bank, q)
        order = np.argsort(S, kind="stable")[:k]
        idx[qi] = order
        s = S[order].astype(np.float64)
        dist[qi] = (s / float(d) if integers else s * (4.0 / (65025.0 * d))).astype(np.float32)
    return dist, idx


def check_all_k(gl, coracle, bank, queries, batch_size, ks=KS, **kw):
    n_eff = (len(bank) // batch_size) * batch_size
    od, oi = oracle_topk(coracle, bank, queries, n_eff, max(ks))
    d1, i1 = gl.attack(queries, bank, distance="l2", batch_size=batch_size, **kw)
    for k in ks:
        dist, idx = gl.attack(queries, bank, distance="l2", batch_size=batch_size, k=k, **kw)
        assert dist.shape == (len(queries), k) and dist.dtype == np.float32 and idx.shape == (len(queries), k) and idx.dtype == np.int64
        assert np.array_equal(idx, oi[:, :k]), k
        assert np.array_equal(dist, od[:, :k]), k
        # column 0 is the k-less result bit for bit
        assert np.array_equal(idx[:, 0], i1) and np.array_equal(dist[:, 0].view(np.uint32), d1.view(np.uint32)), k
    return od, oi


def _case(synth, seed, n_bank, n_q, res):
    case = synth.attack_case(seed, n_bank, n_q - n_q // 2, n_q // 2, res)
    return case["bank"], np.concatenate([case["pos"], case["neg"]])


def test_golden_from_the_reference(gl, synth, golden_dir):
    g = np.load(os.path.join(golden_dir, "knn_topk.npz"))
    for c in range(int(g["n_cases"])):
        seed, nb, npos, nneg, res, bs = (int(v) for v in g["case%d" % c])
        case = synth.attack_case(seed, nb, npos, nneg, res)
        q = np.concatenate([case["pos"], case["neg"]])
        for k in (1, 5, 8):
            dist, idx = gl.attack(q, case["bank"], distance="l2", batch_size=bs, k=k)
            assert np.array_equal(idx, g["idx%d" % c][:, :k]), (c, k)
            err = np.max(np.abs(dist.astype(np.float64) - g["dist%d" % c][:, :k].astype(np.float64)))
            print("case %d k %d: largest distance difference to the reference %.3e" % (c, k, err))
            assert err <= 1e-6, (c, k, err)


def test_small_tile_ragged(gl, coracle, synth):
    bank, q = _case(synth, 51, 333, 37, 16)               # 128 x 128 tile; Q, N ragged; batch 30 truncates 333 -> 330
    check_all_k(gl, coracle, bank, q, 30)


def test_res64_ragged(gl, coracle, synth):
    """3 x 64 x 64, 515 x 2100: 3 x 9 tiles of 256 are fewer than the 1024 the dispatch rule of gl_l2_knn_i8 asks for, so the shipped library
    runs this shape on the 128 x 128 tile; the 256 x 256 kernel is checked against the oracle in test_large_tile and at this shape against the
    128 x 128 one in test_both_tiles_give_the_same_lists"""
    rng = np.random.default_rng(52)
    bank = rng.integers(0, 256, size=(2100, 3, 64, 64), dtype=np.uint8)
    q = rng.integers(0, 256, size=(515, 3, 64, 64), dtype=np.uint8)
    q[:40] = synth.perturb_u8(53, bank[rng.integers(0, 2100, size=40)], 6.0)
    check_all_k(gl, coracle, bank, q, 50)                 # n_eff = 2100: not a multiple of 128 or 256


def test_large_tile(gl, coracle):
    """enough tiles for the 256 x 256 kernel (the rule of gl_l2_knn_i8: at least 1024 of them): 9 x 130"""
    rng = np.random.default_rng(54)
    bank = rng.integers(0, 256, size=(33068, 3, 8, 8), dtype=np.uint8)
    q = rng.integers(0, 256, size=(2125, 3, 8, 8), dtype=np.uint8)
    bank[777] = bank[12]
    bank[30001] = bank[12]
    q[5] = bank[12]
    _, oi = check_all_k(gl, coracle, bank, q, 1)
    assert oi[5, :3].tolist() == [12, 777, 30001]


def test_big_and_wide(gl, coracle):
    rng = np.random.default_rng(55)
    for shape, n, nq in (((3, 256, 256), 150, 5), ((3, 512, 512), 40, 3)):       # 64-bit totals; int64 norms
        bank = rng.integers(0, 256, size=(n,) + shape, dtype=np.uint8)
        q = rng.integers(0, 256, size=(nq,) + shape, dtype=np.uint8)
        bank[3] = 0
        bank[5] = 255                                     # the largest S = 65025 d against a zero query
        q[0] = 0
        q[1] = bank[9]
        bank[20] = bank[9]
        check_all_k(gl, coracle, bank, q, 1)


def test_k_equals_n_eff_and_k_beyond(gl, coracle, synth):
    bank, q = _case(synth, 56, 25, 6, 16)
    check_all_k(gl, coracle, bank, q, 10, ks=(20,))       # n_eff = 20
    with pytest.raises(ValueError):
        gl.attack(q, bank, distance="l2", batch_size=10, k=21)
    for bad in (0, 33):
        with pytest.raises(ValueError):
            gl.attack(q, bank, distance="l2", batch_size=10, k=bad)
    with pytest.raises(NotImplementedError) as e:
        gl.attack(q.astype(np.float32) / 300.0, bank, distance="l2", batch_size=10, k=2)     # off both lattices
    assert "exact-integer" in str(e.value)
    with pytest.raises(NotImplementedError):
        gl.attack(q, bank, distance="l2-lpips", batch_size=10, k=2)


def test_ties_go_to_the_smaller_index(gl, coracle, synth):
    base = synth.lowpass_u8_images(57, 12, 16)
    bank = base[np.arange(72) % 12]                       # every row 6 times: every distance value is shared by 6 rows
    q = np.concatenate([synth.perturb_u8(58, base[[0, 5, 11]], 5.0), synth.lowpass_u8_images(59, 4, 16)])
    for k in (1, 3, 5, 6, 7, 13, 32):                     # 5 / 7 / 13: the k-th and (k+1)-th neighbours are tied
        dist, idx = gl.attack(q, bank, distance="l2", batch_size=12, k=k)
        od, oi = oracle_topk(coracle, bank, q, 72, k)
        assert np.array_equal(idx, oi) and np.array_equal(dist, od), k
        for row_d, row_i in zip(dist, idx):
            for a in range(k - 1):
                assert row_d[a] < row_d[a + 1] or (row_d[a] == row_d[a + 1] and row_i[a] < row_i[a + 1])
    assert np.array_equal(idx[:, :6] % 12, np.repeat(idx[:, :1] % 12, 6, axis=1))


def test_norm_widths_agree(gl, synth):
    from ganleaks_amd.attack import Bank, topk_keys
    ctx = gl.Context.get()
    rng = np.random.default_rng(60)
    for d, n, nq in ((12288, 300, 20), (196608, 40, 4)):
        bank = rng.integers(0, 256, size=(n, d), dtype=np.uint8)
        q = rng.integers(0, 256, size=(nq, d), dtype=np.uint8)
        out = []
        for wide in (False, True):
            b, f = Bank.from_images(bank, ctx, norms64=wide), Bank.from_images(q, ctx, norms64=wide)
            assert b.wide == wide
            keys, _, _ = topk_keys(b, f, 16)
            out.append(keys.numpy())
            d16 = gl.attack(f, b, distance="l2", batch_size=1, k=16)
            out.append(d16)
        assert np.array_equal(out[0], out[2])
        assert np.array_equal(out[1][0], out[3][0]) and np.array_equal(out[1][1], out[3][1])
        with pytest.raises(ValueError):
            topk_keys(Bank.from_images(bank, ctx, norms64=True), Bank.from_images(q, ctx, norms64=False), 4)


def test_integer_table(gl, coracle):
    rng = np.random.default_rng(61)
    F = 300
    bank = (rng.random((500, F)) < 0.3).astype(np.float32)             # 0 / 1 rows, as medGAN's thresholded samples
    q = (rng.random((21, F)) < 0.3).astype(np.float32)
    q[0] = bank[17]
    bank[400] = bank[17]
    for k in (1, 5, 32):
        dist, idx = gl.attack(q, bank, distance="l2", batch_size=100, k=k)
        od, oi = oracle_topk(coracle, bank.astype(np.uint8), q.astype(np.uint8), 500, k, integers=True)
        assert np.array_equal(idx, oi) and np.array_equal(dist, od), k
    d1, i1 = gl.attack(q, bank, distance="l2", batch_size=100)
    assert np.array_equal(idx[:, 0], i1) and np.array_equal(dist[:, 0], d1)
    assert idx[0, :2].tolist() == [17, 400] and dist[0, 0] == 0


class _RowsGenerator:
    """stands in for a generator: `z` are bank row numbers"""

    def __init__(self, ctx, bank):
        self.ctx, self.bank = ctx, bank

    def generate_u8(self, z):
        return self.ctx.to_device(self.bank[np.asarray(z)])


def test_resident_streamed_generated_and_shards_agree(gl, coracle, synth):
    from ganleaks_amd.attack import Bank, GeneratedBank, topk_keys, unpack_topk
    from ganleaks_amd.shard import merge_topk_host
    ctx = gl.Context.get()
    bank, q = _case(synth, 62, 1000, 45, 16)              # d = 768
    bs, k = 30, 16
    n_eff = 990
    od, oi = oracle_topk(coracle, bank, q, n_eff, k)
    res = gl.attack(q, bank, distance="l2", batch_size=bs, k=k)
    assert np.array_equal(res[1], oi) and np.array_equal(res[0], od)
    # streamed: 2 * 768 bytes per row -> 301 rows per chunk, 4 chunks, boundaries not multiples of the tile
    streamed = gl.attack(q, bank, distance="l2", batch_size=bs, k=k, chunk_bytes=2 * 768 * 301)
    dev = gl.attack(q, ctx.to_device(bank), distance="l2", batch_size=bs, k=k, chunk_bytes=2 * 768 * 301)
    gen = gl.attack(q, GeneratedBank(_RowsGenerator(ctx, bank), np.arange(1000)), distance="l2", batch_size=bs, k=k, chunk_bytes=2 * 768 * 177)
    prepared = gl.attack(q, Bank.from_images(bank, ctx), distance="l2", batch_size=bs, k=k)
    for name, other in (("streamed", streamed), ("device array", dev), ("generated", gen), ("prepared", prepared)):
        assert np.array_equal(other[0].view(np.uint32), res[0].view(np.uint32)) and np.array_equal(other[1], res[1]), name
    # unequal index_base shards, merged on the host
    fq = Bank.from_images(q, ctx)
    whole, _, _ = topk_keys(Bank.from_images(bank[:n_eff], ctx), fq, k)
    whole = whole.numpy()
    for bounds in ((0, 130, 990), (0, 7, 500, 990), (0, 990, 990)):
        parts = []
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            keys = ctx.empty((len(q), k), np.uint64)
            gl._lib.check(ctx.lib.gl_topk_init(ctx.handle, p(keys.ptr), len(q), k))
            if hi > lo:
                keys, _, _ = topk_keys(Bank.from_images(bank[lo:hi], ctx, index_base=lo), fq, k, keys=keys)
            parts.append(keys.numpy())
        merged = merge_topk_host(parts, k)
        assert np.array_equal(merged, whole), bounds
        # the same through attack(): a shard with index_base and a reduce_fn that folds in the other shards' lists
        lo, hi = bounds[0], bounds[1]
        others = parts[1:]
        got = gl.attack(fq, bank[lo:hi], distance="l2", batch_size=bs, k=k, index_base=lo,
                        reduce_fn=lambda keys: ctx.to_device(merge_topk_host([keys.numpy()] + others, k)))
        assert np.array_equal(got[1], res[1]) and np.array_equal(got[0], res[0]), bounds
    # the device-side merge gives what the host statement gives
    stacked = ctx.to_device(np.stack(parts))
    dst = ctx.empty((len(q), k), np.uint64)
    gl._lib.check(ctx.lib.gl_topk_init(ctx.handle, p(dst.ptr), len(q), k))
    gl._lib.check(ctx.lib.gl_topk_merge(ctx.handle, p(dst.ptr), p(stacked.ptr), len(q), k, len(parts)))
    assert np.array_equal(dst.numpy(), whole)
    d2, i2 = unpack_topk(ctx, dst, len(q), k, 768)
    assert np.array_equal(i2, res[1]) and np.array_equal(d2, res[0])
    # fewer rows than k in a list: empty slots unpack to +inf / -1
    few, _, _ = topk_keys(Bank.from_images(bank[:3], ctx), fq, 5)
    d3, i3 = unpack_topk(ctx, few, len(q), 5, 768)
    assert np.all(i3[:, 3:] == -1) and np.all(np.isinf(d3[:, 3:])) and np.all(i3[:, :3] >= 0)


def test_workspace_slicing_does_not_change_the_result(gl, synth):
    from ganleaks_amd.attack import set_topk_workspace
    ctx = gl.Context.get()
    bank, q = _case(synth, 63, 700, 300, 16)
    ref = {k: gl.attack(q, bank, distance="l2", batch_size=1, k=k) for k in (2, 32)}
    try:
        for budget in (256 * 1024, 1):                    # 6 slices of bank rows; slices of 128 queries x 128 rows
            set_topk_workspace(ctx, budget)
            for k in (2, 32):
                dist, idx = gl.attack(q, bank, distance="l2", batch_size=1, k=k)
                assert np.array_equal(idx, ref[k][1]) and np.array_equal(dist, ref[k][0]), (budget, k)
    finally:
        set_topk_workspace(ctx, 0)


def test_one_pass_over_the_pairs(gl, synth):
    from ganleaks_amd.attack import Bank, knn_keys, set_topk_workspace, topk_keys
    ctx = gl.Context.get()
    bank, q = _case(synth, 64, 700, 300, 16)
    b, f = Bank.from_images(bank, ctx), Bank.from_images(q, ctx)

    def launches(fn):
        ctx.prof_reset()
        fn()
        prof = ctx.prof_read()
        return prof["l2_knn"][1], prof["topk_select"][1]

    ctx.prof_enable(True)
    try:
        top1 = launches(lambda: knn_keys(b, f))
        assert top1 == (1, 0)
        for k in (1, 32):
            pair, select = launches(lambda: topk_keys(b, f, k))
            assert pair == top1[0] and select >= 1, (k, pair, select)
        set_topk_workspace(ctx, 256 * 1024)
        sliced = {k: launches(lambda: topk_keys(b, f, k)) for k in (2, 32)}
        assert sliced[2][0] == sliced[32][0] and sliced[2][0] > 1, sliced
    finally:
        set_topk_workspace(ctx, 0)
        ctx.prof_enable(False)
        ctx.prof_reset()


def test_bad_arguments_leave_the_device_usable(gl, synth):
    from ganleaks_amd.attack import Bank
    ctx = gl.Context.get()
    lib = ctx.lib
    bank, q = _case(synth, 65, 200, 10, 16)
    b, f = Bank.from_images(bank, ctx), Bank.from_images(q, ctx)
    k = 4
    keys = ctx.empty((10, k), np.uint64)

    def fails(rc, needle):
        assert rc < 0, rc
        msg = lib.gl_last_error().decode()
        assert needle in msg, msg

    args = lambda **kw: [kw.get(n, v) for n, v in (("ctx", ctx.handle), ("bank", p(b.rows_i8.ptr)), ("bn", p(b.norms.ptr)), ("n", 200), ("base", 0),   # noqa: E731
                                                   ("q", p(f.rows_i8.ptr)), ("qn", p(f.norms.ptr)), ("nq", 10), ("d", 768), ("k", k), ("keys", p(keys.ptr)))]
    fails(lib.gl_l2_topk_i8(*args(k=0)), "k=0")
    fails(lib.gl_l2_topk_i8(*args(k=33)), "k=33")
    fails(lib.gl_l2_topk_i8(*args(ctx=None)), "NULL ctx")
    fails(lib.gl_l2_topk_i8(*args(keys=None)), "NULL device pointer")
    fails(lib.gl_l2_topk_i8(*args(bn=None)), "NULL device pointer")
    fails(lib.gl_l2_topk_i8(*args(bank=p(b.rows_i8.ptr + 8))), "16-byte aligned")
    fails(lib.gl_l2_topk_i8(*args(keys=p(keys.ptr + 4))), "8-byte aligned")
    fails(lib.gl_l2_topk_i8(*args(d=int(lib.gl_l2_max_d(0)) + 1)), "bad sizes")
    fails(lib.gl_l2_topk_i8_wide(*args(d=int(lib.gl_l2_max_d(1)) + 1)), "bad sizes")
    fails(lib.gl_l2_topk_i8(*args(n=-1)), "bad sizes")
    fails(lib.gl_l2_topk_i8(*args(base=(1 << 32) - 100)), "index bits")
    fails(lib.gl_topk_init(ctx.handle, p(keys.ptr), 10, 0), "k=0")
    fails(lib.gl_topk_init(ctx.handle, None, 10, k), "NULL")
    fails(lib.gl_topk_merge(ctx.handle, p(keys.ptr), None, 10, k, 2), "NULL")
    fails(lib.gl_topk_merge(ctx.handle, p(keys.ptr), p(keys.ptr), 10, 40, 2), "k=40")
    fails(lib.gl_topk_unpack(ctx.handle, p(keys.ptr), 10, k, 768, 0, None, None), "NULL")
    fails(lib.gl_topk_unpack(ctx.handle, p(keys.ptr), 10, k, 0, 0, None, None), "bad")
    fails(lib.gl_topk_set_workspace(None, 0), "NULL ctx")
    # no rows / no queries: nothing happens, nothing is dereferenced
    assert lib.gl_topk_init(ctx.handle, p(keys.ptr), 10, k) == 0
    assert lib.gl_l2_topk_i8(*args(n=0, bank=None, bn=None)) == 0
    assert lib.gl_l2_topk_i8(*args(nq=0, q=None, qn=None, keys=None)) == 0
    assert np.all(keys.numpy() == EMPTY)
    # and the next call works
    dist, idx = gl.attack(f, b, distance="l2", batch_size=1, k=k)
    d1, i1 = gl.attack(f, b, distance="l2", batch_size=1)
    assert np.array_equal(idx[:, 0], i1) and np.array_equal(dist[:, 0], d1)


def test_custom_knn_k(gl, coracle, synth):
    import types
    from ganleaks_amd.attack_models import fbb
    from ganleaks_amd.attack_models.utils import Loss
    bank, q = _case(synth, 66, 100, 4, 16)
    args = types.SimpleNamespace(BATCH_SIZE=30, K=5)
    loss = Loss("l2", if_norm_reg=False)
    od, oi = oracle_topk(coracle, bank, q, 90, 5)
    for qi in range(len(q)):
        dists, idxs = fbb.custom_knn_k(bank, q[qi], loss, args)
        assert idxs == oi[qi].tolist() and dists == [float(v) for v in od[qi]]
        assert all(isinstance(v, float) for v in dists) and all(isinstance(v, int) for v in idxs)
        d1, i1 = fbb.custom_knn(bank, q[qi], loss, args)
        assert (d1, i1) == (dists[0], idxs[0])


TILE_CHILD = r'''
import json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
import ganleaks_amd as gl
from ganleaks_amd import _lib
from ganleaks_amd.attack import Bank, knn_keys, topk_keys
assert _lib.LIB_PATH.endswith("libganleaks_hip_tuning.so")
ctx = gl.Context.get()
rng = np.random.default_rng(67)
bank = Bank.from_images(rng.integers(0, 256, size=(2100, 3, 64, 64), dtype=np.uint8), ctx)      # ragged last tiles of either size
q = Bank.from_images(rng.integers(0, 256, size=(515, 3, 64, 64), dtype=np.uint8), ctx)
keys = {}
for tile in (128, 256):
    os.environ["GL_L2_TILE"] = str(tile)
    keys[tile] = topk_keys(bank, q, 16)[0].numpy().copy()
    keys[tile, 1] = knn_keys(bank, q)[0].numpy().copy()
print(json.dumps({"tiles_equal": bool(np.array_equal(keys[128], keys[256])),
                  "column0_is_top1": bool(np.array_equal(keys[256][:, 0], keys[256, 1]) and np.array_equal(keys[128][:, 0], keys[128, 1])),
                  "ascending": bool(np.all(keys[256][:, 1:] > keys[256][:, :-1]))}))
'''


def test_both_tiles_give_the_same_lists():
    """3 x 64 x 64, 515 x 2100: the 256 x 256 and the 128 x 128 pairwise kernels forced in turn (GL_L2_TILE, read by the tuning build only)"""
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
    assert out == {"tiles_equal": True, "column0_is_top1": True, "ascending": True}, out
