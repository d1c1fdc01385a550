"""GPU: the exact-integer L2 search for images of more than 262143 values (3x512x512, 3x1024x1024, up to 2^24 = 3x2048x2048): int64 row
norms (gl_l2_prepare_wide) and the 128 x 128 int8-MFMA tile with 64-bit totals (gl_l2_knn_i8_wide).  Indices and distances equal the C
oracle's bit for bit; where both forms apply (d <= 262143) the wide keys equal the int32-norm keys."""
import ctypes

import numpy as np
import pytest

import gpu_common  # noqa: F401

pytestmark = pytest.mark.gpu
p = ctypes.c_void_p
WIDE_MAX = 1 << 24


@pytest.fixture(scope="module")
def gl():
    import ganleaks_amd
    return ganleaks_amd


@pytest.fixture(scope="module")
def coracle():
    import c_oracle
    return c_oracle


@pytest.fixture(scope="module")
def lib():
    from ganleaks_amd import _lib
    return _lib.load()


def _fails(lib, rc, needle=None):
    assert rc < 0, rc
    msg = lib.gl_last_error().decode()
    assert msg and (needle is None or needle in msg), msg


def _bank(shape, n, seed):
    """random rows with all-0 / all-255 rows and a row repeated three times (ties: the first index wins)"""
    rng = np.random.default_rng(seed)
    bank = rng.integers(0, 256, size=(n,) + shape, dtype=np.uint8)
    bank[3] = 0
    bank[5] = 255
    bank[20] = bank[9]
    bank[30] = bank[9]
    return bank, rng


@pytest.mark.parametrize("shape", [(262144,), (3, 512, 512), (3, 300, 700), (3, 1024, 1024), (1 << 24,)])
def test_attack_matches_c_oracle(shape, gl, coracle):
    bank, rng = _bank(shape, 40, sum(shape))
    q = np.stack([np.full(shape, 255, np.uint8), np.zeros(shape, np.uint8), bank[9],
                  bank[36],                                        # its twin lies in the truncated tail (40 -> 32 rows): not found
                  rng.integers(0, 256, size=shape, dtype=np.uint8), rng.integers(100, 140, size=shape, dtype=np.uint8)])
    dist, idx = gl.attack(q, bank, distance="l2", batch_size=16)
    od, oi, _ = coracle.knn_l2_u8(bank, q, 16)
    assert np.array_equal(idx, oi) and np.array_equal(dist, od)
    assert idx[:3].tolist() == [5, 3, 9] and dist[:3].tolist() == [0, 0, 0]
    assert idx[3] < 32
    # the largest S = 65025 d (the top of the key range), all rows tied: index 0, distance 4
    d2, i2 = gl.attack(q[:2], np.zeros((16,) + shape, np.uint8), batch_size=16)
    assert i2.tolist() == [0, 0] and d2[0] == np.float32(4.0) and d2[1] == 0


@pytest.mark.parametrize("d", [12288, 66051, 66052, 196608, 262143])
def test_wide_keys_equal_int32_norm_keys(d, gl):
    from ganleaks_amd.attack import Bank, knn_keys
    ctx = gl.Context.get()
    rng = np.random.default_rng(d)
    bank = rng.integers(0, 256, size=(200, d), dtype=np.uint8)
    bank[7] = 0
    bank[150] = 255
    q = rng.integers(0, 256, size=(130, d), dtype=np.uint8)
    q[0] = 255
    q[1] = 0
    q[2] = bank[120]
    narrow_b, wide_b = Bank.from_images(bank, ctx), Bank.from_images(bank, ctx, norms64=True)
    narrow_q, wide_q = Bank.from_images(q, ctx), Bank.from_images(q, ctx, norms64=True)
    assert narrow_b.norms.dtype == np.int32 and wide_b.norms.dtype == np.int64 and wide_b.wide and not narrow_b.wide
    assert np.array_equal(narrow_b.rows_i8.numpy(), wide_b.rows_i8.numpy())
    assert np.array_equal(narrow_b.norms.numpy().view(np.uint32).astype(np.int64), wide_b.norms.numpy())
    k_narrow, _, _ = knn_keys(narrow_b, narrow_q)
    k_wide, _, _ = knn_keys(wide_b, wide_q)
    k_narrow, k_wide = k_narrow.numpy()[:130], k_wide.numpy()[:130]
    assert k_wide.dtype == np.uint64 and np.array_equal(k_narrow, k_wide)
    # raw queries follow the bank's width
    k_auto, qb, _ = knn_keys(wide_b, q)
    assert qb.wide and np.array_equal(k_auto.numpy()[:130], k_wide)
    # a prepared query Bank of the other width is refused
    with pytest.raises(ValueError, match="norms64"):
        knn_keys(wide_b, narrow_q)
    with pytest.raises(ValueError, match="norms64"):
        knn_keys(narrow_b, wide_q)


@pytest.mark.parametrize("k", [1, 4, 5])
def test_flush_boundaries(k, gl, coracle):
    """d = 65536 k + {-1, 0, 1}: the int32 accumulators are flushed every 64 KiB of K.  Rows of u = 0 / 255 (int8 -128 / 127) put each
    segment's partial cross term at +2^30 (0 against 0) or -2^30 + 2^23 (0 against 255), the largest magnitudes one segment can hold."""
    from ganleaks_amd.attack import Bank, knn_keys, unpack_keys
    ctx = gl.Context.get()
    for d in (65536 * k - 1, 65536 * k, 65536 * k + 1):
        rng = np.random.default_rng(d)
        bank = np.zeros((24, d), np.uint8)
        bank[1] = 255
        bank[2, ::2] = 255
        bank[3, : d // 2] = 255
        bank[4:12] = np.where(rng.random((8, d)) < 0.5, 0, 255).astype(np.uint8)
        bank[12:] = rng.integers(0, 256, size=(12, d), dtype=np.uint8)
        bank[0, -1] = 1                                              # rows 0 and the queries below are not all tied
        q = np.stack([np.zeros(d, np.uint8), np.full(d, 255, np.uint8), bank[3], bank[7], bank[15],
                      np.where(rng.random(d) < 0.5, 0, 255).astype(np.uint8)])
        qb = Bank.from_images(q, ctx, norms64=True)
        keys, _, _ = knn_keys(Bank.from_images(bank, ctx, norms64=True), qb)
        dist, idx = unpack_keys(ctx, keys, qb.n, d)
        od, oi, ssd = coracle.knn_l2_u8(bank, q, 24)
        assert np.array_equal(idx, oi) and np.array_equal(dist, od), d
        shift = 63 - int(65025 * d).bit_length() if 63 - int(65025 * d).bit_length() < 32 else 32
        assert np.array_equal(keys.numpy()[:qb.n], (ssd.astype(np.uint64) << np.uint64(shift)) | oi.astype(np.uint64)), d
        # every S of one query, through a bank of single rows (one key per row)
        for n in range(0, 24, 5):
            kn, _, _ = knn_keys(Bank.from_images(bank[n:n + 1], ctx, norms64=True, index_base=n), qb)
            s = kn.numpy()[:qb.n] >> np.uint64(shift)
            assert np.array_equal(s.astype(np.int64), [coracle.ssd_row_u8(bank[n:n + 1], qq)[0] for qq in q]), (d, n)


def test_index_field_at_shift_25(gl):
    """3x1024x1024: key shift 25, so a shard may hold global indices up to 2^25 - 1"""
    from ganleaks_amd.attack import Bank, knn_keys, unpack_keys
    ctx = gl.Context.get()
    shape = (3, 1024, 1024)
    d = 3 * 1024 * 1024
    rng = np.random.default_rng(25)
    bank = rng.integers(0, 256, size=(33,) + shape, dtype=np.uint8)
    q = np.stack([bank[17], bank[31], rng.integers(0, 256, size=shape, dtype=np.uint8)])
    qb = Bank.from_images(q, ctx, norms64=True)
    base = (1 << 25) - 32
    keys, _, _ = knn_keys(Bank.from_images(bank[:32], ctx, norms64=True, index_base=base), qb)
    dist, idx = unpack_keys(ctx, keys, qb.n, d)
    assert idx[:2].tolist() == [base + 17, base + 31] and dist[:2].tolist() == [0, 0]
    assert base <= idx[2] < base + 32
    with pytest.raises(gl.GanLeaksError, match="index bits"):
        knn_keys(Bank.from_images(bank, ctx, norms64=True, index_base=base), qb)


def test_streamed_equals_resident(gl, coracle):
    shape = (3, 512, 512)
    d = 3 * 512 * 512
    bank, rng = _bank(shape, 45, 7)
    q = np.concatenate([bank[[9, 44, 3]], rng.integers(0, 256, size=(3,) + shape, dtype=np.uint8)])
    dr, ir = gl.attack(q, bank, batch_size=15)
    ds, is_ = gl.attack(q, bank, batch_size=15, chunk_bytes=3 * 2 * d)             # 3 rows per chunk
    assert np.array_equal(ir, is_) and np.array_equal(dr.view(np.uint32), ds.view(np.uint32))
    od, oi, _ = coracle.knn_l2_u8(bank, q, 15)
    assert np.array_equal(ir, oi) and np.array_equal(dr, od)
    assert ir[:3].tolist() == [9, 44, 3]


@pytest.mark.parametrize("shape", [(3, 512, 512), (1 << 24,)])
def test_loss_l2_rows(shape, gl, coracle):
    from ganleaks_amd.attack_models.utils import Loss
    d = int(np.prod(shape))
    rng = np.random.default_rng(d + 1)
    x_hat = rng.integers(0, 256, size=(6,) + shape, dtype=np.uint8)
    x_hat[0] = 0
    x_hat[1] = 255
    x_gt = np.full((1,) + shape, 255, np.uint8)
    v = np.asarray(Loss("l2")(x_hat, x_gt), np.float32)
    ref = (coracle.ssd_row_u8(x_hat, x_gt[0]).astype(np.float64) * (4.0 / (65025.0 * d))).astype(np.float32)
    assert np.array_equal(v, ref) and v[0] == np.float32(4.0) and v[1] == 0
    # one x_gt row per x_hat row
    x_gt6 = x_hat[::-1].copy()
    v6 = np.asarray(Loss("l2")(x_hat, x_gt6), np.float32)
    ref6 = np.array([coracle.ssd_row_u8(x_hat[i:i + 1], x_gt6[i])[0] for i in range(6)], np.float64) * (4.0 / (65025.0 * d))
    assert np.array_equal(v6, ref6.astype(np.float32))


def test_float_lattice_inputs_and_custom_knn(gl, coracle):
    """float images on the 8-bit lattice (what fbb.main reads from PNG files) take the same wide path, one query at a time"""
    import types
    from ganleaks_amd.attack_models.fbb import custom_knn
    from ganleaks_amd.attack_models.utils import Loss
    shape = (3, 512, 512)
    bank, rng = _bank(shape, 34, 11)
    q = np.stack([bank[9], rng.integers(0, 256, size=shape, dtype=np.uint8)])
    to_f = lambda u: (2.0 * (u.astype(np.float64) / 255.0) - 1.0).astype(np.float32)   # noqa: E731
    od, oi, _ = coracle.knn_l2_u8(bank, q, 16)
    dist, idx = gl.attack(to_f(q), to_f(bank), batch_size=16)
    assert np.array_equal(idx, oi) and np.array_equal(dist, od)
    loss = Loss("l2")
    fb = to_f(bank)
    for i in range(len(q)):
        dd, ii = custom_knn(fb, to_f(q[i]), loss, types.SimpleNamespace(BATCH_SIZE=16))
        assert ii == oi[i] and dd == float(od[i])


def test_host_one_call_abi(gl, lib, coracle):
    """gl_fbb_knn_l2_host takes the wide pair above 262143 values"""
    ctx = gl.Context.get()
    shape = (3, 512, 512)
    bank, rng = _bank(shape, 40, 13)
    q = np.ascontiguousarray(np.stack([bank[30], np.zeros(shape, np.uint8), rng.integers(0, 256, size=shape, dtype=np.uint8)]))
    dist = np.empty(len(q), np.float32)
    idx = np.empty(len(q), np.int64)
    rc = lib.gl_fbb_knn_l2_host(ctx.handle, bank.ctypes.data_as(p), len(bank), q.ctypes.data_as(p), len(q), bank[0].size, 16,
                                dist.ctypes.data_as(p), idx.ctypes.data_as(p))
    assert rc == 0, lib.gl_last_error()
    od, oi, _ = coracle.knn_l2_u8(bank, q, 16)
    assert np.array_equal(idx, oi) and np.array_equal(dist, od) and idx.tolist()[:2] == [9, 3]


@pytest.mark.parametrize("d", [1000, 196608, 3 * 512 * 512, 1 << 24])
def test_prepare_wide_abi(d, gl, lib):
    ctx = gl.Context.get()
    rng = np.random.default_rng(d)
    u = rng.integers(0, 256, size=(4, d), dtype=np.uint8)
    u[0] = 0                                                       # the largest norm, 16384 d (2^38 at d = 2^24)
    ud = ctx.to_device(u)
    stride = int(lib.gl_l2_row_stride(d))
    rows = ctx.empty((4, stride), np.int8)
    norms = ctx.empty((4,), np.int64)
    assert lib.gl_l2_prepare_wide(ctx.handle, p(ud.ptr), 4, d, p(rows.ptr), p(norms.ptr)) == 0, lib.gl_last_error()
    ctx.sync()
    ref = ((u.astype(np.int64) - 128) ** 2).sum(axis=1)
    assert np.array_equal(norms.numpy(), ref) and ref[0] == 16384 * d
    r = rows.numpy()
    assert np.array_equal(r[:, :d], (u ^ 0x80).view(np.int8)) and not r[:, d:].any()
    if d <= 262143:
        rows32 = ctx.empty((4, stride), np.int8)
        norms32 = ctx.empty((4,), np.int32)
        assert lib.gl_l2_prepare(ctx.handle, p(ud.ptr), 4, d, p(rows32.ptr), p(norms32.ptr)) == 0
        ctx.sync()
        assert rows32.numpy().tobytes() == r.tobytes()


def test_wide_abi_rejects_bad_arguments(gl, lib):
    assert lib.gl_l2_max_d(0) == 262143 and lib.gl_l2_max_d(1) == WIDE_MAX
    ctx = gl.Context.get()
    h = ctx.handle
    a = ctx.zeros((256, 128), np.int8)
    n = ctx.zeros((256,), np.int64)
    k = ctx.zeros((256,), np.uint64)
    u = ctx.zeros((4, 128), np.uint8)
    knn = lib.gl_l2_knn_i8_wide
    _fails(lib, knn(h, p(a.ptr), p(n.ptr), 256, 0, p(a.ptr), p(n.ptr), 256, 0, p(k.ptr)), "bad sizes")                 # d = 0
    _fails(lib, knn(h, p(a.ptr), p(n.ptr), -1, 0, p(a.ptr), p(n.ptr), 256, 128, p(k.ptr)), "bad sizes")
    _fails(lib, knn(h, p(a.ptr), p(n.ptr), 256, 0, p(a.ptr), p(n.ptr), -1, 128, p(k.ptr)), "bad sizes")
    _fails(lib, knn(h, p(a.ptr), p(n.ptr), 256, 0, p(a.ptr), p(n.ptr), 256, WIDE_MAX + 1, p(k.ptr)), "bad sizes")     # d too large
    _fails(lib, knn(h, p(a.ptr + 4), p(n.ptr), 256, 0, p(a.ptr), p(n.ptr), 256, 128, p(k.ptr)), "aligned")
    _fails(lib, knn(h, p(a.ptr), p(n.ptr), 256, 0, p(a.ptr + 8), p(n.ptr), 256, 128, p(k.ptr)), "aligned")
    _fails(lib, knn(h, p(0), p(n.ptr), 256, 0, p(a.ptr), p(n.ptr), 256, 128, p(k.ptr)), "NULL")
    _fails(lib, knn(h, p(a.ptr), p(0), 256, 0, p(a.ptr), p(n.ptr), 256, 128, p(k.ptr)), "NULL")
    _fails(lib, knn(h, p(a.ptr), p(n.ptr), 256, 0, p(a.ptr), p(n.ptr), 256, 128, p(0)), "NULL")
    _fails(lib, knn(h, p(a.ptr), p(n.ptr), 256, (1 << 32) - 8, p(a.ptr), p(n.ptr), 256, 128, p(k.ptr)), "global index")
    _fails(lib, knn(h, p(a.ptr), p(n.ptr), 256, (1 << 23) - 8, p(a.ptr), p(n.ptr), 256, WIDE_MAX, p(k.ptr)), "global index")
    _fails(lib, knn(p(0), p(a.ptr), p(n.ptr), 256, 0, p(a.ptr), p(n.ptr), 256, 128, p(k.ptr)), "NULL ctx")
    assert knn(h, p(0), p(0), 0, 0, p(0), p(0), 0, 128, p(0)) == 0                                                      # empty problem
    assert knn(h, p(0), p(0), 5, 0, p(0), p(0), 0, WIDE_MAX, p(0)) == 0
    prep = lib.gl_l2_prepare_wide
    _fails(lib, prep(h, p(u.ptr), 4, 0, p(a.ptr), p(n.ptr)), "bad")
    _fails(lib, prep(h, p(u.ptr), -1, 128, p(a.ptr), p(n.ptr)), "bad")
    _fails(lib, prep(h, p(u.ptr), 4, WIDE_MAX + 1, p(a.ptr), p(n.ptr)), "exceeds")
    _fails(lib, prep(h, p(0), 4, 128, p(a.ptr), p(n.ptr)), "NULL")
    _fails(lib, prep(h, p(u.ptr), 4, 128, p(a.ptr), p(0)), "NULL")
    _fails(lib, prep(h, p(u.ptr), 4, 128, p(a.ptr + 4), p(n.ptr)), "aligned")
    _fails(lib, prep(p(0), p(u.ptr), 4, 128, p(a.ptr), p(n.ptr)), "bad")
    assert prep(h, p(0), 0, 128, p(0), p(0)) == 0
    assert prep(h, p(0), 0, WIDE_MAX, p(0), p(0)) == 0
    _fails(lib, lib.gl_l2_rows_u8(h, p(u.ptr), 4, p(u.ptr), 1, WIDE_MAX + 1, p(k.ptr)), "bad")


def test_defaults_unchanged(gl):
    from ganleaks_amd.attack import Bank
    ctx = gl.Context.get()
    b = Bank.from_images(np.zeros((2, 3, 64, 64), np.uint8), ctx)
    assert b.norms.dtype == np.int32 and not b.wide
    with pytest.raises(gl.GanLeaksError):
        Bank.from_images(np.zeros((2, 262144), np.uint8), ctx)
    with pytest.raises(gl.GanLeaksError):
        Bank.from_images(np.zeros((2, 3, 512, 512), np.uint8), ctx)
    assert Bank.from_images(np.zeros((2, 262144), np.uint8), ctx, norms64=True).norms.dtype == np.int64
    assert Bank.from_images(np.zeros((2, 262144), np.uint8), ctx, norms64="auto").wide
    assert not Bank.from_images(np.zeros((2, 262143), np.uint8), ctx, norms64="auto").wide
    with pytest.raises(gl.GanLeaksError):
        Bank.from_images(np.zeros((1, WIDE_MAX + 1), np.uint8), ctx, norms64=True)
    with pytest.raises(ValueError):
        Bank.from_images(np.zeros((2, 16), np.uint8), ctx, norms64="yes")


def test_attack_matches_reference_golden_res512(gl, synth, golden_dir, coracle):
    """tests/golden/knn_res512.npz: the reference's custom_knn with the utils.py:163 lambda on 3 x 512 x 512 images"""
    import os
    g = np.load(os.path.join(golden_dir, "knn_res512.npz"))
    case = synth.attack_case(int(g["seed"]), int(g["n_bank"]), int(g["n_pos"]), int(g["n_neg"]), int(g["res"]))
    bs = int(g["batch_size"])
    for kind in ("pos", "neg"):
        dist, idx = gl.attack(case[kind], case["bank"], distance="l2", batch_size=bs)
        assert dist.dtype == np.float32 and idx.dtype == np.int64
        assert np.array_equal(idx, g[kind + "_idx"])
        np.testing.assert_allclose(dist.astype(np.float64), g[kind + "_dist"], rtol=0, atol=1e-6)
        od, oi, _ = coracle.knn_l2_u8(case["bank"], case[kind], bs)
        assert np.array_equal(idx, oi) and np.array_equal(dist, od)
