"""GPU: top-K and eps-ball counts for rows off both lattices (nearest_neighbours / ball_counts with float_path='exact', gl_l2_topk_f32,
gl_l2_count_f32).  Everything is compared with the CPU chain matrix M[q, n] = c_oracle.l2_pair_f32(q, bank[n]) -- the fixed-order float32
distance D32 the device shares bit for bit -- so lists and counts are checked with array_equal.  Shapes are the smallest at which the
kernel can go wrong: the 64 x 64 tile, 32-float K slices, the float4 path (d % 4 == 0) and pieces of 4 rows."""
import ctypes
import functools
import os

import numpy as np
import pytest

import float_rows_common as common

pytestmark = pytest.mark.gpu

# (Q, N, batch, d or image shape)
CASES = {
    "ragged": (70, 203, 7, (37,)),           # two query tiles, four ragged row tiles, n_eff = 203 = 3 (mod 4), scalar loads, a K tail
    "images": (5, 130, 10, (3, 8, 8)),       # d = 192: the float4 path
    "exact_tiles": (64, 64, 64, (32,)),      # whole tiles, one K slice
    "d1": (3, 40, 10, (1,)),
}
# unsorted, with a negative radius, 0.0, a repeated radius and inf; the rest are quantiles of the case's distances
QUANTILES = [0.9, 0.01, 0.5, 0.25, 0.05, 0.75, 0.1, 0.6, 0.3, 0.02, 0.99]


@functools.lru_cache(maxsize=None)
def case(name):
    """(queries, bank, batch, n_eff, M): seeded normal rows and their chain matrix, computed once and shared (never written to)"""
    nq, nb, bs, shape = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    bank = rng.normal(0.0, 1.0, (nb,) + shape).astype(np.float32)
    queries = rng.normal(0.0, 1.0, (nq,) + shape).astype(np.float32)
    if name == "ragged":                     # some queries near bank rows, one of them in the ragged last tile
        queries[:4] = bank[[0, 63, 64, 202]] + rng.normal(0.0, 0.05, (4,) + shape).astype(np.float32)
    n_eff = (nb // bs) * bs
    M = common.chain_matrix(queries, bank[:n_eff])
    for a in (queries, bank, M):
        a.setflags(write=False)
    return queries, bank, bs, n_eff, M


def radii16(M):
    with np.errstate(over="ignore"):
        return np.asarray([-1.0, np.inf, 0.0] + [np.quantile(M, v, method="lower") for v in QUANTILES] + [np.quantile(M, 0.5, method="lower"), 1e-30],
                          np.float32)


def expect_lists(M, k):
    order = np.argsort(M, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(M, order, axis=1), order


def expect_counts(M, eps32):
    return (M[:, :, None] <= np.asarray(eps32, np.float32)[None, None, :]).sum(axis=1).astype(np.int64)


def check_lists(dist, idx, M, k):
    want_d, want_i = expect_lists(M, k)
    assert idx.dtype == np.int64 and dist.dtype == np.float32 and idx.shape == want_i.shape
    assert np.array_equal(idx, want_i)
    assert np.array_equal(dist.view(np.uint32), np.ascontiguousarray(want_d).view(np.uint32))
    assert all(len(set(row)) == len(row) for row in idx.tolist())


@pytest.mark.parametrize("name", list(CASES))
def test_lists_and_counts_against_the_chain(name):
    import ganleaks_amd as gl
    queries, bank, bs, n_eff, M = case(name)
    top1_d, top1_i = gl.attack(queries, bank, distance="l2", batch_size=bs, float_path="exact")
    for k in (1, 5, 32):
        dist, idx = gl.nearest_neighbours(queries, bank, k, distance="l2", batch_size=bs, float_path="exact")
        check_lists(dist, idx, M, k)
        assert np.array_equal(dist[:, 0], top1_d) and np.array_equal(idx[:, 0], top1_i)
    for eps in (np.asarray([np.quantile(M, 0.3, method="lower")], np.float32), radii16(M)):
        counts = gl.ball_counts(queries, bank, eps, batch_size=bs, float_path="exact")
        assert counts.dtype == np.int64 and np.array_equal(counts, expect_counts(M, eps))
    assert len(eps) == 16 and np.all(counts[:, 1] == n_eff) and np.all(counts[:, 0] == 0)       # inf: the ragged tiles are masked; -1: nothing
    # the ball of the j-th neighbour's own distance holds at least j + 1 samples
    mine = gl.ball_counts(queries, bank, dist[0, :5], batch_size=bs, float_path="exact")[0]
    assert np.all(mine >= np.arange(1, 6))


def test_k_equal_to_the_whole_bank():
    import ganleaks_amd as gl
    queries, bank, _, _, _ = case("ragged")
    small = bank[:30]
    M = common.chain_matrix(queries[:3], small)
    dist, idx = gl.nearest_neighbours(queries[:3], small, 30, distance="l2", batch_size=30, float_path="exact")
    check_lists(dist, idx, M, 30)
    assert np.array_equal(np.sort(idx, axis=1), np.tile(np.arange(30), (3, 1)))
    with pytest.raises(ValueError):
        gl.nearest_neighbours(queries[:3], small, 31, distance="l2", batch_size=30, float_path="exact")
    with pytest.raises(ValueError):
        gl.nearest_neighbours(queries[:3], small, 5, distance="l2", batch_size=31, float_path="exact")      # no full batch
    with pytest.raises(ValueError):
        gl.ball_counts(queries[:3], small, 0.5, batch_size=31, float_path="exact")


def test_ties_go_to_the_smaller_index():
    import ganleaks_amd as gl
    queries, bank, bs, n_eff, _ = case("ragged")
    bank, queries = bank.copy(), queries.copy()
    bank[150] = bank[17]
    queries[0] = bank[17]
    dist, idx = gl.nearest_neighbours(queries, bank, 5, distance="l2", batch_size=bs, float_path="exact")
    assert idx[0, :2].tolist() == [17, 150] and dist[0, :2].tolist() == [0.0, 0.0] and not np.signbit(dist[0, :2]).any()
    counts = gl.ball_counts(queries, bank, 0.0, batch_size=bs, float_path="exact")
    assert counts[0, 0] == 2 and np.all(counts[1:, 0] == 0)


def _keys_to_lists(keys):
    keys = np.asarray(keys, np.uint64)
    return (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)


def test_invariance():
    """streamed, sliced, prepared, sharded by hand and by a DeviceGroup: the resident result, array_equal"""
    import ganleaks_amd as gl
    from ganleaks_amd import shard
    from ganleaks_amd.attack import set_topk_workspace
    queries, bank, bs, n_eff, M = case("ragged")
    ctx = gl.Context.get()
    k, eps = 5, radii16(M)
    want_d, want_i = gl.nearest_neighbours(queries, bank, k, distance="l2", batch_size=bs, float_path="exact")
    want_c = gl.ball_counts(queries, bank, eps, batch_size=bs, float_path="exact")
    check_lists(want_d, want_i, M, k)
    assert np.array_equal(want_c, expect_counts(M, eps))

    def same(lists=None, counts=None):
        if lists is not None:
            assert np.array_equal(lists[1], want_i) and np.array_equal(lists[0].view(np.uint32), want_d.view(np.uint32))
        if counts is not None:
            assert np.array_equal(counts, want_c)

    # a streamed bank: chunks of 90 fp32 rows
    chunk = 90 * 4 * 37
    same(gl.nearest_neighbours(queries, bank, k, distance="l2", batch_size=bs, float_path="exact", chunk_bytes=chunk),
         gl.ball_counts(queries, bank, eps, batch_size=bs, float_path="exact", chunk_bytes=chunk))
    # a workspace of one tile: 2 query slices x 4 row slices
    set_topk_workspace(ctx, 64 * 64 * 4)
    try:
        same(gl.nearest_neighbours(queries, bank, k, distance="l2", batch_size=bs, float_path="exact"))
        d32, i32 = gl.nearest_neighbours(queries, bank, 32, distance="l2", batch_size=bs, float_path="exact")
        check_lists(d32, i32, M, 32)
    finally:
        set_topk_workspace(ctx, 0)
    # prepared 'f32' Banks on either side
    pb, pq = gl.Bank.from_images(bank, ctx, force_kind="f32"), gl.Bank.from_images(queries, ctx, force_kind="f32")
    assert pb.kind == "f32" and pq.kind == "f32"
    same(gl.nearest_neighbours(pq, pb, k, distance="l2", batch_size=bs, float_path="exact"), gl.ball_counts(pq, pb, eps, batch_size=bs, float_path="exact"))
    same(gl.nearest_neighbours(queries, pb, k, distance="l2", batch_size=bs, float_path="exact"), gl.ball_counts(pq, bank, eps, batch_size=bs, float_path="exact"))
    # two half-banks with index_base, merged on the host; then with an empty third shard
    first = []
    gl.nearest_neighbours(queries, bank[:100], k, distance="l2", float_path="exact", reduce_fn=lambda keys: (first.append(keys.numpy()), keys)[1])
    merged = []
    gl.nearest_neighbours(queries, bank[100:n_eff], k, distance="l2", float_path="exact", index_base=100,
                          reduce_fn=lambda keys: (merged.append(shard.merge_topk_host([first[0], keys.numpy()], k)), keys)[1])
    same(_keys_to_lists(merged[0][:len(queries)]))
    empty = gl.nearest_neighbours(queries, bank[:0], k, distance="l2", float_path="exact", index_base=n_eff,
                                  reduce_fn=lambda keys: ctx.to_device(shard.merge_topk_host([merged[0], keys.numpy()], k)))
    same(empty)
    first_c = []
    gl.ball_counts(queries, bank[:100], eps, float_path="exact", reduce_fn=lambda c: (first_c.append(c.numpy()), c)[1])
    same(counts=gl.ball_counts(queries, bank[100:n_eff], eps, float_path="exact", index_base=100,
                               reduce_fn=lambda c: ctx.to_device(shard.merge_counts_host([first_c[0], c.numpy()]))))
    # two contexts on one device, uneven shards
    with shard.DeviceGroup([0, 0]) as group:
        same(group.nearest_neighbours(queries, bank=bank, k=k, batch_size=bs, distance="l2", weights=[1, 3], float_path="exact"),
             group.ball_counts(queries, bank=bank, eps=eps, batch_size=bs, weights=[1, 3], float_path="exact"))


def test_one_layout_per_call():
    """as soon as either side is off both lattices the whole call runs on decoded fp32 rows"""
    import ganleaks_amd as gl
    queries, bank, bs, n_eff, _ = case("images")
    rng = np.random.default_rng(77)
    q_u8 = rng.integers(0, 256, queries.shape, dtype=np.uint8)
    b_u8 = rng.integers(0, 256, bank.shape, dtype=np.uint8)
    fbank = np.clip(bank * np.float32(0.4), -1.0, 1.0)
    fq = np.clip(queries * np.float32(0.4), -1.0, 1.0)
    # a float bank whose first 100 rows are on the 8-bit lattice: the exact-integer pass gets through two chunks of 50 rows before the third
    # turns out to be off the lattice
    mixed = fbank.copy()
    mixed[:100] = common.decode_u8(b_u8[:100])
    d = 192
    for q_in, b_in, q_f, b_f, kw in ((q_u8, fbank, common.decode_u8(q_u8), fbank, {}),
                                     (fq, b_u8, fq, common.decode_u8(b_u8), {}),
                                     (q_u8, mixed, common.decode_u8(q_u8), mixed, {"chunk_bytes": 50 * 2 * d})):
        M = common.chain_matrix(q_f, b_f[:n_eff])
        for k in (1, 5):
            dist, idx = gl.nearest_neighbours(q_in, b_in, k, distance="l2", batch_size=bs, float_path="exact", **kw)
            check_lists(dist, idx, M, k)
        top1 = gl.attack(q_in, b_in, distance="l2", batch_size=bs, float_path="exact", **kw)
        assert np.array_equal(top1[0], dist[:, 0]) and np.array_equal(top1[1], idx[:, 0])
        eps = radii16(M)
        assert np.array_equal(gl.ball_counts(q_in, b_in, eps, batch_size=bs, float_path="exact", **kw), expect_counts(M, eps))
    # prepared banks: a u8 Bank without its codes cannot be decoded
    ctx = gl.Context.get()
    with pytest.raises(ValueError, match="keep_u8"):
        gl.ball_counts(fq, gl.Bank.from_images(b_u8, ctx), 0.5, batch_size=bs, float_path="exact")
    kept = gl.Bank.from_images(b_u8, ctx, keep_u8=True)
    M = common.chain_matrix(fq, common.decode_u8(b_u8)[:n_eff])
    check_lists(*gl.nearest_neighbours(fq, kept, 5, distance="l2", batch_size=bs, float_path="exact"), M, 5)


def test_unchanged_behaviour():
    import ganleaks_amd as gl
    from ganleaks_amd import shard
    queries, bank, bs, n_eff, _ = case("images")
    rng = np.random.default_rng(78)
    q_u8 = rng.integers(0, 256, queries.shape, dtype=np.uint8)
    b_u8 = rng.integers(0, 256, bank.shape, dtype=np.uint8)
    b_u8[:3] = q_u8[:3]
    eps = [0.0, 0.5, 0.7, -1.0, np.inf]
    # on-lattice inputs: the exact-integer path answers, with or without the keyword (u8 codes, and floats that sit on the lattice)
    for q_in, b_in in ((q_u8, b_u8), (common.decode_u8(q_u8), b_u8)):
        plain, keyed = (gl.nearest_neighbours(q_in, b_in, 5, distance="l2", batch_size=bs, float_path=fp) for fp in (None, "exact"))
        assert np.array_equal(plain[0].view(np.uint32), keyed[0].view(np.uint32)) and np.array_equal(plain[1], keyed[1])
        assert np.array_equal(gl.ball_counts(q_in, b_in, eps, batch_size=bs), gl.ball_counts(q_in, b_in, eps, batch_size=bs, float_path="exact"))
    with shard.DeviceGroup([0, 0]) as group:
        grouped = group.nearest_neighbours(q_u8, bank=b_u8, k=5, batch_size=bs, distance="l2", float_path="exact")
    assert np.array_equal(plain[0].view(np.uint32), grouped[0].view(np.uint32)) and np.array_equal(plain[1], grouped[1])
    # off-lattice rows without the keyword: refused as ever
    for call in (lambda: gl.nearest_neighbours(queries, bank, 5, distance="l2", batch_size=bs),
                 lambda: gl.attack(queries, bank, distance="l2", batch_size=bs, k=5),
                 lambda: gl.attack(queries, bank, distance="l2", batch_size=bs, k=5, float_path="exact"),
                 lambda: gl.ball_counts(queries, bank, 0.5, batch_size=bs),
                 lambda: gl.ball_counts(q_u8, bank, 0.5, batch_size=bs)):
        with pytest.raises(NotImplementedError, match="exact-integer"):
            call()
    for call in (lambda: gl.nearest_neighbours(queries, bank, 5, distance="l2", batch_size=bs, float_path="mfma"),
                 lambda: gl.ball_counts(queries, bank, 0.5, batch_size=bs, float_path="mfma")):
        with pytest.raises(NotImplementedError, match="mfma"):
            call()
    with pytest.raises(ValueError):
        gl.pair_distances(queries, bank, distance="l2", batch_size=bs)


def test_reference_pin(synth, golden_dir):
    """tests/golden/knn_float_rows.npz: the reference's own custom_knn on off-lattice rows.  Indices in every slot of every query; distances
    within twice the stored error (reference against the CPU chain, neither being the code under test)."""
    import ganleaks_amd as gl
    g = np.load(os.path.join(golden_dir, "knn_float_rows.npz"))
    for c in range(int(g["n_cases"])):
        bank, queries, bs = common.derive(synth, str(g["kind%d" % c]), g["params%d" % c])
        dist, idx = gl.nearest_neighbours(queries, bank, int(g["keep"]), distance="l2", batch_size=bs, float_path="exact")
        assert np.array_equal(idx, g["idx%d" % c]), str(g["name%d" % c])
        worst = float(np.max(np.abs(dist.astype(np.float64) - g["dist%d" % c].astype(np.float64))))
        print("%s: largest |device - reference| %.3e, stored error %.3e" % (g["name%d" % c], worst, float(g["err%d" % c])))
        assert worst <= 2.0 * float(g["err%d" % c]), str(g["name%d" % c])


def test_abi_refuses_bad_arguments():
    import ganleaks_amd as gl
    ctx = gl.Context.get()
    lib, h, p = ctx.lib, ctx.handle, ctypes.c_void_p
    rows = ctx.to_device(np.zeros((8, 4), np.float32))
    keys = ctx.empty((8, 32), np.uint64)
    thr = lambda *v: np.asarray(v, np.float32).ctypes.data_as(p)      # noqa: E731

    def expect(rc, text):
        message = lib.gl_last_error().decode()
        assert rc != 0 and text in message, (rc, message)

    expect(lib.gl_l2_topk_f32(h, p(rows.ptr), 8, 0, p(rows.ptr), 8, 4, 33, p(keys.ptr)), "outside [1, 32]")
    expect(lib.gl_l2_topk_f32(h, p(rows.ptr), 8, 0xFFFFFFFF, p(rows.ptr), 8, 4, 5, p(keys.ptr)), "32 bits")
    expect(lib.gl_l2_topk_f32(h, None, 8, 0, p(rows.ptr), 8, 4, 5, p(keys.ptr)), "NULL device pointer")
    expect(lib.gl_l2_count_f32(h, p(rows.ptr), 8, p(rows.ptr), 8, 4, thr(0.5), 17, p(keys.ptr)), "outside [1, 16]")
    expect(lib.gl_l2_count_f32(h, p(rows.ptr), 8, p(rows.ptr), 8, 4, thr(0.5, 0.25), 2, p(keys.ptr)), "ascending")
    expect(lib.gl_l2_count_f32(h, p(rows.ptr), 8, p(rows.ptr), 8, 4, thr(np.nan), 1, p(keys.ptr)), "NaN")
    expect(lib.gl_l2_count_f32(h, p(rows.ptr), 8, p(rows.ptr), 8, 4, thr(0.5), 1, None), "NULL device pointer")
    assert lib.gl_l2_count_f32(h, None, 0, None, 8, 4, thr(0.5), 1, None) == 0 and lib.gl_l2_topk_f32(h, None, 0, 0, None, 8, 4, 5, None) == 0
