"""GPU: the K nearest samples under 'l2-lpips' (nearest_neighbours, lpips.feat_topk_keys, gl_feat_topk*, gl_topk_unpack_f32,
DeviceGroup.nearest_neighbours, attack_models/knn.py).

The chain of evidence: (1) the lists are a stable argsort of the stored matrix M = pair_distances(...), which tests/test_gpu_count_lpips.py
ties to the shipped search bit for bit -- distances and indices compared with array_equal, for every query and every slot; (2) they do not
depend on workspace slices, K-blocked row offsets, chunking, query slicing, sharding, device groups, prepared rows, a mid-stream change
of the row layout or on which persistent kernel ran; (3) the order is the reference's own order on the golden cases, where every gap
between consecutive reference values exceeds twice the per-distance bound, and the distances are within 5e-6 of the fp64 oracle.
Seeded synthetic VGG16 weights and the reference's lin weights, as in tests/test_gpu_count_lpips.py."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_common  # noqa: F401
from test_gpu_count_lpips import _RowsGenerator, _images

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
p = ctypes.c_void_p
ORACLE_BOUND = 5e-6            # |device - fp64 oracle| of an l2-lpips distance at <= 64 x 64 (tests/test_gpu_lpips.py)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def gl():
    import ganleaks_amd
    return ganleaks_amd


@pytest.fixture(scope="module")
def lin(golden_dir):
    z = np.load(os.path.join(golden_dir, "lpips_lin_v0.1.npz"))
    return {"lin%d" % i: z["lin%d" % i] for i in range(5)}


@pytest.fixture(scope="module")
def model(gl, synth, lin):
    from ganleaks_amd.lpips import LpipsModel
    return LpipsModel().load_state_dicts(synth.vgg16_state_dict(7), lin)


def want(M, k):
    """(dist, idx) of the k nearest columns of every row of M, ordered by (value, index)"""
    idx = np.argsort(M, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(M, idx, axis=1), idx.astype(np.int64)


def same(got, M, k):
    wd, wi = want(M, k)
    assert got[0].dtype == np.float32 and got[1].dtype == np.int64 and got[0].shape == got[1].shape == (len(M), k)
    assert np.array_equal(got[1], wi), np.argwhere(got[1] != wi)[:5]
    assert np.array_equal(got[0], wd), np.argwhere(got[0] != wd)[:5]


@pytest.mark.parametrize("nq", [1, 63, 300])
@pytest.mark.parametrize("route", ["u8", "float", "split"])
@pytest.mark.parametrize("res", [16, 64])
def test_lists_are_the_matrix(res, route, nq, gl, synth, oracle, model):
    """resident, ragged: 333 bank images of which batch 30 lets 330 take part (no multiple of 4, 128 or 256: the last piece is ragged),
    two query tiles at nq = 300; lattice rows (u8), hi / lo rows (off-lattice floats) and split rows"""
    bank, q = _images(synth, oracle, 300 + res, 333, nq, res, route)
    model.search_rows = "split" if route == "split" else "fp16"
    kw = dict(batch_size=30, lpips=model)
    try:
        M = gl.pair_distances(q, bank, **kw)
        assert M.shape == (nq, 330)
        top1 = gl.attack(q, bank, distance="l2-lpips", **kw)
        for k in (1, 5, 32):
            dist, idx = gl.nearest_neighbours(q, bank, k, **kw)                  # 'l2-lpips' is the default
            same((dist, idx), M, k)
            assert np.array_equal(dist[:, 0], top1[0]) and np.array_equal(idx[:, 0], top1[1])
            assert np.all(dist[:, :-1] <= dist[:, 1:])
        # an exact tie in D32 goes to the smaller index (M[0, 12] == M[0, 303] is pinned by tests/test_gpu_count_lpips.py)
        assert M[0, 12] == M[0, 303] and idx[0, :2].tolist() == [12, 303]
        # the ball of radius dist[q, j] holds at least j + 1 samples: on the matrix for every query and slot, through ball_counts itself (up
        # to 16 radii per call) for the first and the last query
        for j in range(32):
            assert np.all((M <= dist[:, j:j + 1]).sum(axis=1) >= j + 1)
        picks = [(qi, j) for qi in sorted({0, nq - 1}) for j in (0, 1, 4, 31)]
        counts = gl.ball_counts(q, bank, [dist[qi, j] for qi, j in picks], distance="l2-lpips", **kw)
        for t, (qi, j) in enumerate(picks):
            assert counts[qi, t] >= j + 1, (qi, j, counts[qi, t])
    finally:
        model.search_rows = "fp16"


@pytest.mark.parametrize("route", ["u8", "split"])
def test_workspace_slices(route, gl, synth, oracle, model):
    """a workspace of one tile: 700 rows x 300 queries go in 3 x 2 (fp16 rows, 256) or 6 x 3 (split rows, 128) slices"""
    from ganleaks_amd.attack import set_topk_workspace
    ctx = gl.Context.get()
    bank, q = _images(synth, oracle, 371, 700, 300, 16, route)
    model.search_rows = "split" if route == "split" else "fp16"
    tile = 128 if route == "split" else 256
    kw = dict(batch_size=7, lpips=model)
    try:
        M = gl.pair_distances(q, bank, **kw)
        assert M.shape == (300, 700)
        whole = gl.nearest_neighbours(q, bank, 5, **kw)
        set_topk_workspace(ctx, tile * tile * 4)
        try:
            for k in (1, 5, 32):
                same(gl.nearest_neighbours(q, bank, k, **kw), M, k)
            sliced = gl.nearest_neighbours(q, bank, 5, **kw)
        finally:
            set_topk_workspace(ctx, 0)
        assert np.array_equal(sliced[0], whole[0]) and np.array_equal(sliced[1], whole[1])
        # the integer path shares the selection and its sizing: still its own result
        d2, i2 = gl.attack(q, bank, distance="l2", batch_size=7, k=5)
        d1, i1 = gl.attack(q, bank, distance="l2", batch_size=7)
        assert np.array_equal(d2[:, 0], d1) and np.array_equal(i2[:, 0], i1)
    finally:
        model.search_rows = "fp16"


def test_k_blocked_rows_across_blocks(gl, synth, oracle, model):
    """96 x 96: search rows of 2 MiB and more are stored K-blocked in blocks of 256 rows; with a workspace of one tile the second row slice
    and the second query slice start at block 1 of their buffers"""
    from ganleaks_amd.attack import set_topk_workspace
    ctx = gl.Context.get()
    bank, q = _images(synth, oracle, 396, 300, 260, 96, "u8")
    kw = dict(batch_size=30, lpips=model)
    fb, fq = model.features(bank, role="bank"), model.features(q, role="query")
    assert fb.blocked and fq.blocked
    M = gl.pair_distances(fq, fb, **kw)
    assert M.shape == (260, 300)
    top1 = gl.attack(fq, fb, distance="l2-lpips", **kw)
    set_topk_workspace(ctx, 256 * 256 * 4)
    try:
        for k in (5, 32):
            got = gl.nearest_neighbours(fq, fb, k, **kw)
            same(got, M, k)
            assert np.array_equal(got[0][:, 0], top1[0]) and np.array_equal(got[1][:, 0], top1[1])
        same(gl.nearest_neighbours(q, bank, 5, **kw), M, 5)                      # from the images
    finally:
        set_topk_workspace(ctx, 0)
    same(gl.nearest_neighbours(fq, fb, 5, **kw), M, 5)


@pytest.mark.parametrize("route", ["u8", "float"])
def test_k_blocked_rows(route, gl, synth, oracle, model):
    """128 x 128, 20 bank rows and 4 queries inside one block of 256 (the case of tests/test_gpu_count_lpips.py)"""
    bank, q = _images(synth, oracle, 131, 50, 4, 128, route)
    bank = bank[:23]
    bank[7] = bank[12]
    M = gl.pair_distances(q, bank, batch_size=4, lpips=model)
    got = gl.nearest_neighbours(q, bank, 5, batch_size=4, lpips=model)
    same(got, M, 5)
    assert got[1][0, :2].tolist() == [7, 12]


def test_lists_do_not_depend_on_chunks_slices_shards_or_prepared_rows(gl, synth, oracle, model, lin, monkeypatch):
    from ganleaks_amd import shard
    from ganleaks_amd.attack import GeneratedBank
    from ganleaks_amd.lpips import LpipsModel
    ctx = gl.Context.get()
    bank, q = _images(synth, oracle, 351, 333, 63, 32, "u8")
    bs, n_eff, k = 30, 330, 5
    M = gl.pair_distances(q, bank, batch_size=bs, lpips=model)
    kw = dict(batch_size=bs, lpips=model)
    resident = gl.nearest_neighbours(q, bank, k, **kw)
    same(resident, M, k)

    def equal(got, ref=resident):
        assert np.array_equal(got[1], ref[1]), np.argwhere(got[1] != ref[1])[:5]
        assert np.array_equal(got[0], ref[0])

    row = 2 * int(ctx.lib.gl_lpips_lattice_dim(32, 32))
    # the bank in 4 chunks: an image array, a DeviceArray of images, a GeneratedBank
    equal(gl.nearest_neighbours(q, bank, k, chunk_bytes=100 * row, **kw))
    equal(gl.nearest_neighbours(q, ctx.to_device(bank), k, chunk_bytes=100 * row, **kw))
    gen = GeneratedBank(_RowsGenerator(ctx, bank), np.arange(len(bank)))
    equal(gl.nearest_neighbours(q, gen, k, chunk_bytes=100 * row, **kw))
    # the queries in 4 slices of 20 on top of that
    monkeypatch.setenv("GANLEAKS_QUERY_GB", repr(20.5 * row / (1 << 30)))
    equal(gl.nearest_neighbours(q, bank, k, chunk_bytes=100 * row, **kw))
    equal(gl.nearest_neighbours(q, gen, k, chunk_bytes=100 * row, **kw))
    # reduce_fn fires once per pass over the bank with the key lists of ALL queries, not once per slice
    shapes = []

    def recording(keys):
        shapes.append(tuple(keys.shape))
        return keys

    equal(gl.nearest_neighbours(q, bank[:n_eff], k, chunk_bytes=100 * row, reduce_fn=recording, **kw))    # (a shard is not truncated again)
    assert shapes == [(len(q), k)]
    monkeypatch.delenv("GANLEAKS_QUERY_GB")
    # two shards of the truncated bank: index_base on the second, a world-of-one reduction on the first; merged on the host
    a = gl.nearest_neighbours(q, bank[:150], k, reduce_fn=lambda keys: shard.allreduce_topk_keys(keys, k), **kw)
    b = gl.nearest_neighbours(q, bank[150:n_eff], k, index_base=150, **kw)
    assert a[1].max() < 150 and b[1].min() >= 150
    pack = lambda d, i: (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | i.astype(np.uint64)          # noqa: E731
    merged = shard.merge_topk_host([pack(*a), pack(*b)], k)
    assert np.array_equal((merged >> np.uint64(32)).astype(np.uint32).view(np.float32), resident[0])
    assert np.array_equal((merged & np.uint64(0xFFFFFFFF)).astype(np.int64), resident[1])
    # prepared rows on both sides, and prepared queries against streamed images
    fb, fq = model.features(bank[:n_eff], role="bank"), model.features(q, role="query")
    equal(gl.nearest_neighbours(fq, fb, k, **kw))
    equal(gl.nearest_neighbours(fq, fb, k, batch_size=bs))                              # prepared rows on both sides need no model
    equal(gl.nearest_neighbours(fq, bank, k, chunk_bytes=100 * row, **kw))
    # the refusals
    with pytest.raises(ValueError, match="exceeds"):
        gl.nearest_neighbours(q, bank[:40], 31, **kw)                                   # k > n_eff = 30
    with pytest.raises(ValueError, match="full batch"):
        gl.nearest_neighbours(q, bank[:20], k, **kw)
    with pytest.raises(ValueError, match="distance"):
        gl.nearest_neighbours(q, bank, k, distance="bogus", **kw)
    with pytest.raises(NotImplementedError):
        gl.attack(q, bank, distance="l2-lpips", k=k, **kw)                              # attack(k=) stays exact-integer only
    # distance='l2' is attack(k=)
    l2 = gl.nearest_neighbours(q, bank, k, distance="l2", batch_size=bs)
    equal(l2, gl.attack(q, bank, distance="l2", batch_size=bs, k=k))
    # off-lattice float queries against the 8-bit bank: hi / lo rows on both sides, resident and streamed alike
    qf = np.clip(oracle.dequantize_u8(q) + np.random.default_rng(3).normal(0, 0.01, q.shape).astype(np.float32), -1, 1)
    Mf = gl.pair_distances(qf, bank, batch_size=bs, lpips=model)
    mixed = gl.nearest_neighbours(qf, bank, k, **kw)
    same(mixed, Mf, k)
    hilo_row = 2 * int(ctx.lib.gl_lpips_search_dim(32, 32))
    streamed = gl.nearest_neighbours(qf, bank, k, chunk_bytes=100 * hilo_row, **kw)
    same(streamed, Mf, k)
    # a float bank whose first chunk lies exactly on the 8-bit lattice and whose later rows do not, streamed: the first chunk is searched
    # as lattice rows, the second makes the stream start over in the hi / lo layout -- and the lists with it
    bank_f = oracle.dequantize_u8(bank).astype(np.float32)
    bank_f[100:] = np.clip(bank_f[100:] + np.random.default_rng(4).normal(0, 0.01, bank_f[100:].shape).astype(np.float32), -1, 1)
    whole = gl.nearest_neighbours(q, bank_f, k, **kw)
    same(whole, gl.pair_distances(q, bank_f, batch_size=bs, lpips=model), k)
    restarted = gl.nearest_neighbours(q, bank_f, k, chunk_bytes=100 * row, **kw)
    for r in restarted[1]:
        assert len(set(r.tolist())) == k, r                                             # nothing of the abandoned layout survives
    equal(restarted, whole)
    # a device group of two contexts on one device (host merge), images and generated rows
    make = lambda c: LpipsModel(c).load_state_dicts(synth.vgg16_state_dict(7), lin)                     # noqa: E731
    with shard.DeviceGroup(devices=[0, 0]) as group:
        two = group.nearest_neighbours(q, bank=bank, k=k, batch_size=bs, make_lpips=make)
        uneven = group.nearest_neighbours(q, bank=bank, k=k, batch_size=bs, weights=[1.0, 3.0], make_lpips=make)
        plain = group.nearest_neighbours(q, bank=bank, k=k, batch_size=bs, distance="l2")
        with pytest.raises(ValueError):
            group.nearest_neighbours(q, bank=bank, k=k, batch_size=bs, distance="bogus")
        with pytest.raises(ValueError):
            group.nearest_neighbours(q, bank=bank[:40], k=31, batch_size=bs, make_lpips=make)
        with pytest.raises(NotImplementedError):
            group.attack(q, bank=bank, distance="l2-lpips", batch_size=bs, make_lpips=make, k=k)
    equal(two)
    equal(uneven)
    equal(plain, l2)
    gen2 = shard.nearest_neighbours_on_devices(q, lambda c: _RowsGenerator(c, bank), np.arange(len(bank)), devices=[0, 0], k=k, batch_size=bs,
                                               make_lpips=make)
    equal(gen2)


@pytest.mark.parametrize("name", ["lpips_res32", "lpips_res64"])
def test_order_is_the_reference_order(name, gl, synth, oracle, model, golden_dir):
    """the reference's own matrix R = 0.2 * LPIPS (its PNetLin, tests/golden/make_golden.py) + the exact L2: every gap between consecutive
    sorted values of a row exceeds twice the per-distance bound, so the device's order must be R's for every query and every slot"""
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    case = synth.attack_case(int(g["seed"]), int(g["n_bank"]), int(g["n_pos"]), int(g["n_neg"]), int(g["res"]), sigma=20.0)
    bank, q = case["bank"], np.concatenate([case["pos"], case["neg"]])
    bs = int(g["batch_size"])
    n_eff = (len(bank) // bs) * bs
    assert n_eff == {"lpips_res32": 32, "lpips_res64": 24}[name]
    S = np.stack([oracle.ssd_u8(bank[:n_eff], x) for x in q]).astype(np.int64)
    R = 0.2 * g["lpips"][:, :n_eff].astype(np.float64) + S * (4.0 / (65025.0 * q[0].size))
    gap = float(np.diff(np.sort(R, axis=1), axis=1).min())
    print("smallest gap between consecutive reference values: %.3g" % gap)
    assert gap > 2 * ORACLE_BOUND, gap
    dist, idx = gl.nearest_neighbours(q, bank, n_eff, batch_size=bs, lpips=model)
    order = np.argsort(R, axis=1, kind="stable")
    err = float(np.abs(dist.astype(np.float64) - np.take_along_axis(R, order, axis=1)).max())
    print("max |dist - sorted R| = %.3g" % err)
    assert np.array_equal(idx, order), np.argwhere(idx != order)[:5]
    assert err <= ORACLE_BOUND, err


@pytest.mark.parametrize("route", ["u8", "float"])
def test_lists_against_the_fp64_oracle(route, gl, synth, oracle, model, lin):
    """order statistics move by at most the per-pair error; the distance of the sample named in a slot is within twice of it of the
    oracle's order statistic.  Every slot, nothing left out."""
    import lpips_oracle
    bank, q = _images(synth, oracle, 345, 70, 40, 32, route)
    f = (lambda x: x) if route == "float" else oracle.dequantize_u8
    D, _, _ = lpips_oracle.l2_lpips_matrix(synth.vgg16_state_dict(7), [lin["lin%d" % i] for i in range(5)], f(q), f(bank[:64]))
    k = 8
    dist, idx = gl.nearest_neighbours(q, bank, k, batch_size=16, lpips=model)
    sorted_D = np.sort(D, axis=1)[:, :k]
    e1 = float(np.abs(dist.astype(np.float64) - sorted_D).max())
    e2 = float(np.abs(np.take_along_axis(D, idx, axis=1) - sorted_D).max())
    print("max |dist - sort(D)| = %.3g, max |D[idx] - sort(D)| = %.3g" % (e1, e2))
    assert e1 <= ORACLE_BOUND, e1
    assert e2 <= 2 * ORACLE_BOUND, e2


CHILD = r'''
import ctypes, json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
import ganleaks_amd as gl
from ganleaks_amd import _lib
assert _lib.LIB_PATH.endswith("libganleaks_hip_tuning.so")
ctx = gl.Context.get()
p = ctypes.c_void_p
rng = np.random.default_rng(6)
# fp16 search rows: K = 2 segments + a ragged one (2048 slices of 64 halves per segment); 3 x 3 tiles with ragged edges
K = 64 * (2 * 2048 + 100)
nb, nq, k = 700, 600, 5
bh = (rng.standard_normal((nb, K)) * 40).astype(np.float16)
qh = (rng.standard_normal((nq, K)) * 40).astype(np.float16)
qh[5] = bh[650]
bh[20] = bh[650]
bv, qv = ctx.to_device(bh), ctx.to_device(qh)
bn = ctx.to_device((bh.astype(np.float32) ** 2).sum(1).astype(np.float32) / 16384.0 ** 2)
qn = ctx.to_device((qh.astype(np.float32) ** 2).sum(1).astype(np.float32) / 16384.0 ** 2)
res = {}
for v in (3, 5):
    os.environ["GL_PAIR_VARIANT"] = str(v)
    M = ctx.empty((nq, nb), np.float32)
    _lib.check(ctx.lib.gl_feat_pair_dist_h1_scaled(ctx.handle, p(bv.ptr), p(bn.ptr), nb, p(qv.ptr), p(qn.ptr), nq, K, 16384.0, p(M.ptr), nb))
    t = ctx.empty((nq, k), np.uint64)
    _lib.check(ctx.lib.gl_topk_init(ctx.handle, p(t.ptr), nq, k))
    _lib.check(ctx.lib.gl_feat_topk_h1_scaled(ctx.handle, p(bv.ptr), p(bn.ptr), nb, 0, p(qv.ptr), p(qn.ptr), nq, K, 16384.0, k, p(t.ptr)))
    res[v] = (t.numpy().copy(), M.numpy())
out = {}
for v in (3, 5):
    keys, M = res[v]
    order = np.argsort(M, axis=1, kind="stable")[:, :k]
    d = np.take_along_axis(M, order, axis=1)
    out["lists_are_matrix_%%d" %% v] = bool(np.array_equal(keys, (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | order.astype(np.uint64)))
out["keys_equal"] = bool(np.array_equal(res[3][0], res[5][0]))
out["tie_to_smaller_index"] = bool((res[3][0][5, :2] & np.uint64(0xFFFFFFFF)).tolist() == [20, 650])
print("RESULT " + json.dumps(out))
'''


def test_cluster_and_cluster_free_kernels_list_alike():
    """the two persistent kernels (clusters: a whole MI355X; without: a device with fewer than 256 CUs, forced through the tuning build's
    GL_PAIR_VARIANT=5) on random fp16 rows spanning three K segments: the same key lists, and they are the stored matrix's"""
    tuning = os.path.join(ROOT, "gan-leaks_amd", "libganleaks_hip_tuning.so")
    if not os.path.exists(tuning):
        subprocess.run(["make", "-C", os.path.join(ROOT, "gan-leaks_amd", "csrc"), "-j8", "tuning"], check=True)
    env = dict(os.environ, GANLEAKS_LIB=tuning)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    out = json.loads([l for l in r.stdout.decode().splitlines() if l.startswith("RESULT ")][-1][7:])
    assert all(v is True for v in out.values()), out


def test_c_abi_through_ctypes(gl, synth, model):
    """the three exports called as a foreign host would: every bad argument is an error code with a message and leaves the lists as
    gl_topk_init left them; empty sides are fine; a second call over other rows accumulates"""
    from ganleaks_amd import _lib
    from ganleaks_amd.attack import unpack_topk_f32
    lib = _lib.load()
    ctx = gl.Context.get()
    case = synth.attack_case(361, 40, 3, 2, 16, sigma=20.0)
    h, k = ctx.handle, 5

    def expect(rc, text):
        assert rc == -1, (rc, text)
        assert text.encode() in lib.gl_last_error(), (text, lib.gl_last_error())

    def fresh(nq, kk=k):
        keys = ctx.empty((nq, kk), np.uint64)
        _lib.check(lib.gl_topk_init(h, p(keys.ptr), nq, kk))
        return keys

    for split in (False, True):
        fb = model.features(case["bank"], role=None if split else "bank")
        fq = model.features(case["pos"], role=None if split else "query")
        K, item = fb.K, 4 if split else 2
        keys = fresh(fq.n)

        def topk(ctx_h=h, bank=fb.V.ptr, bnorm=fb.norms.ptr, n=fb.n, base=0, query=fq.V.ptr, nq=fq.n, K=K, kk=k, out=keys):
            o = p(out.ptr) if out is not None else None
            if split:
                return lib.gl_feat_topk(ctx_h, p(bank) if bank else None, p(bnorm), n, base, p(query), p(fq.norms.ptr), nq, K, kk, o)
            return lib.gl_feat_topk_h1_scaled(ctx_h, p(bank) if bank else None, p(bnorm), n, base, p(query), p(fq.norms.ptr), nq, K, fb.scale, kk, o)

        expect(topk(ctx_h=None), "NULL ctx")
        expect(topk(kk=0), "outside [1, 32]")
        expect(topk(kk=33), "outside [1, 32]")
        expect(topk(K=K + 8), "multiple of %d" % (32 if split else 64))
        expect(topk(bank=fb.V.ptr + 2), "16-byte aligned")
        expect(topk(bank=None), "NULL device pointer")
        expect(topk(base=(1 << 32) - fb.n + 1), "index bits")
        expect(topk(base=-1), "index bits")
        expect(topk(out=None), "NULL key lists")
        if not split:
            expect(lib.gl_feat_topk_h1_scaled(h, p(fb.V.ptr), p(fb.norms.ptr), fb.n, 0, p(fq.V.ptr), p(fq.norms.ptr), fq.n, K, 0.0, k, p(keys.ptr)), "row scale")
        ctx.sync()
        assert np.all(keys.numpy() == EMPTY)                            # the refused calls folded nothing in
        assert topk(n=0) == 0 and topk(nq=0) == 0, lib.gl_last_error()
        ctx.sync()
        assert np.all(keys.numpy() == EMPTY)
        # the largest index base that fits is accepted
        top = fresh(fq.n)
        assert topk(base=(1 << 32) - fb.n, out=top) == 0, lib.gl_last_error()
        assert int(top.numpy()[0, 0] & np.uint64(0xFFFFFFFF)) >= (1 << 32) - fb.n
        # one call over all rows = a call over rows [0, 25) and one over rows [25, 40) with their index base
        assert topk() == 0, lib.gl_last_error()
        parts = fresh(fq.n)
        assert topk(n=25, out=parts) == 0, lib.gl_last_error()
        assert topk(bank=fb.V.ptr + 25 * K * item, bnorm=fb.norms.ptr + 25 * 4, n=fb.n - 25, base=25, out=parts) == 0, lib.gl_last_error()
        ctx.sync()
        assert np.array_equal(parts.numpy(), keys.numpy())
        from ganleaks_amd.lpips import feat_pair_dist
        M = feat_pair_dist(fb, fq)
        dist, idx = unpack_topk_f32(ctx, keys, fq.n, k)
        same((dist, idx), M, k)
    # unpack: an empty slot gives +inf and -1; a list longer than the bank keeps its tail empty
    wide = fresh(fq.n, 32)
    dist, idx = unpack_topk_f32(ctx, wide, fq.n, 32)
    assert np.all(np.isposinf(dist)) and np.all(idx == -1)
    expect(lib.gl_topk_unpack_f32(None, p(wide.ptr), fq.n, 32, None, None), "bad ctx")
    expect(lib.gl_topk_unpack_f32(h, p(wide.ptr), fq.n, 33, None, None), "outside [1, 32]")
    expect(lib.gl_topk_unpack_f32(h, p(wide.ptr), fq.n, 32, None, None), "NULL device pointer")


def test_knn_main(tmp_path, monkeypatch, gl, synth, lin, model):
    """attack_models/knn.py on PNG directories with local synthetic weights; --K 1 writes fbb.py's pos_loss.npy"""
    import torch
    import PIL.Image
    from ganleaks_amd import lpips
    from ganleaks_amd.attack_models import eval_roc, fbb, knn, utils
    torch.save({"features.%s" % k: torch.from_numpy(v) for k, v in synth.vgg16_state_dict(7).items()}, tmp_path / "vgg16.pth")
    torch.save({"lin%d.model.1.weight" % i: torch.from_numpy(lin["lin%d" % i]).view(1, -1, 1, 1) for i in range(5)}, tmp_path / "vgg_lin.pth")
    monkeypatch.setenv("GANLEAKS_VGG16_PATH", str(tmp_path / "vgg16.pth"))
    monkeypatch.setenv("GANLEAKS_LPIPS_LIN_PATH", str(tmp_path / "vgg_lin.pth"))
    lpips.set_default_model(None)
    case = synth.attack_case(195, 75, 13, 11, 32, sigma=20.0)              # 75 is not a multiple of BATCH_SIZE 16: 64 rows take part
    for name in ("bank", "pos", "neg"):
        os.makedirs(tmp_path / name)
        for j, im in enumerate(case[name]):
            PIL.Image.fromarray(im.transpose(1, 2, 0)).save(tmp_path / name / ("image_%d.png" % j))
    monkeypatch.chdir(tmp_path)
    base = ["--syn_data_path", str(tmp_path / "bank"), "--pos_data_dir", str(tmp_path / "pos"), "--neg_data_dir", str(tmp_path / "neg"),
            "--resolution", "32", "--BATCH_SIZE", "16"]
    # refused before any file is read, nothing written
    for bad in (["--K", "0"], ["--K", "33"]):
        with pytest.raises(SystemExit):
            knn.main(knn.parse_arguments(base + ["--exp_name", "bad"] + bad))
    with pytest.raises(SystemExit):
        knn.parse_arguments(base + ["--exp_name", "bad", "--distance", "cosine"])
    args = knn.parse_arguments(base + ["--exp_name", "bad"])
    args.distance = "cosine"                                               # as a YAML overlay could set it
    with pytest.raises(SystemExit):
        knn.main(args)
    assert not os.path.exists(tmp_path / "knn_attack")
    try:
        knn.main(knn.parse_arguments(base + ["--exp_name", "lp"]))                                         # --K 5, l2-lpips
        knn.main(knn.parse_arguments(base + ["--exp_name", "lp2", "--devices", "0,0"]))
        knn.main(knn.parse_arguments(base + ["--exp_name", "one", "--K", "1", "--distance", "l2-lpips"]))
        knn.main(knn.parse_arguments(base + ["--exp_name", "l2", "--K", "7", "--distance", "l2"]))
        fbb.main(fbb.parse_arguments(base + ["--exp_name", "ref"]))
    finally:
        lpips.set_default_model(None)
    files = ("pos_knn_loss.npy", "neg_knn_loss.npy", "pos_knn_idx.npy", "neg_knn_idx.npy", "pos_loss.npy", "neg_loss.npy")
    out = {n: tmp_path / "knn_attack" / n for n in ("lp", "lp2", "one", "l2")}
    for d in out.values():
        assert sorted(os.listdir(d)) == sorted(files + ("params.txt",)), os.listdir(d)
    assert "distance:l2-lpips" in open(out["lp"] / "params.txt").read().splitlines() and "K:5" in open(out["lp"] / "params.txt").read().splitlines()
    for f in files:
        assert open(out["lp"] / f, "rb").read() == open(out["lp2"] / f, "rb").read(), f              # the sharded run, byte for byte

    order = lambda name: [int(os.path.basename(x)[6:-4]) for x in utils.get_filepaths_from_dir(str(tmp_path / name), "png")]   # noqa: E731
    bank = case["bank"][order("bank")]
    queries = np.concatenate([case["pos"][order("pos")], case["neg"][order("neg")]])
    n_pos = 13
    M = gl.pair_distances(queries, bank, batch_size=16, lpips=model)
    for name, K, ref in (("lp", 5, want(M, 5)), ("one", 1, want(M, 1)), ("l2", 7, gl.attack(queries, bank, distance="l2", batch_size=16, k=7))):
        for kind, sl in (("pos", slice(0, n_pos)), ("neg", slice(n_pos, None))):
            d, i, loss = (np.load(out[name] / (kind + suffix)) for suffix in ("_knn_loss.npy", "_knn_idx.npy", "_loss.npy"))
            assert d.dtype == np.float64 and d.shape == (len(queries[sl]), K) and np.array_equal(d, ref[0][sl].astype(np.float64)), (name, kind)
            assert i.dtype == np.int64 and i.shape == d.shape and np.array_equal(i, ref[1][sl]), (name, kind)
            assert loss.dtype == np.float64 and loss.shape == (len(d), 1) and np.array_equal(loss, d.mean(axis=1, keepdims=True))
    for f in ("pos_loss.npy", "neg_loss.npy"):
        assert open(out["one"] / f, "rb").read() == open(tmp_path / "fbb_attack" / "ref" / f, "rb").read(), f
    auc, ap, precision = eval_roc.main(eval_roc.parse_arguments(["--attack_type", "fbb", "-ldir", str(out["lp"])]))
    assert auc == eval_roc.plot_roc(-np.load(out["lp"] / "pos_loss.npy")[:, 0], -np.load(out["lp"] / "neg_loss.npy")[:, 0])[3]
