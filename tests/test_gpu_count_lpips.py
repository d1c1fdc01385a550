"""GPU: epsilon-ball counts and the stored distance matrix under 'l2-lpips' (ball_counts(distance='l2-lpips'), pair_distances,
lpips.feat_count / feat_pair_dist, gl_feat_count* / gl_feat_pair_dist*).

The chain of evidence: (1) the stored matrix M is tied to the shipped search -- its row minimum and first argmin ARE attack()'s (dist, idx),
bit for bit; (2) the counts are exactly (M <= float32(eps)).sum(axis=1); (3) M is within the bound of tests/test_gpu_lpips.py (5e-6) of the
fp64 oracle 0.2 * lpips_matrix + L2, and the counts lie between the oracle's counts at eps -+ that bound; (4) the counts do not depend on
chunking, query slicing, sharding, device groups, prepared rows or on which persistent kernel ran.  Seeded synthetic VGG16 weights and the
reference's lin weights, as in tests/test_gpu_lpips.py.  Every query is checked; counts are compared with array_equal."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_common  # noqa: F401
from test_gpu_count import eps_sets, oracle_counts

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
p = ctypes.c_void_p
ORACLE_BOUND = 5e-6            # |device - fp64 oracle| of an l2-lpips distance at <= 64 x 64 (tests/test_gpu_lpips.py)


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


def _images(synth, oracle, seed, n_bank, nq, res, route):
    """bank and queries with an exact duplicate of bank row 12 among the queries (the first) and in the bank (row n_bank - 30);
    route 'float': off the 8-bit lattice on both sides (hi / lo rows)"""
    case = synth.attack_case(seed, n_bank, max(nq - nq // 2, 1), max(nq // 2, 1), res, sigma=20.0)
    bank, q = case["bank"].copy(), np.concatenate([case["pos"], case["neg"]])[:nq].copy()
    if route == "float":
        rng = np.random.default_rng(seed)
        bank = np.clip(oracle.dequantize_u8(bank) + rng.normal(0, 0.01, bank.shape).astype(np.float32), -1, 1)
        q = np.clip(oracle.dequantize_u8(q) + rng.normal(0, 0.01, q.shape).astype(np.float32), -1, 1)
    bank[n_bank - 30] = bank[12]
    q[0] = bank[12]
    return bank, q


def _tie_and_count(gl, model, q, bank, batch_size, n_eff):
    """checks 1 and 2 for one case; returns M"""
    M = gl.pair_distances(q, bank, batch_size=batch_size, lpips=model)
    assert M.dtype == np.float32 and M.shape == (len(q), n_eff)
    dist, idx = gl.attack(q, bank, distance="l2-lpips", batch_size=batch_size, lpips=model)
    assert np.array_equal(M.min(axis=1), dist), np.argwhere(M.min(axis=1) != dist)[:5]
    assert np.array_equal(M.argmin(axis=1), idx)                      # numpy's argmin is the first one, attack()'s the smallest index
    for eps in eps_sets(M):
        got = gl.ball_counts(q, bank, eps, batch_size=batch_size, distance="l2-lpips", lpips=model)
        assert got.dtype == np.int64 and got.shape == (len(q), len(eps))
        want = oracle_counts(M, eps)
        assert np.array_equal(got, want), (len(eps), np.argwhere(got != want)[:5])
        e32 = np.asarray(eps, np.float64).astype(np.float32)
        assert np.array_equal(got >= 1, dist[:, None] <= e32[None, :])
        assert np.all(got[:, e32 < 0] == 0) and np.all(got[:, np.isinf(e32)] == n_eff)
    return M


@pytest.mark.parametrize("nq", [1, 63, 300])
@pytest.mark.parametrize("route", ["u8", "float", "split"])
@pytest.mark.parametrize("res", [16, 32, 64])
def test_matrix_is_the_search_and_counts_are_the_matrix(res, route, nq, gl, synth, oracle, model):
    """resident, ragged: 333 bank images of which batch 30 lets 330 take part (no multiple of a 128 or 256 tile); lattice rows (u8), hi / lo
    rows (off-lattice floats) and split rows"""
    bank, q = _images(synth, oracle, 300 + res, 333, nq, res, route)
    model.search_rows = "split" if route == "split" else "fp16"
    try:
        M = _tie_and_count(gl, model, q, bank, 30, 330)
    finally:
        model.search_rows = "fp16"
    # the duplicate pair is one value, wherever its rows sit in a tile (not required to be 0)
    assert M[0, 12] == M[0, 303] == M[0].min()


@pytest.mark.parametrize("route", ["u8", "float"])
def test_counts_bracketed_by_the_fp64_oracle(route, gl, synth, oracle, model, lin):
    import lpips_oracle
    bank, q = _images(synth, oracle, 345, 70, 40, 32, route)
    f = (lambda x: x) if route == "float" else oracle.dequantize_u8
    D, _, _ = lpips_oracle.l2_lpips_matrix(synth.vgg16_state_dict(7), [lin["lin%d" % i] for i in range(5)], f(q), f(bank[:64]))
    M = gl.pair_distances(q, bank, batch_size=16, lpips=model)
    err = float(np.abs(M.astype(np.float64) - D).max())
    print("max |M - D| = %.3g" % err)
    assert err <= ORACLE_BOUND, err
    # radii between attained values (linear-interpolated quantiles of D): the bracket is then tight except where a pair sits within the
    # bound of a radius
    eps = [float(np.quantile(D, v)) for v in (0.002, 0.01, 0.03, 0.1, 0.2, 0.35, 0.5, 0.65, 0.8, 0.9, 0.97, 0.995)]
    eps += [float(np.quantile(D.min(axis=1), v)) for v in (0.25, 0.5, 0.75)] + [float(D.max()) + 1.0]
    got = gl.ball_counts(q, bank, eps, batch_size=16, distance="l2-lpips", lpips=model)
    lo = np.stack([(D <= e - ORACLE_BOUND).sum(axis=1) for e in eps], axis=1)
    hi = np.stack([(D <= e + ORACLE_BOUND).sum(axis=1) for e in eps], axis=1)
    assert np.all(lo <= got) and np.all(got <= hi), np.argwhere((got < lo) | (got > hi))[:5]
    loose = float((lo != hi).mean())
    print("oracle bounds differ in %.2f %% of the cells" % (100 * loose))
    assert loose <= 0.05, loose
    assert np.all(got[:, -1] == 64)


class _RowsGenerator:
    def __init__(self, ctx, bank):
        self.ctx, self.bank = ctx, bank

    def generate_u8(self, z):
        return self.ctx.to_device(self.bank[np.asarray(z)])


def test_counts_do_not_depend_on_chunks_slices_shards_or_prepared_rows(gl, synth, oracle, model, lin, monkeypatch):
    from ganleaks_amd import shard
    from ganleaks_amd.attack import GeneratedBank
    from ganleaks_amd.lpips import LpipsModel
    ctx = gl.Context.get()
    bank, q = _images(synth, oracle, 351, 333, 63, 32, "u8")
    bs, n_eff = 30, 330
    M = gl.pair_distances(q, bank, batch_size=bs, lpips=model)
    eps = eps_sets(M)[2]
    kw = dict(batch_size=bs, distance="l2-lpips", lpips=model)
    resident = gl.ball_counts(q, bank, eps, **kw)
    assert np.array_equal(resident, oracle_counts(M, eps))
    row = 2 * int(ctx.lib.gl_lpips_lattice_dim(32, 32))
    # the bank in 4 chunks: an image array, a DeviceArray of images, a GeneratedBank
    assert np.array_equal(gl.ball_counts(q, bank, eps, chunk_bytes=100 * row, **kw), resident)
    assert np.array_equal(gl.ball_counts(q, ctx.to_device(bank), eps, chunk_bytes=100 * row, **kw), resident)
    gen = GeneratedBank(_RowsGenerator(ctx, bank), np.arange(len(bank)))
    assert np.array_equal(gl.ball_counts(q, gen, eps, chunk_bytes=100 * row, **kw), resident)
    # the queries in 4 slices of 20 on top of that
    monkeypatch.setenv("GANLEAKS_QUERY_GB", repr(20.5 * row / (1 << 30)))
    assert np.array_equal(gl.ball_counts(q, bank, eps, chunk_bytes=100 * row, **kw), resident)
    assert np.array_equal(gl.ball_counts(q, gen, eps, chunk_bytes=100 * row, **kw), resident)
    # reduce_fn fires once per pass over the bank with the counters of ALL queries, not once per slice
    shapes = []

    def recording(counts):
        shapes.append(tuple(counts.shape))
        return counts

    sliced = gl.ball_counts(q, bank[:n_eff], eps, chunk_bytes=100 * row, reduce_fn=recording, **kw)    # (a shard is not truncated again)
    assert shapes == [(len(q), len(eps))]
    assert np.array_equal(sliced, resident)
    monkeypatch.delenv("GANLEAKS_QUERY_GB")
    # two shards of the truncated bank: index_base on the second, a world-of-one reduction on the first
    a = gl.ball_counts(q, bank[:150], eps, reduce_fn=shard.allreduce_sum_counts, **kw)
    b = gl.ball_counts(q, bank[150:n_eff], eps, index_base=150, **kw)
    assert np.array_equal(a + b, resident)
    # prepared rows on both sides, and prepared queries against streamed images
    fb, fq = model.features(bank[:n_eff], role="bank"), model.features(q, role="query")
    assert np.array_equal(gl.ball_counts(fq, fb, eps, **kw), resident)
    assert np.array_equal(gl.ball_counts(fq, bank, eps, chunk_bytes=100 * row, **kw), resident)
    assert np.array_equal(gl.pair_distances(fq, fb, batch_size=bs), M)
    with pytest.raises(NotImplementedError):
        gl.ball_counts(fq, fb, eps, batch_size=bs)                     # 'l2' on feature rows stays refused
    with pytest.raises(ValueError):
        gl.ball_counts(q, bank[:20], eps, **kw)                        # no full batch
    # off-lattice float queries against the 8-bit bank: hi / lo rows on both sides, resident and streamed alike
    qf = np.clip(oracle.dequantize_u8(q) + np.random.default_rng(3).normal(0, 0.01, q.shape).astype(np.float32), -1, 1)
    Mf = gl.pair_distances(qf, bank, batch_size=bs, lpips=model)
    mixed = gl.ball_counts(qf, bank, eps, **kw)
    assert np.array_equal(mixed, oracle_counts(Mf, eps))
    assert np.array_equal(gl.ball_counts(qf, bank, eps, chunk_bytes=100 * 2 * int(ctx.lib.gl_lpips_search_dim(32, 32)), **kw), mixed)
    # a device group of two contexts on one device (host merge), images and generated rows
    make = lambda c: LpipsModel(c).load_state_dicts(synth.vgg16_state_dict(7), lin)                     # noqa: E731
    with shard.DeviceGroup(devices=[0, 0]) as group:
        two = group.ball_counts(q, bank=bank, eps=eps, batch_size=bs, distance="l2-lpips", make_lpips=make)
        uneven = group.ball_counts(q, bank=bank, eps=eps, batch_size=bs, weights=[1.0, 3.0], distance="l2-lpips", make_lpips=make)
        d2, i2 = group.attack(q, bank=bank, distance="l2-lpips", batch_size=bs, make_lpips=make)
        plain = group.ball_counts(q, bank=bank, eps=0.01, batch_size=bs)                                 # the default is still 'l2'
        with pytest.raises(ValueError):
            group.ball_counts(q, bank=bank, eps=eps, batch_size=bs, distance="bogus")
    assert two.dtype == np.int64 and np.array_equal(two, resident) and np.array_equal(uneven, resident)
    assert np.array_equal(d2, M.min(axis=1)) and np.array_equal(i2, M.argmin(axis=1))
    assert np.array_equal(plain, gl.ball_counts(q, bank, 0.01, batch_size=bs))
    gen2 = shard.ball_counts_on_devices(q, lambda c: _RowsGenerator(c, bank), np.arange(len(bank)), devices=[0, 0], eps=eps, batch_size=bs,
                                        distance="l2-lpips", make_lpips=make)
    assert np.array_equal(gen2, resident)


@pytest.mark.parametrize("route", ["u8", "float"])
def test_k_blocked_rows(route, gl, synth, oracle, model):
    """128 x 128: a search row is 4.1 MB (lattice) / 4.3 MB (hi / lo), stored K-blocked; 20 bank rows and 4 queries, inside one block of 256"""
    bank, q = _images(synth, oracle, 131, 50, 4, 128, route)
    bank = bank[:23]
    bank[7] = bank[12]
    fb = model.features(bank[:20], role="bank")
    assert fb.blocked and fb.fmt == ("lattice" if route == "u8" else "hilo")
    M = _tie_and_count(gl, model, q, bank, 4, 20)
    assert M[0, 12] == M[0, 7] == M[0].min()


def test_mc_main_with_l2_lpips(tmp_path, monkeypatch, gl, synth, lin, model):
    """attack_models/mc.py --distance l2-lpips on PNG directories with local synthetic weights; the run without the flag is the 'l2' run"""
    import torch
    import PIL.Image
    from ganleaks_amd import lpips
    from ganleaks_amd.attack_models import eval_roc, mc, utils
    torch.save({"features.%s" % k: torch.from_numpy(v) for k, v in synth.vgg16_state_dict(7).items()}, tmp_path / "vgg16.pth")
    torch.save({"lin%d.model.1.weight" % i: torch.from_numpy(lin["lin%d" % i]).view(1, -1, 1, 1) for i in range(5)}, tmp_path / "vgg_lin.pth")
    monkeypatch.setenv("GANLEAKS_VGG16_PATH", str(tmp_path / "vgg16.pth"))
    monkeypatch.setenv("GANLEAKS_LPIPS_LIN_PATH", str(tmp_path / "vgg_lin.pth"))
    lpips.set_default_model(None)
    case = synth.attack_case(195, 75, 13, 11, 32, sigma=20.0)              # 75 is not a multiple of BATCH_SIZE 16: 64 rows take part
    for name in ("bank", "pos", "neg"):
        os.makedirs(tmp_path / name)
        for k, im in enumerate(case[name]):
            PIL.Image.fromarray(im.transpose(1, 2, 0)).save(tmp_path / name / ("image_%d.png" % k))
    monkeypatch.chdir(tmp_path)
    base = ["--syn_data_path", str(tmp_path / "bank"), "--pos_data_dir", str(tmp_path / "pos"), "--neg_data_dir", str(tmp_path / "neg"),
            "--resolution", "32", "--BATCH_SIZE", "16"]
    quantiles = (0.9, 0.1, 0.5)
    try:
        mc.main(mc.parse_arguments(base + ["--exp_name", "lp", "--distance", "l2-lpips", "--eps_quantile", "0.9,0.1,0.5"]))
        mc.main(mc.parse_arguments(base + ["--exp_name", "lp2", "--distance", "l2-lpips", "--eps_quantile", "0.9,0.1,0.5", "--devices", "0,0"]))
        mc.main(mc.parse_arguments(base + ["--exp_name", "lpfixed", "--distance", "l2-lpips", "--eps", "0.05,-1,1e9"]))
        mc.main(mc.parse_arguments(base + ["--exp_name", "plain", "--eps_quantile", "0.9,0.1,0.5"]))
        mc.main(mc.parse_arguments(base + ["--exp_name", "plain_l2", "--distance", "l2", "--eps_quantile", "0.9,0.1,0.5"]))
    finally:
        lpips.set_default_model(None)
    files = ("eps.npy", "pos_count.npy", "neg_count.npy", "pos_mc.npy", "neg_mc.npy", "pos_loss.npy", "neg_loss.npy")
    out = {n: tmp_path / "mc_attack" / n for n in ("lp", "lp2", "lpfixed", "plain", "plain_l2")}
    for d in out.values():
        assert sorted(os.listdir(d)) == sorted(files + ("params.txt",)), os.listdir(d)
    assert "distance:l2-lpips" in open(out["lp"] / "params.txt").read().splitlines()
    for f in files:
        assert open(out["lp"] / f, "rb").read() == open(out["lp2"] / f, "rb").read(), f              # the sharded run, byte for byte
        assert open(out["plain"] / f, "rb").read() == open(out["plain_l2"] / f, "rb").read(), f      # no flag = 'l2'

    order = lambda name: [int(os.path.basename(x)[6:-4]) for x in utils.get_filepaths_from_dir(str(tmp_path / name), "png")]   # noqa: E731
    bank = case["bank"][order("bank")]
    queries = np.concatenate([case["pos"][order("pos")], case["neg"][order("neg")]])
    n_pos, n_eff = 13, 64
    # without the flag: what the 'l2' entry points give on the same inputs (the parent's behaviour, pinned by tests/test_gpu_cli_mc.py)
    d_l2 = gl.attack(queries, bank, distance="l2", batch_size=16)[0]
    eps_l2 = np.asarray([np.quantile(d_l2, v, method="lower") for v in quantiles], np.float32)
    c_l2 = gl.ball_counts(queries, bank, eps_l2, batch_size=16)
    assert np.array_equal(np.load(out["plain"] / "eps.npy"), eps_l2)
    assert np.array_equal(np.load(out["plain"] / "pos_count.npy"), c_l2[:n_pos]) and np.array_equal(np.load(out["plain"] / "neg_count.npy"), c_l2[n_pos:])
    # with it: radii = the stated quantiles of attack()'s l2-lpips distances, scores = ball_counts / n_eff
    dist = gl.attack(queries, bank, distance="l2-lpips", batch_size=16, lpips=model)[0]
    M = gl.pair_distances(queries, bank, batch_size=16, lpips=model)
    for name, eps in (("lp", np.asarray([np.quantile(dist, v, method="lower") for v in quantiles], np.float32)),
                      ("lpfixed", np.asarray([0.05, -1, 1e9], np.float32))):
        got_eps = np.load(out[name] / "eps.npy")
        assert got_eps.dtype == np.float32 and np.array_equal(got_eps, eps), name
        want = gl.ball_counts(queries, bank, eps, batch_size=16, distance="l2-lpips", lpips=model)
        assert np.array_equal(want, oracle_counts(M, eps))
        for kind, sl in (("pos", slice(0, n_pos)), ("neg", slice(n_pos, None))):
            count, score, loss = (np.load(out[name] / (kind + suffix)) for suffix in ("_count.npy", "_mc.npy", "_loss.npy"))
            assert count.dtype == np.int64 and np.array_equal(count, want[sl]), (name, kind)
            assert score.dtype == np.float64 and np.array_equal(score, want[sl] / float(n_eff))
            assert loss.shape == (len(count), 1) and np.array_equal(loss, -score[:, :1])
    assert not np.array_equal(np.load(out["lp"] / "eps.npy"), eps_l2)
    assert np.all(np.load(out["lpfixed"] / "pos_count.npy")[:, 1] == 0) and np.all(np.load(out["lpfixed"] / "neg_count.npy")[:, 2] == n_eff)
    auc, ap, precision = eval_roc.main(eval_roc.parse_arguments(["--attack_type", "fbb", "-ldir", str(out["lp"])]))
    assert auc == eval_roc.plot_roc(np.load(out["lp"] / "pos_mc.npy")[:, 0], np.load(out["lp"] / "neg_mc.npy")[:, 0])[3]


def test_bad_arguments_through_ctypes(gl, synth, model):
    """the four exports called as a foreign host would: every bad argument is an error code with a message, nothing is launched"""
    from ganleaks_amd import _lib
    from ganleaks_amd.attack import new_counts
    lib = _lib.load()
    ctx = gl.Context.get()
    case = synth.attack_case(361, 40, 3, 2, 16, sigma=20.0)
    h = ctx.handle
    thr = (ctypes.c_float * 3)(0.1, 0.2, 0.3)

    def expect(rc, text):
        assert rc == -1, (rc, text)
        assert text.encode() in lib.gl_last_error(), (text, lib.gl_last_error())

    for split in (False, True):
        fb = model.features(case["bank"], role=None if split else "bank")
        fq = model.features(case["pos"], role=None if split else "query")
        K, counts = fb.K, new_counts(ctx, fq.n, 3)
        out = ctx.empty((fq.n, fb.n), np.float32)
        rows = (p(fb.V.ptr), p(fb.norms.ptr), fb.n, p(fq.V.ptr), p(fq.norms.ptr), fq.n)

        def count(rows=rows, K=K, t=thr, n=3, col0=0, pitch=3, c=counts):
            if split:
                return lib.gl_feat_count(h, *rows, K, t, n, col0, pitch, p(c.ptr) if c is not None else None)
            return lib.gl_feat_count_h1_scaled(h, *rows, K, fb.scale, t, n, col0, pitch, p(c.ptr) if c is not None else None)

        def store(rows=rows, K=K, o=out, ld=None):
            ld = fb.n if ld is None else ld
            if split:
                return lib.gl_feat_pair_dist(h, *rows, K, p(o.ptr) if o is not None else None, ld)
            return lib.gl_feat_pair_dist_h1_scaled(h, *rows, K, fb.scale, p(o.ptr) if o is not None else None, ld)

        assert count() == 0 and store() == 0, lib.gl_last_error()
        before = counts.numpy().copy()
        for fn in (count, store):
            expect(fn(rows=(None,) + rows[1:]), "NULL device pointer")
            expect(fn(rows=rows[:4] + (None, fq.n)), "NULL device pointer")
            expect(fn(K=K + 8), "multiple of %d" % (32 if split else 64))
            expect(fn(K=0), "bad sizes")
            expect(fn(rows=(p(fb.V.ptr + 2),) + rows[1:]), "16-byte aligned")
            expect(fn(rows=rows[:2] + (-1,) + rows[3:]), "bad sizes")
        expect(count(c=None), "NULL counters")
        expect(count(t=None), "NULL thresholds")
        expect(count(n=0), "outside [1, 16]")
        expect(count(n=17), "outside [1, 16]")
        expect(count(t=(ctypes.c_float * 3)(0.3, 0.2, 0.4)), "ascending")
        expect(count(t=(ctypes.c_float * 3)(-0.1, 0.2, 0.4)), "non-negative")
        expect(count(t=(ctypes.c_float * 3)(0.1, float("nan"), 0.4)), "NaN")
        expect(count(col0=1), "do not fit")
        expect(count(col0=-1, pitch=3), "do not fit")
        expect(count(pitch=17), "do not fit")
        expect(store(o=None), "NULL output")
        expect(store(ld=fb.n - 1), "shorter than a row")
        if not split:
            expect(lib.gl_feat_count_h1_scaled(h, *rows, K, 0.0, thr, 3, 0, 3, p(counts.ptr)), "row scale")
            expect(lib.gl_feat_pair_dist_h1_scaled(h, *rows, K, -1.0, p(out.ptr), fb.n), "row scale")
        expect(lib.gl_feat_count(None, *rows, K, thr, 3, 0, 3, p(counts.ptr)) if split else
               lib.gl_feat_count_h1_scaled(None, *rows, K, fb.scale, thr, 3, 0, 3, p(counts.ptr)), "NULL ctx")
        ctx.sync()
        assert np.array_equal(counts.numpy(), before)                   # the refused calls counted nothing
        # empty sides are fine and touch nothing; +inf is a threshold like any other
        assert count(rows=rows[:2] + (0,) + rows[3:]) == 0 and count(rows=rows[:5] + (0,)) == 0
        assert np.array_equal(counts.numpy(), before)
        inf = new_counts(ctx, fq.n, 3)
        assert count(t=(ctypes.c_float * 2)(0.0, float("inf")), n=2, col0=1, c=inf) == 0, lib.gl_last_error()
        got = inf.numpy()[:fq.n]
        assert np.all(got[:, 0] == 0) and np.all(got[:, 2] == fb.n)


CHILD = r'''
import ctypes, json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
import ganleaks_amd as gl
from ganleaks_amd import _lib
from ganleaks_amd.attack import new_counts
assert _lib.LIB_PATH.endswith("libganleaks_hip_tuning.so")
ctx = gl.Context.get()
p = ctypes.c_void_p
rng = np.random.default_rng(6)
# fp16 search rows: K = 2 segments + a ragged one (2048 slices of 64 halves per segment); 3 x 3 tiles with ragged edges
K = 64 * (2 * 2048 + 100)
nb, nq = 700, 600
bh = (rng.standard_normal((nb, K)) * 40).astype(np.float16)
qh = (rng.standard_normal((nq, K)) * 40).astype(np.float16)
qh[5] = bh[650]
bv, qv = ctx.to_device(bh), ctx.to_device(qh)
bn = ctx.to_device((bh.astype(np.float32) ** 2).sum(1).astype(np.float32) / 16384.0 ** 2)
qn = ctx.to_device((qh.astype(np.float32) ** 2).sum(1).astype(np.float32) / 16384.0 ** 2)
res = {}
for v in (3, 5):
    os.environ["GL_PAIR_VARIANT"] = str(v)
    k = ctx.empty((nq,), np.uint64)
    _lib.check(ctx.lib.gl_keys_init(ctx.handle, p(k.ptr), nq))
    _lib.check(ctx.lib.gl_feat_knn_h1_scaled(ctx.handle, p(bv.ptr), p(bn.ptr), nb, 0, p(qv.ptr), p(qn.ptr), nq, K, p(k.ptr), 16384.0))
    M = ctx.empty((nq, nb), np.float32)
    _lib.check(ctx.lib.gl_feat_pair_dist_h1_scaled(ctx.handle, p(bv.ptr), p(bn.ptr), nb, p(qv.ptr), p(qn.ptr), nq, K, 16384.0, p(M.ptr), nb))
    M = M.numpy()
    thr = np.sort(np.concatenate([np.quantile(M, [0.001, 0.01, 0.1, 0.5, 0.9]), np.quantile(M.min(axis=1), [0.1, 0.5, 0.9]), [0.0, np.inf]])).astype(np.float32)
    c = new_counts(ctx, nq, len(thr))
    _lib.check(ctx.lib.gl_feat_count_h1_scaled(ctx.handle, p(bv.ptr), p(bn.ptr), nb, p(qv.ptr), p(qn.ptr), nq, K, 16384.0, thr.ctypes.data_as(p), len(thr), 0,
                                               len(thr), p(c.ptr)))
    res[v] = (k.numpy().copy(), M, c.numpy()[:nq].copy(), thr)
out = {}
for v in (3, 5):
    keys, M, c, thr = res[v]
    d = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    out["min_is_key_%%d" %% v] = bool(np.array_equal(M.min(axis=1), d) and np.array_equal(M.argmin(axis=1), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)))
    out["counts_are_matrix_%%d" %% v] = bool(np.array_equal(c, np.stack([(M <= t).sum(axis=1) for t in thr], axis=1).astype(np.uint64)))
out["matrix_equal"] = bool(np.array_equal(res[3][1], res[5][1]))
out["counts_equal"] = bool(np.array_equal(res[3][2], res[5][2]) and np.array_equal(res[3][3], res[5][3]))
out["some_hits"] = int(res[3][2][:, 1:-1].sum())           # the finite radii above 0 (column 0 is the radius 0, the last one inf)
print("RESULT " + json.dumps(out))
'''


def test_cluster_and_cluster_free_kernels_count_alike():
    """the two persistent kernels (clusters: a whole MI355X; without: a device with fewer than 256 CUs, forced through the tuning build's
    GL_PAIR_VARIANT=5) on random fp16 rows spanning three K segments: the same matrix, the same counts, and the matrix minimum is the key
    of the shipped search in both"""
    tuning = os.path.join(ROOT, "gan-leaks_amd", "libganleaks_hip_tuning.so")
    if not os.path.exists(tuning):
        subprocess.run(["make", "-C", os.path.join(ROOT, "gan-leaks_amd", "csrc"), "-j8", "tuning"], check=True)
    env = dict(os.environ, GANLEAKS_LIB=tuning)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    out = json.loads([l for l in r.stdout.decode().splitlines() if l.startswith("RESULT ")][-1][7:])
    assert out.pop("some_hits") > 0
    assert all(v is True for v in out.values()), out
