"""GPU: kernel-density (soft-min) sums and scores on the float paths (gl_l2_kde_rows_f32, gl_feat_kde_rows*, kde_sums_f32,
lpips.feat_kde_rows, pair_kde_scores and its DeviceGroup forms).
The expected sums never pass through the kernels under test: they are the numpy weights of tests/pair_kde_common.py over the oracle's
float32 distance of every pair -- the committed C chain (float_rows_common.chain_matrix) for fp32 rows, exact int64 arithmetic on
condition-C integer rows (pair_rows_common) for the LPIPS kernels, the stored matrix pair_distances gives under the real 'l2-lpips'
distance.  Sums and keys are compared bit for bit; every case asserts on its host data that it does not pass vacuously."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_common  # noqa: F401
import float_rows_common as frc
import kde_common as kc
import pair_kde_common as pk
import test_gpu_pair_rows_exact as ex

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
p = ctypes.c_void_p


@pytest.fixture(scope="module")
def gl():
    import ganleaks_amd
    return ganleaks_amd


# ---- the fp32 kernel against the C chain

_f32 = {}


def f32_case(name):
    """(queries, bank, M) of one fp32 case; bank row 33 holds +inf (every distance to it is +inf), the oracle matrix computed once"""
    if name not in _f32:
        q, bank = pk.f32_case(*pk.F32_CASES[name])
        bank = bank.copy()
        bank[33, 7] = np.inf
        M = frc.chain_matrix(q, bank)
        assert np.all(np.isinf(M[:, 33])) and np.isfinite(np.delete(M, 33, axis=1)).all()
        M.setflags(write=False)
        _f32[name] = (q, bank, M)
    return _f32[name]


def f32_sums(gl, q, bank, D0, coef, **kw):
    from ganleaks_amd.attack import Bank, kde_sums_f32
    ctx = gl.Context.get()
    b, f = Bank.from_images(bank, ctx, force_kind="f32"), Bank.from_images(q, ctx, force_kind="f32")
    return kde_sums_f32(b, f, D0, gl.kde_cut_bits_rows(D0, coef[-1]), coef, **kw).numpy()[:len(q)]


@pytest.mark.parametrize("name", list(pk.F32_CASES))
@pytest.mark.parametrize("T", [1, 3, 16])
def test_fp32_kernel(gl, name, T):
    """70 x 150: 2 x 3 ragged 64-tiles; d = 50 takes the scalar loads, d = 96 vector loads over 3 K slices"""
    q, bank, M = f32_case(name)
    D0 = M.min(axis=1)
    assert (D0 == 0).sum() >= 5
    coef = pk.pick_coef(M, D0, T)                          # (asserts that the weights do not pass vacuously)
    got = f32_sums(gl, q, bank, D0, coef)
    want = pk.want_sums(M, D0, coef)
    assert got.dtype == np.uint64 and np.array_equal(got, want), np.argwhere(got != want)[:6].tolist()
    assert np.all(got >= kc.ONE)
    if T == 3:
        # two chunk calls accumulating into one table, and the first rows of a prepared bank only
        from ganleaks_amd.attack import Bank, kde_sums_f32
        ctx = gl.Context.get()
        f = Bank.from_images(q, ctx, force_kind="f32")
        bound = gl.kde_cut_bits_rows(D0, coef[-1])
        acc = kde_sums_f32(Bank.from_images(bank[:70], ctx, force_kind="f32"), f, D0, bound, coef)
        kde_sums_f32(Bank.from_images(bank[70:], ctx, force_kind="f32"), f, ctx.to_device(D0), ctx.to_device(bound), coef, sums=acc)
        assert np.array_equal(acc.numpy()[:len(q)], want)
        part = f32_sums(gl, q, bank, D0, coef, n_rows=100)
        assert np.array_equal(part, pk.want_sums(M[:, :100], D0, coef))


def test_fp32_kernel_errors_are_returns_and_leave_the_context_clean(gl):
    q, bank, M = f32_case("d50_scalar_loads")
    D0 = M.min(axis=1)
    coef = pk.pick_coef(M, D0, 3)
    want = pk.want_sums(M, D0, coef)
    bad = bank.copy()
    bad[101, 3] = np.nan
    with pytest.raises(gl.GanLeaksError, match="NaN"):
        f32_sums(gl, q, bad, D0, coef)
    assert np.array_equal(f32_sums(gl, q, bank, D0, coef), want)          # the flag is cleared
    above = D0.copy()
    above[41] = np.nextafter(above[41], np.float32(np.inf))               # one pattern above the true minimum of one query
    with pytest.raises(gl.GanLeaksError, match="below the offset"):
        f32_sums(gl, q, bank, above, coef)
    assert np.array_equal(f32_sums(gl, q, bank, D0, coef), want)
    # bad coefficients are refused on the host
    from ganleaks_amd.attack import Bank, kde_sums_f32
    ctx = gl.Context.get()
    b, f = Bank.from_images(bank, ctx, force_kind="f32"), Bank.from_images(q, ctx, force_kind="f32")
    bound = gl.kde_cut_bits_rows(D0, coef[-1])
    for c in ([], [1.0] * 17, [1.0, 2.0], [-1.0], [np.nan], [np.inf]):
        with pytest.raises(ValueError):
            kde_sums_f32(b, f, D0, bound, np.asarray(c, np.float32))
    with pytest.raises(ValueError):
        kde_sums_f32(b, f, D0[:-1], bound, coef)
    assert np.array_equal(f32_sums(gl, q, bank, D0, coef), want)


# ---- the LPIPS kernels against exact integer arithmetic (the rows go straight into the C ABI)

def feat_sums(pair, D0, bound, coef, sums=None, row0=0, n_rows=None):
    from ganleaks_amd.attack import new_counts
    ctx = pair.ctx
    b, q = pair._ops(row0, n_rows)
    d0, bd = ctx.to_device(np.ascontiguousarray(D0, np.float32)), ctx.to_device(np.ascontiguousarray(bound, np.uint32))
    c32 = np.ascontiguousarray(coef, np.float32)
    if sums is None:
        sums = new_counts(ctx, pair.Q.n, len(c32))
    if pair.h1:
        pair.check(pair.lib.gl_feat_kde_rows_h1_scaled(pair.h, *b, *q, pair.B.K, pair.scale, p(d0.ptr), p(bd.ptr), c32.ctypes.data_as(p), len(c32),
                                                       p(sums.ptr)))
    else:
        pair.check(pair.lib.gl_feat_kde_rows(pair.h, *b, *q, pair.B.K, p(d0.ptr), p(bd.ptr), c32.ctypes.data_as(p), len(c32), p(sums.ptr)))
    return sums


def check_feat_kde(gl, ctx, kind, case, Ts=(1, 16), split_at=None, errors=False):
    """the sums of one condition-C case against the host weights of its exact D32, for every T; optionally in two bank parts accumulating
    into one table, and the below-offset error"""
    M, Nq, Nb = pk.int_case_matrix(kind, case)
    B, Q = ex.Rows(ctx, kind, case["b"], Nb), ex.Rows(ctx, kind, case["q"], Nq)
    pair = ex.Pair(ctx, B, Q)
    D0 = M.min(axis=1)
    assert np.array_equal(pair.top1().numpy() >> np.uint64(32), pk.bits_of(D0).astype(np.uint64))      # D0 is the search's key
    for T in Ts:
        coef = pk.pick_coef(M, D0, T)                      # (asserts that the weights do not pass vacuously)
        bound = gl.kde_cut_bits_rows(D0, coef[-1])
        want = pk.want_sums(M, D0, coef)
        got = feat_sums(pair, D0, bound, coef).numpy()[:case["nq"]]
        assert np.array_equal(got, want), (kind, T, np.argwhere(got != want)[:6].tolist())
        if split_at:
            acc = feat_sums(pair, D0, bound, coef, row0=split_at)
            feat_sums(pair, D0, bound, coef, sums=acc, n_rows=split_at)
            assert np.array_equal(acc.numpy()[:case["nq"]], want), (kind, T, "two parts")
    if errors:
        above = D0.copy()
        above[case["nq"] - 1] = np.nextafter(above[case["nq"] - 1], np.float32(np.inf))
        with pytest.raises(gl.GanLeaksError, match="below the offset"):
            feat_sums(pair, above, bound, coef)
        assert np.array_equal(feat_sums(pair, D0, bound, coef).numpy()[:case["nq"]], want)      # the flag is cleared


@pytest.fixture(scope="module")
def ctx(gl):
    ctx = gl.Context.get()
    yield ctx
    ctx.trim()


def test_fp16_rows_kernel(gl, ctx):
    """300 queries x 520 bank rows at K1 = 128: two 256-tiles, ragged both ways (on a whole MI355X the clustered form)"""
    seed, nq, nb, K = pk.FP16_CASE
    check_feat_kde(gl, ctx, "fp16", pk.fp16_case(seed, nq, nb, K), split_at=264, errors=True)


def test_split_rows_kernel(gl, ctx):
    """130 x 260 at K = 64: 2 x 3 ragged 128-tiles"""
    seed, nq, nb, K = pk.SPLIT_CASE
    check_feat_kde(gl, ctx, "split", pk.split_case(seed, nq, nb, K), split_at=136, errors=True)


def test_blocked_rows_kernel(gl, ctx):
    """the smallest K-blocked row length: 20 bank rows x 4 queries, 8 segments"""
    seed, nq, nb, K = pk.BLOCKED_CASE
    case = pk.fp16_case(seed, nq, nb, K, long=True, copies=1)
    check_feat_kde(gl, ctx, "fp16", case, Ts=(3,))
    ctx.trim()


CHILD = r'''
import os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import ganleaks_amd as gl
from ganleaks_amd import _lib
import pair_kde_common as pk
import test_gpu_pair_kde as t
assert _lib.LIB_PATH.endswith("libganleaks_hip_tuning.so")
os.environ["GL_PAIR_VARIANT"] = "5"
ctx = gl.Context.get()
seed, nq, nb, K = pk.FP16_CASE
t.check_feat_kde(gl, ctx, "fp16", pk.fp16_case(seed, nq, nb, K), split_at=264, errors=True)
print("RESULT ok")
'''


def test_cluster_free_kernel_against_the_same_oracle():
    """the fp16 case through feat_pairs_h1_kernel<5, false> (what a device with fewer than 256 CUs runs), forced in the tuning build by
    GL_PAIR_VARIANT=5"""
    tuning = os.path.join(ROOT, "gan-leaks_amd", "libganleaks_hip_tuning.so")
    if not os.path.exists(tuning):
        subprocess.run(["make", "-C", os.path.join(ROOT, "gan-leaks_amd", "csrc"), "-j8", "tuning"], check=True)
    env = dict(os.environ, GANLEAKS_LIB=tuning)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert "RESULT ok" in r.stdout.decode()


# ---- pair_kde_scores end to end

class _RowsGenerator:
    def __init__(self, ctx, bank):
        self.ctx, self.bank = ctx, bank

    def generate_u8(self, z):
        return self.ctx.to_device(self.bank[np.asarray(z)])


def check_scores(got, M, h, n_eff, want_key=None):
    """(loss, W, key) against the host weights and a float64 log-sum-exp over the float32 matrix M at the bandwidths the rounded
    coefficients stand for; returns (c32, h_eff)"""
    from ganleaks_amd.attack import kde_coef
    loss, W, key = got
    T = len(h)
    assert loss.dtype == np.float64 and W.dtype == np.uint64 and key.dtype == np.int64
    assert loss.shape == W.shape == (len(M), T) and key.shape == (len(M),)
    c32, h_eff = kde_coef(h, 1, "f32")
    D0 = M.min(axis=1)
    assert np.array_equal(key, pk.bits_of(D0).astype(np.int64))
    if want_key is not None:
        assert np.array_equal(key, want_key)
    assert np.array_equal(W, pk.want_sums(M, D0, c32)), np.argwhere(W != pk.want_sums(M, D0, c32))[:6].tolist()
    assert np.array_equal(loss, D0.astype(np.float64)[:, None] + h_eff[None, :] * np.log(float(n_eff) / (W.astype(np.float64) * 2.0 ** -40)))
    return c32, h_eff


def check_loss(loss, M, c32, h_eff, n_eff, cols):
    """|loss - float64 log-sum-exp| <= h_eff ln(1 + 2 E), E the measured weight error plus n_eff 2^-40 for the pairs whose weight falls
    below a unit (2 x measured = pk.E_F32), plus the float64 rounding of the reference itself"""
    ref = pk.host_loss(M, h_eff, n_eff)
    for t in cols:
        err = np.abs(loss[:, t] - ref[:, t])
        bound = h_eff[t] * np.log1p(pk.E_F32 + 2 * n_eff * 2.0 ** -40) + 4 * np.spacing(np.abs(ref[:, t]))
        print("h = %.3e: largest |loss - ref| = %.3e, bound %.3e" % (h_eff[t], err.max(), bound.min()))
        assert np.all(err <= bound), (t, err.max(), bound.min())


def test_scores_on_float_rows(gl, synth):
    """distance='l2', float_path='exact': a float table off both lattices, 150 rows, batch 50: all take part; resident, permuted, streamed
    in 4 chunks, as a DeviceArray, generated, prepared, and on two contexts of one device -- W and key bit-identical"""
    from ganleaks_amd import shard
    from ganleaks_amd.attack import Bank
    ctx = gl.Context.get()
    q, bank = pk.f32_case(4220, 64, 150, 50)
    bank[149] = bank[7]
    q[0] = bank[7]                                                       # two rows tie at the minimum of query 0
    M = frc.chain_matrix(q, bank)
    D0 = M.min(axis=1)
    n_eff = 150
    h = pk.bandwidths_of(pk.pick_coef(M, D0, 3))[[1, 0, 2]].tolist() + [1e-30]      # any order; the last so small that only ties weigh
    kw = dict(distance="l2", batch_size=50, float_path="exact")
    ref = gl.pair_kde_scores(q, bank, h, **kw)
    nn, _ = gl.nearest_neighbours(q, bank, 1, **kw)
    c32, h_eff = check_scores(ref, M, h, n_eff, want_key=pk.bits_of(nn[:, 0]).astype(np.int64))
    pk.check_not_vacuous(M, D0, np.sort(c32[:3])[::-1])
    check_loss(ref[0], M, c32, h_eff, n_eff, range(3))
    ties = (pk.bits_of(M) == pk.bits_of(D0)[:, None]).sum(axis=1)
    assert ties[0] == 2 and np.array_equal(ref[1][:, 3], ties.astype(np.uint64) * kc.ONE)
    assert np.array_equal(ref[0][:, 3], D0.astype(np.float64) + h_eff[3] * np.log(float(n_eff) / (ties * 1.0)))
    perm = np.random.default_rng(4221).permutation(150)
    d = 50
    others = {
        "permuted": gl.pair_kde_scores(q, bank[perm], h, **kw),
        "streamed": gl.pair_kde_scores(q, bank, h, chunk_bytes=40 * 4 * d, **kw),                        # 4 chunks, the last ragged
        "device array": gl.pair_kde_scores(ctx.to_device(q), ctx.to_device(bank), h, chunk_bytes=40 * 4 * d, **kw),
        "prepared": gl.pair_kde_scores(Bank.from_images(q, ctx, force_kind="f32"), Bank.from_images(bank, ctx, force_kind="f32"), h, **kw),
    }
    with shard.DeviceGroup(devices=[0, 0]) as group:
        assert group.collective == "host-merge"
        others["two shards"] = group.pair_kde_scores(q, bank=bank, bandwidths=h, batch_size=50, distance="l2", float_path="exact")
        others["two uneven shards"] = group.pair_kde_scores(q, bank=bank, bandwidths=h, batch_size=50, distance="l2", float_path="exact",
                                                            weights=[1.0, 2.0])
        with pytest.raises(ValueError):
            group.pair_kde_scores(q, bank=bank, bandwidths=[0.1, -1.0], batch_size=50, distance="l2", float_path="exact")
        assert not group._broken
    others["on devices"] = shard.pair_kde_scores_on_devices(q, bank=bank, devices=[0, 0, 0], bandwidths=h, batch_size=50, distance="l2",
                                                            float_path="exact")
    for name, other in others.items():
        for a, r in zip(other, ref):
            assert a.dtype == r.dtype and np.array_equal(a, r), name
    # without the keyword such rows raise what kde_scores raises; a bank row at +inf weighs nothing; NaN and an infinite nearest are errors
    with pytest.raises(NotImplementedError, match="off both lattices"):
        gl.pair_kde_scores(q, bank, h, distance="l2", batch_size=50)
    far = bank.copy()
    far[17, 3] = np.float32(3.0e38)                                      # the difference squared overflows: every distance to row 17 is +inf
    Mf = M.copy()
    Mf[:, 17] = np.inf
    assert not np.any(M.argmin(axis=1) == 17)
    check_scores(gl.pair_kde_scores(q, far, h, **kw), Mf, h, n_eff)
    bad = bank.copy()
    bad[17, 3] = np.nan
    with pytest.raises(gl.GanLeaksError, match="NaN"):
        gl.pair_kde_scores(q, bad, h, **kw)
    with pytest.raises(ValueError, match="finite nearest distance"):
        gl.pair_kde_scores(q, np.full((50, d), np.float32(3.0e38)), h, **kw)
    check_scores(gl.pair_kde_scores(q, bank, h, **kw), M, h, n_eff)       # the context is clean afterwards


def test_lattice_rows_take_the_exact_integer_path(gl, synth):
    bank, q = kc.planted_case(synth, 4230, 128, 40, (3, 8, 8))
    S = kc.host_S(q, bank)
    unit = 65025.0 * 192 / 4.0
    h = (np.log2(np.e) / (kc.pick_coef(S, S.min(axis=1), 3).astype(np.float64) * unit)).tolist()
    want = gl.kde_scores(q, bank, h, batch_size=64)
    assert np.array_equal(want[2], S.min(axis=1))
    for fp in (None, "exact"):
        got = gl.pair_kde_scores(q, bank, h, distance="l2", batch_size=64, float_path=fp)
        for a, r in zip(got, want):
            assert a.dtype == r.dtype and np.array_equal(a, r), fp                                       # key == S0


@pytest.fixture(scope="module")
def lin(golden_dir):
    z = np.load(os.path.join(golden_dir, "lpips_lin_v0.1.npz"))
    return {"lin%d" % i: z["lin%d" % i] for i in range(5)}


@pytest.fixture(scope="module")
def model(gl, synth, lin):
    from ganleaks_amd.lpips import LpipsModel
    return LpipsModel().load_state_dicts(synth.vgg16_state_dict(7), lin)


@pytest.fixture(scope="module")
def lpips_case(gl, synth, model):
    """64 queries x 270 planted images of 32 x 32 (batch 64: 256 rows take part), the stored matrix computed once"""
    planted, q = kc.planted_case(synth, 4240, 256, 64, (3, 32, 32), sigmas=(2.0, 6.0, 12.0, 20.0))
    bank = np.concatenate([planted, np.random.default_rng(4242).integers(0, 256, size=(14, 3, 32, 32), dtype=np.uint8)])
    bank[200] = bank[12]
    q[0] = bank[12]                                                      # two rows tie at the minimum of query 0
    M = gl.pair_distances(q, bank[:256], batch_size=64, lpips=model)
    assert M.shape == (64, 256)
    M.setflags(write=False)
    return bank, q, M


def test_scores_under_l2_lpips(gl, model, lpips_case):
    bank, q, M = lpips_case
    n_eff = 256
    D0 = M.min(axis=1)
    h = pk.bandwidths_of(pk.pick_coef(M, D0, 3))[[2, 0, 1]].tolist() + [1e-30]
    kw = dict(distance="l2-lpips", batch_size=64, lpips=model)
    got = gl.pair_kde_scores(q, bank, h, **kw)
    nn, _ = gl.nearest_neighbours(q, bank, 1, **kw)
    c32, h_eff = check_scores(got, M, h, n_eff, want_key=pk.bits_of(nn[:, 0]).astype(np.int64))
    pk.check_not_vacuous(M, D0, np.sort(c32[:3])[::-1])
    check_loss(got[0], M, c32, h_eff, n_eff, range(3))
    ties = (pk.bits_of(M) == pk.bits_of(D0)[:, None]).sum(axis=1)
    assert ties[0] == 2 and np.array_equal(got[1][:, 3], ties.astype(np.uint64) * kc.ONE)
    assert np.array_equal(got[0][:, 3], D0.astype(np.float64) + h_eff[3] * np.log(float(n_eff) / (ties * 1.0)))
    # soft-min: at least the nearest distance, at most the mean distance
    assert np.all(got[0] >= D0.astype(np.float64)[:, None]) and np.all(got[0][:, :3] <= M.astype(np.float64).mean(axis=1)[:, None])


def test_l2_lpips_bank_forms_and_shards_agree(gl, synth, lin, model, lpips_case, monkeypatch):
    import importlib
    from ganleaks_amd import shard
    from ganleaks_amd.attack import GeneratedBank
    from ganleaks_amd.lpips import LpipsModel
    attack = importlib.import_module("ganleaks_amd.attack")
    ctx = gl.Context.get()
    bank, q, M = lpips_case
    h = pk.bandwidths_of(pk.pick_coef(M, M.min(axis=1), 3)).tolist()
    kw = dict(distance="l2-lpips", batch_size=64, lpips=model)
    ref = gl.pair_kde_scores(q, bank, h, **kw)
    check_scores(ref, M, h, 256)
    row = 2 * int(ctx.lib.gl_lpips_lattice_dim(32, 32))
    fb, fq = model.features(bank[:256], role="bank"), model.features(q, role="query")
    gen = _RowsGenerator(ctx, bank)
    perm = np.concatenate([np.random.default_rng(4241).permutation(256), np.arange(256, 270)])
    others = {
        "feature banks": gl.pair_kde_scores(fq, fb, h, **kw),
        "images against a feature bank": gl.pair_kde_scores(q, fb, h, **kw),
        "permuted": gl.pair_kde_scores(q, bank[perm], h, **kw),
        "streamed": gl.pair_kde_scores(q, bank, h, chunk_bytes=100 * row, **kw),                          # 100 + 100 + 56 rows
        "device array": gl.pair_kde_scores(q, ctx.to_device(bank), h, chunk_bytes=100 * row, **kw),
        "generated": gl.pair_kde_scores(q, GeneratedBank(gen, np.arange(len(bank))), h, chunk_bytes=100 * row, **kw),
        "feature queries, streamed": gl.pair_kde_scores(fq, bank, h, chunk_bytes=100 * row, **kw),
    }
    # the queries in 3 slices on top of the chunks: D0, the bounds, the keys and the sums are sliced with them
    monkeypatch.setattr(attack, "_query_budget_bytes", lambda chunk_bytes, ctx=None: int(25.5 * row))
    others["query slices"] = gl.pair_kde_scores(q, bank, h, chunk_bytes=100 * row, **kw)
    monkeypatch.undo()
    make = lambda c: LpipsModel(c).load_state_dicts(synth.vgg16_state_dict(7), lin)                      # noqa: E731
    with shard.DeviceGroup(devices=[0, 0]) as group:
        assert group.collective == "host-merge"
        others["two shards"] = group.pair_kde_scores(q, bank=bank, bandwidths=h, batch_size=64, make_lpips=make)
        assert not group._broken
    for name, other in others.items():
        for a, r in zip(other, ref):
            assert a.dtype == r.dtype and np.array_equal(a, r), name
