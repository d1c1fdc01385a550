"""GPU: the histogram of all pair distances on the two float paths (lpips.feat_hist / gl_feat_hist*: 0.2 * LPIPS + L2;
attack.pair_histogram_f32 / gl_l2_hist_f32: fixed-order fp32 rows) and the exact quantiles built on it (pair_distance_quantiles,
DeviceGroup.pair_distance_quantiles, mc.py --eps_percentile).

The expected values never pass through the kernels under test or through select_ranks: under 'l2-lpips' they are numpy on the uint32
patterns of the stored matrix pair_distances gives (tied to the search and to the fp64 oracle by tests/test_gpu_count_lpips.py), on fp32
rows numpy on the patterns of the CPU chain matrix (float_rows_common.chain_matrix).  np.bincount gives the histograms, np.sort the value
at a rank.  Every comparison is array_equal and every query takes part."""
import ctypes
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import gpu_common  # noqa: F401
import float_rows_common as frc
from test_gpu_count_lpips import _images, _RowsGenerator

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
p = ctypes.c_void_p
ORACLE_BOUND = 5e-6            # |device - reference| of an l2-lpips distance at <= 64 x 64 (tests/test_gpu_lpips.py, test_gpu_topk_lpips.py)
INF_BITS = 0x7F800000
QS = [0, 0.001, 0.25, 0.5, 1]


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


def bits_of(M):
    """int64 array of the uint32 patterns of a float32 matrix"""
    return np.ascontiguousarray(M, np.float32).view(np.uint32).astype(np.int64)


def oracle_hist(B, lo, shift, n_bins):
    x = B.reshape(-1)
    x = x[(x >= lo) & (x <= INF_BITS)]
    b = (x - lo) >> shift
    return np.bincount(b[b < n_bins], minlength=n_bins).astype(np.int64)


def windows_of(B):
    """the windows of the issue: the three levels of the radix-select around the median, an unaligned lo, n_bins in {1, 2048}, shift = 0, a
    window without a pair, windows above every pattern (one whose end passes 2^32)"""
    flat = np.sort(B.reshape(-1))
    med, top = int(flat[flat.size // 2]), int(flat[-1])
    assert top < INF_BITS
    return [(0, 20, 2048), (med >> 20 << 20, 9, 2048), (med >> 9 << 9, 0, 512),
            (max(med - 12345, 0), 3, 1000), (med | 1, 1, 77),
            (0, 31, 1), (med, 5, 1), (max(med - 1000, 0), 0, 2048),
            (top + 1, 0, 2048), (top + 1, 12, 2048),
            (INF_BITS + 1, 0, 2048), (0xFFFFF000, 4, 2048), (0xFFFFFFFF, 31, 1)]


def host(hist):
    return hist.numpy().reshape(-1).astype(np.int64)


def oracle_ranks(quantiles, pairs):
    return [int(Fraction(float(v)) * (pairs - 1)) for v in quantiles]


def oracle_quantiles(M, quantiles):
    """(eps float32 [T], key int64 [T], pairs) by the definition: sorted(bits)[floor(v * (pairs - 1))]"""
    flat = np.sort(bits_of(M).reshape(-1))
    key = np.asarray([flat[r] for r in oracle_ranks(quantiles, flat.size)], np.int64)
    return key.astype(np.uint32).view(np.float32), key, int(flat.size)


def check_quantiles(got, want):
    eps, key, pairs = got
    assert eps.dtype == np.float32 and key.dtype == np.int64 and isinstance(pairs, int)
    assert np.array_equal(key, want[1]), (key, want[1])
    assert np.array_equal(eps.view(np.uint32), want[0].view(np.uint32)) and pairs == want[2]


def check_definition(eps, ranks, count):
    """the two inequalities of the definition by the ball counts of the same path: count(eps float32 [T]) -> int64 [Q, T]"""
    at = count(eps).sum(axis=0)
    with np.errstate(over="ignore"):
        below = count(np.nextafter(eps, np.float32(-np.inf))).sum(axis=0)
    for t, r in enumerate(ranks):
        assert at[t] >= r + 1 and below[t] <= r, (t, r, at[t], below[t])


# ---- 1 + 2: 0.2 * LPIPS + L2

def _lpips_hist_and_quantiles(gl, model, q, bank, bs, n_eff):
    from ganleaks_amd import lpips
    attack = sys.modules["ganleaks_amd.attack"]
    M = gl.pair_distances(q, bank, batch_size=bs, lpips=model)
    assert M.shape == (len(q), n_eff)
    B = bits_of(M)
    fb, fq = attack._lpips_resident_rows(q, bank[:n_eff], False, model, 0)
    for w in windows_of(B):
        h = lpips.feat_hist(fb, fq, *w)
        assert h.dtype == np.dtype(np.uint64) and tuple(h.shape) == (w[2], 1)
        got, want = host(h), oracle_hist(B, *w)
        assert np.array_equal(got, want), (w, np.flatnonzero(got != want)[:5])
    assert host(lpips.feat_hist(fb, fq, 0, 20, 2048)).sum() == len(q) * n_eff
    # a second call into the same bins doubles them; n_rows cuts the bank
    w = windows_of(B)[1]
    h = lpips.feat_hist(fb, fq, *w)
    assert lpips.feat_hist(fb, fq, *w, hist=h) is h
    assert np.array_equal(host(h), 2 * oracle_hist(B, *w))
    assert np.array_equal(host(lpips.feat_hist(fb, fq, *w, n_rows=n_eff - 7)), oracle_hist(B[:, :n_eff - 7], *w))
    # quantiles
    kw = dict(batch_size=bs, distance="l2-lpips", lpips=model)
    want = oracle_quantiles(M, QS)
    got = gl.pair_distance_quantiles(q, bank, QS, batch_size=bs, lpips=model)           # 'l2-lpips' is the default
    check_quantiles(got, want)
    eps, key, pairs = got
    assert pairs == len(q) * n_eff
    check_definition(eps, oracle_ranks(QS, pairs), lambda e: gl.ball_counts(q, bank, e, **kw))
    assert eps[0] == gl.attack(q, bank, **kw)[0].min() and eps[-1] == M.max()
    return M


@pytest.mark.parametrize("nq", [1, 63, 300])
@pytest.mark.parametrize("route", ["u8", "float", "split"])
@pytest.mark.parametrize("res", [16, 32])
def test_histogram_is_the_matrix_and_quantiles_are_its_order_statistics(res, route, nq, gl, synth, oracle, model):
    """test_gpu_count_lpips.py's cases: 333 bank images of which batch 30 lets 330 take part (ragged against the 128 and the 256 tile);
    lattice rows (u8), hi / lo rows (off-lattice floats), split rows"""
    bank, q = _images(synth, oracle, 300 + res, 333, nq, res, route)
    model.search_rows = "split" if route == "split" else "fp16"
    try:
        _lpips_hist_and_quantiles(gl, model, q, bank, 30, 330)
    finally:
        model.search_rows = "fp16"


@pytest.mark.parametrize("route", ["u8", "float"])
def test_k_blocked_rows(route, gl, synth, oracle, model):
    """test_gpu_count_lpips.py's K-blocked shape: 128 x 128 images (rows of 4.1 / 4.3 MB, stored K-blocked), 20 bank rows and 4 queries"""
    bank, q = _images(synth, oracle, 131, 50, 4, 128, route)
    bank = bank[:23]
    bank[7] = bank[12]
    assert model.features(bank[:20], role="bank").blocked
    _lpips_hist_and_quantiles(gl, model, q, bank, 4, 20)


CHILD = r'''
import ctypes, json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
import ganleaks_amd as gl
from ganleaks_amd import _lib
from ganleaks_amd.attack import new_hist
assert _lib.LIB_PATH.endswith("libganleaks_hip_tuning.so")
ctx = gl.Context.get()
p = ctypes.c_void_p
rng = np.random.default_rng(8)
# fp16 search rows: K = 1 segment + a ragged one (2048 slices of 64 halves per segment); 3 x 2 tiles with ragged edges
K = 64 * (2048 + 100)
nb, nq = 520, 300
bh = (rng.standard_normal((nb, K), dtype=np.float32) * 40).astype(np.float16)
qh = (rng.standard_normal((nq, K), dtype=np.float32) * 40).astype(np.float16)
qh[5] = bh[515]
bv, qv = ctx.to_device(bh), ctx.to_device(qh)
bn = ctx.to_device((bh.astype(np.float32) ** 2).sum(1).astype(np.float32) / 16384.0 ** 2)
qn = ctx.to_device((qh.astype(np.float32) ** 2).sum(1).astype(np.float32) / 16384.0 ** 2)
out = {}
mats = {}
for v in (3, 5):
    os.environ["GL_PAIR_VARIANT"] = str(v)
    M = ctx.empty((nq, nb), np.float32)
    _lib.check(ctx.lib.gl_feat_pair_dist_h1_scaled(ctx.handle, p(bv.ptr), p(bn.ptr), nb, p(qv.ptr), p(qn.ptr), nq, K, 16384.0, p(M.ptr), nb))
    B = M.numpy().view(np.uint32).astype(np.int64).reshape(-1)
    mats[v] = B
    med = int(np.sort(B)[B.size // 2])
    ok = True
    for lo, shift, n_bins in ((0, 20, 2048), (med >> 20 << 20, 9, 2048), (med >> 9 << 9, 0, 512), (max(med - 777, 0), 2, 1999), (int(B.max()) + 1, 0, 64)):
        h = new_hist(ctx, n_bins)
        _lib.check(ctx.lib.gl_feat_hist_h1_scaled(ctx.handle, p(bv.ptr), p(bn.ptr), nb, p(qv.ptr), p(qn.ptr), nq, K, 16384.0, lo, shift, n_bins, p(h.ptr)))
        x = B[B >= lo]
        b = (x - lo) >> shift
        want = np.bincount(b[b < n_bins], minlength=n_bins)
        ok = ok and bool(np.array_equal(h.numpy().reshape(-1).astype(np.int64), want))
    out["hist_is_matrix_%%d" %% v] = ok
out["matrix_equal"] = bool(np.array_equal(mats[3], mats[5]))
print("RESULT " + json.dumps(out))
'''


def test_cluster_and_cluster_free_kernels_bin_alike():
    """the two persistent kernels (clusters: a whole MI355X; without: forced through the tuning build's GL_PAIR_VARIANT=5, as
    tests/test_gpu_count_lpips.py forces it) on random fp16 rows spanning two K segments: the histogram is the stored matrix in both"""
    tuning = os.path.join(ROOT, "gan-leaks_amd", "libganleaks_hip_tuning.so")
    if not os.path.exists(tuning):
        subprocess.run(["make", "-C", os.path.join(ROOT, "gan-leaks_amd", "csrc"), "-j8", "tuning"], check=True)
    env = dict(os.environ, GANLEAKS_LIB=tuning)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    out = json.loads([l for l in r.stdout.decode().splitlines() if l.startswith("RESULT ")][-1][7:])
    assert all(v is True for v in out.values()), out


# ---- 3: invariance

def test_quantiles_do_not_depend_on_chunks_slices_shards_or_prepared_rows(gl, synth, oracle, model, lin, monkeypatch):
    from ganleaks_amd import lpips, shard
    from ganleaks_amd.attack import GeneratedBank
    from ganleaks_amd.lpips import LpipsModel
    ctx = gl.Context.get()
    bank, q = _images(synth, oracle, 351, 333, 63, 32, "u8")
    bs, n_eff = 30, 330
    M = gl.pair_distances(q, bank, batch_size=bs, lpips=model)
    want = oracle_quantiles(M, QS)
    kw = dict(batch_size=bs, lpips=model)
    check_quantiles(gl.pair_distance_quantiles(q, bank, QS, **kw), want)
    check_quantiles(gl.pair_distance_quantiles(q, bank, 0.25, **kw), oracle_quantiles(M, [0.25]))         # a scalar gives one value
    row = 2 * int(ctx.lib.gl_lpips_lattice_dim(32, 32))
    # the bank in 4 chunks: an image array, a DeviceArray of images, a GeneratedBank
    check_quantiles(gl.pair_distance_quantiles(q, bank, QS, chunk_bytes=100 * row, **kw), want)
    check_quantiles(gl.pair_distance_quantiles(q, ctx.to_device(bank), QS, chunk_bytes=100 * row, **kw), want)
    gen = GeneratedBank(_RowsGenerator(ctx, bank), np.arange(len(bank)))
    check_quantiles(gl.pair_distance_quantiles(q, gen, QS, chunk_bytes=100 * row, **kw), want)
    # the queries in 4 slices of 20 on top of that: the bins add over the slices
    monkeypatch.setenv("GANLEAKS_QUERY_GB", repr(20.5 * row / (1 << 30)))
    check_quantiles(gl.pair_distance_quantiles(q, bank, QS, chunk_bytes=100 * row, **kw), want)
    check_quantiles(gl.pair_distance_quantiles(q, gen, QS, chunk_bytes=100 * row, **kw), want)
    monkeypatch.delenv("GANLEAKS_QUERY_GB")
    # prepared rows on both sides, and prepared queries against streamed images
    fb, fq = model.features(bank[:n_eff], role="bank"), model.features(q, role="query")
    check_quantiles(gl.pair_distance_quantiles(fq, fb, QS, batch_size=bs), want)
    check_quantiles(gl.pair_distance_quantiles(fq, bank, QS, chunk_bytes=100 * row, **kw), want)
    # two index_base shards, [0, 150) and [150, 330): the bins of every level are summed with the other shard's (allreduce_sum_counts as far
    # as one rank takes it, then the other shard's bins of the window the launch used).  The first reduction is the pair count.
    real = lpips.feat_hist
    windows = []

    def recording(bank_, queries_, lo, shift, n_bins, n_rows=None, hist=None):
        windows.append((lo, shift, n_bins))
        return real(bank_, queries_, lo, shift, n_bins, n_rows, hist)

    monkeypatch.setattr(lpips, "feat_hist", recording)
    comm = gl._lib.Comm(ctx)
    parts = {0: bank[:150], 150: bank[150:n_eff]}
    for mine, other in ((0, 150), (150, 0)):
        rest = model.features(parts[other], role="bank", index_base=other)
        seen = []

        def reduce_fn(hist):
            hist = shard.allreduce_sum_counts(hist, comm=comm, _even_alone=True)
            if not seen:                                  # the pairs the shards hold
                seen.append(None)
                assert tuple(hist.shape) == (1, 1)
                return ctx.to_device(hist.numpy() + np.uint64(len(q) * len(parts[other])))
            lo, shift, n_bins = windows[-1]
            seen.append(n_bins)
            assert hist.dtype == np.dtype(np.uint64) and tuple(hist.shape) == (n_bins, 1)
            return ctx.to_device(shard.merge_counts_host([hist.numpy(), real(rest, fq, lo, shift, n_bins).numpy()]))

        check_quantiles(gl.pair_distance_quantiles(q, parts[mine], QS, index_base=mine, reduce_fn=reduce_fn, **kw), want)
        assert len(seen) >= 4 and seen[1] == 2048
    monkeypatch.setattr(lpips, "feat_hist", real)
    comm.destroy()
    with pytest.raises(ValueError):
        gl.pair_distance_quantiles(q, bank[:20], QS, **kw)                      # no full batch
    with pytest.raises(ValueError):
        gl.pair_distance_quantiles(q, bank[:0], QS, reduce_fn=lambda h: h, **kw)    # an empty multiset
    # a device group of three contexts on one device (host merge: one rendezvous per level), images and generated rows
    make = lambda c: LpipsModel(c).load_state_dicts(synth.vgg16_state_dict(7), lin)                     # noqa: E731
    with shard.DeviceGroup(devices=[0, 0, 0]) as group:
        assert group.collective == "host-merge"
        check_quantiles(group.pair_distance_quantiles(q, bank=bank, quantiles=QS, batch_size=bs, make_lpips=make), want)
        rows = [id(entry[1]) for entry in group._queries]
        check_quantiles(group.pair_distance_quantiles(q, bank=bank, quantiles=QS, batch_size=bs, weights=[1.0, 3.0, 1e-9], make_lpips=make), want)
        counts = group.ball_counts(q, bank=bank, eps=want[0], batch_size=bs, distance="l2-lpips", make_lpips=make)     # shares the prepared queries
        assert [id(entry[1]) for entry in group._queries] == rows
        with pytest.raises(ValueError):
            group.pair_distance_quantiles(q, bank=bank, quantiles=[1.5], batch_size=bs)
        with pytest.raises(ValueError):
            group.pair_distance_quantiles(q, bank=bank, batch_size=bs)
        assert not group._broken
    assert np.array_equal(counts, gl.ball_counts(q, bank, want[0], batch_size=bs, distance="l2-lpips", lpips=model))
    check_quantiles(shard.pair_distance_quantiles_on_devices(q, lambda c: _RowsGenerator(c, bank), np.arange(len(bank)), devices=[0, 0, 0], quantiles=QS,
                                                             batch_size=bs, make_lpips=make), want)


def test_one_layout_for_all_levels(gl, synth, oracle, model, lin):
    """a streamed bank whose third chunk is off-lattice floats: the first pass starts over in the hi / lo layout with fresh bins and every
    later pass starts there; the answer is the all-hi / lo resident one.  The same bank through a device group: the host settles it."""
    from ganleaks_amd import shard
    from ganleaks_amd.lpips import LpipsModel
    ctx = gl.Context.get()
    codes, q = _images(synth, oracle, 352, 333, 63, 32, "u8")
    bs, n_eff = 30, 330
    bank = oracle.dequantize_u8(codes).astype(np.float32)                      # floats on the lattice ...
    assert model.features(bank[:100], role="bank").fmt == "lattice"
    rng = np.random.default_rng(5)
    bank[200:300] = np.clip(bank[200:300] + rng.normal(0, 0.01, bank[200:300].shape).astype(np.float32), -1, 1)      # ... but for the third chunk
    fb, fq = model.features(bank[:n_eff], role="bank", fmt="hilo"), model.features(q, role="query", fmt="hilo")
    M = gl.pair_distances(fq, fb, batch_size=bs)
    want = oracle_quantiles(M, QS)
    check_quantiles(gl.pair_distance_quantiles(fq, fb, QS, batch_size=bs), want)
    row = 2 * int(ctx.lib.gl_lpips_search_dim(32, 32))
    check_quantiles(gl.pair_distance_quantiles(q, bank, QS, batch_size=bs, lpips=model, chunk_bytes=100 * row), want)
    check_quantiles(gl.pair_distance_quantiles(q, bank, QS, batch_size=bs, lpips=model), want)          # resident: both sides hi / lo
    at = gl.ball_counts(q, bank, want[0], batch_size=bs, distance="l2-lpips", lpips=model).sum(axis=0)
    assert np.array_equal(at, [(bits_of(M) <= k).sum() for k in want[1]])
    make = lambda c: LpipsModel(c).load_state_dicts(synth.vgg16_state_dict(7), lin)                     # noqa: E731
    with shard.DeviceGroup(devices=[0, 0]) as group:
        check_quantiles(group.pair_distance_quantiles(q, bank=bank, quantiles=QS, batch_size=bs, make_lpips=make), want)


# ---- 4: against the reference

@pytest.mark.parametrize("name", ["lpips_res32", "lpips_res64"])
def test_every_order_statistic_is_within_the_bound_of_the_reference(name, gl, synth, oracle, model, golden_dir):
    """R = 0.2 * LPIPS of the reference's own PNetLin (tests/golden/make_golden.py) + the exact L2, as test_gpu_topk_lpips.py builds it.
    Order statistics are 1-Lipschitz in the sup norm: |eps_r - sort(R)[r]| <= the per-distance bound, for every rank r."""
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    case = synth.attack_case(int(g["seed"]), int(g["n_bank"]), int(g["n_pos"]), int(g["n_neg"]), int(g["res"]), sigma=20.0)
    bank, q = case["bank"], np.concatenate([case["pos"], case["neg"]])
    bs = int(g["batch_size"])
    n_eff = (len(bank) // bs) * bs
    assert n_eff == {"lpips_res32": 32, "lpips_res64": 24}[name]
    S = np.stack([oracle.ssd_u8(bank[:n_eff], x) for x in q]).astype(np.int64)
    R = 0.2 * g["lpips"][:, :n_eff].astype(np.float64) + S * (4.0 / (65025.0 * q[0].size))
    sorted_R = np.sort(R.reshape(-1))
    pairs = sorted_R.size
    fb, fq = model.features(bank[:n_eff], role="bank"), model.features(q, role="query")
    # a quantile in the middle of the interval of v that floors to rank r
    v_of = lambda r: 1.0 if r == pairs - 1 else (r + 0.5) / (pairs - 1)                                  # noqa: E731
    worst = 0.0
    for r0 in range(0, pairs, 16):
        ranks = list(range(r0, min(r0 + 16, pairs)))
        vs = [v_of(r) for r in ranks]
        assert oracle_ranks(vs, pairs) == ranks
        eps, key, n = gl.pair_distance_quantiles(fq, fb, vs, batch_size=bs)
        assert n == pairs
        worst = max(worst, float(np.abs(eps.astype(np.float64) - sorted_R[ranks]).max()))
    print("max over all %d ranks of |eps_r - sort(R)[r]| = %.3g" % (pairs, worst))
    assert worst <= ORACLE_BOUND, worst


# ---- 5: fp32 rows

def _f32_case(synth, kind, params):
    bank, q, bs = frc.derive(synth, kind, params)
    n_eff = (len(bank) // bs) * bs
    M = frc.chain_matrix(q, bank[:n_eff])
    M.setflags(write=False)
    return bank, q, bs, n_eff, M


def _f32_hist_and_quantiles(gl, bank, q, bs, n_eff, M):
    from ganleaks_amd.attack import Bank, pair_histogram_f32
    ctx = gl.Context.get()
    B = bits_of(M)
    b, f = Bank.from_images(bank[:n_eff], ctx, force_kind="f32"), Bank.from_images(q, ctx, force_kind="f32")
    for w in windows_of(B):
        h = pair_histogram_f32(b, f, *w)
        assert h.dtype == np.dtype(np.uint64) and tuple(h.shape) == (w[2], 1)
        got, want = host(h), oracle_hist(B, *w)
        assert np.array_equal(got, want), (w, np.flatnonzero(got != want)[:5])
    w = windows_of(B)[1]
    h = pair_histogram_f32(b, f, *w)
    assert pair_histogram_f32(b, f, *w, hist=h) is h
    assert np.array_equal(host(h), 2 * oracle_hist(B, *w))
    assert np.array_equal(host(pair_histogram_f32(b, f, *w, n_rows=n_eff - 7)), oracle_hist(B[:, :n_eff - 7], *w))
    kw = dict(distance="l2", batch_size=bs, float_path="exact")
    want = oracle_quantiles(M, QS)
    got = gl.pair_distance_quantiles(q, bank, QS, **kw)
    check_quantiles(got, want)
    eps, key, pairs = got
    assert pairs == len(q) * n_eff
    check_definition(eps, oracle_ranks(QS, pairs), lambda e: gl.ball_counts(q, bank, e, batch_size=bs, float_path="exact"))
    assert eps[0] == gl.attack(q, bank, distance="l2", batch_size=bs, float_path="exact")[0].min() and eps[-1] == M.max()
    check_quantiles(gl.pair_distance_quantiles(f, b, QS, **kw), want)                      # prepared rows
    return want


@pytest.mark.parametrize("case", frc.IMAGE_CASES, ids=lambda c: "seed%d" % c[0])
def test_fp32_images(case, gl, synth):
    _f32_hist_and_quantiles(gl, *_f32_case(synth, "image", case))


@pytest.mark.parametrize("case", frc.TABLE_CASES, ids=lambda c: "%dx%d" % (c[1], c[2]))
def test_fp32_tables(case, gl, synth):
    """300 x 37 (d % 4 != 0: scalar loads) and 520 x 1071"""
    _f32_hist_and_quantiles(gl, *_f32_case(synth, "table", case))


def test_fp32_chunks_shards_and_mixed_lattices(gl, synth, monkeypatch):
    from ganleaks_amd import shard
    from ganleaks_amd.attack import Bank
    attack = sys.modules["ganleaks_amd.attack"]
    ctx = gl.Context.get()
    bank, q, bs, n_eff, M = _f32_case(synth, "image", frc.IMAGE_CASES[0])
    d = int(np.prod(bank.shape[1:]))
    want = oracle_quantiles(M, QS)
    kw = dict(distance="l2", batch_size=bs, float_path="exact")
    # 4 chunks (100 rows of fp32 each, the last one ragged): an array and a DeviceArray
    check_quantiles(gl.pair_distance_quantiles(q, bank, QS, chunk_bytes=100 * 4 * d, **kw), want)
    check_quantiles(gl.pair_distance_quantiles(q, ctx.to_device(bank), QS, chunk_bytes=100 * 4 * d, **kw), want)
    # two index_base shards
    real = attack.pair_histogram_f32
    windows = []

    def recording(bank_, queries_, lo, shift, n_bins, n_rows=None, hist=None):
        windows.append((lo, shift, n_bins))
        return real(bank_, queries_, lo, shift, n_bins, n_rows, hist)

    monkeypatch.setattr(attack, "pair_histogram_f32", recording)
    fq = Bank.from_images(q, ctx, force_kind="f32")
    parts = {0: bank[:150], 150: bank[150:n_eff]}
    for mine, other in ((0, 150), (150, 0)):
        rest = Bank.from_images(parts[other], ctx, index_base=other, force_kind="f32")
        seen = []

        def reduce_fn(hist):
            if not seen:
                seen.append(None)
                return ctx.to_device(hist.numpy() + np.uint64(len(q) * len(parts[other])))
            lo, shift, n_bins = windows[-1]
            seen.append(n_bins)
            return ctx.to_device(shard.merge_counts_host([hist.numpy(), real(rest, fq, lo, shift, n_bins).numpy()]))

        check_quantiles(gl.pair_distance_quantiles(q, parts[mine], QS, index_base=mine, reduce_fn=reduce_fn, **kw), want)
        assert len(seen) >= 4 and seen[1] == 2048
    monkeypatch.setattr(attack, "pair_histogram_f32", real)
    with shard.DeviceGroup(devices=[0, 0]) as group:
        check_quantiles(group.pair_distance_quantiles(q, bank=bank, quantiles=QS, batch_size=bs, distance="l2", float_path="exact"), want)
        with pytest.raises(NotImplementedError):
            group.pair_distance_quantiles(q, bank=bank, quantiles=QS, batch_size=bs, distance="l2", float_path="mfma")
    # 8-bit queries against the off-lattice bank: one fp32 layout for all levels, the codes decoded as Bank.as_f32() decodes them
    codes = synth.attack_case(31, 330, 6, 6, 16)
    q8 = np.concatenate([codes["pos"], codes["neg"]])
    M8 = frc.chain_matrix(frc.decode_u8(q8), bank[:n_eff])
    want8 = oracle_quantiles(M8, QS)
    check_quantiles(gl.pair_distance_quantiles(q8, bank, QS, **kw), want8)
    check_quantiles(gl.pair_distance_quantiles(q8, bank, QS, chunk_bytes=100 * 4 * d, **kw), want8)
    # ... and an 8-bit bank whose queries are off the lattice, streamed: the integer pass is refused before it bins anything
    MB = frc.chain_matrix(q, frc.decode_u8(codes["bank"][:n_eff]))
    check_quantiles(gl.pair_distance_quantiles(q, codes["bank"], QS, chunk_bytes=100 * 4 * d, **kw), oracle_quantiles(MB, QS))
    # both sides on one lattice: the exact-integer answer, unchanged, with or without the keyword
    exact = gl.distance_quantiles(q8, codes["bank"], QS, batch_size=bs)
    for fp in (None, "exact"):
        got = gl.pair_distance_quantiles(q8, codes["bank"], QS, distance="l2", batch_size=bs, float_path=fp)
        assert np.array_equal(got[0], exact[0]) and np.array_equal(got[1], exact[1]) and got[2] == exact[2]
    # off-lattice rows without the keyword: ball_counts' refusal
    with pytest.raises(NotImplementedError):
        gl.pair_distance_quantiles(q, bank, QS, distance="l2", batch_size=bs)
    with pytest.raises(NotImplementedError):
        gl.ball_counts(q, bank, 0.1, batch_size=bs)


def test_fp32_inf_is_counted_and_nan_is_refused(gl):
    from ganleaks_amd.attack import Bank, pair_histogram_f32
    ctx = gl.Context.get()
    bank, q = frc.table_case(43, 90, 37, 5, 4)
    bank[17] = np.float32(3e38)                         # (3e38 - x)^2 overflows: +inf against every query
    M = frc.chain_matrix(q, bank)
    assert np.isinf(M[:, 17]).all() and np.isfinite(np.delete(M, 17, axis=1)).all()
    B = bits_of(M)
    b, f = Bank.from_images(bank, ctx, force_kind="f32"), Bank.from_images(q, ctx, force_kind="f32")
    first = host(pair_histogram_f32(b, f, 0, 20, 2048))
    assert np.array_equal(first, oracle_hist(B, 0, 20, 2048)) and first[INF_BITS >> 20] == len(q) and first.sum() == M.size
    assert np.array_equal(host(pair_histogram_f32(b, f, INF_BITS, 0, 4)), [len(q), 0, 0, 0])
    assert not host(pair_histogram_f32(b, f, INF_BITS + 1, 0, 4)).any()
    qs = [0, 0.5, 1]
    got = gl.pair_distance_quantiles(q, bank, qs, distance="l2", batch_size=30, float_path="exact")
    check_quantiles(got, oracle_quantiles(M, qs))
    assert np.isinf(got[0][2]) and got[1][2] == INF_BITS
    # a NaN row has no rank
    bank[3, 5] = np.nan
    b = Bank.from_images(bank, ctx, force_kind="f32")
    first = host(pair_histogram_f32(b, f, 0, 20, 2048))
    assert first.sum() == M.size - len(q)                # its pairs lie outside the first window
    with pytest.raises(ValueError, match="NaN"):
        gl.pair_distance_quantiles(q, bank, qs, distance="l2", batch_size=30, float_path="exact")


# ---- the C ABI as a foreign host would call it

def test_bad_arguments_through_ctypes(gl, synth, model):
    from ganleaks_amd import _lib
    from ganleaks_amd.attack import Bank, new_hist
    lib = _lib.load()
    ctx = gl.Context.get()
    h = ctx.handle
    case = synth.attack_case(361, 40, 3, 2, 16, sigma=20.0)

    def expect(rc, text):
        assert rc == -1, (rc, text)
        assert text.encode() in lib.gl_last_error(), (text, lib.gl_last_error())

    hist = new_hist(ctx, 2048)
    for split in (False, True):
        fb = model.features(case["bank"], role=None if split else "bank")
        fq = model.features(case["pos"], role=None if split else "query")
        K = fb.K
        rows = (p(fb.V.ptr), p(fb.norms.ptr), fb.n, p(fq.V.ptr), p(fq.norms.ptr), fq.n)

        def call(rows=rows, K=K, lo=0, shift=20, bins=2048, hs=hist, ctx_=h, scale=fb.scale):
            hp = p(hs.ptr) if hasattr(hs, "ptr") else hs
            if split:
                return lib.gl_feat_hist(ctx_, *rows, K, lo, shift, bins, hp)
            return lib.gl_feat_hist_h1_scaled(ctx_, *rows, K, scale, lo, shift, bins, hp)

        expect(call(rows=(None,) + rows[1:]), "NULL device pointer")
        expect(call(K=K + 8), "multiple of %d" % (32 if split else 64))
        expect(call(rows=(p(fb.V.ptr + 2),) + rows[1:]), "16-byte aligned")
        expect(call(rows=rows[:2] + (-1,) + rows[3:]), "bad sizes")
        expect(call(bins=0), "n_bins=0")
        expect(call(bins=2049), "n_bins=2049")
        expect(call(shift=-1), "shift=-1")
        expect(call(shift=32), "shift=32")
        expect(call(hs=None), "NULL histogram")
        expect(call(hs=p(hist.ptr + 4)), "8-byte aligned")
        expect(call(ctx_=None), "NULL ctx")
        if not split:
            expect(call(scale=0.0), "row scale")
        ctx.sync()
        assert not hist.numpy().any()                       # the refused calls binned nothing
        assert call(rows=rows[:2] + (0,) + rows[3:]) == 0 and call(rows=rows[:5] + (0,), hs=None) == 0
        assert call(lo=INF_BITS + 1, shift=0) == 0          # above every pattern: returns early
        assert not hist.numpy().any()
    f = Bank.from_images(frc.table_case(44, 40, 37, 3, 2)[0], ctx, force_kind="f32")

    def call32(bank=p(f.rows_f32.ptr), n=40, q=p(f.rows_f32.ptr), nq=5, d=37, lo=0, shift=20, bins=2048, hs=p(hist.ptr), ctx_=h):
        return lib.gl_l2_hist_f32(ctx_, bank, n, q, nq, d, lo, shift, bins, hs)

    expect(call32(bins=0), "n_bins=0")
    expect(call32(bins=2049), "n_bins=2049")
    expect(call32(shift=-1), "shift=-1")
    expect(call32(shift=32), "shift=32")
    expect(call32(d=0), "bad sizes")
    expect(call32(n=-1), "bad sizes")
    expect(call32(bank=None), "NULL device pointer")
    expect(call32(hs=None), "NULL device pointer")
    expect(call32(hs=p(hist.ptr + 4)), "8-byte aligned")
    expect(call32(ctx_=None), "bad sizes")
    assert call32(n=0, bank=None) == 0 and call32(nq=0, q=None, hs=None) == 0 and call32(lo=INF_BITS + 1, shift=0) == 0
    assert not hist.numpy().any()
    # accumulates; gl_hist_init zeroes; gl_counts_add sums shards as [n_bins][1] counters; the l2-lpips pass reports as feat_count
    assert call32() == 0
    once = hist.numpy().copy()
    assert once.sum() == 5 * 40
    assert call32() == 0
    assert np.array_equal(hist.numpy(), 2 * once)
    lists = ctx.to_device(np.stack([once, 3 * once]))
    assert lib.gl_counts_add(h, p(hist.ptr), p(lists.ptr), 2048, 1, 2) == 0
    assert np.array_equal(hist.numpy(), 6 * once)
    assert lib.gl_hist_init(h, p(hist.ptr), 2048) == 0 and not hist.numpy().any()
    from ganleaks_amd import lpips
    fb, fq = model.features(case["bank"], role="bank"), model.features(case["pos"], role="query")
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        lpips.feat_hist(fb, fq, 0, 20, 2048)
        prof = ctx.prof_read()
        assert prof["feat_count"][1] == 1 and prof["l2_hist"][1] == 0 and prof["feat_knn"][1] == 0, prof
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()


# ---- 6: the driver

FILES = ("eps.npy", "pos_count.npy", "neg_count.npy", "pos_mc.npy", "neg_mc.npy", "pos_loss.npy", "neg_loss.npy")


def _same_files(a, b):
    for f in FILES:
        assert open(a / f, "rb").read() == open(b / f, "rb").read(), f


def test_mc_percentile_on_tables(gl, tmp_path, monkeypatch):
    """lattice tables: --eps_percentile is --eps_pair_quantile but for the params.txt line; an off-lattice .npy table: the entry point's
    radius and ball_counts at it; alone and with --devices 0,0; a run without the option writes what it wrote before the option existed"""
    from ganleaks_amd.attack_models import mc
    rng = np.random.default_rng(197)
    F, bs = 37, 64
    tables = {"syn": rng.integers(0, 256, size=(150, F)), "pos": rng.integers(0, 256, size=(13, F)), "neg": rng.integers(0, 256, size=(11, F))}
    tables["pos"][3] = tables["syn"][40]
    for name, t in tables.items():
        np.save(tmp_path / (name + ".npy"), t.astype(np.float32))
        np.save(tmp_path / (name + "_off.npy"), (t / 3.0 + rng.normal(0, 0.05, t.shape)).astype(np.float32))
    monkeypatch.chdir(tmp_path)
    paths = lambda tag: ["--syn_data_path", str(tmp_path / ("syn%s.npy" % tag)), "--pos_data_dir", str(tmp_path / ("pos%s.npy" % tag)),     # noqa: E731
                         "--neg_data_dir", str(tmp_path / ("neg%s.npy" % tag)), "--BATCH_SIZE", str(bs)]
    base = paths("")
    out = tmp_path / "mc_attack"
    mc.main(mc.parse_arguments(base + ["--exp_name", "pair", "--eps_pair_quantile", "0.01"]))
    mc.main(mc.parse_arguments(base + ["--exp_name", "pct", "--eps_percentile", "0.01"]))
    mc.main(mc.parse_arguments(base + ["--exp_name", "pct2", "--eps_percentile", "0.01", "--devices", "0,0"]))
    mc.main(mc.parse_arguments(base + ["--exp_name", "plain"]))
    _same_files(out / "pair", out / "pct")
    _same_files(out / "pair", out / "pct2")
    a, b = open(out / "pair" / "params.txt").read().splitlines(), open(out / "pct" / "params.txt").read().splitlines()
    rest = lambda lines, own: [l for l in lines if l != own and not l.startswith("exp_name:")]                                             # noqa: E731
    assert rest(a, "eps_pair_quantile:0.01") == rest(b, "eps_percentile:0.01") and len(a) == len(b)
    assert "eps_percentile:0.01" in b and "eps_percentile:0.01" not in a and not any(l.startswith("eps_pair_quantile") for l in b)
    want_params = ["exp_name:plain", "syn_data_path:%s" % (tmp_path / "syn.npy"), "pos_data_dir:%s" % (tmp_path / "pos.npy"),
                   "neg_data_dir:%s" % (tmp_path / "neg.npy"), "resolution:64", "BATCH_SIZE:64", "local_config:None", "ngpu:1", "devices:None",
                   "eps:None", "distance:l2", "eps_quantile:None"]
    assert open(out / "plain" / "params.txt").read() == "".join(line + "\n" for line in want_params)
    # the plain run: the median heuristic on the nearest distances, as before
    q = np.concatenate([tables["pos"], tables["neg"]]).astype(np.float32)
    top1 = gl.attack(q, tables["syn"].astype(np.float32), distance="l2", batch_size=bs)[0]
    eps_plain = np.asarray([np.quantile(top1, 0.5, method="lower")], np.float32)
    assert np.array_equal(np.load(out / "plain" / "eps.npy"), eps_plain)
    counts = gl.ball_counts(q, tables["syn"].astype(np.float32), eps_plain, batch_size=bs)
    assert np.array_equal(np.concatenate([np.load(out / "plain" / "pos_count.npy"), np.load(out / "plain" / "neg_count.npy")]), counts)
    # off the lattices
    off = paths("_off")
    mc.main(mc.parse_arguments(off + ["--exp_name", "off", "--eps_percentile", "0.5,0.001,0.01"]))
    mc.main(mc.parse_arguments(off + ["--exp_name", "off2", "--eps_percentile", "0.5,0.001,0.01", "--devices", "0,0"]))
    _same_files(out / "off", out / "off2")
    syn, qo = np.load(tmp_path / "syn_off.npy"), np.concatenate([np.load(tmp_path / "pos_off.npy"), np.load(tmp_path / "neg_off.npy")])
    n_eff = 128
    M = frc.chain_matrix(qo, syn[:n_eff])
    want = oracle_quantiles(M, [0.5, 0.001, 0.01])
    eps = np.load(out / "off" / "eps.npy")
    assert eps.dtype == np.float32 and np.array_equal(eps, want[0])
    assert np.array_equal(eps, gl.pair_distance_quantiles(qo, syn, [0.5, 0.001, 0.01], distance="l2", batch_size=bs, float_path="exact")[0])
    counts = np.concatenate([np.load(out / "off" / "pos_count.npy"), np.load(out / "off" / "neg_count.npy")])
    assert np.array_equal(counts, gl.ball_counts(qo, syn, eps, batch_size=bs, float_path="exact"))
    assert np.array_equal(counts, np.stack([(M <= e).sum(axis=1) for e in eps], axis=1))
    assert np.array_equal(np.load(out / "off" / "pos_mc.npy"), counts[:13] / float(n_eff))
    # the older option keeps its refusal on such rows
    with pytest.raises(NotImplementedError):
        mc.main(mc.parse_arguments(off + ["--exp_name", "refused", "--eps_pair_quantile", "0.01"]))


def test_mc_percentile_with_l2_lpips(tmp_path, monkeypatch, gl, synth, lin, model):
    """--distance l2-lpips --eps_percentile on small PNG folders with local synthetic weights, alone and with --devices 0,0"""
    import torch
    import PIL.Image
    from ganleaks_amd import lpips
    from ganleaks_amd.attack_models import mc, utils
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
            "--resolution", "32", "--BATCH_SIZE", "16", "--distance", "l2-lpips"]
    qs = [0.01, 0.5, 0.001]
    try:
        mc.main(mc.parse_arguments(base + ["--exp_name", "lp", "--eps_percentile", "0.01,0.5,0.001"]))
        mc.main(mc.parse_arguments(base + ["--exp_name", "lp2", "--eps_percentile", "0.01,0.5,0.001", "--devices", "0,0"]))
    finally:
        lpips.set_default_model(None)
    out = tmp_path / "mc_attack"
    _same_files(out / "lp", out / "lp2")
    assert "eps_percentile:0.01,0.5,0.001" in open(out / "lp" / "params.txt").read().splitlines()
    order = lambda name: [int(os.path.basename(x)[6:-4]) for x in utils.get_filepaths_from_dir(str(tmp_path / name), "png")]   # noqa: E731
    bank = case["bank"][order("bank")]
    queries = np.concatenate([case["pos"][order("pos")], case["neg"][order("neg")]])
    M = gl.pair_distances(queries, bank, batch_size=16, lpips=model)
    want = oracle_quantiles(M, qs)
    eps = np.load(out / "lp" / "eps.npy")
    assert eps.dtype == np.float32 and np.array_equal(eps, want[0])
    assert np.array_equal(eps, gl.pair_distance_quantiles(queries, bank, qs, batch_size=16, lpips=model)[0])
    counts = np.concatenate([np.load(out / "lp" / "pos_count.npy"), np.load(out / "lp" / "neg_count.npy")])
    assert np.array_equal(counts, gl.ball_counts(queries, bank, eps, batch_size=16, distance="l2-lpips", lpips=model))
    assert np.array_equal(counts, np.stack([(M <= e).sum(axis=1) for e in eps], axis=1))
