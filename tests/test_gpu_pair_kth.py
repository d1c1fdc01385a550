"""GPU: per-query radii and exact k-th neighbour distances on the float paths (pair_ball_counts_rows, pair_kth_distances, their
DeviceGroup forms, attack_models/density.py --pair_distance).
The expected values never pass through the kernels under test or through select_kth_rows: under 'l2-lpips' they are numpy on the stored
matrix pair_distances gives (tied to the search and to the fp64 oracle by tests/test_gpu_count_lpips.py), on fp32 rows numpy on the CPU
chain (float_rows_common.chain_matrix), on lattice rows kth_distances' exact S.  Every comparison is array_equal on bit patterns."""
import os

import numpy as np
import pytest

import gpu_common  # noqa: F401
import float_rows_common as frc
from test_gpu_count_lpips import _images, _RowsGenerator

pytestmark = pytest.mark.gpu
KS = [1, 5, 32, 33, 192]


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


def bits(M):
    return np.ascontiguousarray(M, np.float32).view(np.uint32)


def oracle_counts(M, eps):
    with np.errstate(over="ignore"):
        e32 = np.asarray(eps, np.float64).astype(np.float32)
    return (M[:, None, :] <= e32[:, :, None]).sum(axis=2).astype(np.int64)


def eps_rows(M, d1, seed):
    """[Q, 7] radii per query in shuffled column order: 1.1 * d1, attained values of the query's own row, a value between two of them, a
    negative one and inf"""
    rng = np.random.default_rng(seed)
    srt = np.sort(M, axis=1)
    n = M.shape[1]
    cols = np.stack([np.float32(1.1) * d1, srt[:, 0], srt[:, n // 3], np.float32(0.5) * (srt[:, n // 2] + srt[:, n // 2 + 1]), srt[:, -1],
                     np.full(len(M), -1.0, np.float32), np.full(len(M), np.inf, np.float32)], axis=1).astype(np.float32)
    return np.stack([row[rng.permutation(cols.shape[1])] for row in cols])


def check_kth(got, M, ks, passes=None):
    dist, key, p = got
    assert dist.dtype == np.float32 and key.dtype == np.int64 and dist.shape == key.shape == (len(M), len(ks))
    want = np.sort(M, axis=1)[:, np.asarray(ks) - 1]
    assert np.array_equal(key, bits(want).astype(np.int64)), np.argwhere(key != bits(want))[:5]
    assert np.array_equal(bits(dist), bits(want))
    assert p == (8 * len(set(ks)) if passes is None else passes)


@pytest.fixture(scope="module")
def lpips_case(gl, synth, oracle, model):
    """40 queries x 200 images of 32 x 32 (batch 64: 192 rows take part), the stored matrix computed once"""
    bank, q = _images(synth, oracle, 361, 200, 40, 32, "u8")
    M = gl.pair_distances(q, bank[:192], batch_size=64, lpips=model)
    assert M.shape == (40, 192)
    M.setflags(write=False)
    return bank, q, M


def test_l2_lpips_counts_and_kth(gl, model, lpips_case):
    bank, q, M = lpips_case
    kw = dict(distance="l2-lpips", batch_size=64, lpips=model)
    d1, _ = gl.attack(q, bank, **kw)
    assert np.array_equal(d1, M.min(axis=1))
    eps = eps_rows(M, d1, 1)
    got = gl.pair_ball_counts_rows(q, bank, eps, **kw)
    assert got.dtype == np.int64 and np.array_equal(got, oracle_counts(M, eps))
    # row q is ball_counts of query q alone with its own radii
    for i in (0, 17, 39):
        assert np.array_equal(got[i], gl.ball_counts(q[i:i + 1], bank, eps[i], **kw)[0])
    res = gl.pair_kth_distances(q, bank, KS, **kw)
    check_kth(res, M, KS)
    nn, _ = gl.nearest_neighbours(q, bank, 32, **kw)
    assert np.array_equal(bits(res[0][:, :3]), bits(nn[:, [0, 4, 31]]))
    assert np.all(gl.pair_ball_counts_rows(q, bank, res[0], **kw) >= np.asarray(KS)[None, :])
    # a scalar k, repeats and any order
    check_kth(gl.pair_kth_distances(q, bank, 7, **kw), M, [7])
    check_kth(gl.pair_kth_distances(q, bank, [33, 2, 33], **kw), M, [33, 2, 33])
    with pytest.raises(ValueError, match="k=193 exceeds the 192"):
        gl.pair_kth_distances(q, bank, 193, **kw)
    with pytest.raises(ValueError):
        gl.pair_ball_counts_rows(q, bank, eps[:39], **kw)


def test_l2_lpips_bank_forms_agree(gl, model, lpips_case, monkeypatch):
    import importlib
    from ganleaks_amd.attack import GeneratedBank
    attack = importlib.import_module("ganleaks_amd.attack")
    ctx = gl.Context.get()
    bank, q, M = lpips_case
    kw = dict(distance="l2-lpips", batch_size=64, lpips=model)
    ks = [5, 33]
    d1 = M.min(axis=1)
    eps = eps_rows(M, d1, 2)
    want_c = oracle_counts(M, eps)
    row = 2 * int(ctx.lib.gl_lpips_lattice_dim(32, 32))
    fb, fq = model.features(bank[:192], role="bank"), model.features(q, role="query")
    gen = GeneratedBank(_RowsGenerator(ctx, bank), np.arange(len(bank)))
    forms = [(fq, fb, {}), (q, fb, {}), (q, bank, dict(chunk_bytes=70 * row)), (q, ctx.to_device(bank), dict(chunk_bytes=70 * row)),
             (q, gen, dict(chunk_bytes=70 * row)), (fq, bank, dict(chunk_bytes=70 * row))]
    for qq, bb, extra in forms:
        check_kth(gl.pair_kth_distances(qq, bb, ks, **dict(kw, **extra)), M, ks)
        assert np.array_equal(gl.pair_ball_counts_rows(qq, bb, eps, **dict(kw, **extra)), want_c)
    # the queries in 3 slices on top of the chunks: thresholds and counters are sliced with them
    monkeypatch.setattr(attack, "_query_budget_bytes", lambda chunk_bytes, ctx=None: int(15.5 * row))
    check_kth(gl.pair_kth_distances(q, bank, ks, chunk_bytes=70 * row, **kw), M, ks)
    assert np.array_equal(gl.pair_ball_counts_rows(q, gen, eps, chunk_bytes=70 * row, **kw), want_c)


def test_l2_lpips_one_layout_for_all_passes(gl, synth, oracle, model):
    """a streamed float bank whose middle chunk is off the lattice: the first pass starts over in the hi / lo layout with fresh counters and
    every later pass starts there; the answer is the one with every row given as hi / lo rows from the start"""
    ctx = gl.Context.get()
    codes, q = _images(synth, oracle, 362, 200, 40, 32, "u8")
    bank = oracle.dequantize_u8(codes).astype(np.float32)                      # floats on the lattice ...
    rng = np.random.default_rng(6)
    bank[70:140] = np.clip(bank[70:140] + rng.normal(0, 0.01, bank[70:140].shape).astype(np.float32), -1, 1)      # ... but for the middle chunk
    fb, fq = model.features(bank[:192], role="bank", fmt="hilo"), model.features(q, role="query", fmt="hilo")
    M = gl.pair_distances(fq, fb, batch_size=64)
    ks = [3, 40]
    eps = eps_rows(M, M.min(axis=1), 3)
    row = 2 * int(ctx.lib.gl_lpips_lattice_dim(32, 32))                        # 70 lattice rows per chunk: [0, 70), [70, 140), [140, 192)
    kw = dict(distance="l2-lpips", batch_size=64, lpips=model)
    check_kth(gl.pair_kth_distances(fq, fb, ks, batch_size=64), M, ks)
    check_kth(gl.pair_kth_distances(q, bank, ks, chunk_bytes=70 * row, **kw), M, ks)
    check_kth(gl.pair_kth_distances(q, bank, ks, **kw), M, ks)                # resident: both sides hi / lo
    assert np.array_equal(gl.pair_ball_counts_rows(q, bank, eps, chunk_bytes=70 * row, **kw), oracle_counts(M, eps))


@pytest.fixture(scope="module")
def float_case(synth):
    """off-lattice float images: 330 x 3 x 16 x 16 (batch 30: all take part) against 12 queries; the CPU chain matrix computed once"""
    bank, q = frc.image_case(synth, 31, 330, 6, 6, 16)
    bank[300] = bank[12]
    q[0] = bank[12]
    M = frc.chain_matrix(q, bank)
    M.setflags(write=False)
    return bank, q, M


def test_l2_float_rows(gl, synth, float_case):
    bank, q, M = float_case
    d = 768
    kw = dict(distance="l2", batch_size=30, float_path="exact")
    ks = [1, 18, 33, 330]
    eps = eps_rows(M, M.min(axis=1), 4)
    check_kth(gl.pair_kth_distances(q, bank, ks, **kw), M, ks)
    assert np.array_equal(gl.pair_ball_counts_rows(q, bank, eps, **kw), oracle_counts(M, eps))
    for i in (0, 11):
        assert np.array_equal(gl.pair_ball_counts_rows(q, bank, eps, **kw)[i], gl.ball_counts(q[i:i + 1], bank, eps[i], batch_size=30, float_path="exact")[0])
    nn, _ = gl.nearest_neighbours(q, bank, 32, **kw)
    assert np.array_equal(bits(gl.pair_kth_distances(q, bank, [1, 18], **kw)[0]), bits(nn[:, [0, 17]]))
    # streamed in 4 chunks, the last one ragged
    check_kth(gl.pair_kth_distances(q, bank, ks, chunk_bytes=100 * 4 * d, **kw), M, ks)
    assert np.array_equal(gl.pair_ball_counts_rows(q, bank, eps, chunk_bytes=100 * 4 * d, **kw), oracle_counts(M, eps))
    # without the keyword such rows raise what the old spellings raise
    for call in (lambda: gl.pair_kth_distances(q, bank, 3, distance="l2", batch_size=30),
                 lambda: gl.pair_ball_counts_rows(q, bank, eps, distance="l2", batch_size=30)):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert "exact-integer" in str(e.value)
    with pytest.raises(ValueError, match="k=331 exceeds the 330"):
        gl.pair_kth_distances(q, bank, 331, **kw)
    # a NaN row has no rank; a row at +inf has one
    bad = bank.copy()
    bad[17, 0, 3, 3] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        gl.pair_kth_distances(q, bad, 5, **kw)
    far = bank.copy()
    far[17, 0, 3, 3] = np.float32(3.0e38)
    Mf = M.copy()
    Mf[:, 17] = np.inf
    check_kth(gl.pair_kth_distances(q, far, [5, 330], **kw), Mf, [5, 330])
    assert np.array_equal(gl.pair_ball_counts_rows(q, far, eps, **kw), oracle_counts(Mf, eps))
    # 8-bit queries against the float bank: decoded, the whole call on fp32 rows
    case = synth.attack_case(31, 330, 6, 6, 16)
    q8 = np.concatenate([case["pos"], case["neg"]])
    M8 = frc.chain_matrix(frc.decode_u8(q8), bank)
    check_kth(gl.pair_kth_distances(q8, bank, [2, 40], **kw), M8, [2, 40])


def test_l2_lattice_rows_take_the_exact_integer_path(gl, synth):
    case = synth.attack_case(33, 330, 6, 6, 16)
    bank, q = case["bank"], np.concatenate([case["pos"], case["neg"]])
    want = gl.kth_distances(q, bank, [1, 40], batch_size=30)
    for fp in (None, "exact"):
        got = gl.pair_kth_distances(q, bank, [1, 40], distance="l2", batch_size=30, float_path=fp)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]) and got[2] == want[2]      # key == S
        eps = np.stack([want[0][:, 1], want[0][:, 0] * np.float32(1.1)], axis=1)
        assert np.array_equal(gl.pair_ball_counts_rows(q, bank, eps, distance="l2", batch_size=30, float_path=fp),
                              gl.ball_counts_rows(q, bank, eps, batch_size=30))


def test_device_group_equals_the_single_device(gl, synth, lin, model, lpips_case, float_case):
    from ganleaks_amd import shard
    from ganleaks_amd.lpips import LpipsModel
    bank, q, M = lpips_case
    make = lambda c: LpipsModel(c).load_state_dicts(synth.vgg16_state_dict(7), lin)                     # noqa: E731
    ks = [5, 33]
    eps = eps_rows(M, M.min(axis=1), 5)
    with shard.DeviceGroup(devices=[0, 0]) as group:
        assert group.collective == "host-merge"
        check_kth(group.pair_kth_distances(q, bank=bank, k=ks, batch_size=64, make_lpips=make), M, ks)
        assert np.array_equal(group.pair_ball_counts_rows(q, bank=bank, eps=eps, batch_size=64, make_lpips=make), oracle_counts(M, eps))
        with pytest.raises(ValueError, match="k=193 exceeds the 192"):
            group.pair_kth_distances(q, bank=bank, k=193, batch_size=64, make_lpips=make)
        assert not group._broken
    fbank, fq, FM = float_case
    feps = eps_rows(FM, FM.min(axis=1), 6)
    with shard.DeviceGroup(devices=[0, 0]) as group:
        check_kth(group.pair_kth_distances(fq, bank=fbank, k=ks, batch_size=30, distance="l2", float_path="exact"), FM, ks)
        assert np.array_equal(group.pair_ball_counts_rows(fq, bank=fbank, eps=feps, batch_size=30, distance="l2", float_path="exact"),
                              oracle_counts(FM, feps))
    check_kth(shard.pair_kth_distances_on_devices(fq, bank=fbank, k=[18], devices=[0, 0], batch_size=30, distance="l2", float_path="exact"), FM, [18])
    assert np.array_equal(shard.pair_ball_counts_rows_on_devices(fq, bank=fbank, eps=feps, devices=[0, 0], batch_size=30, distance="l2",
                                                                 float_path="exact"), oracle_counts(FM, feps))


def _write_pngs(d, imgs_u8_nchw):
    import PIL.Image
    os.makedirs(d, exist_ok=True)
    for i, im in enumerate(imgs_u8_nchw):
        PIL.Image.fromarray(im.transpose(1, 2, 0)).save(os.path.join(d, "image_%d.png" % i))


def test_density_cli_with_pair_distance(tmp_path, monkeypatch, gl, synth, lin, model):
    import torch
    from ganleaks_amd import lpips
    from ganleaks_amd.attack_models import density, eval_roc, utils
    torch.save({"features.%s" % k: torch.from_numpy(v) for k, v in synth.vgg16_state_dict(7).items()}, tmp_path / "vgg16.pth")
    torch.save({"lin%d.model.1.weight" % i: torch.from_numpy(lin["lin%d" % i]).view(1, -1, 1, 1) for i in range(5)}, tmp_path / "vgg_lin.pth")
    monkeypatch.setenv("GANLEAKS_VGG16_PATH", str(tmp_path / "vgg16.pth"))
    monkeypatch.setenv("GANLEAKS_LPIPS_LIN_PATH", str(tmp_path / "vgg_lin.pth"))
    lpips.set_default_model(None)
    case = synth.attack_case(295, 75, 9, 8, 16, sigma=20.0)               # 75 is not a multiple of BATCH_SIZE 16: 64 rows take part
    ref = synth.perturb_u8(296, synth.attack_case(297, 40, 1, 1, 16)["bank"], 4.0)       # 40 rows: 32 take part
    for name, rows in (("syn", case["bank"]), ("pos", case["pos"]), ("neg", case["neg"]), ("ref", ref)):
        _write_pngs(tmp_path / name, rows)
    monkeypatch.chdir(tmp_path)
    base = ["--syn_data_path", str(tmp_path / "syn"), "--pos_data_dir", str(tmp_path / "pos"), "--neg_data_dir", str(tmp_path / "neg"),
            "--resolution", "16", "--BATCH_SIZE", "16"]
    order = lambda name: [int(os.path.basename(x)[6:-4]) for x in utils.get_filepaths_from_dir(str(tmp_path / name), "png")]   # noqa: E731
    bank, refs = case["bank"][order("syn")], ref[order("ref")]
    queries = np.concatenate([case["pos"][order("pos")], case["neg"][order("neg")]])
    try:
        density.main(density.parse_arguments(base + ["--exp_name", "k3", "--K", "3", "--pair_distance", "l2-lpips"]))
        density.main(density.parse_arguments(base + ["--exp_name", "ratio", "--K", "3", "--pair_distance", "l2-lpips", "--ref_data_dir", str(tmp_path / "ref"),
                                                     "--K_ref", "2"]))
    finally:
        lpips.set_default_model(None)
    kw = dict(distance="l2-lpips", batch_size=16, lpips=model)
    d_syn, k_syn, _ = gl.pair_kth_distances(queries, bank, 3, **kw)
    d_ref, k_ref, _ = gl.pair_kth_distances(queries, refs, 2, **kw)
    M = gl.pair_distances(queries, bank[:64], batch_size=16, lpips=model)
    assert np.array_equal(bits(d_syn[:, 0]), bits(np.sort(M, axis=1)[:, 2]))
    out = tmp_path / "density_attack"
    load = lambda name, f: np.concatenate([np.load(out / name / ("pos_" + f)), np.load(out / name / ("neg_" + f))])          # noqa: E731
    loss, key = load("k3", "loss.npy"), load("k3", "kth_key.npy")
    assert loss.dtype == np.float64 and loss.shape == (17, 1) and key.dtype == np.int64 and key.shape == (17, 1)
    assert np.array_equal(loss, d_syn.astype(np.float64)) and np.array_equal(key, k_syn)
    assert np.load(out / "k3" / "pos_loss.npy").shape == (9, 1) and not (out / "k3" / "pos_kth_S.npy").exists()
    assert "K:3" in open(out / "k3" / "params.txt").read().splitlines()
    loss, key = load("ratio", "loss.npy"), load("ratio", "kth_key.npy")
    assert key.shape == (17, 2) and np.array_equal(key, np.concatenate([k_syn, k_ref], axis=1))
    assert loss.shape == (17, 1) and np.array_equal(loss[:, 0], gl.density_ratio_loss_f32(d_syn[:, 0], d_ref[:, 0]))
    # --pair_distance l2 on floats off both lattices, from an .npz
    rng = np.random.default_rng(7)
    np.savez(tmp_path / "floats.npz", img_r01=rng.random((70, 16, 16, 3)).astype(np.float32))
    density.main(density.parse_arguments(["--syn_data_path", str(tmp_path / "floats.npz")] + base[2:] + ["--exp_name", "off", "--K", "3", "--pair_distance", "l2"]))
    from ganleaks_amd.bank_io import load_rows
    rows = load_rows(str(tmp_path / "floats.npz"), 16)
    Mf = frc.chain_matrix(frc.decode_u8(queries), rows[:64])
    loss = load("off", "loss.npy")
    assert np.array_equal(loss[:, 0], np.sort(Mf, axis=1)[:, 2].astype(np.float64))
    # eval_roc reads the directories as they stand
    for name in ("k3", "ratio", "off"):
        d = out / name
        auc, ap, precision = eval_roc.main(eval_roc.parse_arguments(["--attack_type", "fbb", "-ldir", str(d)]))
        assert auc == eval_roc.plot_roc(-np.load(d / "pos_loss.npy")[:, 0], -np.load(d / "neg_loss.npy")[:, 0])[3]
