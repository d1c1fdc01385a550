"""GPU: attack_models/kde.py --pair_distance: the files it writes (names, dtypes, shapes), their values against the numpy weights of
tests/pair_kde_common.py over the oracle's float32 distances, pos_loss.npy = column 0, eval_roc on the directory, the sharded run writing
the same bytes, and the refusals that come before any file is read."""
import os

import numpy as np
import pytest

import gpu_common  # noqa: F401
import float_rows_common as frc
import kde_common as kc
import pair_kde_common as pk

pytestmark = pytest.mark.gpu
FILES = ("bandwidth.npy", "pos_kde_loss.npy", "neg_kde_loss.npy", "pos_kde_W.npy", "neg_kde_W.npy", "pos_D0_key.npy", "neg_D0_key.npy", "pos_loss.npy",
         "neg_loss.npy")


def check_dir(d, M, n_pos, h, n_eff):
    """the files of one run against the float32 matrix M [pos + neg, n_eff] of its distance"""
    from ganleaks_amd.attack import kde_coef
    bw = np.load(d / "bandwidth.npy")
    assert bw.dtype == np.float64 and np.array_equal(bw, np.asarray(h, np.float64))
    c32, h_eff = kde_coef(h, 1, "f32")
    pk.check_not_vacuous(M, M.min(axis=1), np.sort(c32)[::-1])
    for kind, rows in (("pos", M[:n_pos]), ("neg", M[n_pos:])):
        n, T = len(rows), len(h)
        loss, W = np.load(d / (kind + "_kde_loss.npy")), np.load(d / (kind + "_kde_W.npy"))
        key, first = np.load(d / (kind + "_D0_key.npy")), np.load(d / (kind + "_loss.npy"))
        assert loss.dtype == np.float64 and loss.shape == (n, T) and W.dtype == np.uint64 and W.shape == (n, T), kind
        assert key.dtype == np.int64 and key.shape == (n, 1) and first.dtype == np.float64 and first.shape == (n, 1), kind
        assert not (d / (kind + "_S0.npy")).exists()
        assert np.array_equal(first[:, 0], loss[:, 0])
        D0 = rows.min(axis=1)
        assert np.array_equal(key[:, 0], pk.bits_of(D0).astype(np.int64)) and np.array_equal(W, pk.want_sums(rows, D0, c32)), kind
        want = D0.astype(np.float64)[:, None] + h_eff[None, :] * np.log(float(n_eff) / (W.astype(np.float64) * 2.0 ** -40))
        assert np.array_equal(loss, want), kind


def test_kde_cli_pair_distance_l2_on_a_float_table(tmp_path, monkeypatch):
    from ganleaks_amd.attack_models import eval_roc, kde
    # 70 rows, BATCH_SIZE 64: the first 64 take part
    q, planted = pk.f32_case(4250, 30, 64, 37)
    # four queries at distance 0.068 of a bank row, so that the 0.9 quantile of the nearest distances is a bandwidth under which a good
    # part of the bank weighs something and the rest nothing (check_not_vacuous, asserted in check_dir)
    v = np.random.default_rng(4252).normal(size=(4, 37))
    q[26:] = planted[[1, 9, 17, 25]] + (v * np.sqrt(37 * 0.068) / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    bank = np.concatenate([planted, np.random.default_rng(4251).normal(0, 1, (6, 37)).astype(np.float32)])
    np.save(tmp_path / "syn.npy", bank)
    np.save(tmp_path / "pos.npy", q[:17])
    np.save(tmp_path / "neg.npy", q[17:])
    monkeypatch.chdir(tmp_path)
    base = ["--syn_data_path", str(tmp_path / "syn.npy"), "--pos_data_dir", str(tmp_path / "pos.npy"), "--neg_data_dir", str(tmp_path / "neg.npy"),
            "--BATCH_SIZE", "64"]
    M = frc.chain_matrix(q, planted)

    # refusals before any file is read (the paths named do not exist)
    nowhere = ["--syn_data_path", str(tmp_path / "nowhere"), "--pos_data_dir", str(tmp_path / "nowhere"), "--neg_data_dir", str(tmp_path / "nowhere")]
    with pytest.raises(SystemExit) as e:
        kde.main(kde.parse_arguments(nowhere + ["--pair_distance", "l2", "--distance", "l2-lpips"]))
    assert "takes the place of --distance" in str(e.value)
    with pytest.raises(SystemExit) as e:
        kde.main(kde.parse_arguments(["--syn_data_path", str(tmp_path / "nowhere.npy")] + nowhere[2:] + ["--pair_distance", "l2-lpips"]))
    assert "needs images" in str(e.value) and "2-D" in str(e.value)
    with pytest.raises(SystemExit):
        kde.main(kde.parse_arguments(base + ["--pair_distance", "l2", "--bandwidth", "0.1,-2"]))
    assert not (tmp_path / "kde_attack").exists()
    # without --pair_distance such rows are refused as ever
    with pytest.raises(SystemExit) as e:
        kde.main(kde.parse_arguments(base + ["--bandwidth", "0.1"]))
    assert "8-bit images or integer tables" in str(e.value)

    hs = pk.bandwidths_of(pk.pick_coef(M, M.min(axis=1), 3))[[1, 0, 2]].tolist()
    out = kde.main(kde.parse_arguments(base + ["--exp_name", "given", "--pair_distance", "l2", "--bandwidth", ",".join(map(repr, hs))]))[0]
    assert out == str(tmp_path / "kde_attack" / "given")
    kde.main(kde.parse_arguments(base + ["--exp_name", "given_s", "--pair_distance", "l2", "--bandwidth", ",".join(map(repr, hs)), "--devices", "0,0"]))
    kde.main(kde.parse_arguments(base + ["--exp_name", "q90", "--pair_distance", "l2", "--bandwidth_quantile", "0.9"]))
    kde.main(kde.parse_arguments(base + ["--exp_name", "q90_s", "--pair_distance", "l2", "--bandwidth_quantile", "0.9", "--devices", "0,0"]))
    q90 = float(np.quantile(M.min(axis=1).astype(np.float64), 0.9, method="lower"))
    for name, h in (("given", hs), ("given_s", hs), ("q90", [q90]), ("q90_s", [q90])):
        check_dir(tmp_path / "kde_attack" / name, M, 17, h, 64)
        lines = open(tmp_path / "kde_attack" / name / "params.txt").read().splitlines()
        assert "BATCH_SIZE:64" in lines and "pair_distance:l2" in lines
    for a, b in (("given", "given_s"), ("q90", "q90_s")):
        for f in FILES:
            assert open(tmp_path / "kde_attack" / a / f, "rb").read() == open(tmp_path / "kde_attack" / b / f, "rb").read(), (a, f)
    d = tmp_path / "kde_attack" / "given"
    auc, ap, precision = eval_roc.main(eval_roc.parse_arguments(["--attack_type", "fbb", "-ldir", str(d)]))
    assert auc == eval_roc.plot_roc(-np.load(d / "pos_loss.npy")[:, 0], -np.load(d / "neg_loss.npy")[:, 0])[3]


def _write_pngs(d, imgs_u8_nchw):
    import PIL.Image
    os.makedirs(d, exist_ok=True)
    for i, im in enumerate(imgs_u8_nchw):
        PIL.Image.fromarray(im.transpose(1, 2, 0)).save(os.path.join(d, "image_%d.png" % i))


def test_kde_cli_pair_distance_l2_lpips_on_pngs(tmp_path, monkeypatch, synth, golden_dir):
    import torch
    import ganleaks_amd as gl
    from ganleaks_amd import lpips
    from ganleaks_amd.attack_models import eval_roc, kde, utils
    from ganleaks_amd.lpips import LpipsModel
    z = np.load(os.path.join(golden_dir, "lpips_lin_v0.1.npz"))
    lin = {"lin%d" % i: z["lin%d" % i] for i in range(5)}
    torch.save({"features.%s" % k: torch.from_numpy(v) for k, v in synth.vgg16_state_dict(7).items()}, tmp_path / "vgg16.pth")
    torch.save({"lin%d.model.1.weight" % i: torch.from_numpy(lin["lin%d" % i]).view(1, -1, 1, 1) for i in range(5)}, tmp_path / "vgg_lin.pth")
    monkeypatch.setenv("GANLEAKS_VGG16_PATH", str(tmp_path / "vgg16.pth"))
    monkeypatch.setenv("GANLEAKS_LPIPS_LIN_PATH", str(tmp_path / "vgg_lin.pth"))
    lpips.set_default_model(None)
    # 75 files, BATCH_SIZE 16: the first 64 in the order of the path STRINGS take part; those are the planted rows
    planted, both = kc.planted_case(synth, 4260, 64, 17, (3, 16, 16), sigmas=(2.0, 6.0, 12.0, 20.0))
    names = sorted(range(75), key=lambda i: "image_%d.png" % i)
    files = np.random.default_rng(4261).integers(0, 256, size=(75, 3, 16, 16), dtype=np.uint8)
    files[names[:64]] = planted
    for name, rows in (("syn", files), ("pos", both[:9]), ("neg", both[9:])):
        _write_pngs(tmp_path / name, rows)
    monkeypatch.chdir(tmp_path)
    base = ["--syn_data_path", str(tmp_path / "syn"), "--pos_data_dir", str(tmp_path / "pos"), "--neg_data_dir", str(tmp_path / "neg"),
            "--resolution", "16", "--BATCH_SIZE", "16", "--pair_distance", "l2-lpips"]
    order = lambda name: [int(os.path.basename(x)[6:-4]) for x in utils.get_filepaths_from_dir(str(tmp_path / name), "png")]   # noqa: E731
    bank = files[order("syn")][:64]
    assert np.array_equal(bank, planted)
    queries = np.concatenate([both[:9][order("pos")], both[9:][order("neg")]])
    model = LpipsModel().load_state_dicts(synth.vgg16_state_dict(7), lin)
    M = gl.pair_distances(queries, bank, batch_size=16, lpips=model)
    hs = pk.bandwidths_of(pk.pick_coef(M, M.min(axis=1), 2)).tolist()
    try:
        kde.main(kde.parse_arguments(base + ["--exp_name", "given", "--bandwidth", ",".join(map(repr, hs))]))
        kde.main(kde.parse_arguments(base + ["--exp_name", "median"]))
    finally:
        lpips.set_default_model(None)
    median = float(np.quantile(M.min(axis=1).astype(np.float64), 0.5, method="lower"))
    check_dir(tmp_path / "kde_attack" / "given", M, 9, hs, 64)
    assert np.array_equal(np.load(tmp_path / "kde_attack" / "median" / "bandwidth.npy"), [median])
    d = tmp_path / "kde_attack" / "given"
    auc, ap, precision = eval_roc.main(eval_roc.parse_arguments(["--attack_type", "fbb", "-ldir", str(d)]))
    assert auc == eval_roc.plot_roc(-np.load(d / "pos_loss.npy")[:, 0], -np.load(d / "neg_loss.npy")[:, 0])[3]
