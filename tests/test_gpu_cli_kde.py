"""GPU: attack_models/kde.py on PNG directories: the files it writes (names, dtypes, shapes), their values against the numpy oracle of
tests/kde_common.py on host-computed S, pos_loss.npy = column 0, eval_roc on the directory, the sharded run writing the same bytes, and the
refusals that come before any file is read."""
import os

import numpy as np
import pytest

import gpu_common  # noqa: F401
import kde_common as kc

pytestmark = pytest.mark.gpu


def _write_pngs(d, imgs_u8_nchw, prefix="image_"):
    import PIL.Image
    os.makedirs(d, exist_ok=True)
    for i, im in enumerate(imgs_u8_nchw):
        PIL.Image.fromarray(im.transpose(1, 2, 0)).save(os.path.join(d, "%s%d.png" % (prefix, i)))


def test_kde_cli(tmp_path, monkeypatch, synth):
    from ganleaks_amd.attack_models import eval_roc, kde, utils
    # 150 files, BATCH_SIZE 64: the first 128 in the order of the path STRINGS take part.  Those 128 are planted rows (clusters and
    # near-duplicate queries at noise levels chosen so that the median heuristic's bandwidth, too, meets both conditions of
    # kde_common.check_not_vacuous, asserted below); the other 22 are random rows that the truncation must drop
    planted, both = kc.planted_case(synth, 4170, 128, 47, (3, 16, 16), sigmas=(2.0, 21.0, 21.0, 40.0))
    names = sorted(range(150), key=lambda i: "image_%d.png" % i)
    files = np.random.default_rng(4171).integers(0, 256, size=(150, 3, 16, 16), dtype=np.uint8)
    files[names[:128]] = planted
    case = {"bank": files, "pos": both[:25], "neg": both[25:]}
    for name, rows in (("syn", case["bank"]), ("pos", case["pos"]), ("neg", case["neg"])):
        _write_pngs(tmp_path / name, rows)
    monkeypatch.chdir(tmp_path)
    base = ["--syn_data_path", str(tmp_path / "syn"), "--pos_data_dir", str(tmp_path / "pos"), "--neg_data_dir", str(tmp_path / "neg"),
            "--resolution", "16", "--BATCH_SIZE", "64"]
    order = lambda name: [int(os.path.basename(x)[6:-4]) for x in utils.get_filepaths_from_dir(str(tmp_path / name), "png")]   # noqa: E731
    bank = case["bank"][order("syn")][:128]
    assert np.array_equal(bank, planted)
    queries = {kind: case[kind][order(kind)] for kind in ("pos", "neg")}
    unit = 65025.0 * 768 / 4.0
    S = {kind: kc.host_S(queries[kind], bank) for kind in ("pos", "neg")}
    pooled = np.concatenate([S["pos"], S["neg"]])
    top1 = pooled.min(axis=1)
    dist32 = (top1.astype(np.float64) / unit).astype(np.float32)

    # --distance l2-lpips: refused with the reason before any file is read (the folders named do not exist)
    with pytest.raises(SystemExit) as e:
        kde.main(kde.parse_arguments(["--syn_data_path", str(tmp_path / "nowhere"), "--pos_data_dir", str(tmp_path / "nowhere"), "--neg_data_dir",
                                      str(tmp_path / "nowhere"), "--distance", "l2-lpips"]))
    assert "rounded float" in str(e.value)
    assert not (tmp_path / "kde_attack").exists()
    with pytest.raises(SystemExit):
        kde.main(kde.parse_arguments(base + ["--bandwidth", "0.1,-2"]))
    with pytest.raises(SystemExit):
        kde.main(kde.parse_arguments(base + ["--bandwidth", "0.1", "--bandwidth_quantile", "0.5"]))

    # bandwidths given, any order; the default (the median heuristic); the sharded runs
    ladder = np.log2(np.e) / (kc.pick_coef(pooled, top1, 3).astype(np.float64) * unit)      # ascending; given out of order
    hs = [float(ladder[1]), float(ladder[0]), float(ladder[2])]
    out = kde.main(kde.parse_arguments(base + ["--exp_name", "given", "--bandwidth", ",".join(map(str, hs))]))[0]
    assert out == str(tmp_path / "kde_attack" / "given")
    kde.main(kde.parse_arguments(base + ["--exp_name", "given_s", "--bandwidth", ",".join(map(str, hs)), "--devices", "0,0"]))
    kde.main(kde.parse_arguments(base + ["--exp_name", "median"]))
    kde.main(kde.parse_arguments(base + ["--exp_name", "median_s", "--ngpu", "1", "--devices", "0,0"]))
    kde.main(kde.parse_arguments(base + ["--exp_name", "q40", "--bandwidth_quantile", "0.4"]))
    median = float(np.quantile(dist32.astype(np.float64), 0.5, method="lower"))
    q40 = float(np.quantile(dist32.astype(np.float64), 0.4, method="lower"))
    for name, h in (("given", hs), ("given_s", hs), ("median", [median]), ("median_s", [median]), ("q40", [q40])):
        d = tmp_path / "kde_attack" / name
        bw = np.load(d / "bandwidth.npy")
        assert bw.dtype == np.float64 and np.array_equal(bw, np.asarray(h, np.float64)), name
        T = len(h)
        c32 = np.float32(np.log2(np.e) / (np.asarray(h, np.float64) * unit))
        h_eff = np.log2(np.e) / (c32.astype(np.float64) * unit)
        for kind, n in (("pos", 25), ("neg", 22)):
            kc.check_not_vacuous(S[kind] - S[kind].min(axis=1)[:, None], np.sort(c32)[::-1])
            loss, W = np.load(d / (kind + "_kde_loss.npy")), np.load(d / (kind + "_kde_W.npy"))
            S0, first = np.load(d / (kind + "_S0.npy")), np.load(d / (kind + "_loss.npy"))
            assert loss.dtype == np.float64 and loss.shape == (n, T) and W.dtype == np.uint64 and W.shape == (n, T), (name, kind)
            assert S0.dtype == np.int64 and S0.shape == (n, 1) and first.dtype == np.float64 and first.shape == (n, 1), (name, kind)
            assert np.array_equal(first[:, 0], loss[:, 0])
            assert np.array_equal(S0[:, 0], S[kind].min(axis=1)) and np.array_equal(W, kc.want_sums(S[kind], S0[:, 0], c32)), (name, kind)
            want = S0.astype(np.float64) / unit + h_eff[None, :] * np.log(128.0 / (W.astype(np.float64) * 2.0 ** -40))
            assert np.array_equal(loss, want), (name, kind)
        assert "BATCH_SIZE:64" in open(d / "params.txt").read().splitlines()
    for a, b in (("given", "given_s"), ("median", "median_s")):
        for f in ("bandwidth.npy", "pos_kde_loss.npy", "neg_kde_loss.npy", "pos_kde_W.npy", "neg_kde_W.npy", "pos_S0.npy", "neg_S0.npy", "pos_loss.npy",
                  "neg_loss.npy"):
            assert open(tmp_path / "kde_attack" / a / f, "rb").read() == open(tmp_path / "kde_attack" / b / f, "rb").read(), (a, f)

    # eval_roc reads the directory as it stands
    d = tmp_path / "kde_attack" / "given"
    auc, ap, precision = eval_roc.main(eval_roc.parse_arguments(["--attack_type", "fbb", "-ldir", str(d)]))
    assert auc == eval_roc.plot_roc(-np.load(d / "pos_loss.npy")[:, 0], -np.load(d / "neg_loss.npy")[:, 0])[3]
    # rows off both lattices: refused before any GPU work
    np.savez(tmp_path / "floats.npz", img_r01=np.random.default_rng(1).random((70, 16, 16, 3)).astype(np.float32))
    with pytest.raises(SystemExit) as e:
        kde.main(kde.parse_arguments(["--syn_data_path", str(tmp_path / "floats.npz")] + base[2:] + ["--exp_name", "off", "--bandwidth", "0.1"]))
    assert "8-bit images or integer tables" in str(e.value)
