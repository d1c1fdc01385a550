"""GPU: fbb's --knn_out on PNG directories: the K nearest samples of every query next to the files of a plain run, which stay
byte-identical."""
import os

import numpy as np
import pytest

import gpu_common  # noqa: F401

pytestmark = pytest.mark.gpu


def _write_pngs(d, imgs_u8_nchw, prefix="image_"):
    import PIL.Image
    os.makedirs(d, exist_ok=True)
    for i, im in enumerate(imgs_u8_nchw):
        PIL.Image.fromarray(im.transpose(1, 2, 0)).save(os.path.join(d, "%s%d.png" % (prefix, i)))


def test_fbb_knn_out(tmp_path, monkeypatch, synth):
    import c_oracle
    from ganleaks_amd.attack_models import fbb, utils
    case = synth.attack_case(82, 150, 25, 22, 16)        # 150 is not a multiple of BATCH_SIZE 64: 128 rows take part
    for name in ("syn", "pos", "neg"):
        _write_pngs(tmp_path / name, case["bank" if name == "syn" else name])
    monkeypatch.chdir(tmp_path)
    base = ["--syn_data_path", str(tmp_path / "syn"), "--pos_data_dir", str(tmp_path / "pos"), "--neg_data_dir", str(tmp_path / "neg"),
            "--resolution", "16", "--BATCH_SIZE", "64", "--distance", "l2", "--K", "5"]
    fbb.main(fbb.parse_arguments(base + ["--exp_name", "plain"]))
    fbb.main(fbb.parse_arguments(base + ["--exp_name", "knn", "--knn_out"]))
    fbb.main(fbb.parse_arguments(base + ["--exp_name", "knn3", "--knn_out", "--devices", "0,0,0"]))
    plain, knn, knn3 = (tmp_path / "fbb_attack" / n for n in ("plain", "knn", "knn3"))
    # without the flag --K stays inert: no new file, and the recorded arguments do not mention the flag
    assert not any(f.startswith(("pos_knn", "neg_knn")) for f in os.listdir(plain))
    recorded = lambda d: [line.split(":")[0] for line in open(d / "params.txt").read().splitlines()]   # noqa: E731
    assert "knn_out" not in recorded(plain) and "knn_out:True" in open(knn / "params.txt").read().splitlines()
    for f in ("pos_loss.npy", "neg_loss.npy", "pos_nn_idx.npy", "neg_nn_idx.npy", "pos_idx.npy", "neg_idx.npy"):
        assert open(plain / f, "rb").read() == open(knn / f, "rb").read() == open(knn3 / f, "rb").read(), f
    order = lambda name: [int(os.path.basename(x)[6:-4]) for x in utils.get_filepaths_from_dir(str(tmp_path / name), "png")]   # noqa: E731
    bank = case["bank"][order("syn")][:128]
    for kind, n in (("pos", 25), ("neg", 22)):
        queries = case[kind][order(kind)]
        loss, idx = np.load(knn / (kind + "_knn_loss.npy")), np.load(knn / (kind + "_knn_idx.npy"))
        assert loss.shape == (n, 5) and loss.dtype == np.float64 and idx.shape == (n, 5) and idx.dtype == np.int64
        for qi in range(n):
            S = c_oracle.ssd_row_u8(bank, queries[qi])
            o = np.argsort(S, kind="stable")[:5]
            assert np.array_equal(idx[qi], o), (kind, qi)
            want = (S[o].astype(np.float64) * (4.0 / (65025.0 * 768))).astype(np.float32).astype(np.float64)
            assert np.array_equal(loss[qi], want), (kind, qi)
        assert np.array_equal(loss[:, :1], np.load(knn / (kind + "_loss.npy"))) and np.array_equal(idx[:, :1], np.load(knn / (kind + "_nn_idx.npy")))
        assert np.array_equal(np.load(knn3 / (kind + "_knn_idx.npy")), idx) and np.array_equal(np.load(knn3 / (kind + "_knn_loss.npy")), loss)


def test_fbb_knn_out_refused_for_lpips(tmp_path, monkeypatch):
    from ganleaks_amd.attack_models import fbb
    monkeypatch.chdir(tmp_path)
    os.makedirs(tmp_path / "syn")
    # the folders are empty and need not exist: the flag is refused before anything is read
    args = fbb.parse_arguments(["--syn_data_path", str(tmp_path / "syn"), "--pos_data_dir", str(tmp_path / "nowhere"), "--neg_data_dir",
                                str(tmp_path / "nowhere"), "--distance", "l2-lpips", "--knn_out"])
    with pytest.raises(SystemExit) as e:
        fbb.main(args)
    assert "--knn_out needs --distance l2" in str(e.value)
    assert not (tmp_path / "fbb_attack").exists()
    with pytest.raises(SystemExit) as e:
        fbb.main(fbb.parse_arguments(["--syn_data_path", str(tmp_path / "syn"), "--distance", "l2", "--knn_out", "--K", "40"]))
    assert "--K" in str(e.value)
