"""GPU: attack_models/density.py on PNG directories: --K 1 reproduces fbb.py --distance l2, a K beyond 32 equals the host oracle, the
calibrated form equals the formula on host-computed S, eval_roc scores the directory, and the sharded run writes the same bytes."""
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


def _host_S(q, b):
    """int64 [Q, N]: the exact sum of squared differences of every pair, from a float64 matmul (exact: every sum stays below 2^53)"""
    qf, bf = q.reshape(len(q), -1).astype(np.float64), b.reshape(len(b), -1).astype(np.float64)
    return ((qf * qf).sum(axis=1)[:, None] + (bf * bf).sum(axis=1)[None, :] - 2.0 * (qf @ bf.T)).astype(np.int64)


def test_density_cli(tmp_path, monkeypatch, synth):
    from ganleaks_amd.attack_models import density, eval_roc, fbb, knn, utils
    case = synth.attack_case(282, 150, 25, 22, 16)        # 150 is not a multiple of BATCH_SIZE 64: 128 rows take part
    ref = synth.perturb_u8(283, synth.attack_case(284, 100, 1, 1, 16)["bank"], 4.0)       # 100 rows: 64 take part
    ref[3] = case["pos"][2]                               # a query that is in the reference set: S_ref = 0 at K_ref = 1
    for name, rows in (("syn", case["bank"]), ("pos", case["pos"]), ("neg", case["neg"]), ("ref", ref)):
        _write_pngs(tmp_path / name, rows)
    monkeypatch.chdir(tmp_path)
    base = ["--syn_data_path", str(tmp_path / "syn"), "--pos_data_dir", str(tmp_path / "pos"), "--neg_data_dir", str(tmp_path / "neg"),
            "--resolution", "16", "--BATCH_SIZE", "64"]
    order = lambda name: [int(os.path.basename(x)[6:-4]) for x in utils.get_filepaths_from_dir(str(tmp_path / name), "png")]   # noqa: E731
    bank, refs = case["bank"][order("syn")][:128], ref[order("ref")][:64]
    queries = {kind: case[kind][order(kind)] for kind in ("pos", "neg")}
    dist64 = lambda S: (S.astype(np.float64) * (4.0 / (65025.0 * 768))).astype(np.float32).astype(np.float64)   # noqa: E731

    # --K 1: fbb.py --distance l2's loss files, bit for bit
    fbb.main(fbb.parse_arguments(base + ["--exp_name", "plain", "--distance", "l2"]))
    out1 = density.main(density.parse_arguments(base + ["--exp_name", "k1", "--K", "1"]))[0]
    assert out1 == str(tmp_path / "density_attack" / "k1")
    for f in ("pos_loss.npy", "neg_loss.npy"):
        assert open(tmp_path / "fbb_attack" / "plain" / f, "rb").read() == open(tmp_path / "density_attack" / "k1" / f, "rb").read(), f

    # --K 40: the host oracle; --K 5: column 4 of knn.py; the default K is floor(sqrt(128)) = 11; the sharded run writes the same bytes
    density.main(density.parse_arguments(base + ["--exp_name", "k40", "--K", "40"]))
    density.main(density.parse_arguments(base + ["--exp_name", "k40s", "--K", "40", "--devices", "0,0"]))
    density.main(density.parse_arguments(base + ["--exp_name", "k5", "--K", "5"]))
    density.main(density.parse_arguments(base + ["--exp_name", "auto"]))
    knn.main(knn.parse_arguments(base + ["--exp_name", "knn5", "--K", "5", "--distance", "l2"]))
    assert "K:11" in open(tmp_path / "density_attack" / "auto" / "params.txt").read().splitlines()
    for kind, n in (("pos", 25), ("neg", 22)):
        srt = np.sort(_host_S(queries[kind], bank), axis=1)
        for name, k in (("k40", 40), ("k40s", 40), ("auto", 11), ("k1", 1)):
            S = np.load(tmp_path / "density_attack" / name / (kind + "_kth_S.npy"))
            loss = np.load(tmp_path / "density_attack" / name / (kind + "_loss.npy"))
            assert S.dtype == np.int64 and S.shape == (n, 1) and loss.dtype == np.float64 and loss.shape == (n, 1)
            assert np.array_equal(S[:, 0], srt[:, k - 1]), (name, kind)
            assert np.array_equal(loss, dist64(S)), (name, kind)
        assert np.array_equal(np.load(tmp_path / "density_attack" / "k5" / (kind + "_loss.npy"))[:, 0],
                              np.load(tmp_path / "knn_attack" / "knn5" / (kind + "_knn_loss.npy"))[:, 4]), kind
        for f in ("_loss.npy", "_kth_S.npy"):
            assert open(tmp_path / "density_attack" / "k40" / (kind + f), "rb").read() == open(tmp_path / "density_attack" / "k40s" / (kind + f), "rb").read()

    # with a reference set: the formula on host-computed S
    density.main(density.parse_arguments(base + ["--exp_name", "ratio", "--K", "9", "--ref_data_dir", str(tmp_path / "ref"), "--K_ref", "1"]))
    density.main(density.parse_arguments(base + ["--exp_name", "ratio9", "--K", "9", "--ref_data_dir", str(tmp_path / "ref")]))
    for kind, n in (("pos", 25), ("neg", 22)):
        s_syn, s_ref = np.sort(_host_S(queries[kind], bank), axis=1), np.sort(_host_S(queries[kind], refs), axis=1)
        for name, k_ref in (("ratio", 1), ("ratio9", 9)):
            S = np.load(tmp_path / "density_attack" / name / (kind + "_kth_S.npy"))
            loss = np.load(tmp_path / "density_attack" / name / (kind + "_loss.npy"))
            assert S.dtype == np.int64 and S.shape == (n, 2) and loss.dtype == np.float64 and loss.shape == (n, 1)
            assert np.array_equal(S[:, 0], s_syn[:, 8]) and np.array_equal(S[:, 1], s_ref[:, k_ref - 1]), (name, kind)
            want = 0.5 * (np.log(np.maximum(s_syn[:, 8], 1).astype(np.float64)) - np.log(np.maximum(s_ref[:, k_ref - 1], 1).astype(np.float64)))
            assert np.array_equal(loss[:, 0], want) and np.all(np.isfinite(loss)), (name, kind)
    pos_S = np.load(tmp_path / "density_attack" / "ratio" / "pos_kth_S.npy")
    member = order("pos").index(2)
    assert pos_S[member, 1] == 0, "the query planted in the reference set"
    assert "K_ref:9" in open(tmp_path / "density_attack" / "ratio9" / "params.txt").read().splitlines()

    # eval_roc reads the directories as they stand
    for name in ("k40", "ratio"):
        d = tmp_path / "density_attack" / name
        auc, ap, precision = eval_roc.main(eval_roc.parse_arguments(["--attack_type", "fbb", "-ldir", str(d)]))
        assert auc == eval_roc.plot_roc(-np.load(d / "pos_loss.npy")[:, 0], -np.load(d / "neg_loss.npy")[:, 0])[3]
    # K beyond the rows that take part, and rows off both lattices: refused before any GPU work
    with pytest.raises(SystemExit) as e:
        density.main(density.parse_arguments(base + ["--exp_name", "big", "--K", "129"]))
    assert "--K 129 exceeds the 128" in str(e.value)
    with pytest.raises(SystemExit) as e:
        density.main(density.parse_arguments(base + ["--exp_name", "big", "--K", "9", "--ref_data_dir", str(tmp_path / "ref"), "--K_ref", "65"]))
    assert "--K_ref 65 exceeds the 64" in str(e.value)
    np.savez(tmp_path / "floats.npz", img_r01=np.random.default_rng(1).random((70, 16, 16, 3)).astype(np.float32))
    with pytest.raises(SystemExit) as e:
        density.main(density.parse_arguments(["--syn_data_path", str(tmp_path / "floats.npz")] + base[2:] + ["--exp_name", "off", "--K", "3"]))
    assert "8-bit images or integer tables" in str(e.value)
