"""GPU: the Monte-Carlo / eps-ball attack driver (attack_models/mc.py) on PNG directories: files, shapes and dtypes, counts against the
oracle, the median heuristic against fbb's own distances, eval_roc on the result, and the sharded run byte for byte."""
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


def test_mc_main(tmp_path, monkeypatch, synth):
    import c_oracle
    from ganleaks_amd.attack_models import eval_roc, fbb, mc, utils
    case = synth.attack_case(182, 150, 25, 22, 16)        # 150 is not a multiple of BATCH_SIZE 64: 128 rows take part
    for name in ("syn", "pos", "neg"):
        _write_pngs(tmp_path / name, case["bank" if name == "syn" else name])
    monkeypatch.chdir(tmp_path)
    base = ["--syn_data_path", str(tmp_path / "syn"), "--pos_data_dir", str(tmp_path / "pos"), "--neg_data_dir", str(tmp_path / "neg"),
            "--resolution", "16", "--BATCH_SIZE", "64"]
    fbb.main(fbb.parse_arguments(base + ["--distance", "l2", "--exp_name", "plain"]))
    mc.main(mc.parse_arguments(base + ["--exp_name", "median"]))                                     # default: --eps_quantile 0.5
    mc.main(mc.parse_arguments(base + ["--exp_name", "median2", "--eps_quantile", "0.5", "--devices", "0,0"]))
    mc.main(mc.parse_arguments(base + ["--exp_name", "three", "--eps_quantile", "0.9,0.1,0.5"]))
    mc.main(mc.parse_arguments(base + ["--exp_name", "fixed", "--eps", "0.02,0.005,0.02,1e9,-1"]))
    mc.main(mc.parse_arguments(base + ["--exp_name", "fixed2", "--eps", "0.02,0.005,0.02,1e9,-1", "--ngpu", "1", "--devices", "0,0,0"]))
    out = {n: tmp_path / "mc_attack" / n for n in ("median", "median2", "three", "fixed", "fixed2")}
    files = ("eps.npy", "pos_count.npy", "neg_count.npy", "pos_mc.npy", "neg_mc.npy", "pos_loss.npy", "neg_loss.npy")
    for d in out.values():
        assert sorted(os.listdir(d)) == sorted(files + ("params.txt",)), os.listdir(d)
    # the sharded runs: the same .npy files byte for byte
    for a, b in (("median", "median2"), ("fixed", "fixed2")):
        for f in files:
            assert open(out[a] / f, "rb").read() == open(out[b] / f, "rb").read(), (a, f)
    assert "eps_quantile:0.9,0.1,0.5" in open(out["three"] / "params.txt").read().splitlines()

    order = lambda name: [int(os.path.basename(x)[6:-4]) for x in utils.get_filepaths_from_dir(str(tmp_path / name), "png")]   # noqa: E731
    bank = case["bank"][order("syn")][:128]
    queries = {kind: case[kind][order(kind)] for kind in ("pos", "neg")}
    dist = {kind: np.stack([(c_oracle.ssd_row_u8(bank, x).astype(np.float64) * (4.0 / (65025.0 * 768))).astype(np.float32) for x in queries[kind]])
            for kind in ("pos", "neg")}
    # the median heuristic: the 'lower' median of fbb's pooled nearest-sample distances
    pooled = np.concatenate([np.load(tmp_path / "fbb_attack" / "plain" / "pos_loss.npy"), np.load(tmp_path / "fbb_attack" / "plain" / "neg_loss.npy")])
    pooled32 = pooled.reshape(-1).astype(np.float32)
    assert np.array_equal(pooled32.astype(np.float64), pooled.reshape(-1))
    assert np.array_equal(pooled32, np.concatenate([dist["pos"].min(axis=1), dist["neg"].min(axis=1)]))
    want_eps = {"median": np.asarray([np.quantile(pooled32, 0.5, method="lower")], np.float32),
                "three": np.asarray([np.quantile(pooled32, v, method="lower") for v in (0.9, 0.1, 0.5)], np.float32),
                "fixed": np.asarray([0.02, 0.005, 0.02, 1e9, -1], np.float32)}
    for name, eps in want_eps.items():
        got_eps = np.load(out[name] / "eps.npy")
        assert got_eps.dtype == np.float32 and np.array_equal(got_eps, eps), name
        T = len(eps)
        for kind, n in (("pos", 25), ("neg", 22)):
            count, score, loss = (np.load(out[name] / (kind + suffix)) for suffix in ("_count.npy", "_mc.npy", "_loss.npy"))
            assert count.shape == (n, T) and count.dtype == np.int64
            assert score.shape == (n, T) and score.dtype == np.float64
            assert loss.shape == (n, 1) and loss.dtype == np.float64
            want = np.stack([(dist[kind] <= e).sum(axis=1) for e in eps], axis=1)
            assert np.array_equal(count, want), (name, kind)              # every query
            assert np.array_equal(score, want / 128.0) and np.array_equal(loss, -score[:, :1])
    # half of the pooled queries (rounded up: 'lower') have their nearest sample inside the median ball
    inside = np.concatenate([np.load(out["median"] / "pos_count.npy"), np.load(out["median"] / "neg_count.npy")])[:, 0] >= 1
    assert inside.sum() >= (47 + 1) // 2 and np.array_equal(inside, pooled32 <= want_eps["median"][0])
    assert np.all(np.load(out["fixed"] / "pos_count.npy")[:, 3] == 128) and np.all(np.load(out["fixed"] / "neg_count.npy")[:, 4] == 0)
    # eval_roc scores the first eps unchanged
    auc, ap, precision = eval_roc.main(eval_roc.parse_arguments(["--attack_type", "fbb", "-ldir", str(out["three"])]))
    want_auc = eval_roc.plot_roc(np.load(out["three"] / "pos_mc.npy")[:, 0], np.load(out["three"] / "neg_mc.npy")[:, 0])[3]
    assert auc == want_auc


def test_mc_refuses_bad_radii_before_reading(tmp_path, monkeypatch):
    from ganleaks_amd.attack_models import mc
    monkeypatch.chdir(tmp_path)
    os.makedirs(tmp_path / "syn")
    common = ["--syn_data_path", str(tmp_path / "syn"), "--pos_data_dir", str(tmp_path / "nowhere"), "--neg_data_dir", str(tmp_path / "nowhere")]
    for extra in (["--eps", "0.1", "--eps_quantile", "0.5"], ["--eps_quantile", "2"], ["--eps", "nan"], ["--eps", ",".join(["1"] * 17)], ["--eps", "x"]):
        with pytest.raises(SystemExit):
            mc.main(mc.parse_arguments(common + extra))
    assert not (tmp_path / "mc_attack").exists()
