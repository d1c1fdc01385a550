"""GPU: the attack drivers knn.py and mc.py on the float files the generators write -- a continuous table (.npy, medGAN's synthetic.npy) and
float images (.npz with img_r01, VAEGAN's generated.npz) -- under --distance l2: the files equal the API results on the rows
bank_io.load_rows reads, --K 1 gives attack(float_path='exact'), eval_roc scores the directories."""
import os

import numpy as np
import pytest

import float_rows_common as common

pytestmark = pytest.mark.gpu


def _table_files(tmp_path):
    seed, nb, cols, bs, npos, nneg = common.TABLE_CASES[0]                 # 300 x 37, 8 + 8 queries, BATCH_SIZE 30
    bank, queries = common.table_case(seed, nb, cols, npos, nneg)
    for name, rows in (("syn", bank), ("pos", queries[:npos]), ("neg", queries[npos:])):
        np.save(tmp_path / (name + ".npy"), rows)
    return [str(tmp_path / (n + ".npy")) for n in ("syn", "pos", "neg")], bs, 64


def _image_files(tmp_path):
    rng = np.random.default_rng(9)
    bank = rng.random((64, 8, 8, 3), dtype=np.float32)                      # NHWC in [0, 1)
    pos = np.clip(bank[[3, 40, 59, 7, 21, 33, 50, 12]] + rng.normal(0.0, 0.02, (8, 8, 8, 3)).astype(np.float32), 0.0, 1.0)
    neg = rng.random((8, 8, 8, 3), dtype=np.float32)
    for name, x in (("syn", bank), ("pos", pos), ("neg", neg)):
        np.savez_compressed(tmp_path / (name + ".npz"), noise=np.zeros((len(x), 4), np.float32), img_r01=x)
    return [str(tmp_path / (n + ".npz")) for n in ("syn", "pos", "neg")], 30, 8


@pytest.mark.parametrize("make", [_table_files, _image_files], ids=["table", "images"])
def test_drivers_on_float_files(tmp_path, monkeypatch, make):
    import ganleaks_amd as gl
    from ganleaks_amd.attack_models import eval_roc, knn, mc
    from ganleaks_amd.bank_io import load_rows
    (syn, pos, neg), bs, res = make(tmp_path)
    monkeypatch.chdir(tmp_path)
    base = ["--syn_data_path", syn, "--pos_data_dir", pos, "--neg_data_dir", neg, "--resolution", str(res), "--BATCH_SIZE", str(bs)]
    bank = load_rows(syn, res)
    both = np.concatenate([load_rows(pos, res), load_rows(neg, res)])
    assert bank.dtype == np.float32 and both.dtype == np.float32 and len(both) == 16
    n_eff = (len(bank) // bs) * bs
    M = common.chain_matrix(both, bank[:n_eff])

    knn.main(knn.parse_arguments(base + ["--distance", "l2", "--K", "5", "--exp_name", "k5"]))
    knn.main(knn.parse_arguments(base + ["--distance", "l2", "--K", "5", "--exp_name", "k5s", "--devices", "0,0"]))
    knn.main(knn.parse_arguments(base + ["--distance", "l2", "--K", "1", "--exp_name", "k1"]))
    want_d, want_i = gl.nearest_neighbours(both, bank, 5, distance="l2", batch_size=bs, float_path="exact")
    assert np.array_equal(want_i, np.argsort(M, axis=1, kind="stable")[:, :5])
    out = tmp_path / "knn_attack"
    for kind, part in (("pos", slice(0, 8)), ("neg", slice(8, 16))):
        assert np.array_equal(np.load(out / "k5" / (kind + "_knn_loss.npy")), want_d[part].astype(np.float64))
        assert np.array_equal(np.load(out / "k5" / (kind + "_knn_idx.npy")), want_i[part])
        assert np.array_equal(np.load(out / "k5" / (kind + "_loss.npy")), want_d[part].astype(np.float64).mean(axis=1, keepdims=True))
    for f in ("pos_knn_loss.npy", "neg_knn_loss.npy", "pos_knn_idx.npy", "neg_knn_idx.npy", "pos_loss.npy", "neg_loss.npy"):
        assert open(out / "k5" / f, "rb").read() == open(out / "k5s" / f, "rb").read(), f
    top1 = gl.attack(both, bank, distance="l2", batch_size=bs, float_path="exact")[0]
    assert np.array_equal(top1, M.min(axis=1))
    assert np.array_equal(np.concatenate([np.load(out / "k1" / "pos_loss.npy"), np.load(out / "k1" / "neg_loss.npy")]).reshape(-1), top1.astype(np.float64))

    fixed = [float(np.quantile(M, 0.2)), -1.0, float(np.quantile(M, 0.02)), 1e9]
    mc.main(mc.parse_arguments(base + ["--exp_name", "fixed", "--eps=" + ",".join(repr(v) for v in fixed)]))
    mc.main(mc.parse_arguments(base + ["--exp_name", "quant", "--eps_quantile", "0.5,0.9"]))
    mc.main(mc.parse_arguments(base + ["--exp_name", "quants", "--eps_quantile", "0.5,0.9", "--devices", "0,0"]))
    want_eps = {"fixed": np.asarray(fixed, np.float32), "quant": np.asarray([np.quantile(top1, v, method="lower") for v in (0.5, 0.9)], np.float32)}
    out = tmp_path / "mc_attack"
    for name, eps in want_eps.items():
        assert np.array_equal(np.load(out / name / "eps.npy"), eps)
        counts = gl.ball_counts(both, bank, eps, batch_size=bs, float_path="exact")
        assert np.array_equal(counts, (M[:, :, None] <= eps[None, None, :]).sum(axis=1))
        got = np.concatenate([np.load(out / name / "pos_count.npy"), np.load(out / name / "neg_count.npy")])
        assert np.array_equal(got, counts), name
        assert np.array_equal(np.load(out / name / "pos_mc.npy"), counts[:8] / float(n_eff))
        assert np.array_equal(np.load(out / name / "neg_loss.npy"), -(counts[8:, :1] / float(n_eff)))
    # the median radius is an attained distance: half of the queries (rounded up) have their nearest sample inside it
    inside = np.concatenate([np.load(out / "quant" / "pos_count.npy"), np.load(out / "quant" / "neg_count.npy")])[:, 0] >= 1
    assert np.array_equal(inside, top1 <= want_eps["quant"][0]) and inside.sum() >= 8
    for f in ("eps.npy", "pos_count.npy", "neg_count.npy", "pos_mc.npy", "neg_mc.npy", "pos_loss.npy", "neg_loss.npy"):
        assert open(out / "quant" / f, "rb").read() == open(out / "quants" / f, "rb").read(), f

    for ldir in (tmp_path / "knn_attack" / "k5", tmp_path / "mc_attack" / "quant"):
        auc, ap, precision = eval_roc.main(eval_roc.parse_arguments(["--attack_type", "fbb", "-ldir", str(ldir)]))
        assert 0.0 <= auc <= 1.0
    pos_loss, neg_loss = (np.load(tmp_path / "knn_attack" / "k5" / f).reshape(-1) for f in ("pos_loss.npy", "neg_loss.npy"))
    assert pos_loss.mean() < neg_loss.mean()                 # members sit nearer to the bank
