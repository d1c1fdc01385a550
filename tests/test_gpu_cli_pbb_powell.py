"""GPU: attack_models/pbb.py --optimizer powell on a tiny generator.pth and PNG folders: the usual files, a trace of sweeps + 1 rows,
params.txt naming the optimiser and what it ran with, the search never scoring worse than the full-black-box start, and eval_roc reading
the directory as attack_type 'pbb'."""
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


def test_pbb_cli_powell(tmp_path, monkeypatch, synth):
    import torch
    import ganleaks_amd as gl
    from ganleaks_amd.attack import _dist32
    from ganleaks_amd.attack_models import eval_roc, pbb, utils
    from ganleaks_amd.gan_models.dcgan.model_torch import Generator
    sd = synth.dcgan_state_dict(1234, features_g=16)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, tmp_path / "generator.pth")
    gen = Generator(100, 3, 16)
    gen.load_state_dict(sd)
    z_bank = np.random.default_rng(3).standard_normal((64, 100)).astype(np.float32)      # what --num_init 64 --init_seed 3 draws
    pos = gen.generate_u8(z_bank[:6] + np.float32(0.2) * synth.latent(52, 6).reshape(6, 100)).numpy()
    neg = gen.generate_u8(synth.latent(53, 5).reshape(5, 100)).numpy()
    _write_pngs(tmp_path / "pos", pos)
    _write_pngs(tmp_path / "neg", neg)
    monkeypatch.chdir(tmp_path)
    base = ["--pos_data_dir", str(tmp_path / "pos"), "--neg_data_dir", str(tmp_path / "neg"), "--BATCH_SIZE", "64", "--gan", "dcgan",
            "--generator_path", str(tmp_path / "generator.pth"), "--ngf", "16", "--num_init", "64", "--init_seed", "3"]
    out = pbb.main(pbb.parse_arguments(base + ["--exp_name", "run", "--optimizer", "powell", "--sweeps", "1", "--ladder", "4"]))[0]
    d = tmp_path / "pbb_attack" / "run"
    assert out == str(d)
    names = ["%s_%s.npy" % (k, f) for k in ("pos", "neg") for f in ("loss", "z", "S", "init_loss", "trace")]
    assert sorted(os.listdir(d)) == sorted(["params.txt"] + names)
    order = lambda name: [int(os.path.basename(x)[6:-4]) for x in utils.get_filepaths_from_dir(str(tmp_path / name), "png")]   # noqa: E731
    for kind, rows in (("pos", pos[order("pos")]), ("neg", neg[order("neg")])):
        n = len(rows)
        loss, z, S = np.load(d / (kind + "_loss.npy")), np.load(d / (kind + "_z.npy")), np.load(d / (kind + "_S.npy"))
        init, trace = np.load(d / (kind + "_init_loss.npy")), np.load(d / (kind + "_trace.npy"))
        assert loss.dtype == np.float64 and loss.shape == (n, 1) and init.dtype == np.float64 and init.shape == (n, 1)
        assert z.dtype == np.float32 and z.shape == (n, 100) and S.dtype == np.int64 and S.shape == (n, 1)
        assert trace.dtype == np.int64 and trace.shape == (2, n) and np.array_equal(trace[-1], S[:, 0]) and (np.diff(trace, axis=0) <= 0).all()
        assert (loss <= init).all()
        fbb, _ = gl.attack(rows, gl.GeneratedBank(gen, z_bank), distance="l2", batch_size=64)
        assert np.array_equal(init[:, 0], fbb.astype(np.float64))
        per_query = ((gen.generate_u8(z).numpy().astype(np.int64) - rows.astype(np.int64)) ** 2).reshape(n, -1).sum(axis=1)
        assert np.array_equal(per_query, S[:, 0]) and np.array_equal(loss[:, 0], _dist32(S[:, 0], 12288, "u8").astype(np.float64))
    assert (np.load(d / "pos_loss.npy") < np.load(d / "pos_init_loss.npy")).all()
    params = open(d / "params.txt").read().splitlines()
    for line in ("optimizer:powell", "sweeps:1", "ladder:4", "step0:1.0"):
        assert line in params, line
    # the files are what pbb_attack gives for the same request
    both = np.concatenate([pos[order("pos")], neg[order("neg")]])
    z_init, _ = gl.pbb_init_from_bank(both, gen, z_bank, batch_size=64)
    _, z_star, S, _ = gl.pbb_attack(both, gen, z_init, optimizer="powell", sweeps=1, ladder=4, history=True)
    assert np.array_equal(np.concatenate([np.load(d / "pos_z.npy"), np.load(d / "neg_z.npy")]), z_star)
    assert np.array_equal(np.concatenate([np.load(d / "pos_S.npy"), np.load(d / "neg_S.npy")])[:, 0], S)
    auc, ap, precision = eval_roc.main(eval_roc.parse_arguments(["--attack_type", "pbb", "-ldir", str(d)]))
    assert auc == eval_roc.plot_roc(-np.load(d / "pos_loss.npy")[:, 0], -np.load(d / "neg_loss.npy")[:, 0])[3] and 0.0 <= auc <= 1.0
    # without the switch params.txt is what it was before the switch existed
    pbb.main(pbb.parse_arguments(base + ["--rounds", "1", "--population", "4", "--exp_name", "es"]))
    assert not [line for line in open(tmp_path / "pbb_attack" / "es" / "params.txt").read().splitlines()
                if line.split(":")[0] in ("optimizer", "sweeps", "ladder", "step0")]
    assert np.load(tmp_path / "pbb_attack" / "es" / "pos_trace.npy").shape == (2, 6)
