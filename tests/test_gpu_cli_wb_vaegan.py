"""GPU: attack_models/wb.py and attack_models/pbb.py with --gan vaegan --sn_forwards 1 on a tiny generator.pth and PNG folders: the files equal
what the API gives for Generator(nz, d).frozen(1), params.txt records K, and eval_roc scores both directories."""
import os

import numpy as np
import pytest

import gpu_common  # noqa: F401

pytestmark = pytest.mark.gpu
D, NZ = 32, 100


def _write_pngs(d, imgs_u8_nchw, prefix="image_"):
    import PIL.Image
    os.makedirs(d, exist_ok=True)
    for i, im in enumerate(imgs_u8_nchw):
        PIL.Image.fromarray(im.transpose(1, 2, 0)).save(os.path.join(d, "%s%d.png" % (prefix, i)))


@pytest.fixture(scope="module")
def folder(tmp_path_factory, synth):
    import torch
    from ganleaks_amd.gan_models.vaegan.train import Generator
    tmp = tmp_path_factory.mktemp("vaegan_cli")
    sd = synth.vaegan_state_dict(z_dim=NZ, d=D)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, tmp / "generator.pth")
    parent = Generator(NZ, d=D)
    parent.load_state_dict(sd)
    view = parent.frozen(1)
    z_bank = np.random.default_rng(3).standard_normal((64, NZ)).astype(np.float32)      # what --num_init 64 --init_seed 3 draws
    pos = view.generate_u8(z_bank[:4] + np.float32(0.2) * synth.latent(52, 4).reshape(4, NZ)).numpy()
    neg = view.generate_u8(synth.latent(53, 3).reshape(3, NZ)).numpy()
    _write_pngs(tmp / "pos", pos)
    _write_pngs(tmp / "neg", neg)
    base = ["--pos_data_dir", str(tmp / "pos"), "--neg_data_dir", str(tmp / "neg"), "--BATCH_SIZE", "64", "--gan", "vaegan", "--sn_forwards", "1",
            "--generator_path", str(tmp / "generator.pth"), "--nz", str(NZ), "--ngf", str(D), "--num_init", "64", "--init_seed", "3"]
    return tmp, view, z_bank, pos, neg, base


def _rows(tmp, pos, neg):
    from ganleaks_amd.attack_models import utils
    order = lambda name: [int(os.path.basename(x)[6:-4]) for x in utils.get_filepaths_from_dir(str(tmp / name), "png")]   # noqa: E731
    return np.concatenate([pos[order("pos")], neg[order("neg")]])


def _load(d, name):
    return np.concatenate([np.load(d / ("pos_%s.npy" % name)), np.load(d / ("neg_%s.npy" % name))], axis=1 if name == "trace" else 0)


def test_wb_cli(folder, monkeypatch):
    import ganleaks_amd as gl
    from ganleaks_amd.attack_models import eval_roc, wb
    tmp, view, z_bank, pos, neg, base = folder
    monkeypatch.chdir(tmp)
    out = wb.main(wb.parse_arguments(base + ["--steps", "4", "--exp_name", "run"]))[0]
    d = tmp / "wb_attack" / "run"
    assert out == str(d)
    both = _rows(tmp, pos, neg)
    z_init, _ = gl.pbb_init_from_bank(both, view, z_bank, batch_size=64)
    dist, z_star, S, trace = gl.wb_attack(both, view, z_init, steps=4, history=True)
    assert np.array_equal(_load(d, "loss")[:, 0], dist.astype(np.float64)) and np.array_equal(_load(d, "z"), z_star)
    assert np.array_equal(_load(d, "S")[:, 0], S) and np.array_equal(_load(d, "trace"), trace)
    assert (_load(d, "loss") <= _load(d, "init_loss")).all()
    lines = open(d / "params.txt").read().splitlines()
    assert "sn_forwards:1" in lines and "gan:vaegan" in lines
    auc, ap, precision = eval_roc.main(eval_roc.parse_arguments(["--attack_type", "wb", "-ldir", str(d)]))
    assert auc == eval_roc.plot_roc(-np.load(d / "pos_loss.npy")[:, 0], -np.load(d / "neg_loss.npy")[:, 0])[3] and 0.0 <= auc <= 1.0
    with pytest.raises(SystemExit, match=r"vaegan.*--sn_forwards"):
        wb.main(wb.parse_arguments([a for a in base if a not in ("--sn_forwards", "1")] + ["--exp_name", "refused"]))
    assert not (tmp / "wb_attack" / "refused").exists()


def test_pbb_cli(folder, monkeypatch):
    import ganleaks_amd as gl
    from ganleaks_amd.attack_models import eval_roc, pbb
    tmp, view, z_bank, pos, neg, base = folder
    monkeypatch.chdir(tmp)
    out = pbb.main(pbb.parse_arguments(base + ["--rounds", "3", "--population", "8", "--exp_name", "run"]))[0]
    d = tmp / "pbb_attack" / "run"
    assert out == str(d)
    both = _rows(tmp, pos, neg)
    z_init, _ = gl.pbb_init_from_bank(both, view, z_bank, batch_size=64)
    dist, z_star, S, trace = gl.pbb_attack(both, view, z_init, rounds=3, population=8, sigma=0.5, seed=0, history=True)
    assert np.array_equal(_load(d, "loss")[:, 0], dist.astype(np.float64)) and np.array_equal(_load(d, "z"), z_star)
    assert np.array_equal(_load(d, "S")[:, 0], S) and np.array_equal(_load(d, "trace"), trace)
    assert (_load(d, "loss") <= _load(d, "init_loss")).all()
    assert "sn_forwards:1" in open(d / "params.txt").read().splitlines()
    auc, ap, precision = eval_roc.main(eval_roc.parse_arguments(["--attack_type", "pbb", "-ldir", str(d)]))
    assert auc == eval_roc.plot_roc(-np.load(d / "pos_loss.npy")[:, 0], -np.load(d / "neg_loss.npy")[:, 0])[3] and 0.0 <= auc <= 1.0
