"""GPU: attack_models/pbb.py with --gan medgan on saved state dicts and .npy tables: the files it writes, the loss being fl32(S / F) of the
exact number of differing columns, the attack never scoring worse than the full-black-box start it records, eval_roc reading the directory,
the reference's decoder.pth naming the same decoder, and --pair_distance refused with the reason."""
import os

import numpy as np
import pytest

import gpu_common  # noqa: F401

pytestmark = pytest.mark.gpu
F = 65


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    import torch
    import ganleaks_amd as gl
    from ganleaks_amd.gan_models.medgan.model import Autoencoder, Generator, generate_synthetic
    tmp = tmp_path_factory.mktemp("medgan_cli")
    gsd, asd = gl.synth.medgan_state_dicts(665, F)
    as_torch = lambda sd: {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}                 # noqa: E731
    torch.save(as_torch(gsd), tmp / "generator.pth")
    torch.save(as_torch(asd), tmp / "autoencoder.pth")
    torch.save(as_torch({"0.weight": asd["decoder.0.weight"], "0.bias": asd["decoder.0.bias"]}), tmp / "decoder.pth")   # the reference's file
    gen, ae = Generator(128, 128), Autoencoder(F, 128, binary=True)
    gen.load_state_dict(gsd)
    ae.load_state_dict(asd)
    z_bank = np.random.default_rng(3).standard_normal((64, 128)).astype(np.float32)      # what --num_init 64 --init_seed 3 draws
    rng = np.random.default_rng(41)
    pos = generate_synthetic(gen, ae, z_bank[:6] + np.float32(0.2) * rng.standard_normal((6, 128)).astype(np.float32))
    neg = generate_synthetic(gen, ae, rng.standard_normal((6, 128)).astype(np.float32))
    np.save(tmp / "pos.npy", pos)
    np.save(tmp / "neg.npy", neg)
    base = ["--pos_data_dir", str(tmp / "pos.npy"), "--neg_data_dir", str(tmp / "neg.npy"), "--BATCH_SIZE", "64", "--gan", "medgan",
            "--generator_path", str(tmp / "generator.pth"), "--input_size", str(F), "--binary", "--num_init", "64", "--init_seed", "3"]
    return tmp, base, gen, ae, z_bank, pos, neg


def _check_directory(d, case, attack_type, rounds):
    import ganleaks_amd as gl
    from ganleaks_amd.attack_models import eval_roc
    from ganleaks_amd.gan_models.medgan.model import generate_synthetic
    _, _, gen, ae, z_bank, pos, neg = case
    names = ["%s_%s.npy" % (k, f) for k in ("pos", "neg") for f in ("loss", "z", "S", "init_loss", "trace")]
    assert sorted(os.listdir(d)) == sorted(["params.txt"] + names)
    bank = generate_synthetic(gen, ae, z_bank)
    for kind, rows in (("pos", pos), ("neg", neg)):
        n = len(rows)
        loss, z, S = np.load(d / (kind + "_loss.npy")), np.load(d / (kind + "_z.npy")), np.load(d / (kind + "_S.npy"))
        init, trace = np.load(d / (kind + "_init_loss.npy")), np.load(d / (kind + "_trace.npy"))
        assert loss.dtype == np.float64 and loss.shape == (n, 1) and init.shape == (n, 1) and z.dtype == np.float32 and z.shape == (n, 128)
        assert S.dtype == np.int64 and S.shape == (n, 1) and trace.shape == (rounds + 1, n) and np.array_equal(trace[-1], S[:, 0])
        assert np.array_equal(loss[:, 0], (S[:, 0].astype(np.float64) / F).astype(np.float32).astype(np.float64))       # fl32(S / 65)
        assert (init >= loss).all()
        hamming = ((generate_synthetic(gen, ae, z).astype(np.int64) - rows.astype(np.int64)) ** 2).sum(axis=1)
        assert np.array_equal(hamming, S[:, 0])
        fbb, _ = gl.attack(rows, bank, distance="l2", batch_size=64)
        assert np.array_equal(init[:, 0], fbb.astype(np.float64))
    lines = open(d / "params.txt").read().splitlines()
    assert "gan:medgan" in lines and "input_size:%d" % F in lines and "binary:True" in lines and "nz:128" in lines
    auc, ap, precision = eval_roc.main(eval_roc.parse_arguments(["--attack_type", attack_type, "-ldir", str(d)]))
    assert auc == eval_roc.plot_roc(-np.load(d / "pos_loss.npy")[:, 0], -np.load(d / "neg_loss.npy")[:, 0])[3] and 0.0 <= auc <= 1.0


def test_pbb_cli_medgan(case, monkeypatch):
    from ganleaks_amd.attack_models import pbb
    tmp, base = case[:2]
    monkeypatch.chdir(tmp)
    out = pbb.main(pbb.parse_arguments(base + ["--autoencoder_path", str(tmp / "autoencoder.pth"), "--rounds", "4", "--population", "16",
                                               "--exp_name", "run"]))[0]
    assert out == str(tmp / "pbb_attack" / "run")
    _check_directory(tmp / "pbb_attack" / "run", case, "pbb", 4)
    # the reference's decoder.pth names the same decoder
    pbb.main(pbb.parse_arguments(base + ["--autoencoder_path", str(tmp / "decoder.pth"), "--rounds", "4", "--population", "16", "--exp_name", "decoder"]))
    for name in ("pos_S.npy", "neg_z.npy"):
        assert open(tmp / "pbb_attack" / "run" / name, "rb").read() == open(tmp / "pbb_attack" / "decoder" / name, "rb").read()
    with pytest.raises(SystemExit, match="LPIPS is defined on images"):
        pbb.main(pbb.parse_arguments(base + ["--autoencoder_path", str(tmp / "autoencoder.pth"), "--pair_distance", "l2-lpips", "--exp_name", "refused"]))
    assert not (tmp / "pbb_attack" / "refused").exists()
