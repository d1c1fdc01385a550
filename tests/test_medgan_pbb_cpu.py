"""CPU: the host restatement of medGAN's generator and decoder reproduces the reference's outputs (tests/golden/medgan_gen.npz), and the
refusals of the latent attacks on tables that need no GPU."""
import os

import numpy as np
import pytest
import torch

import medgan_pbb_common as mc


def test_restatement_reproduces_the_golden_outputs(synth, golden_dir):
    """the float32 restatement -- the golden file's own arithmetic class -- within 2e-6 on the hidden rows and on both decoded arrays"""
    g = np.load(os.path.join(golden_dir, "medgan_gen.npz"))
    gsd, asd = synth.medgan_state_dicts(555, 1071)
    z = np.random.default_rng(8).standard_normal((37, 128)).astype(np.float32)
    for binary in (True, False):
        net = mc.Net(gsd, asd, binary, torch.float32)
        hidden = net.hidden(z)
        errs = np.abs(hidden - g["hidden"]).max(), np.abs(net.decode(hidden) - g["decoded_binary%d" % int(binary)]).max()
        print("float32", "sigmoid" if binary else "relu", "hidden %.3e decoded %.3e" % errs)
        assert max(errs) < 2e-6


def test_float64_restatement_is_within_the_golden_file_s_own_rounding(synth, golden_dir):
    """the same code in float64.  The hidden rows: 2e-6 as above.  The decoded values are compared from the golden hidden rows on, so that
    the only difference is the float32 rounding inside the golden values themselves: a float32 dot product of 128 terms plus the bias is
    within gamma_129 M of the exact one, gamma_n = n u / (1 - n u), u = 2^-24, M = sum |h_k| |W_fk| + |b_f| (Higham, Accuracy and
    Stability of Numerical Algorithms, (3.5)); ReLU is 1-Lipschitz, the sigmoid 1/4-Lipschitz with a few roundings of a value below 1 of
    its own (4 u allowed).  No constant is taken from what the comparison gives (measured: ReLU 2.9e-6 at values up to 6.4, 0.03 of its bound)."""
    g = np.load(os.path.join(golden_dir, "medgan_gen.npz"))
    gsd, asd = synth.medgan_state_dicts(555, 1071)
    z = np.random.default_rng(8).standard_normal((37, 128)).astype(np.float32)
    u = 2.0 ** -24
    gamma = 129 * u / (1 - 129 * u)
    for binary in (True, False):
        net = mc.Net(gsd, asd, binary)
        assert np.abs(net.hidden(z) - g["hidden"]).max() < 2e-6
        err = np.abs(net.decode(g["hidden"]) - g["decoded_binary%d" % int(binary)])
        bound = gamma * net.dot_magnitude(g["hidden"]) * (0.25 if binary else 1.0) + (4 * u if binary else 0.0)
        print("float64", "sigmoid" if binary else "relu", "decoded error %.3e, smallest bound %.3e, largest error / bound %.3f"
              % (err.max(), bound.min(), (err / bound).max()))
        assert (err <= bound).all()


class _Table:
    """what the attacks look at before any GPU work"""
    row_kind, z_dim, image_shape = "int", 128, (65,)

    def generate_u8(self, z):
        raise AssertionError("no GPU work before the refusal")

    generate_rows = vjp_z = generate_u8

    @property
    def ctx(self):
        raise AssertionError("no GPU work before the refusal")


def test_pair_attacks_refuse_a_table_generator():
    from ganleaks_amd import pbb, wb
    q, z = np.zeros((2, 65), np.float32), np.zeros((2, 128), np.float32)
    for call in (lambda: pbb.pair_pbb_attack(q, _Table(), z), lambda: wb.pair_wb_attack(q, _Table(), z),
                 lambda: pbb.pair_pbb_init_from_bank(q, _Table(), z), lambda: wb.pair_grad_z(_Table(), z, q.astype(np.uint8))):
        with pytest.raises(NotImplementedError, match="LPIPS is defined on images"):
            call()


def test_white_box_attack_names_what_a_table_generator_lacks():
    from ganleaks_amd import wb
    with pytest.raises(NotImplementedError, match="l2_grad_z"):
        wb.wb_attack(np.zeros((2, 65), np.float32), _Table(), np.zeros((2, 128), np.float32))


def test_command_line_refusals():
    from ganleaks_amd.attack_models import pbb as cli
    base = ["--gan", "medgan", "--generator_path", "generator.pth", "--num_init", "64"]
    for extra, reason in (([], "--autoencoder_path"), (["--autoencoder_path", "ae.pth"], "--input_size"),
                          (["--autoencoder_path", "ae.pth", "--input_size", "65", "--nz", "100"], "128"),
                          (["--autoencoder_path", "ae.pth", "--input_size", "65", "--pair_distance", "l2-lpips"], "LPIPS is defined on images")):
        with pytest.raises(SystemExit) as e:
            cli._request(cli.parse_arguments(base + extra))
        assert reason in str(e.value)
    args = cli.parse_arguments(base + ["--autoencoder_path", "ae.pth", "--input_size", "65", "--binary"])
    cli._request(args)
    assert args.nz == 128 and args.binary is True
    with pytest.raises(SystemExit, match="belongs to --gan medgan"):
        cli._request(cli.parse_arguments(["--gan", "dcgan", "--generator_path", "generator.pth", "--num_init", "64", "--input_size", "65"]))
    # an invocation that does not use the new options keeps the params.txt it had
    plain = cli.parse_arguments(["--gan", "dcgan", "--generator_path", "generator.pth", "--num_init", "64"])
    cli._request(plain)
    assert all(name in cli.MEDGAN_OPTIONS and getattr(plain, name) is None for name in ("autoencoder_path", "input_size", "binary"))
    assert plain.nz is None
