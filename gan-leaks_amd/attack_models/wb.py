"""[build] The white-box attack of GAN-Leaks (section 5.4 of the paper) on the data fbb.py reads.

The attacker holds the generator's weights: for every query x, z* = argmin_z L(x, G(z)) is found by gradient descent (Adam on the exact
gradient through the generator) and the query is scored by L(x, G(z*)), L the L2 distance of Loss('l2') (attack_models/utils.py:161-164).
The reference fork has no driver for it; the data flags, the YAML overlay, the start and the layout of the result directory are pbb.py's,
so that eval_roc.py scores the result unchanged.  The search is ganleaks_amd.wb.wb_attack, started from the nearest of a bank of latents
(the full-black-box answer), which it can only improve on.

    python -m ganleaks_amd.attack_models.wb --local_config config_attack_fbb.yaml --gan {dcgan,wgangp} --generator_path generator.pth
           [--nz --ngf] [--noise_path npz | --num_init N --init_seed s] [--steps --lr --beta1 --beta2] [--BATCH_SIZE]
           [--optimizer {adam,lbfgs} [--memory m --ladder L --step0 s]]
    python -m ganleaks_amd.attack_models.wb ... --gan pggan --pg_steps N [--alpha a] [--in_channels C] --nz Z --resolution R ...
    python -m ganleaks_amd.attack_models.wb ... --gan vaegan --sn_forwards K [--nz Z --ngf d] [--encoder_path encoder.pth]
    python -m ganleaks_amd.attack_models.wb ... --pair_distance l2-lpips

--gan, --generator_path  the generator class and its state dict (what the training scripts save as generator.pth)
--sn_forwards            VAEGAN only, no default: VAEGAN's spectral normalisation advances with every forward, so the generator attacked is the one
                         its K-th forward after loading would have run, held from then on (Generator(nz, d=--ngf).frozen(K)); K >= 1,
                         --resolution 64.  Without it --gan vaegan is refused
--nz, --ngf              latent length and width (features_g)
--pg_steps, --alpha, --in_channels   PGGAN only: the depth (images of 4 * 2^pg_steps pixels; no default, --steps is the descent's), the
                         fade-in weight of the last block (default 1) and the channel count of the first block (default 256)
--encoder_path           VAEGAN only: the encoder's state dict (or a checkpoint dict with netE_state_dict).  The start is then the encoder's
                         posterior mean of every query (ganleaks_amd.recon), not the nearest bank latent: no bank is read, and --noise_path
                         and --num_init are not needed (and refused).  Exact l2 only
--noise_path             the .npz the generate branches write under npz_noise/ (array `noise`): the latents of the sample bank
--num_init, --init_seed  without --noise_path: that many standard-normal latents drawn from numpy's default_rng(init_seed)
--BATCH_SIZE             only the first (N // BATCH_SIZE) * BATCH_SIZE latents take part in the start, as in fbb.py:77
--steps, --lr, --beta1, --beta2   the descent (ganleaks_amd.wb.wb_attack)
--optimizer              adam (the default) or lbfgs, the paper's optimiser: L-BFGS over the last --memory pairs (default 8, 1..16), every step
                         scoring a ladder of --ladder step widths (default 8, 1..32) in one batched forward; a steepest-descent step first tries
                         length --step0 (default 1) in latent space.  --steps counts gradient evaluations under both; --lr, --beta1, --beta2
                         are not used by lbfgs, and --memory, --ladder, --step0 belong to it
--pair_distance l2-lpips (default absent) the same attack under 0.2 * LPIPS + L2, the distance fbb.py hard-wires and the paper's white-box loss
                         (ganleaks_amd.wb.pair_wb_attack); VGG16 and lin weights from $GANLEAKS_VGG16_PATH / $GANLEAKS_LPIPS_LIN_PATH; the
                         start is the bank latent nearest under that distance; the resolution must be a multiple of 16.  {pos,neg}_key.npy
                         (int64 [n, 1]: the uint32 pattern of the float32 distance, the exact and ordered score) takes the place of the S
                         files, and the trace holds keys
Files under ./wb_attack/<exp_name>/:
    {pos,neg}_loss.npy float64 [n, 1]: L(x, G(z*)); {pos,neg}_z.npy float32 [n, nz]: z*; {pos,neg}_S.npy int64 [n, 1]: the exact sum of
    squared differences behind the loss; {pos,neg}_init_loss.npy float64 [n, 1]: the full-black-box score the descent started from;
    {pos,neg}_trace.npy int64 [steps + 1, n]: the best S after every step; params.txt.  Small = member-like:
    `eval_roc --attack_type wb -ldir wb_attack/<exp_name>` scores the attack.
One GPU.
"""
from __future__ import annotations

import argparse
import os
import warnings

import numpy as np

from ..attack import _dist32
from ..pbb import pbb_init_from_bank
from ..wb import pair_wb_attack, wb_attack
from .fbb import update_args  # noqa: F401  (the YAML overlay of the command line)
from .utils import check_folder, get_filepaths_from_dir, read_images_u8_nchw, save_files

# options added after params.txt got its form: an unused one leaves the file as it was before the option existed
LATER_OPTIONS = ("pg_steps", "alpha", "in_channels", "pair_distance", "sn_forwards", "optimizer", "memory", "ladder", "step0", "encoder_path")
LBFGS_DEFAULTS = (("memory", 8), ("ladder", 8), ("step0", 1.0))
PGGAN_OPTIONS = LATER_OPTIONS[:3]


def parse_arguments(argv=None):
    parser = argparse.ArgumentParser()
    data_root = os.path.join(os.getcwd(), 'data', 'miniCelebA')
    parser.add_argument('--exp_name', '-name', type=str, default='debug', help='experiment name; results go to ./wb_attack/<exp_name>')
    parser.add_argument('--pos_data_dir', type=str, default=os.path.join(data_root, 'train'), help='folder with the member (training) query images')
    parser.add_argument('--neg_data_dir', type=str, default=os.path.join(data_root, 'test'), help='folder with the non-member (held-out) query images')
    parser.add_argument('--resolution', '-resolution', type=int, default=64, help='images that differ are resized to this square size')
    parser.add_argument('--BATCH_SIZE', type=int, default=30)
    parser.add_argument('--local_config', type=str, default=None)
    parser.add_argument('--gan', type=str, default='dcgan', help='the generator class: dcgan, wgangp, pggan or vaegan (with --sn_forwards)')
    parser.add_argument('--generator_path', type=str, default=None, help="the generator's state dict (generator.pth)")
    parser.add_argument('--nz', type=int, default=100, help='length of a latent vector')
    parser.add_argument('--ngf', type=int, default=64, help='width parameter of the generator (features_g)')
    parser.add_argument('--nc', type=int, default=3, help='image channels')
    parser.add_argument('--noise_path', type=str, default=None, help="npz with the bank's latents (array 'noise'), as the generate branches write it")
    parser.add_argument('--num_init', type=int, default=None, help='without --noise_path: draw this many starting latents')
    parser.add_argument('--init_seed', type=int, default=0, help='seed of the drawn starting latents')
    parser.add_argument('--pg_steps', type=int, default=None, help='pggan: resolution steps (4 * 2^pg_steps pixels); no default')
    parser.add_argument('--alpha', type=float, default=None, help='pggan: fade-in weight of the last block (default 1)')
    parser.add_argument('--in_channels', type=int, default=None, help='pggan: channel count of the first block (default 256)')
    parser.add_argument('--sn_forwards', type=int, default=None, help='vaegan: hold the spectral-norm state of the K-th forward after loading; no default')
    parser.add_argument('--encoder_path', type=str, default=None,
                        help="vaegan: start from the encoder's posterior mean instead of the nearest bank latent (state dict, or a checkpoint with netE_state_dict)")
    parser.add_argument('--steps', type=int, default=64, help='gradient steps')
    parser.add_argument('--lr', type=float, default=0.05, help="Adam's step size")
    parser.add_argument('--beta1', type=float, default=0.9)
    parser.add_argument('--beta2', type=float, default=0.999)
    parser.add_argument('--pair_distance', type=str, default=None, choices=['l2-lpips'],
                        help='run the descent under 0.2 * LPIPS + L2 (weights from $GANLEAKS_VGG16_PATH / $GANLEAKS_LPIPS_LIN_PATH)')
    parser.add_argument('--optimizer', type=str, default=None, choices=['adam', 'lbfgs'], help="adam (the default) or lbfgs, the paper's optimiser")
    parser.add_argument('--memory', type=int, default=None, help='lbfgs: pairs kept per query (default 8, 1..16)')
    parser.add_argument('--ladder', type=int, default=None, help='lbfgs: step widths scored per step (default 8, 1..32)')
    parser.add_argument('--step0', type=float, default=None, help='lbfgs: length of the first steepest-descent trial in latent space (default 1)')
    return parser.parse_args(argv)


def _optimizer_keywords(args):
    """the optimiser's keywords for wb_attack / pair_wb_attack"""
    if getattr(args, "optimizer", None) != "lbfgs":
        return {}
    kw = {"optimizer": "lbfgs"}
    for name, default in LBFGS_DEFAULTS:
        v = getattr(args, name, None)
        kw[name] = default if v is None else v
    return kw


def _request(args):
    """what can be refused before any file is read"""
    if args.gan not in ("dcgan", "wgangp", "pggan", "vaegan"):
        raise SystemExit("--gan must be dcgan, wgangp, pggan or vaegan, got %r: the backward pass is built for the DCGAN / WGAN-GP generator, "
                         "for PGGAN and for VAEGAN with its spectral-norm state held" % (args.gan,))
    sn = getattr(args, "sn_forwards", None)
    if args.gan == "vaegan":
        if sn is None:
            raise SystemExit("--gan vaegan needs --sn_forwards K: vaegan's spectral normalisation advances with every forward, so the generator "
                             "to attack has to be named -- the one its K-th forward after loading runs, held from then on; there is no default")
        if int(sn) < 1:
            raise SystemExit("--sn_forwards must be at least 1, got %s" % (sn,))
        if int(args.resolution) != 64:
            raise SystemExit("--gan vaegan makes 64 x 64 images; --resolution is %s" % (args.resolution,))
    elif sn is not None:
        raise SystemExit("--sn_forwards belongs to --gan vaegan, got --gan %s" % (args.gan,))
    pg = [getattr(args, name, None) for name in PGGAN_OPTIONS]
    pair = getattr(args, "pair_distance", None)
    if pair not in (None, "l2-lpips"):
        raise SystemExit("--pair_distance must be l2-lpips, got %r (without it the descent runs on exact l2)" % (pair,))
    if pair is not None and int(args.resolution) % 16:
        raise SystemExit("--pair_distance l2-lpips needs a --resolution that is a multiple of 16 (VGG16 pools four times), got %s" % (args.resolution,))
    if args.gan == "pggan":
        if pg[0] is None:
            raise SystemExit("--gan pggan needs --pg_steps: PGGAN's depth (images of 4 * 2^pg_steps pixels) has no default here, and --steps "
                             "is the number of gradient steps")
        if not 0 <= int(pg[0]) <= 8 or (pg[1] is not None and not 0.0 <= float(pg[1]) <= 1.0) or (pg[2] is not None and int(pg[2]) < 32):
            raise SystemExit("PGGAN: --pg_steps must lie in [0, 8], --alpha in [0, 1] and --in_channels be at least 32, got %s, %s, %s" % tuple(pg))
        if int(args.resolution) != 4 * 2 ** int(pg[0]):
            raise SystemExit("PGGAN at --pg_steps %d makes %d x %d images; --resolution is %s" % (pg[0], 4 * 2 ** int(pg[0]), 4 * 2 ** int(pg[0]),
                                                                                                   args.resolution))
    elif any(v is not None for v in pg):
        raise SystemExit("--pg_steps, --alpha and --in_channels belong to --gan pggan (PGGAN), got --gan %s" % (args.gan,))
    opt = getattr(args, "optimizer", None)
    if opt not in (None, "adam", "lbfgs"):
        raise SystemExit("--optimizer must be adam or lbfgs, got %r" % (opt,))
    given = [name for name, _ in LBFGS_DEFAULTS if getattr(args, name, None) is not None]
    if opt != "lbfgs" and given:
        raise SystemExit("--%s belongs to --optimizer lbfgs" % given[0])
    if opt == "lbfgs":
        kw = _optimizer_keywords(args)
        if not 1 <= int(kw["memory"]) <= 16 or not 1 <= int(kw["ladder"]) <= 32 or not (np.isfinite(kw["step0"]) and kw["step0"] > 0):
            raise SystemExit("--memory must lie in 1..16, --ladder in 1..32 and --step0 be finite and positive, got %s, %s, %s"
                             % (kw["memory"], kw["ladder"], kw["step0"]))
    if getattr(args, "generator_path", None) is None:
        raise SystemExit("--generator_path is needed: the white-box attacker holds the generator")
    if getattr(args, "encoder_path", None) is not None:
        if args.gan != "vaegan":
            raise SystemExit("--encoder_path belongs to --gan vaegan (the family with an encoder), got --gan %s" % (args.gan,))
        if pair is not None:
            raise SystemExit("--encoder_path starts the exact-l2 descent; with --pair_distance l2-lpips the start is the bank latent nearest under that distance")
        if getattr(args, "noise_path", None) is not None or getattr(args, "num_init", None) is not None:
            raise SystemExit("--encoder_path starts from the encoder's posterior mean: no bank is read, so --noise_path and --num_init do not apply")
    elif (getattr(args, "noise_path", None) is None) == (getattr(args, "num_init", None) is None):
        raise SystemExit("give exactly one of --noise_path (the bank's latents) and --num_init (draw that many)")
    if args.num_init is not None and int(args.num_init) < 1:
        raise SystemExit("--num_init must be at least 1, got %s" % (args.num_init,))
    if int(args.steps) < 0 or not (np.isfinite(args.lr) and args.lr > 0) or not (0 <= args.beta1 < 1) or not (0 <= args.beta2 < 1):
        raise SystemExit("--steps must be >= 0, --lr positive and --beta1, --beta2 in [0, 1), got %s, %s, %s, %s"
                         % (args.steps, args.lr, args.beta1, args.beta2))


def load_generator(args):
    """-> (generator, nz); PGGAN: the generator at the requested depth"""
    import torch
    sd = torch.load(args.generator_path, map_location="cpu", weights_only=True)
    nz = int(args.nz)
    if args.gan == "pggan":
        from ..gan_models.pggan.model_torch import Generator as PgganGenerator
        pg = PgganGenerator(nz, 256 if args.in_channels is None else int(args.in_channels), int(args.nc))
        pg.load_state_dict(sd)
        return pg.at(int(args.pg_steps), 1.0 if args.alpha is None else float(args.alpha)), nz
    if args.gan == "vaegan":
        from ..gan_models.vaegan.train import Generator as VaeganGenerator
        vg = VaeganGenerator(nz, d=int(args.ngf))
        vg.load_state_dict(sd)
        return vg.frozen(int(args.sn_forwards)), nz
    from ..gan_models.dcgan.model_torch import Generator     # wgangp shares it (gan_models/wgangp/model.py)
    gen = Generator(nz, int(args.nc), int(args.ngf))
    gen.load_state_dict(sd)
    return gen, nz


def main(args):
    _request(args)
    assert os.path.exists(args.generator_path)
    save_dir = check_folder(os.path.join(os.getcwd(), 'wb_attack', args.exp_name))
    for name, value in _optimizer_keywords(args).items():                             # params.txt names what the optimiser ran with
        setattr(args, name, value)
    lines = ["%s:%s" % (key, value) for key, value in vars(args).items() if not (key in LATER_OPTIONS and value is None)]
    with open(os.path.join(save_dir, 'params.txt'), 'w') as handle:
        handle.write("".join(line + "\n" for line in lines))
    print("\n".join(lines))

    resolution = args.resolution
    pos_query_imgs = read_images_u8_nchw(get_filepaths_from_dir(args.pos_data_dir, ext='png'), resolution)
    neg_query_imgs = read_images_u8_nchw(get_filepaths_from_dir(args.neg_data_dir, ext='png'), resolution)
    both = np.concatenate([pos_query_imgs, neg_query_imgs])
    n_pos = len(pos_query_imgs)

    gen, nz = load_generator(args)
    if getattr(args, "encoder_path", None) is not None:
        return _main_l2(args, save_dir, both, n_pos, encoder_start(args, both, gen, nz))
    if args.noise_path is not None:
        with np.load(args.noise_path) as data:
            z_bank = np.asarray(data["noise"], np.float32)
        z_bank = z_bank.reshape(len(z_bank), -1)
        if z_bank.shape[1] != nz:
            raise SystemExit("--noise_path holds latents of length %d, the generator takes %d" % (z_bank.shape[1], nz))
    else:
        z_bank = np.random.default_rng(int(args.init_seed)).standard_normal((int(args.num_init), nz)).astype(np.float32)
    if len(z_bank) < int(args.BATCH_SIZE):
        raise SystemExit("the %d starting latents hold no full batch of %d" % (len(z_bank), args.BATCH_SIZE))

    if getattr(args, "pair_distance", None) is not None:
        return _main_pair(args, save_dir, both, n_pos, gen, z_bank)
    z_init, _ = pbb_init_from_bank(both, gen, z_bank, batch_size=int(args.BATCH_SIZE))
    return _main_l2(args, save_dir, both, n_pos, (gen, z_init))


def encoder_start(args, both, gen, nz):
    """--encoder_path: -> (gen, z_init), the start the encoder's (clamped) posterior mean of every query -- no bank is read"""
    from ..recon import recon_attack
    from .recon import load_encoder
    enc = load_encoder(args.encoder_path, nz)
    return gen, recon_attack(both, enc, gen, samples=0)[3]


def _main_l2(args, save_dir, both, n_pos, start):
    """the descent on exact l2 from the start (generator, z_init), and its files"""
    gen, z_init = start
    dist, z_star, S, trace = wb_attack(both, gen, z_init, steps=int(args.steps), lr=float(args.lr), beta1=float(args.beta1), beta2=float(args.beta2),
                                       history=True, **_optimizer_keywords(args))
    d = int(np.prod(both.shape[1:]))
    init = _dist32(trace[0], d, "u8")                                                 # attack()'s float32 for the starting S
    loss, init_loss, S = dist.astype(np.float64).reshape(-1, 1), init.astype(np.float64).reshape(-1, 1), S.reshape(-1, 1)
    save_files(save_dir, ['pos_loss', 'neg_loss'], [np.ascontiguousarray(loss[:n_pos]), np.ascontiguousarray(loss[n_pos:])])
    save_files(save_dir, ['pos_z', 'neg_z'], [np.ascontiguousarray(z_star[:n_pos]), np.ascontiguousarray(z_star[n_pos:])])
    save_files(save_dir, ['pos_S', 'neg_S'], [np.ascontiguousarray(S[:n_pos]), np.ascontiguousarray(S[n_pos:])])
    save_files(save_dir, ['pos_init_loss', 'neg_init_loss'], [np.ascontiguousarray(init_loss[:n_pos]), np.ascontiguousarray(init_loss[n_pos:])])
    save_files(save_dir, ['pos_trace', 'neg_trace'], [np.ascontiguousarray(trace[:, :n_pos]), np.ascontiguousarray(trace[:, n_pos:])])
    return save_dir, loss[:n_pos], loss[n_pos:], z_star, S


def _main_pair(args, save_dir, both, n_pos, gen, z_bank):
    """main() under --pair_distance l2-lpips: started from the bank latent nearest under that distance"""
    from .. import lpips as _lp
    from ..attack import GeneratedBank, attack
    model = _lp.default_model()                          # FileNotFoundError names the two weight files
    n_eff = (len(z_bank) // int(args.BATCH_SIZE)) * int(args.BATCH_SIZE)
    _, idx = attack(both, GeneratedBank(gen, z_bank), distance="l2-lpips", batch_size=int(args.BATCH_SIZE), lpips=model)
    assert (np.asarray(idx) < n_eff).all()
    z_init = z_bank[np.asarray(idx)]
    dist, z_star, key, trace = pair_wb_attack(both, gen, z_init, steps=int(args.steps), lr=float(args.lr), beta1=float(args.beta1),
                                              beta2=float(args.beta2), history=True, lpips=model, **_optimizer_keywords(args))
    init = trace[0].astype(np.uint32).view(np.float32)                                # attack()'s float32 for the start
    loss, init_loss, key = dist.astype(np.float64).reshape(-1, 1), init.astype(np.float64).reshape(-1, 1), key.reshape(-1, 1)
    save_files(save_dir, ['pos_loss', 'neg_loss'], [np.ascontiguousarray(loss[:n_pos]), np.ascontiguousarray(loss[n_pos:])])
    save_files(save_dir, ['pos_z', 'neg_z'], [np.ascontiguousarray(z_star[:n_pos]), np.ascontiguousarray(z_star[n_pos:])])
    save_files(save_dir, ['pos_key', 'neg_key'], [np.ascontiguousarray(key[:n_pos]), np.ascontiguousarray(key[n_pos:])])
    save_files(save_dir, ['pos_init_loss', 'neg_init_loss'], [np.ascontiguousarray(init_loss[:n_pos]), np.ascontiguousarray(init_loss[n_pos:])])
    save_files(save_dir, ['pos_trace', 'neg_trace'], [np.ascontiguousarray(trace[:, :n_pos]), np.ascontiguousarray(trace[:, n_pos:])])
    return save_dir, loss[:n_pos], loss[n_pos:], z_star, key


if __name__ == '__main__':
    import yaml
    cli = parse_arguments()
    if cli.local_config is None:
        warnings.warn("No config file was provided. Using default parameters.")
    else:
        with open(str(cli.local_config)) as handle:
            update_args(cli, yaml.safe_load(handle))
    main(cli)
