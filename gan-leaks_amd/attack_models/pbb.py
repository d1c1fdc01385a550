"""[build] The partial-black-box attack of GAN-Leaks (section 5.3 of the paper) on the data fbb.py reads.

The attacker holds the generator: for every query x the latent space is searched for z* = argmin_z L(x, G(z)) without gradients and the
query is scored by L(x, G(z*)), L the L2 distance of Loss('l2') (attack_models/utils.py:161-164).  The reference fork has no driver for it;
the data flags, the YAML overlay and the layout of the result directory are fbb.py's (attack_models/fbb.py:18-67), so that eval_roc.py
scores the result unchanged.  The search is ganleaks_amd.pbb.pbb_attack -- a (1 + lambda) evolution strategy for all queries at once, the
candidates generated and compared on the device -- started from the nearest of a bank of latents (the full-black-box answer), which it can
only improve on.

    python -m ganleaks_amd.attack_models.pbb --local_config config_attack_fbb.yaml --gan {dcgan,wgangp,pggan} --generator_path generator.pth
           [--nz --ngf --in_channels --steps --alpha] [--noise_path npz | --num_init N --init_seed s]
           [--rounds --population --sigma --seed] [--BATCH_SIZE]
           [--optimizer {es,powell} [--sweeps n --ladder L --step0 s]]
    python -m ganleaks_amd.attack_models.pbb ... --gan vaegan --sn_forwards K [--nz Z --ngf d]
    python -m ganleaks_amd.attack_models.pbb ... --pair_distance l2-lpips
    python -m ganleaks_amd.attack_models.pbb ... --gan medgan --generator_path generator.pth --autoencoder_path FILE --input_size F [--binary]

--gan, --generator_path  the generator class and its state dict (what the training scripts save as generator.pth)
--sn_forwards            VAEGAN only, no default: VAEGAN's spectral normalisation advances with every forward, so the generator searched is the one
                         its K-th forward after loading would have run, held from then on (Generator(nz, d=--ngf).frozen(K)); K >= 1,
                         --resolution 64.  Without it --gan vaegan is refused
--nz, --ngf              DCGAN / WGAN-GP: latent length and width (features_g); --nz, --in_channels, --steps, --alpha: PGGAN
--gan medgan             medGAN's tables: the generator is decoder(generator(z)) >= 0.5, the 0/1 rows of synthetic.npy (gan_models/medgan/train.py:
                         306-312).  --autoencoder_path: the Autoencoder's state dict (decoder.0.{weight,bias}) or the reference's decoder.pth
                         (0.{weight,bias}); --input_size F: the table's columns; --binary: the sigmoid decoder (default: ReLU); --nz is 128.
                         --pos_data_dir / --neg_data_dir name 2-D .npy tables of whole numbers (bank_io.load_rows); --resolution is not
                         consulted; the loss files hold fl32(S / F), S the number of differing columns; --pair_distance is refused (LPIPS is
                         defined on images)
--encoder_path           VAEGAN only: the encoder's state dict (or a checkpoint dict with netE_state_dict).  The start is then the encoder's
                         posterior mean of every query (ganleaks_amd.recon), not the nearest bank latent: no bank is read, and --noise_path
                         and --num_init are not needed (and refused).  Exact l2 only
--noise_path             the .npz the generate branches write under npz_noise/ (array `noise`): the latents of the sample bank
--num_init, --init_seed  without --noise_path: that many standard-normal latents drawn from numpy's default_rng(init_seed)
--BATCH_SIZE             only the first (N // BATCH_SIZE) * BATCH_SIZE latents take part in the start, as in fbb.py:77
--rounds, --population, --sigma, --seed   the search (ganleaks_amd.pbb.pbb_attack)
--optimizer              es (the default) or powell, the paper's optimiser: --sweeps sweeps (default 2) of Powell's conjugate-direction method,
                         every line search a two-sided ladder of --ladder step widths (default 8; even, 2..32) scored in one batched forward,
                         every direction starting at width --step0 (default 1).  --rounds, --population, --sigma and --seed are not used by
                         powell, and --sweeps, --ladder, --step0 belong to it (--steps is PGGAN's depth here).  The trace then has
                         sweeps + 1 rows; the other files are the same
--pair_distance l2-lpips (default absent) the same attack under 0.2 * LPIPS + L2, the distance fbb.py hard-wires and the paper's loss
                         (ganleaks_amd.pbb.pair_pbb_attack); VGG16 and lin weights from $GANLEAKS_VGG16_PATH / $GANLEAKS_LPIPS_LIN_PATH; the
                         start is the bank latent nearest under that distance (pair_pbb_init_from_bank); the resolution must be a multiple
                         of 16.  {pos,neg}_key.npy (int64 [n, 1]: the uint32 pattern of the float32 distance, the exact and ordered score)
                         takes the place of the S files, and the trace holds keys
Files under ./pbb_attack/<exp_name>/:
    {pos,neg}_loss.npy float64 [n, 1]: L(x, G(z*)); {pos,neg}_z.npy float32 [n, nz]: z*; {pos,neg}_S.npy int64 [n, 1]: the exact sum of
    squared differences behind the loss; {pos,neg}_init_loss.npy float64 [n, 1]: the full-black-box score the search started from;
    {pos,neg}_trace.npy int64 [rounds + 1, n]: S after every round ([sweeps + 1, n] under --optimizer powell); params.txt (an absent --pair_distance leaves no line).  Small = member-like:
    `eval_roc --attack_type pbb -ldir pbb_attack/<exp_name>` scores the attack.
One GPU; the queries of a larger set can be split by hand (pbb_attack's query_base keeps the noise of every query what it was).
"""
from __future__ import annotations

import argparse
import os
import warnings

import numpy as np

from ..attack import _dist32
from ..pbb import pair_pbb_attack, pair_pbb_init_from_bank, pbb_attack, pbb_init_from_bank
from .fbb import update_args  # noqa: F401  (the YAML overlay of the command line)
from .utils import check_folder, get_filepaths_from_dir, read_images_u8_nchw, save_files

# options added after params.txt got its form: an unused one leaves the file as it was before the option existed
LATER_OPTIONS = ("pair_distance",)
VAEGAN_OPTIONS = ("sn_forwards", "encoder_path")        # the same: params.txt names K and the encoder only where --gan vaegan gave them
MEDGAN_OPTIONS = ("autoencoder_path", "input_size", "binary")        # and these only where --gan medgan gave them
POWELL_OPTIONS = ("optimizer", "sweeps", "ladder", "step0")          # and these only where --optimizer was given (powell: what it ran with)


def parse_arguments(argv=None):
    parser = argparse.ArgumentParser()
    data_root = os.path.join(os.getcwd(), 'data', 'miniCelebA')
    parser.add_argument('--exp_name', '-name', type=str, default='debug', help='experiment name; results go to ./pbb_attack/<exp_name>')
    parser.add_argument('--pos_data_dir', type=str, default=os.path.join(data_root, 'train'), help='folder with the member (training) query images')
    parser.add_argument('--neg_data_dir', type=str, default=os.path.join(data_root, 'test'), help='folder with the non-member (held-out) query images')
    parser.add_argument('--resolution', '-resolution', type=int, default=64, help='images that differ are resized to this square size')
    parser.add_argument('--BATCH_SIZE', type=int, default=30)
    parser.add_argument('--local_config', type=str, default=None)
    parser.add_argument('--gan', type=str, default='dcgan', choices=['dcgan', 'wgangp', 'pggan', 'vaegan', 'medgan'], help='the generator class (vaegan: with --sn_forwards)')
    parser.add_argument('--generator_path', type=str, default=None, help="the generator's state dict (generator.pth)")
    parser.add_argument('--nz', type=int, default=None, help='length of a latent vector (default 100; 256 for pggan)')
    parser.add_argument('--ngf', type=int, default=64, help='dcgan / wgangp: width parameter of the generator (features_g)')
    parser.add_argument('--nc', type=int, default=3, help='image channels')
    parser.add_argument('--in_channels', type=int, default=256, help='pggan: channel count of the first block')
    parser.add_argument('--steps', type=int, default=4, help='pggan: resolution steps (4 * 2^steps pixels)')
    parser.add_argument('--alpha', type=float, default=1.0, help='pggan: fade-in weight of the last block')
    parser.add_argument('--sn_forwards', type=int, default=None, help='vaegan: hold the spectral-norm state of the K-th forward after loading; no default')
    parser.add_argument('--encoder_path', type=str, default=None,
                        help="vaegan: start from the encoder's posterior mean instead of the nearest bank latent (state dict, or a checkpoint with netE_state_dict)")
    parser.add_argument('--noise_path', type=str, default=None, help="npz with the bank's latents (array 'noise'), as the generate branches write it")
    parser.add_argument('--num_init', type=int, default=None, help='without --noise_path: draw this many starting latents')
    parser.add_argument('--init_seed', type=int, default=0, help='seed of the drawn starting latents')
    parser.add_argument('--rounds', type=int, default=32)
    parser.add_argument('--population', type=int, default=64, help='candidates per query and round')
    parser.add_argument('--sigma', type=float, default=0.5, help='initial step width')
    parser.add_argument('--seed', type=int, default=0, help='seed of the search noise')
    parser.add_argument('--pair_distance', type=str, default=None, choices=['l2-lpips'],
                        help='run the search under 0.2 * LPIPS + L2 (weights from $GANLEAKS_VGG16_PATH / $GANLEAKS_LPIPS_LIN_PATH)')
    parser.add_argument('--optimizer', type=str, default=None, choices=['es', 'powell'], help="es (the default) or powell, the paper's optimiser")
    parser.add_argument('--sweeps', type=int, default=None, help='powell: sweeps over the direction set (default 2)')
    parser.add_argument('--ladder', type=int, default=None, help='powell: step widths scored per line search (default 8; even, 2..32)')
    parser.add_argument('--step0', type=float, default=None, help='powell: first trial width of every direction (default 1)')
    parser.add_argument('--autoencoder_path', type=str, default=None, help="medgan: the autoencoder's state dict (decoder.0.*), or decoder.pth (0.*)")
    parser.add_argument('--input_size', type=int, default=None, help="medgan: columns of the table")
    parser.add_argument('--binary', action='store_const', const=True, default=None, help="medgan: the sigmoid decoder (default: ReLU)")
    return parser.parse_args(argv)


def _optimizer_keywords(args):
    """the keywords --optimizer adds to pbb_attack / pair_pbb_attack: none unless it is powell"""
    if getattr(args, "optimizer", None) != "powell":
        return {}
    kw = {"optimizer": "powell"}
    for name, default in (("sweeps", 2), ("ladder", 8), ("step0", 1.0)):
        v = getattr(args, name, None)
        kw[name] = default if v is None else v
    return kw


def _request_optimizer(args):
    opt = getattr(args, "optimizer", None)
    if opt not in (None, "es", "powell"):
        raise SystemExit("--optimizer must be es or powell, got %r" % (opt,))
    given = [name for name in ("sweeps", "ladder", "step0") if getattr(args, name, None) is not None]
    if opt != "powell" and given:
        raise SystemExit("--%s belongs to --optimizer powell" % given[0])
    if opt == "powell":
        kw = _optimizer_keywords(args)
        if int(kw["sweeps"]) != kw["sweeps"] or kw["sweeps"] < 0:
            raise SystemExit("--sweeps must be an integer >= 0, got %s" % (kw["sweeps"],))
        if int(kw["ladder"]) != kw["ladder"] or not 2 <= kw["ladder"] <= 32 or int(kw["ladder"]) % 2:
            raise SystemExit("--ladder must be an even integer in 2..32, got %s" % (kw["ladder"],))
        if not (np.isfinite(kw["step0"]) and kw["step0"] > 0):
            raise SystemExit("--step0 must be finite and positive, got %s" % (kw["step0"],))
        args.sweeps, args.ladder, args.step0 = int(kw["sweeps"]), int(kw["ladder"]), float(kw["step0"])      # params.txt names what ran


def _request(args):
    """what can be refused before any file is read"""
    _request_optimizer(args)
    pair = getattr(args, "pair_distance", None)
    if pair not in (None, "l2-lpips"):
        raise SystemExit("--pair_distance must be l2-lpips, got %r (without it the search runs on exact l2)" % (pair,))
    if pair is not None and args.gan != "medgan" and int(args.resolution) % 16:
        raise SystemExit("--pair_distance l2-lpips needs a --resolution that is a multiple of 16 (VGG16 pools four times), got %s" % (args.resolution,))
    if getattr(args, "generator_path", None) is None:
        raise SystemExit("--generator_path is needed: the partial-black-box attacker holds the generator")
    if getattr(args, "encoder_path", None) is not None:
        if args.gan != "vaegan":
            raise SystemExit("--encoder_path belongs to --gan vaegan (the family with an encoder), got --gan %s" % (args.gan,))
        if pair is not None:
            raise SystemExit("--encoder_path starts the exact-l2 search; with --pair_distance l2-lpips the start is the bank latent nearest under that distance")
        if getattr(args, "noise_path", None) is not None or getattr(args, "num_init", None) is not None:
            raise SystemExit("--encoder_path starts from the encoder's posterior mean: no bank is read, so --noise_path and --num_init do not apply")
    elif (getattr(args, "noise_path", None) is None) == (getattr(args, "num_init", None) is None):
        raise SystemExit("give exactly one of --noise_path (the bank's latents) and --num_init (draw that many)")
    if args.num_init is not None and int(args.num_init) < 1:
        raise SystemExit("--num_init must be at least 1, got %s" % (args.num_init,))
    if int(args.rounds) < 0 or int(args.population) < 1 or not (np.isfinite(args.sigma) and args.sigma > 0):
        raise SystemExit("--rounds must be >= 0, --population >= 1 and --sigma positive, got %s, %s, %s" % (args.rounds, args.population, args.sigma))
    if args.gan not in ("dcgan", "wgangp", "pggan", "vaegan", "medgan"):
        raise SystemExit("--gan must be dcgan, wgangp, pggan, vaegan or medgan, got %r" % (args.gan,))
    if args.gan == "medgan" or any(getattr(args, name, None) is not None for name in ("autoencoder_path", "input_size", "binary")):
        medgan_request(args)
    sn = getattr(args, "sn_forwards", None)
    if args.gan == "vaegan":
        if sn is None:
            raise SystemExit("--gan vaegan needs --sn_forwards K: vaegan's generator changes with every forward, so the generator to search has "
                             "to be named -- the one its K-th forward after loading runs, held from then on; there is no default")
        if int(sn) < 1:
            raise SystemExit("--sn_forwards must be at least 1, got %s" % (sn,))
        if int(args.resolution) != 64:
            raise SystemExit("--gan vaegan makes 64 x 64 images; --resolution is %s" % (args.resolution,))
    elif sn is not None:
        raise SystemExit("--sn_forwards belongs to --gan vaegan, got --gan %s" % (args.gan,))


def medgan_request(args):
    """--gan medgan and its options, before any file is read; settles --nz where it was not given"""
    own = [name for name in MEDGAN_OPTIONS if getattr(args, name, None) is not None]
    if args.gan != "medgan":
        raise SystemExit("--%s belongs to --gan medgan, got --gan %s" % (own[0], args.gan))
    if getattr(args, "autoencoder_path", None) is None:
        raise SystemExit("--gan medgan needs --autoencoder_path: the rows are decoder(generator(z)), and the decoder belongs to the autoencoder "
                         "(its state dict with decoder.0.{weight,bias}, or decoder.pth)")
    if getattr(args, "input_size", None) is None or int(args.input_size) < 1:
        raise SystemExit("--gan medgan needs --input_size F >= 1: the number of columns of the table")
    if getattr(args, "nz", None) is None:
        args.nz = 128
    if int(args.nz) != 128:
        raise SystemExit("--gan medgan has latents of length 128 (the residual generator, gan_models/medgan/model.py:49-71); --nz is %s" % (args.nz,))
    if getattr(args, "pair_distance", None) is not None:
        raise SystemExit("--pair_distance %s is refused for --gan medgan: LPIPS is defined on images, and medGAN's rows are a table; the "
                         "search runs on exact l2" % (args.pair_distance,))


def load_tables(args):
    """--pos_data_dir and --neg_data_dir of --gan medgan: 2-D tables of --input_size columns (bank_io.load_rows)"""
    from ..bank_io import load_rows
    tables = []
    for name in ("pos_data_dir", "neg_data_dir"):
        rows = load_rows(getattr(args, name))
        if rows.ndim != 2 or rows.shape[1] != int(args.input_size):
            raise SystemExit("--%s: --gan medgan takes a 2-D .npy table of %d columns, got shape %r" % (name, int(args.input_size), rows.shape))
        tables.append(rows)
    return tables


def load_generator(args):
    """-> (generator, generate_kwargs, nz)"""
    if args.gan == "medgan":
        from ..gan_models.medgan.model import load_table_generator
        return load_table_generator(args.generator_path, args.autoencoder_path, args.input_size, bool(args.binary)), {}, 128
    import torch
    sd = torch.load(args.generator_path, map_location="cpu", weights_only=True)
    if args.gan == "pggan":
        from ..gan_models.pggan.model_torch import Generator
        nz = 256 if args.nz is None else int(args.nz)
        gen, kw = Generator(nz, int(args.in_channels), int(args.nc)), {"steps": int(args.steps), "alpha": float(args.alpha)}
    elif args.gan == "vaegan":
        from ..gan_models.vaegan.train import Generator
        nz = 100 if args.nz is None else int(args.nz)
        gen = Generator(nz, d=int(args.ngf))
        gen.load_state_dict(sd)
        return gen.frozen(int(args.sn_forwards)), {}, nz
    else:
        from ..gan_models.dcgan.model_torch import Generator     # wgangp shares it (gan_models/wgangp/model.py)
        nz = 100 if args.nz is None else int(args.nz)
        gen, kw = Generator(nz, int(args.nc), int(args.ngf)), {}
    gen.load_state_dict(sd)
    return gen, kw, nz


def _params_lines(args):
    """the lines of params.txt: every option, except a later one that was not given"""
    return ["%s:%s" % (key, value) for key, value in vars(args).items() if not (key in LATER_OPTIONS + VAEGAN_OPTIONS + MEDGAN_OPTIONS + POWELL_OPTIONS and value is None)]


def main(args):
    _request(args)
    assert os.path.exists(args.generator_path)
    save_dir = check_folder(os.path.join(os.getcwd(), 'pbb_attack', args.exp_name))
    lines = _params_lines(args)
    with open(os.path.join(save_dir, 'params.txt'), 'w') as handle:
        handle.write("".join(line + "\n" for line in lines))
    print("\n".join(lines))

    kind = "u8"
    if args.gan == "medgan":
        kind = "int"
        pos_query_imgs, neg_query_imgs = load_tables(args)
    else:
        resolution = args.resolution
        pos_query_imgs = read_images_u8_nchw(get_filepaths_from_dir(args.pos_data_dir, ext='png'), resolution)
        neg_query_imgs = read_images_u8_nchw(get_filepaths_from_dir(args.neg_data_dir, ext='png'), resolution)
    both = np.concatenate([pos_query_imgs, neg_query_imgs])
    n_pos = len(pos_query_imgs)

    gen, kw, nz = load_generator(args)
    if getattr(args, "encoder_path", None) is not None:
        # the start is the encoder's (clamped) posterior mean of every query: no bank is read
        from ..recon import recon_attack
        from .recon import load_encoder
        z_init = recon_attack(both, load_encoder(args.encoder_path, nz), gen, samples=0)[3]
        return _main_l2(args, save_dir, both, n_pos, gen, kw, kind, z_init)
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
        return _main_pair(args, save_dir, both, n_pos, gen, kw, z_bank)
    z_init, _ = pbb_init_from_bank(both, gen, z_bank, batch_size=int(args.BATCH_SIZE), **kw)
    return _main_l2(args, save_dir, both, n_pos, gen, kw, kind, z_init)


def _main_l2(args, save_dir, both, n_pos, gen, kw, kind, z_init):
    """the search on exact l2 from z_init, and its files"""
    dist, z_star, S, trace = pbb_attack(both, gen, z_init, rounds=int(args.rounds), population=int(args.population), sigma=float(args.sigma),
                                        seed=int(args.seed), history=True, **_optimizer_keywords(args), **kw)
    d = int(np.prod(both.shape[1:]))
    init = _dist32(trace[0], d, kind)                                                 # attack()'s float32 for the starting S
    loss, init_loss, S = dist.astype(np.float64).reshape(-1, 1), init.astype(np.float64).reshape(-1, 1), S.reshape(-1, 1)
    save_files(save_dir, ['pos_loss', 'neg_loss'], [np.ascontiguousarray(loss[:n_pos]), np.ascontiguousarray(loss[n_pos:])])
    save_files(save_dir, ['pos_z', 'neg_z'], [np.ascontiguousarray(z_star[:n_pos]), np.ascontiguousarray(z_star[n_pos:])])
    save_files(save_dir, ['pos_S', 'neg_S'], [np.ascontiguousarray(S[:n_pos]), np.ascontiguousarray(S[n_pos:])])
    save_files(save_dir, ['pos_init_loss', 'neg_init_loss'], [np.ascontiguousarray(init_loss[:n_pos]), np.ascontiguousarray(init_loss[n_pos:])])
    save_files(save_dir, ['pos_trace', 'neg_trace'], [np.ascontiguousarray(trace[:, :n_pos]), np.ascontiguousarray(trace[:, n_pos:])])
    return save_dir, loss[:n_pos], loss[n_pos:], z_star, S


def _main_pair(args, save_dir, both, n_pos, gen, kw, z_bank):
    """main() under --pair_distance l2-lpips: started from the bank latent nearest under that distance"""
    from .. import lpips as _lp
    model = _lp.default_model()                          # FileNotFoundError names the two weight files
    z_init, _ = pair_pbb_init_from_bank(both, gen, z_bank, batch_size=int(args.BATCH_SIZE), lpips=model, **kw)
    dist, z_star, key, trace = pair_pbb_attack(both, gen, z_init, rounds=int(args.rounds), population=int(args.population), sigma=float(args.sigma),
                                               seed=int(args.seed), history=True, lpips=model, **_optimizer_keywords(args), **kw)
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
