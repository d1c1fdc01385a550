"""[build] The reconstruction attack for VAEGAN (Hilprecht et al., the paper of mc.py's attacks) on the data fbb.py reads.

The attacker holds the whole VAEGAN: for every query x the encoder gives the posterior (mu, logvar), the generator reconstructs x from the
posterior mean and from --samples draws of the posterior, and the query is scored by the mean L2 distance of the draws' reconstructions
(ganleaks_amd.recon.recon_attack).  No sample bank and no search.  The reference fork has no driver for it; the data flags, the YAML overlay
and the layout of the result directory are wb.py's, so that eval_roc.py scores the result unchanged.

    python -m ganleaks_amd.attack_models.recon --local_config config_attack_fbb.yaml --gan vaegan --generator_path generator.pth
           --encoder_path encoder.pth --sn_forwards K [--nz Z --ngf d] [--samples n --seed k]

--gan                    vaegan only: the model family with an encoder
--generator_path, --sn_forwards, --nz, --ngf   as wb.py: the generator attacked is Generator(nz, d=--ngf).frozen(K)
--encoder_path           the encoder's state dict (netE.state_dict()), or a checkpoint dict that holds it under `netE_state_dict` (what the
                         reference's training loop saves).  The reference's pickled module netE.pt is refused: unpickling executes code
                         from the file
--samples, --seed        posterior draws per query (default 16; 0 scores by the reconstruction at the mean alone) and the seed of their noise
Files under ./recon_attack/<exp_name>/:
    {pos,neg}_loss.npy float64 [n, 1]: the mean distance over the draws; {pos,neg}_dist_mu.npy float64 [n, 1]: the distance to the
    reconstruction at the posterior mean; {pos,neg}_S.npy int64 [n, samples + 1]: the exact sums of squared differences, column 0 at the
    mean; {pos,neg}_z.npy float32 [n, nz]: the (clamped) posterior means; params.txt.  Small = member-like:
    `eval_roc --attack_type recon -ldir recon_attack/<exp_name>` scores the attack.
One GPU.
"""
from __future__ import annotations

import argparse
import os
import warnings

import numpy as np

from ..recon import recon_attack
from . import wb as _wb
from .fbb import update_args  # noqa: F401  (the YAML overlay of the command line)
from .utils import check_folder, get_filepaths_from_dir, read_images_u8_nchw, save_files


def parse_arguments(argv=None):
    parser = argparse.ArgumentParser()
    data_root = os.path.join(os.getcwd(), 'data', 'miniCelebA')
    parser.add_argument('--exp_name', '-name', type=str, default='debug', help='experiment name; results go to ./recon_attack/<exp_name>')
    parser.add_argument('--pos_data_dir', type=str, default=os.path.join(data_root, 'train'), help='folder with the member (training) query images')
    parser.add_argument('--neg_data_dir', type=str, default=os.path.join(data_root, 'test'), help='folder with the non-member (held-out) query images')
    parser.add_argument('--resolution', '-resolution', type=int, default=64, help='images that differ are resized to this square size')
    parser.add_argument('--local_config', type=str, default=None)
    parser.add_argument('--gan', type=str, default='vaegan', help='vaegan: the model family with an encoder')
    parser.add_argument('--generator_path', type=str, default=None, help="the generator's state dict (generator.pth)")
    parser.add_argument('--encoder_path', type=str, default=None, help="the encoder's state dict, or a checkpoint dict with netE_state_dict")
    parser.add_argument('--nz', type=int, default=100, help='length of a latent vector')
    parser.add_argument('--ngf', type=int, default=64, help="width parameter d of the generator (the encoder's is 64: its heads are hard-wired)")
    parser.add_argument('--nc', type=int, default=3, help='image channels')
    parser.add_argument('--sn_forwards', type=int, default=None, help='hold the spectral-norm state of the K-th forward after loading; no default')
    parser.add_argument('--samples', type=int, default=16, help='posterior draws per query')
    parser.add_argument('--seed', type=int, default=0, help="seed of the draws' noise")
    return parser.parse_args(argv)


def load_encoder(path, nz, d=64):
    """-> Encoder with the state dict at `path` loaded: a state dict, or a checkpoint dict that holds one under netE_state_dict"""
    import torch
    from ..gan_models.vaegan.train import Encoder
    if not os.path.exists(path):
        raise SystemExit("--encoder_path %s does not exist" % path)
    try:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    except Exception as e:                       # a pickled nn.Module (the reference's netE.pt): not loaded, it would execute code from the file
        raise SystemExit("--encoder_path %s must hold netE.state_dict() or a checkpoint dict with netE_state_dict; a pickled module object "
                         "(the reference's netE.pt) is not loaded, because unpickling executes code from the file (%s)" % (path, type(e).__name__)) from e
    if not isinstance(sd, dict):
        raise SystemExit("--encoder_path %s holds a %s, not a state dict" % (path, type(sd).__name__))
    if "netE_state_dict" in sd:
        sd = sd["netE_state_dict"]
    enc = Encoder(int(nz), d=int(d))
    enc.load_state_dict(sd)
    return enc


def _request(args):
    """what can be refused before any file is read"""
    if args.gan != "vaegan":
        raise SystemExit("--gan must be vaegan, got %r: the reconstruction attack needs the model's encoder, and VAEGAN is the family that has one" % (args.gan,))
    sn = getattr(args, "sn_forwards", None)
    if sn is None:
        raise SystemExit("--gan vaegan needs --sn_forwards K: vaegan's spectral normalisation advances with every forward, so the generator "
                         "to attack has to be named -- the one its K-th forward after loading runs, held from then on; there is no default")
    if int(sn) < 1:
        raise SystemExit("--sn_forwards must be at least 1, got %s" % (sn,))
    if int(args.resolution) != 64:
        raise SystemExit("--gan vaegan makes 64 x 64 images; --resolution is %s" % (args.resolution,))
    if getattr(args, "generator_path", None) is None:
        raise SystemExit("--generator_path is needed: the attacker holds the generator")
    if getattr(args, "encoder_path", None) is None:
        raise SystemExit("--encoder_path is needed: the attacker holds the encoder")
    if int(args.samples) < 0:
        raise SystemExit("--samples must be >= 0, got %s" % (args.samples,))


def main(args):
    _request(args)
    if not os.path.exists(args.generator_path):
        raise SystemExit("--generator_path %s does not exist" % args.generator_path)
    enc = load_encoder(args.encoder_path, args.nz)
    save_dir = check_folder(os.path.join(os.getcwd(), 'recon_attack', args.exp_name))
    lines = ["%s:%s" % (key, value) for key, value in vars(args).items()]
    with open(os.path.join(save_dir, 'params.txt'), 'w') as handle:
        handle.write("".join(line + "\n" for line in lines))
    print("\n".join(lines))

    pos_query_imgs = read_images_u8_nchw(get_filepaths_from_dir(args.pos_data_dir, ext='png'), args.resolution)
    neg_query_imgs = read_images_u8_nchw(get_filepaths_from_dir(args.neg_data_dir, ext='png'), args.resolution)
    both = np.concatenate([pos_query_imgs, neg_query_imgs])
    n_pos = len(pos_query_imgs)

    gen, _ = _wb.load_generator(args)
    loss, dist_mu, S, z_mu = recon_attack(both, enc, gen, samples=int(args.samples), seed=int(args.seed))
    loss, dist_mu = loss.reshape(-1, 1), dist_mu.astype(np.float64).reshape(-1, 1)
    save_files(save_dir, ['pos_loss', 'neg_loss'], [np.ascontiguousarray(loss[:n_pos]), np.ascontiguousarray(loss[n_pos:])])
    save_files(save_dir, ['pos_dist_mu', 'neg_dist_mu'], [np.ascontiguousarray(dist_mu[:n_pos]), np.ascontiguousarray(dist_mu[n_pos:])])
    save_files(save_dir, ['pos_S', 'neg_S'], [np.ascontiguousarray(S[:n_pos]), np.ascontiguousarray(S[n_pos:])])
    save_files(save_dir, ['pos_z', 'neg_z'], [np.ascontiguousarray(z_mu[:n_pos]), np.ascontiguousarray(z_mu[n_pos:])])
    return save_dir, loss[:n_pos], loss[n_pos:], z_mu, S


if __name__ == '__main__':
    import yaml
    cli = parse_arguments()
    if cli.local_config is None:
        warnings.warn("No config file was provided. Using default parameters.")
    else:
        with open(str(cli.local_config)) as handle:
            update_args(cli, yaml.safe_load(handle))
    main(cli)
