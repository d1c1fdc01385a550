"""[build] The K-nearest-samples membership attack on the data fbb.py reads: the score of a query is the mean of its distances to the
--K nearest samples of the bank (custom_knn, attack_models/fbb.py:73-88, keeping the args.K nearest samples of fbb.py:32 instead of one),
under either distance of the full-black-box attack.  The reference carries the --K flag but never uses it; the data flags, the YAML
overlay and the layout of the result directory are fbb.py's (attack_models/fbb.py:18-67), so that eval_roc.py scores the result
unchanged.  All K neighbours come from ONE pass over the bank (ganleaks_amd.attack.nearest_neighbours).

    python -m ganleaks_amd.attack_models.knn --syn_data_path ... --pos_data_dir ... --neg_data_dir ... [--K k] [--distance {l2,l2-lpips}]

--syn_data_path, --pos_data_dir, --neg_data_dir: a folder of PNG files (8-bit codes), or a file of floats (bank_io.load_rows): an .npz with
                img_r01 [N,H,W,C] in [0, 1] (VAEGAN's generated.npz; must be --resolution sized), or a 2-D .npy table (medGAN's
                synthetic.npy; --distance l2 only)
--K             1..32 (default 5, fbb.py:32)
--distance      l2: Loss('l2'), attack_models/utils.py:161-164, exact-integer L2 on the int8 matrix cores; rows off both lattices (float
                images, continuous tables) in the fixed-order float32 arithmetic of attack(float_path='exact').
                l2-lpips: 0.2 * LPIPS + L2, the distance fbb.main hard-wires (fbb.py:148, utils.py:166-176): the l2-lpips search kernel with
                a storing epilogue and a selection; weights from $GANLEAKS_VGG16_PATH / $GANLEAKS_LPIPS_LIN_PATH as in fbb.py
Files under ./knn_attack/<exp_name>/:
    {pos,neg}_knn_loss.npy float64 [n, K], ordered by (distance, bank index); {pos,neg}_knn_idx.npy int64 [n, K]; params.txt;
    {pos,neg}_loss.npy float64 [n, 1] = the mean of the K distances taken in float64 -- with --K 1 fbb.py's pos_loss.npy bit for bit -- so
    `eval_roc --attack_type fbb -ldir knn_attack/<exp_name>` scores the attack.
"""
from __future__ import annotations

import argparse
import os
import warnings

import numpy as np

from ..attack import GL_TOPK_MAX, nearest_neighbours, prepare_queries
from .fbb import shard_devices, update_args  # noqa: F401  (update_args: the YAML overlay of the command line)
from .utils import check_folder, save_files


def parse_arguments(argv=None):
    parser = argparse.ArgumentParser()
    data_root = os.path.join(os.getcwd(), 'data', 'miniCelebA')
    parser.add_argument('--exp_name', '-name', type=str, default='debug', help='experiment name; results go to ./knn_attack/<exp_name>')
    parser.add_argument('--syn_data_path', type=str, help='folder with the generated sample bank (image_*.png)')
    parser.add_argument('--pos_data_dir', type=str, default=os.path.join(data_root, 'train'), help='folder with the member (training) query images')
    parser.add_argument('--neg_data_dir', type=str, default=os.path.join(data_root, 'test'), help='folder with the non-member (held-out) query images')
    parser.add_argument('--resolution', '-resolution', type=int, default=64, help='images that differ are resized to this square size')
    parser.add_argument('--BATCH_SIZE', type=int, default=30)
    parser.add_argument('--local_config', type=str, default=None)
    parser.add_argument('--ngpu', type=int, default=1, help='shard the bank over the first N GPUs (key lists merged across them)')
    parser.add_argument('--devices', type=str, default=None, help='explicit device ordinals for the shards, e.g. 0,1,2,3 (overrides --ngpu)')
    parser.add_argument('--K', type=int, default=5, help='nearest samples kept per query (1..%d)' % GL_TOPK_MAX)
    parser.add_argument('--distance', type=str, default='l2-lpips', choices=['l2', 'l2-lpips'],
                        help="distance of the search: 'l2', or 'l2-lpips' = 0.2 * LPIPS + L2 (the reference's fbb distance)")
    return parser.parse_args(argv)


def knn_request(args):
    """(K, distance) from the command line or the YAML overlay; refused before any file is read"""
    distance = getattr(args, "distance", "l2-lpips")
    if distance not in ("l2", "l2-lpips"):
        raise SystemExit("--distance must be l2 or l2-lpips, got %r" % (distance,))
    K = getattr(args, "K", 5)
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= int(K) <= GL_TOPK_MAX:
        raise SystemExit("--K must be an integer in 1..%d, got %r" % (GL_TOPK_MAX, K))
    return int(K), distance


def main(args):
    K, distance = knn_request(args)
    assert os.path.exists(args.syn_data_path)
    save_dir = check_folder(os.path.join(os.getcwd(), 'knn_attack', args.exp_name))
    lines = ["%s:%s" % (key, value) for key, value in vars(args).items()]
    with open(os.path.join(save_dir, 'params.txt'), 'w') as handle:
        handle.write("".join(line + "\n" for line in lines))
    print("\n".join(lines))

    resolution = args.resolution
    from ..bank_io import concat_rows, load_rows
    syn_imgs = load_rows(args.syn_data_path, resolution)
    pos_query_imgs = load_rows(args.pos_data_dir, resolution)
    neg_query_imgs = load_rows(args.neg_data_dir, resolution)
    both = concat_rows(pos_query_imgs, neg_query_imgs)
    n_pos = len(pos_query_imgs)
    if distance == "l2-lpips" and (syn_imgs.ndim != 4 or both.ndim != 4):
        raise SystemExit("--distance l2-lpips needs images; a 2-D table takes --distance l2")
    float_path = "exact" if distance == "l2" else None
    floats = syn_imgs.dtype != np.uint8 or both.dtype != np.uint8

    devices = shard_devices(args)
    if devices is not None:
        from ..shard import DeviceGroup
        with DeviceGroup(devices) as group:
            dist, idx = group.nearest_neighbours(both, bank=syn_imgs, k=K, batch_size=args.BATCH_SIZE, distance=distance, float_path=float_path)
    else:
        model = None
        if distance == "l2-lpips":
            from ..lpips import default_model
            model = default_model()
        # prepared only when the rows fit the streaming budget; otherwise nearest_neighbours slices the raw queries itself
        # (float images under l2-lpips stay raw too: the search settles the row layout of both sides itself)
        queries = both if floats and distance == "l2-lpips" else prepare_queries(both, distance, lpips=model)
        dist, idx = nearest_neighbours(queries, syn_imgs, K, distance=distance, batch_size=args.BATCH_SIZE, lpips=model, float_path=float_path)

    dist64 = dist.astype(np.float64)
    loss = dist64.mean(axis=1, keepdims=True)            # K = 1: the distance itself, fbb.py's pos_loss.npy
    save_files(save_dir, ['pos_knn_loss', 'pos_knn_idx'], [np.ascontiguousarray(dist64[:n_pos]), np.ascontiguousarray(idx[:n_pos])])
    save_files(save_dir, ['neg_knn_loss', 'neg_knn_idx'], [np.ascontiguousarray(dist64[n_pos:]), np.ascontiguousarray(idx[n_pos:])])
    save_files(save_dir, ['pos_loss', 'neg_loss'], [np.ascontiguousarray(loss[:n_pos]), np.ascontiguousarray(loss[n_pos:])])
    return save_dir, dist[:n_pos], idx[:n_pos], dist[n_pos:], idx[n_pos:]


if __name__ == '__main__':
    import yaml
    cli = parse_arguments()
    if cli.local_config is None:
        warnings.warn("No config file was provided. Using default parameters.")
    else:
        with open(str(cli.local_config)) as handle:
            update_args(cli, yaml.safe_load(handle))
    main(cli)
