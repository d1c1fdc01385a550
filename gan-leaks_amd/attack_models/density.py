"""[build] The k-NN density membership attack on the data fbb.py reads, and its calibrated (density-ratio) form.

The score of a query is its exact L2 distance to the --K-th nearest sample of the bank: the k-NN density estimate at the query is
K / (N r_K^d), so a small r_K is a dense spot of the synthetic distribution.  K is any integer up to the number of samples that take part
(the default is floor(sqrt(n_eff)), 316 for a bank of 100k); knn.py and fbb.py --knn_out carry K keys per query and stop at 32.  With
--ref_data_dir the density under the bank is compared with the density under a reference set drawn from the population (the DOMIAS idea;
the density-based form of GAN-Leaks' calibration): the score is the log ratio of the two k-NN radii.  The reference has no driver for
either; the data flags, the YAML overlay and the layout of the result directory are fbb.py's (attack_models/fbb.py:18-67), so that
eval_roc.py scores the result unchanged.  The K-th distance comes from ganleaks_amd.attack.kth_distances: a host search over per-query
counts, at most 8 passes of the counting kernels over the bank for 3 x 64 x 64 images, no pairwise value stored.

    python -m ganleaks_amd.attack_models.density --syn_data_path ... --pos_data_dir ... --neg_data_dir ... [--K k] [--ref_data_dir ... [--K_ref k]]

--syn_data_path, --pos_data_dir, --neg_data_dir, --ref_data_dir: a folder of PNG files (8-bit codes), or a file of floats
                (bank_io.load_rows): an .npz with img_r01 [N,H,W,C] in [0, 1], or a 2-D .npy table (medGAN's synthetic.npy)
--K             1..n_eff, n_eff = (N // BATCH_SIZE) * BATCH_SIZE samples of the bank (default floor(sqrt(n_eff)))
--K_ref         the same for the reference set (default --K)
--distance      l2 only: Loss('l2'), attack_models/utils.py:161-164, on the exact-integer path.  l2-lpips is refused before any file is
                read; rows off both lattices (float images that are not 8-bit codes, continuous tables) are refused once the files show
                it, before any GPU work: the search runs on the exact integer S, which such rows do not have.
--pair_distance {l2-lpips,l2}: (default absent; not together with a non-default --distance) the same attack on the float paths, through
                ganleaks_amd.attack.pair_kth_distances: a search over the uint32 patterns of the float32 distance, 8 passes per K.
                l2-lpips: 0.2 * LPIPS + L2, the distance fbb.main hard-wires (fbb.py:148, utils.py:166-176); weights from
                $GANLEAKS_VGG16_PATH / $GANLEAKS_LPIPS_LIN_PATH as in mc.py; images only (a 2-D table is refused: LPIPS needs images).
                l2: float_path='exact', so .npz / .npy float rows off both lattices work (rows on one lattice take the exact-integer path).
                Files: {pos,neg}_kth_key.npy int64 [n, 1] ([n, 2] with --ref_data_dir) in place of kth_S -- the uint32 pattern of the K-th
                distance (S where the exact-integer path ran); {pos,neg}_loss.npy float64 [n, 1]: the distance itself -- with K <= 32 column
                K - 1 of knn.py's {pos,neg}_knn_loss.npy, with --K 1 --pair_distance l2-lpips fbb.py's default pos_loss.npy -- or, with a
                reference set, 0.5 * (ln max(d_syn, 2^-149) - ln max(d_ref, 2^-149)) (attack.density_ratio_loss_f32); params.txt.
Files under ./density_attack/<exp_name>/:
    {pos,neg}_kth_S.npy int64 [n, 1]: the exact sum of squared differences to the K-th nearest sample ([n, 2] with --ref_data_dir: bank,
    reference set); params.txt;
    {pos,neg}_loss.npy float64 [n, 1]: without a reference set float64 of the float32 distance attack() reports for that S -- with --K 1
    fbb.py --distance l2's pos_loss.npy bit for bit, with K <= 32 column K - 1 of knn.py's {pos,neg}_knn_loss.npy; with a reference set
    0.5 * (ln max(S_syn, 1) - ln max(S_ref, 1)) (attack.density_ratio_loss), the log density ratio up to the constants d and
    ln(N_ref / N_syn), which do not change a ROC.  Small = member-like, so `eval_roc --attack_type fbb -ldir density_attack/<exp_name>`
    scores the attack.
"""
from __future__ import annotations

import argparse
import math
import os
import warnings

import numpy as np

from ..attack import _budget_bytes, density_ratio_loss, density_ratio_loss_f32, host_rows_kind, kth_distances, pair_kth_distances, prepare_queries
from .fbb import shard_devices, update_args  # noqa: F401  (update_args: the YAML overlay of the command line)
from .utils import check_folder, save_files


def parse_arguments(argv=None):
    parser = argparse.ArgumentParser()
    data_root = os.path.join(os.getcwd(), 'data', 'miniCelebA')
    parser.add_argument('--exp_name', '-name', type=str, default='debug', help='experiment name; results go to ./density_attack/<exp_name>')
    parser.add_argument('--syn_data_path', type=str, help='folder with the generated sample bank (image_*.png)')
    parser.add_argument('--pos_data_dir', type=str, default=os.path.join(data_root, 'train'), help='folder with the member (training) query images')
    parser.add_argument('--neg_data_dir', type=str, default=os.path.join(data_root, 'test'), help='folder with the non-member (held-out) query images')
    parser.add_argument('--ref_data_dir', type=str, default=None, help='optional reference set drawn from the population: the score becomes the log density ratio')
    parser.add_argument('--resolution', '-resolution', type=int, default=64, help='images that differ are resized to this square size')
    parser.add_argument('--BATCH_SIZE', type=int, default=30)
    parser.add_argument('--local_config', type=str, default=None)
    parser.add_argument('--ngpu', type=int, default=1, help='shard the bank over the first N GPUs (counts summed across them)')
    parser.add_argument('--devices', type=str, default=None, help='explicit device ordinals for the shards, e.g. 0,1,2,3 (overrides --ngpu)')
    parser.add_argument('--K', type=int, default=None, help='rank of the neighbour whose distance is the score (1..n_eff; default floor(sqrt(n_eff)))')
    parser.add_argument('--K_ref', type=int, default=None, help='the same for --ref_data_dir (default --K)')
    parser.add_argument('--distance', type=str, default='l2', help="l2 only (exact-integer L2)")
    parser.add_argument('--pair_distance', type=str, default=None, choices=['l2-lpips', 'l2'],
                        help="score on the float paths instead: 'l2-lpips' = 0.2 * LPIPS + L2 (the reference's fbb distance), or 'l2' with rows off both lattices")
    return parser.parse_args(argv)


def density_request(args):
    """(K or None, K_ref or None) from the command line or the YAML overlay; refused before any file is read"""
    distance = getattr(args, "distance", "l2")
    if distance == "l2-lpips":
        raise SystemExit("--distance l2-lpips is not built for the density attack: the K-th neighbour beyond 32 is found by a search over "
                         "exact integer distances, and 0.2 * LPIPS + L2 is a rounded float (knn.py gives its 32 nearest samples)")
    if distance != "l2":
        raise SystemExit("--distance must be l2, got %r" % (distance,))
    out = []
    for name in ("K", "K_ref"):
        v = getattr(args, name, None)
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 1):
            raise SystemExit("--%s must be an integer >= 1, got %r" % (name, v))
        out.append(None if v is None else int(v))
    if out[1] is not None and getattr(args, "ref_data_dir", None) is None:
        raise SystemExit("--K_ref needs --ref_data_dir")
    return tuple(out)


def pair_request(args):
    """None, 'l2-lpips' or 'l2' from --pair_distance; refused before any file is read"""
    pair = getattr(args, "pair_distance", None)
    if pair is None:
        return None
    if pair not in ("l2", "l2-lpips"):
        raise SystemExit("--pair_distance must be l2-lpips or l2, got %r" % (pair,))
    if getattr(args, "distance", "l2") != "l2":
        raise SystemExit("--pair_distance takes the place of --distance: give one of them (got --distance %r)" % (args.distance,))
    if pair == "l2-lpips":
        for name in ("syn_data_path", "pos_data_dir", "neg_data_dir", "ref_data_dir"):
            path = getattr(args, name, None)
            if isinstance(path, str) and path.endswith(".npy"):
                raise SystemExit("--pair_distance l2-lpips needs images: LPIPS is computed from VGG16 features of an image, and --%s %s is a 2-D "
                                 "table; a table takes --pair_distance l2" % (name, path))
    return pair


def _n_eff(rows, batch_size):
    return (len(rows) // int(batch_size)) * int(batch_size)


def _main_pair(args, pair, K, K_ref):
    """main() under --pair_distance: the K-th distance on the float paths (attack.pair_kth_distances)"""
    assert os.path.exists(args.syn_data_path)
    ref_dir = getattr(args, "ref_data_dir", None)
    if ref_dir is not None:
        assert os.path.exists(ref_dir)
    resolution = args.resolution
    from ..bank_io import concat_rows, load_rows
    syn_imgs = load_rows(args.syn_data_path, resolution)
    pos_query_imgs = load_rows(args.pos_data_dir, resolution)
    neg_query_imgs = load_rows(args.neg_data_dir, resolution)
    ref_imgs = load_rows(ref_dir, resolution) if ref_dir is not None else None
    both = concat_rows(pos_query_imgs, neg_query_imgs)
    n_pos = len(pos_query_imgs)
    if pair == "l2-lpips" and any(rows is not None and rows.ndim != 4 for rows in (syn_imgs, both, ref_imgs)):
        raise SystemExit("--pair_distance l2-lpips needs images (LPIPS is computed from VGG16 features); a 2-D table takes --pair_distance l2")
    for name, rows in (("--syn_data_path", syn_imgs), ("--ref_data_dir", ref_imgs)):
        if rows is not None and _n_eff(rows, args.BATCH_SIZE) == 0:
            raise SystemExit("%s holds no full batch of %d samples" % (name, args.BATCH_SIZE))
    n_syn = _n_eff(syn_imgs, args.BATCH_SIZE)
    if K is None:
        K = max(1, math.isqrt(n_syn))
    if K > n_syn:
        raise SystemExit("--K %d exceeds the %d samples of the bank that take part" % (K, n_syn))
    if ref_imgs is not None:
        K_ref = K if K_ref is None else K_ref
        if K_ref > _n_eff(ref_imgs, args.BATCH_SIZE):
            raise SystemExit("--K_ref %d exceeds the %d samples of the reference set that take part" % (K_ref, _n_eff(ref_imgs, args.BATCH_SIZE)))
    args.K, args.K_ref = K, K_ref
    save_dir = check_folder(os.path.join(os.getcwd(), 'density_attack', args.exp_name))
    lines = ["%s:%s" % (key, value) for key, value in vars(args).items()]
    with open(os.path.join(save_dir, 'params.txt'), 'w') as handle:
        handle.write("".join(line + "\n" for line in lines))
    print("\n".join(lines))

    jobs = [(syn_imgs, K)] + ([(ref_imgs, K_ref)] if ref_imgs is not None else [])
    fpath = "exact" if pair == "l2" else None
    results = []
    devices = shard_devices(args)
    if devices is not None:
        from ..shard import DeviceGroup
        with DeviceGroup(devices) as group:
            for rows, k in jobs:
                results.append(group.pair_kth_distances(both, bank=rows, k=k, batch_size=args.BATCH_SIZE, distance=pair, float_path=fpath))
    elif pair == "l2-lpips":
        from ..lpips import default_model
        model = default_model()
        # (float images stay raw: the search settles the row layout of both sides itself)
        queries = both if both.dtype != np.uint8 else prepare_queries(both, pair, lpips=model)
        for rows, k in jobs:
            bank, n_eff = rows, _n_eff(rows, args.BATCH_SIZE)
            if (getattr(queries, "kind", None) == "feat" and rows.dtype == np.uint8
                    and n_eff * queries.K * queries.V.dtype.itemsize <= _budget_bytes()):
                # every pass of the search is a pass over the bank: its feature rows are computed once when they fit the streaming budget
                bank = model.features(rows[:n_eff], role=model.search_role("bank"), fmt=queries.fmt)
            results.append(pair_kth_distances(queries, bank, k, distance=pair, batch_size=args.BATCH_SIZE, lpips=model))
    else:
        queries = prepare_queries(both, "l2")
        for rows, k in jobs:
            results.append(pair_kth_distances(queries, rows, k, distance="l2", batch_size=args.BATCH_SIZE, float_path=fpath))

    key = np.concatenate([r[1] for r in results], axis=1)                # [n, 1] or [n, 2]
    if ref_imgs is None:
        loss = results[0][0].astype(np.float64)                          # the distance itself
    else:
        loss = density_ratio_loss_f32(results[0][0][:, 0], results[1][0][:, 0]).reshape(-1, 1)
    save_files(save_dir, ['pos_kth_key', 'neg_kth_key'], [np.ascontiguousarray(key[:n_pos]), np.ascontiguousarray(key[n_pos:])])
    save_files(save_dir, ['pos_loss', 'neg_loss'], [np.ascontiguousarray(loss[:n_pos]), np.ascontiguousarray(loss[n_pos:])])
    return save_dir, loss[:n_pos], loss[n_pos:], key[:n_pos], key[n_pos:]


def main(args):
    pair = pair_request(args)
    K, K_ref = density_request(args)
    if pair is not None:
        return _main_pair(args, pair, K, K_ref)
    assert os.path.exists(args.syn_data_path)
    ref_dir = getattr(args, "ref_data_dir", None)
    if ref_dir is not None:
        assert os.path.exists(ref_dir)
    save_dir = check_folder(os.path.join(os.getcwd(), 'density_attack', args.exp_name))

    resolution = args.resolution
    from ..bank_io import concat_rows, load_rows
    syn_imgs = load_rows(args.syn_data_path, resolution)
    pos_query_imgs = load_rows(args.pos_data_dir, resolution)
    neg_query_imgs = load_rows(args.neg_data_dir, resolution)
    ref_imgs = load_rows(ref_dir, resolution) if ref_dir is not None else None
    both = concat_rows(pos_query_imgs, neg_query_imgs)
    n_pos = len(pos_query_imgs)

    # refused on the host, before any GPU work: both sides of every search on one lattice
    kq = host_rows_kind(both)
    for name, rows in (("--syn_data_path", syn_imgs), ("--ref_data_dir", ref_imgs)):
        if rows is None:
            continue
        n_eff = _n_eff(rows, args.BATCH_SIZE)
        if n_eff == 0:
            raise SystemExit("%s holds no full batch of %d samples" % (name, args.BATCH_SIZE))
        kb = host_rows_kind(rows[:n_eff])
        if kq == "f32" or kb != kq:
            raise SystemExit("the density attack needs 8-bit images or integer tables on both sides (the search runs on the exact integer "
                             "distance); got %r queries, %r rows in %s" % (kq, kb, name))
    n_syn = _n_eff(syn_imgs, args.BATCH_SIZE)
    if K is None:
        K = max(1, math.isqrt(n_syn))
    if K > n_syn:
        raise SystemExit("--K %d exceeds the %d samples of the bank that take part" % (K, n_syn))
    if ref_imgs is not None:
        K_ref = K if K_ref is None else K_ref
        if K_ref > _n_eff(ref_imgs, args.BATCH_SIZE):
            raise SystemExit("--K_ref %d exceeds the %d samples of the reference set that take part" % (K_ref, _n_eff(ref_imgs, args.BATCH_SIZE)))
    args.K, args.K_ref = K, K_ref
    lines = ["%s:%s" % (key, value) for key, value in vars(args).items()]
    with open(os.path.join(save_dir, 'params.txt'), 'w') as handle:
        handle.write("".join(line + "\n" for line in lines))
    print("\n".join(lines))

    jobs = [(syn_imgs, K)] + ([(ref_imgs, K_ref)] if ref_imgs is not None else [])
    results = []
    devices = shard_devices(args)
    if devices is not None:
        from ..shard import DeviceGroup
        with DeviceGroup(devices) as group:
            for rows, k in jobs:
                results.append(group.kth_distances(both, bank=rows, k=k, batch_size=args.BATCH_SIZE))
    else:
        # prepared only when the rows fit the streaming budget
        queries = prepare_queries(both, "l2")
        for rows, k in jobs:
            results.append(kth_distances(queries, rows, k, batch_size=args.BATCH_SIZE))

    S = np.concatenate([r[1] for r in results], axis=1)                  # [n, 1] or [n, 2]
    if ref_imgs is None:
        loss = results[0][0].astype(np.float64)                          # the distance itself: with --K 1 fbb.py's pos_loss.npy
    else:
        loss = density_ratio_loss(S[:, 0], S[:, 1]).reshape(-1, 1)
    save_files(save_dir, ['pos_kth_S', 'neg_kth_S'], [np.ascontiguousarray(S[:n_pos]), np.ascontiguousarray(S[n_pos:])])
    save_files(save_dir, ['pos_loss', 'neg_loss'], [np.ascontiguousarray(loss[:n_pos]), np.ascontiguousarray(loss[n_pos:])])
    return save_dir, loss[:n_pos], loss[n_pos:], S[:n_pos], S[n_pos:]


if __name__ == '__main__':
    import yaml
    cli = parse_arguments()
    if cli.local_config is None:
        warnings.warn("No config file was provided. Using default parameters.")
    else:
        with open(str(cli.local_config)) as handle:
            update_args(cli, yaml.safe_load(handle))
    main(cli)
