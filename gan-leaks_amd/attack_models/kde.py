"""[build] The soft-min (Gaussian-kernel density) membership attack on the data fbb.py reads.

GAN-Leaks derives its full-black-box score from a Parzen estimate of the generator's distribution, P(x|G) ~ 1/n sum_i phi(x, G(z_i)), and
keeps the largest term: the nearest sample (fbb.py:73-88).  This driver keeps every term under a Gaussian kernel: the score of a query is
the soft-min distance
    L_h(x) = -h ln( 1/n_eff sum_i exp(-D(x, g_i) / h) ),   D the L2 distance of Loss('l2') (attack_models/utils.py:161-164),
for 1..16 bandwidths h in one pass over the bank.  L_h -> the nearest-sample distance as h -> 0 (fbb.py's score) and the mean distance as
h -> inf; -L_h / h is the kernel log density up to constants.  The reference has no driver for it; the data flags, the YAML overlay and
the layout of the result directory are fbb.py's (attack_models/fbb.py:18-67), so that eval_roc.py scores the result unchanged.  The sums
come from ganleaks_amd.attack.kde_scores: the exact nearest-sample search, then one pass of the pair kernels with a fixed-point weight
epilogue; no pairwise value is stored, and the integer sums do not depend on chunking or sharding.

    python -m ganleaks_amd.attack_models.kde --syn_data_path ... --pos_data_dir ... --neg_data_dir ... [--bandwidth h1,h2,... | --bandwidth_quantile q]

--syn_data_path, --pos_data_dir, --neg_data_dir: a folder of PNG files (8-bit codes), or a file of floats (bank_io.load_rows): an .npz with
                img_r01 [N,H,W,C] in [0, 1], or a 2-D .npy table (medGAN's synthetic.npy)
--bandwidth     1..16 positive bandwidths in units of the distance, comma-separated; column t of the [n, T] files belongs to the t-th
--bandwidth_quantile  (default 0.5: the median heuristic mc.py uses for its radius) h = that quantile (method 'lower': an attained
                distance) of the pooled nearest-sample distances of all queries; one more search pass.  Refused when that distance is 0.
--distance      l2 only, on the exact-integer path.  l2-lpips is refused before any file is read; rows off both lattices (float images
                that are not 8-bit codes, continuous tables) are refused once the files show it, before any GPU work: the fixed-point sums
                run on the exact integer S, which such rows do not have.
--pair_distance {l2-lpips,l2}: (default absent; not together with a non-default --distance) the same attack on the float paths, through
                ganleaks_amd.attack.pair_kde_scores: the weights are fixed-point functions of the float32 distance minus the float32 nearest
                distance (one rounded subtraction, one rounded product), so the sums stay integers that do not depend on chunking or sharding.
                l2-lpips: 0.2 * LPIPS + L2, the distance fbb.main hard-wires (fbb.py:148, utils.py:166-176); weights from
                $GANLEAKS_VGG16_PATH / $GANLEAKS_LPIPS_LIN_PATH as in mc.py; images only (a 2-D table is refused: LPIPS needs images).
                l2: float_path='exact', so .npz / .npy float rows off both lattices work (rows on one lattice take the exact-integer path).
                --bandwidth_quantile takes its quantile from the nearest distances under that distance.  Two passes over the bank.
                Files: {pos,neg}_D0_key.npy int64 [n, 1] in place of S0 -- the uint32 pattern of the float32 nearest distance (S0 where the
                exact-integer path ran); the others as below.
Files under ./kde_attack/<exp_name>/:
    bandwidth.npy float64 [T]: the bandwidths as given (or found);
    {pos,neg}_kde_loss.npy float64 [n, T]: L_h per query and bandwidth; {pos,neg}_kde_W.npy uint64 [n, T]: the integer sums of weights in
    units of 2^-40; {pos,neg}_S0.npy int64 [n, 1]: the exact sum of squared differences to the nearest sample (loss, W, S0 as
    attack.kde_scores returns them); {pos,neg}_loss.npy float64 [n, 1]: column 0 of kde_loss.  Small = member-like, so
    `eval_roc --attack_type fbb -ldir kde_attack/<exp_name>` scores the attack; params.txt.
"""
from __future__ import annotations

import argparse
import os
import warnings

import numpy as np

from ..attack import GL_COUNT_MAX_T, _budget_bytes, attack, host_rows_kind, kde_scores, nearest_neighbours, pair_kde_scores, prepare_queries
from .fbb import shard_devices, update_args  # noqa: F401  (update_args: the YAML overlay of the command line)
from .utils import check_folder, save_files


def parse_arguments(argv=None):
    parser = argparse.ArgumentParser()
    data_root = os.path.join(os.getcwd(), 'data', 'miniCelebA')
    parser.add_argument('--exp_name', '-name', type=str, default='debug', help='experiment name; results go to ./kde_attack/<exp_name>')
    parser.add_argument('--syn_data_path', type=str, help='folder with the generated sample bank (image_*.png)')
    parser.add_argument('--pos_data_dir', type=str, default=os.path.join(data_root, 'train'), help='folder with the member (training) query images')
    parser.add_argument('--neg_data_dir', type=str, default=os.path.join(data_root, 'test'), help='folder with the non-member (held-out) query images')
    parser.add_argument('--resolution', '-resolution', type=int, default=64, help='images that differ are resized to this square size')
    parser.add_argument('--BATCH_SIZE', type=int, default=30)
    parser.add_argument('--local_config', type=str, default=None)
    parser.add_argument('--ngpu', type=int, default=1, help='shard the bank over the first N GPUs (sums added across them)')
    parser.add_argument('--devices', type=str, default=None, help='explicit device ordinals for the shards, e.g. 0,1,2,3 (overrides --ngpu)')
    parser.add_argument('--bandwidth', type=str, default=None, help='comma-separated bandwidths in units of the distance (1..16 positive values)')
    parser.add_argument('--bandwidth_quantile', type=str, default=None,
                        help='quantile of the pooled nearest-sample distances to use as the bandwidth (default 0.5, the median heuristic)')
    parser.add_argument('--distance', type=str, default='l2', help="l2 only (exact-integer L2)")
    parser.add_argument('--pair_distance', type=str, default=None, choices=['l2-lpips', 'l2'],
                        help="score on the float paths instead: 'l2-lpips' = 0.2 * LPIPS + L2 (the reference's fbb distance), or 'l2' with rows off both lattices")
    return parser.parse_args(argv)


def _floats(text, flag):
    try:
        if isinstance(text, (int, float)) and not isinstance(text, bool):
            return [float(text)]
        if isinstance(text, (list, tuple)):
            return [float(v) for v in text]
        return [float(v) for v in str(text).split(",") if v.strip() != ""]
    except (TypeError, ValueError):
        raise SystemExit("%s needs comma-separated numbers, got %r" % (flag, text)) from None


def kde_request(args):
    """('bandwidth', values) or ('quantile', [q]) from the command line or the YAML overlay; refused before any file is read"""
    distance = getattr(args, "distance", "l2")
    if distance == "l2-lpips":
        raise SystemExit("--distance l2-lpips is not built for the kernel-density attack: the weights are fixed-point functions of an exact "
                         "integer distance, and 0.2 * LPIPS + L2 is a rounded float (mc.py counts samples within a radius under it)")
    if distance != "l2":
        raise SystemExit("--distance must be l2, got %r" % (distance,))
    bw, qt = getattr(args, "bandwidth", None), getattr(args, "bandwidth_quantile", None)
    if bw is not None and qt is not None:
        raise SystemExit("--bandwidth and --bandwidth_quantile exclude each other")
    if bw is not None:
        values = _floats(bw, "--bandwidth")
        if not 1 <= len(values) <= GL_COUNT_MAX_T or not all(np.isfinite(v) and v > 0 for v in values):
            raise SystemExit("--bandwidth needs 1..%d positive finite values, got %r" % (GL_COUNT_MAX_T, values))
        return "bandwidth", values
    values = _floats("0.5" if qt is None else qt, "--bandwidth_quantile")
    if len(values) != 1 or not 0.0 <= values[0] <= 1.0:
        raise SystemExit("--bandwidth_quantile needs one value in [0, 1], got %r" % (values,))
    return "quantile", values


def pair_request(args):
    """None, 'l2-lpips' or 'l2' from --pair_distance; refused before any file is read (density.py's rule)"""
    pair = getattr(args, "pair_distance", None)
    if pair is None:
        return None
    if pair not in ("l2", "l2-lpips"):
        raise SystemExit("--pair_distance must be l2-lpips or l2, got %r" % (pair,))
    if getattr(args, "distance", "l2") != "l2":
        raise SystemExit("--pair_distance takes the place of --distance: give one of them (got --distance %r)" % (args.distance,))
    if pair == "l2-lpips":
        for name in ("syn_data_path", "pos_data_dir", "neg_data_dir"):
            path = getattr(args, name, None)
            if isinstance(path, str) and path.endswith(".npy"):
                raise SystemExit("--pair_distance l2-lpips needs images: LPIPS is computed from VGG16 features of an image, and --%s %s is a 2-D "
                                 "table; a table takes --pair_distance l2" % (name, path))
    return pair


def _main_pair(args, pair, mode, values):
    """main() under --pair_distance: the soft-min scores on the float paths (attack.pair_kde_scores)"""
    assert os.path.exists(args.syn_data_path)
    resolution = args.resolution
    from ..bank_io import concat_rows, load_rows
    syn_imgs = load_rows(args.syn_data_path, resolution)
    pos_query_imgs = load_rows(args.pos_data_dir, resolution)
    neg_query_imgs = load_rows(args.neg_data_dir, resolution)
    both = concat_rows(pos_query_imgs, neg_query_imgs)
    n_pos = len(pos_query_imgs)
    if pair == "l2-lpips" and any(rows.ndim != 4 for rows in (syn_imgs, both)):
        raise SystemExit("--pair_distance l2-lpips needs images (LPIPS is computed from VGG16 features); a 2-D table takes --pair_distance l2")
    n_eff = (len(syn_imgs) // int(args.BATCH_SIZE)) * int(args.BATCH_SIZE)
    if n_eff == 0:
        raise SystemExit("--syn_data_path holds no full batch of %d samples" % args.BATCH_SIZE)
    if n_eff >= 1 << 23:
        raise SystemExit("the kernel-density attack takes fewer than 2^23 samples (%d take part): the 64-bit sums of weights could overflow" % n_eff)
    save_dir = check_folder(os.path.join(os.getcwd(), 'kde_attack', args.exp_name))
    lines = ["%s:%s" % (key, value) for key, value in vars(args).items()]
    with open(os.path.join(save_dir, 'params.txt'), 'w') as handle:
        handle.write("".join(line + "\n" for line in lines))
    print("\n".join(lines))

    def bandwidths(top1):
        h = float(np.quantile(np.asarray(top1, np.float64).reshape(-1), values[0], method="lower"))
        if not (h > 0 and np.isfinite(h)):
            raise SystemExit("--bandwidth_quantile %g of the nearest-sample distances is %g: give --bandwidth" % (values[0], h))
        return [h]

    fpath = "exact" if pair == "l2" else None
    devices = shard_devices(args)
    if devices is not None:
        from ..shard import DeviceGroup
        with DeviceGroup(devices) as group:
            kw = dict(bank=syn_imgs, batch_size=args.BATCH_SIZE, distance=pair, float_path=fpath)
            h = values if mode == "bandwidth" else bandwidths(group.nearest_neighbours(both, k=1, **kw)[0])
            loss, W, key = group.pair_kde_scores(both, bandwidths=h, **kw)
    else:
        kw = dict(distance=pair, batch_size=args.BATCH_SIZE, float_path=fpath)
        queries, bank = both, syn_imgs
        if pair == "l2-lpips":
            from ..lpips import default_model
            model = kw["lpips"] = default_model()
            # (float images stay raw: the search settles the row layout of both sides itself)
            queries = both if both.dtype != np.uint8 else prepare_queries(both, pair, lpips=model)
            if (getattr(queries, "kind", None) == "feat" and syn_imgs.dtype == np.uint8
                    and n_eff * queries.K * queries.V.dtype.itemsize <= _budget_bytes()):
                # both passes (and the quantile's search) are passes over the bank: its feature rows are computed once when they fit
                bank = model.features(syn_imgs[:n_eff], role=model.search_role("bank"), fmt=queries.fmt)
        else:
            queries = prepare_queries(both, "l2")
        h = values if mode == "bandwidth" else bandwidths(nearest_neighbours(queries, bank, 1, **kw)[0])
        loss, W, key = pair_kde_scores(queries, bank, h, **kw)

    key = key.reshape(-1, 1)
    np.save(os.path.join(save_dir, 'bandwidth.npy'), np.asarray(h, np.float64))
    save_files(save_dir, ['pos_kde_loss', 'neg_kde_loss'], [np.ascontiguousarray(loss[:n_pos]), np.ascontiguousarray(loss[n_pos:])])
    save_files(save_dir, ['pos_kde_W', 'neg_kde_W'], [np.ascontiguousarray(W[:n_pos]), np.ascontiguousarray(W[n_pos:])])
    save_files(save_dir, ['pos_D0_key', 'neg_D0_key'], [np.ascontiguousarray(key[:n_pos]), np.ascontiguousarray(key[n_pos:])])
    save_files(save_dir, ['pos_loss', 'neg_loss'], [np.ascontiguousarray(loss[:n_pos, :1]), np.ascontiguousarray(loss[n_pos:, :1])])
    return save_dir, loss[:n_pos], loss[n_pos:], W, key


def main(args):
    pair = pair_request(args)
    mode, values = kde_request(args)
    if pair is not None:
        return _main_pair(args, pair, mode, values)
    assert os.path.exists(args.syn_data_path)
    save_dir = check_folder(os.path.join(os.getcwd(), 'kde_attack', args.exp_name))

    resolution = args.resolution
    from ..bank_io import concat_rows, load_rows
    syn_imgs = load_rows(args.syn_data_path, resolution)
    pos_query_imgs = load_rows(args.pos_data_dir, resolution)
    neg_query_imgs = load_rows(args.neg_data_dir, resolution)
    both = concat_rows(pos_query_imgs, neg_query_imgs)
    n_pos = len(pos_query_imgs)

    # refused on the host, before any GPU work: both sides on one lattice, fewer than 2^23 samples
    n_eff = (len(syn_imgs) // int(args.BATCH_SIZE)) * int(args.BATCH_SIZE)
    if n_eff == 0:
        raise SystemExit("--syn_data_path holds no full batch of %d samples" % args.BATCH_SIZE)
    if n_eff >= 1 << 23:
        raise SystemExit("the kernel-density attack takes fewer than 2^23 samples (%d take part): the 64-bit sums of weights could overflow" % n_eff)
    kq, kb = host_rows_kind(both), host_rows_kind(syn_imgs[:n_eff])
    if kq == "f32" or kb != kq:
        raise SystemExit("the kernel-density attack needs 8-bit images or integer tables on both sides (the weights are functions of the exact "
                         "integer distance); got %r queries, %r rows in --syn_data_path" % (kq, kb))
    lines = ["%s:%s" % (key, value) for key, value in vars(args).items()]
    with open(os.path.join(save_dir, 'params.txt'), 'w') as handle:
        handle.write("".join(line + "\n" for line in lines))
    print("\n".join(lines))

    def bandwidths(top1):
        h = float(np.quantile(top1.astype(np.float64), values[0], method="lower"))
        if not h > 0:
            raise SystemExit("--bandwidth_quantile %g of the nearest-sample distances is %g: give --bandwidth" % (values[0], h))
        return [h]

    devices = shard_devices(args)
    if devices is not None:
        from ..shard import DeviceGroup
        with DeviceGroup(devices) as group:
            h = values if mode == "bandwidth" else bandwidths(group.attack(both, bank=syn_imgs, distance="l2", batch_size=args.BATCH_SIZE)[0])
            loss, W, S0 = group.kde_scores(both, bank=syn_imgs, bandwidths=h, batch_size=args.BATCH_SIZE)
    else:
        queries = prepare_queries(both, "l2")
        h = values if mode == "bandwidth" else bandwidths(attack(queries, syn_imgs, distance="l2", batch_size=args.BATCH_SIZE)[0])
        loss, W, S0 = kde_scores(queries, syn_imgs, h, batch_size=args.BATCH_SIZE)

    S0 = S0.reshape(-1, 1)
    np.save(os.path.join(save_dir, 'bandwidth.npy'), np.asarray(h, np.float64))
    save_files(save_dir, ['pos_kde_loss', 'neg_kde_loss'], [np.ascontiguousarray(loss[:n_pos]), np.ascontiguousarray(loss[n_pos:])])
    save_files(save_dir, ['pos_kde_W', 'neg_kde_W'], [np.ascontiguousarray(W[:n_pos]), np.ascontiguousarray(W[n_pos:])])
    save_files(save_dir, ['pos_S0', 'neg_S0'], [np.ascontiguousarray(S0[:n_pos]), np.ascontiguousarray(S0[n_pos:])])
    save_files(save_dir, ['pos_loss', 'neg_loss'], [np.ascontiguousarray(loss[:n_pos, :1]), np.ascontiguousarray(loss[n_pos:, :1])])
    return save_dir, loss[:n_pos], loss[n_pos:], W, S0


if __name__ == '__main__':
    import yaml
    cli = parse_arguments()
    if cli.local_config is None:
        warnings.warn("No config file was provided. Using default parameters.")
    else:
        with open(str(cli.local_config)) as handle:
            update_args(cli, yaml.safe_load(handle))
    main(cli)
