"""[build] The Monte-Carlo / eps-ball membership attack (Hilprecht et al., "Monte Carlo and Reconstruction Membership Inference Attacks
against Generative Models", PoPETs 2019 -- the `MC` baseline GAN-Leaks is compared with) on the data fbb.py reads.  The reference has
no such driver; the data flags, the YAML overlay and the layout of the result directory are fbb.py's (attack_models/fbb.py:18-67), so
that eval_roc.py scores the result unchanged.

Score of a query x:  f_eps(x) = #{ i < n_eff : dist(x, g_i) <= eps } / n_eff  over the sample bank g and a distance of the
full-black-box attack, n_eff = (N // BATCH_SIZE) * BATCH_SIZE (fbb.py:77).  All eps are counted in ONE pass over the bank
(ganleaks_amd.attack.ball_counts).

    python -m ganleaks_amd.attack_models.mc --syn_data_path ... --pos_data_dir ... --neg_data_dir ... [--eps e1,e2,... | --eps_quantile q1,q2,... | --eps_pair_quantile q1,q2,... | --eps_percentile q1,q2,...]
                                            [--distance {l2,l2-lpips}]

--syn_data_path, --pos_data_dir, --neg_data_dir: a folder of PNG files (8-bit codes), or a file of floats (bank_io.load_rows): an .npz with
                img_r01 [N,H,W,C] in [0, 1] (VAEGAN's generated.npz; must be --resolution sized), or a 2-D .npy table (medGAN's
                synthetic.npy, PCA-projected rows; --distance l2 only)
--distance      l2 (default): Loss('l2'), attack_models/utils.py:161-164, exact-integer L2 on the int8 matrix cores; rows off both lattices
                (float images, continuous tables) in the fixed-order float32 arithmetic of attack(float_path='exact').
                l2-lpips: 0.2 * LPIPS + L2, the distance fbb.main hard-wires (fbb.py:148, utils.py:166-176), counted by the l2-lpips search
                kernel with a counting epilogue; weights from $GANLEAKS_VGG16_PATH / $GANLEAKS_LPIPS_LIN_PATH as in fbb.py

--eps           the radii themselves (up to 16)
--eps_quantile  (default 0.5: Hilprecht's median heuristic) eps = that quantile (method 'lower': an attained distance) of the pooled
                positive + negative nearest-sample distances, which one attack() under the same distance over the same prepared rows gives
--eps_pair_quantile  Hilprecht's percentile heuristic: eps = that quantile (typically 0.001) of ALL query-sample distances d(x_i, g_j), exactly
                (ganleaks_amd.attack.distance_quantiles: an attained distance, rank floor(q * (pairs - 1))); --distance l2 on the exact-integer
                path only
--eps_percentile  the same percentile heuristic under either --distance and for every input the counting pass takes (float images and
                continuous tables in the fixed-order float32 arithmetic, l2-lpips on the distance the counting pass counts):
                ganleaks_amd.attack.pair_distance_quantiles, an attained distance of the counting pass at rank floor(q * (pairs - 1)).  Every
                level of its radix-select (3 per distinct bin, about 7 for two quantiles) is one more pass over the bank.  On 8-bit images
                or integer tables under --distance l2 it is --eps_pair_quantile
Files under ./mc_attack/<exp_name>/:
    eps.npy float32 [T]; {pos,neg}_count.npy int64 [n, T]; {pos,neg}_mc.npy float64 [n, T] = count / n_eff; params.txt;
    {pos,neg}_loss.npy float64 [n, 1] = -mc[:, 0], so `eval_roc --attack_type fbb -ldir mc_attack/<exp_name>` scores the first eps.
"""
from __future__ import annotations

import argparse
import os
import warnings

import numpy as np

from ..attack import GL_COUNT_MAX_T, Bank, _budget_bytes, attack, ball_counts, distance_quantiles, pair_distance_quantiles, prepare_queries
from .fbb import shard_devices, update_args  # noqa: F401  (update_args: the YAML overlay of the command line)
from .utils import check_folder, save_files


# options added after params.txt got its form: an unused one leaves the file as it was before the option existed
LATER_OPTIONS = ("eps_pair_quantile", "eps_percentile")


def parse_arguments(argv=None):
    parser = argparse.ArgumentParser()
    data_root = os.path.join(os.getcwd(), 'data', 'miniCelebA')
    parser.add_argument('--exp_name', '-name', type=str, default='debug', help='experiment name; results go to ./mc_attack/<exp_name>')
    parser.add_argument('--syn_data_path', type=str, help='folder with the generated sample bank (image_*.png)')
    parser.add_argument('--pos_data_dir', type=str, default=os.path.join(data_root, 'train'), help='folder with the member (training) query images')
    parser.add_argument('--neg_data_dir', type=str, default=os.path.join(data_root, 'test'), help='folder with the non-member (held-out) query images')
    parser.add_argument('--resolution', '-resolution', type=int, default=64, help='images that differ are resized to this square size')
    parser.add_argument('--BATCH_SIZE', type=int, default=30)
    parser.add_argument('--local_config', type=str, default=None)
    parser.add_argument('--ngpu', type=int, default=1, help='shard the bank over the first N GPUs (counts summed across them)')
    parser.add_argument('--devices', type=str, default=None, help='explicit device ordinals for the shards, e.g. 0,1,2,3 (overrides --ngpu)')
    parser.add_argument('--eps', type=str, default=None, help='comma-separated radii (1..%d values); write a leading negative radius as --eps=-1,...' % GL_COUNT_MAX_T)
    parser.add_argument('--distance', type=str, default='l2', choices=['l2', 'l2-lpips'],
                        help="distance the balls are measured in: 'l2', or 'l2-lpips' = 0.2 * LPIPS + L2 (the reference's fbb distance)")
    parser.add_argument('--eps_quantile', type=str, default=None,
                        help='comma-separated quantiles of the pooled nearest-sample distances to use as radii (default 0.5, the median heuristic)')
    parser.add_argument('--eps_pair_quantile', type=str, default=None,
                        help='comma-separated quantiles of ALL query-sample distances to use as radii (the percentile heuristic; try 0.001); '
                             '--distance l2 only')
    parser.add_argument('--eps_percentile', type=str, default=None,
                        help='comma-separated quantiles of ALL query-sample distances to use as radii (the percentile heuristic; try 0.001) '
                             'under either --distance and for float inputs too; every level of the selection is one more pass over the bank')
    return parser.parse_args(argv)


def _floats(text, what):
    if isinstance(text, (int, float)):
        return [float(text)]
    if isinstance(text, (list, tuple)):
        return [float(v) for v in text]
    try:
        values = [float(v) for v in str(text).replace(",", " ").split()]
    except ValueError:
        raise SystemExit("%s must be comma-separated numbers, got %r" % (what, text)) from None
    return values


def radii_request(args):
    """('eps', values), ('quantile', values), ('pair_quantile', values) or ('percentile', values) from the command line; refused before any
    file is read"""
    percentile = getattr(args, "eps_percentile", None)
    if percentile is not None:
        if any(getattr(args, other, None) is not None for other in ("eps", "eps_quantile", "eps_pair_quantile")):
            raise SystemExit("--eps, --eps_quantile, --eps_pair_quantile and --eps_percentile exclude each other")
        values = _floats(percentile, "--eps_percentile")
        if any(not 0.0 <= v <= 1.0 for v in values):     # (NaN fails both comparisons)
            raise SystemExit("--eps_percentile needs values in [0, 1], got %r" % (values,))
        if not 1 <= len(values) <= GL_COUNT_MAX_T:
            raise SystemExit("1..%d radii per run, got %d" % (GL_COUNT_MAX_T, len(values)))
        return "percentile", values
    pair = getattr(args, "eps_pair_quantile", None)
    if pair is not None:
        if getattr(args, "eps", None) is not None or getattr(args, "eps_quantile", None) is not None:
            raise SystemExit("--eps, --eps_quantile and --eps_pair_quantile exclude each other")
        if getattr(args, "distance", "l2") != "l2":
            raise SystemExit("--eps_pair_quantile is built for --distance l2 (exact-integer L2), not %r" % (getattr(args, "distance", None),))
        values = _floats(pair, "--eps_pair_quantile")
        if any(not 0.0 <= v <= 1.0 for v in values):     # (NaN fails both comparisons)
            raise SystemExit("--eps_pair_quantile needs values in [0, 1], got %r" % (values,))
        if not 1 <= len(values) <= GL_COUNT_MAX_T:
            raise SystemExit("1..%d radii per run, got %d" % (GL_COUNT_MAX_T, len(values)))
        return "pair_quantile", values
    if getattr(args, "eps", None) is not None and getattr(args, "eps_quantile", None) is not None:
        raise SystemExit("--eps and --eps_quantile exclude each other")
    if getattr(args, "eps", None) is not None:
        mode, values = "eps", _floats(args.eps, "--eps")
        if any(np.isnan(v) for v in values):
            raise SystemExit("--eps holds NaN")
    else:
        mode, values = "quantile", _floats(args.eps_quantile if getattr(args, "eps_quantile", None) is not None else "0.5", "--eps_quantile")
        if any(not 0.0 <= v <= 1.0 for v in values):
            raise SystemExit("--eps_quantile needs values in [0, 1], got %r" % (values,))
    if not 1 <= len(values) <= GL_COUNT_MAX_T:
        raise SystemExit("1..%d radii per run, got %d" % (GL_COUNT_MAX_T, len(values)))
    return mode, values


def main(args):
    mode, values = radii_request(args)
    distance = getattr(args, "distance", "l2")
    if distance not in ("l2", "l2-lpips"):
        raise SystemExit("--distance must be l2 or l2-lpips, got %r" % (distance,))
    assert os.path.exists(args.syn_data_path)
    save_dir = check_folder(os.path.join(os.getcwd(), 'mc_attack', args.exp_name))
    lines = ["%s:%s" % (key, value) for key, value in vars(args).items() if not (key in LATER_OPTIONS and value is None)]
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
    floats = syn_imgs.dtype != np.uint8 or both.dtype != np.uint8
    n_eff = (len(syn_imgs) // args.BATCH_SIZE) * args.BATCH_SIZE
    if n_eff == 0:
        raise ValueError("bank holds no full batch of %d samples (attack_models/fbb.py:77-83)" % args.BATCH_SIZE)

    devices = shard_devices(args)
    group = None
    if devices is not None:
        from ..shard import DeviceGroup
        group = DeviceGroup(devices)                 # every context prepares the (replicated) queries once, for both passes
    try:
        if distance == "l2-lpips":
            from ..lpips import default_model
            if group is None:                        # (a group builds one model per context from the same local files)
                model = default_model()
                # (float images stay raw: the search settles the row layout of both sides itself)
                queries = both if floats else prepare_queries(both, distance, lpips=model)
                bank = syn_imgs
                if getattr(queries, "kind", None) == "feat" and n_eff * queries.K * queries.V.dtype.itemsize <= _budget_bytes():
                    # the bank's feature rows are computed once for both passes when they fit the streaming budget
                    bank = model.features(syn_imgs[:n_eff], role=model.search_role("bank"), fmt=queries.fmt)
                nearest = lambda: attack(queries, bank, distance=distance, batch_size=args.BATCH_SIZE, lpips=model)[0]                # noqa: E731
                count = lambda eps: ball_counts(queries, bank, eps, batch_size=args.BATCH_SIZE, distance=distance, lpips=model)        # noqa: E731
                percentiles = lambda: pair_distance_quantiles(queries, bank, values, distance=distance, batch_size=args.BATCH_SIZE, lpips=model)[0]   # noqa: E731
            else:
                nearest = lambda: group.attack(both, bank=syn_imgs, distance=distance, batch_size=args.BATCH_SIZE)[0]            # noqa: E731
                count = lambda eps: group.ball_counts(both, bank=syn_imgs, eps=eps, batch_size=args.BATCH_SIZE, distance=distance)  # noqa: E731
                percentiles = lambda: group.pair_distance_quantiles(both, bank=syn_imgs, quantiles=values, batch_size=args.BATCH_SIZE,   # noqa: E731
                                                                    distance=distance)[0]
        elif group is None:
            queries = prepare_queries(both, "l2")
            d = int(np.prod(syn_imgs.shape[1:], dtype=np.int64))
            # the bank's int8 rows are prepared once for both passes when they fit the streaming budget; otherwise both stream the images
            # (fp32 rows take 4 bytes per value; 8-bit codes are kept next to the int8 rows when float queries will need them decoded)
            row_bytes = (2 if syn_imgs.dtype == np.uint8 else 4) * d
            bank = (Bank.from_images(syn_imgs[:n_eff], queries.ctx, norms64=queries.wide, keep_u8=queries.kind == "f32")
                    if row_bytes * n_eff <= _budget_bytes() else syn_imgs)
            # float_path='exact' spelt out: the radius read from the nearest distances must be an attained D32 of the counting pass
            nearest = lambda: attack(queries, bank, distance="l2", batch_size=args.BATCH_SIZE, float_path="exact")[0]   # noqa: E731
            count = lambda eps: ball_counts(queries, bank, eps, batch_size=args.BATCH_SIZE, float_path="exact")         # noqa: E731
            pair_quantiles = lambda: distance_quantiles(queries, bank, values, batch_size=args.BATCH_SIZE)[0]           # noqa: E731
            percentiles = lambda: pair_distance_quantiles(queries, bank, values, distance="l2", batch_size=args.BATCH_SIZE,   # noqa: E731
                                                          float_path="exact")[0]
        else:
            nearest = lambda: group.attack(both, bank=syn_imgs, distance="l2", batch_size=args.BATCH_SIZE)[0]      # noqa: E731
            count = lambda eps: group.ball_counts(both, bank=syn_imgs, eps=eps, batch_size=args.BATCH_SIZE, float_path="exact")   # noqa: E731
            pair_quantiles = lambda: group.distance_quantiles(both, bank=syn_imgs, quantiles=values, batch_size=args.BATCH_SIZE)[0]   # noqa: E731
            percentiles = lambda: group.pair_distance_quantiles(both, bank=syn_imgs, quantiles=values, batch_size=args.BATCH_SIZE,   # noqa: E731
                                                                distance="l2", float_path="exact")[0]
        if mode == "eps":
            with np.errstate(over="ignore"):
                eps = np.asarray(values, np.float64).astype(np.float32)
        elif mode == "pair_quantile":
            eps = np.asarray(pair_quantiles(), np.float32)
        elif mode == "percentile":
            eps = np.asarray(percentiles(), np.float32)
        else:
            top1 = np.asarray(nearest(), np.float32)
            eps = np.asarray([np.quantile(top1, v, method="lower") for v in values], np.float32)
        counts = count(eps)
    finally:
        if group is not None:
            group.close()

    mc = counts.astype(np.float64) / float(n_eff)
    save_files(save_dir, ['eps'], [eps])
    save_files(save_dir, ['pos_count', 'neg_count'], [np.ascontiguousarray(counts[:n_pos]), np.ascontiguousarray(counts[n_pos:])])
    save_files(save_dir, ['pos_mc', 'neg_mc'], [np.ascontiguousarray(mc[:n_pos]), np.ascontiguousarray(mc[n_pos:])])
    # eval_roc negates the losses it loads (eval_roc.py:78): a larger score must mean "member"
    save_files(save_dir, ['pos_loss', 'neg_loss'], [np.ascontiguousarray(-mc[:n_pos, :1]), np.ascontiguousarray(-mc[n_pos:, :1])])
    print('eps: ', eps.tolist())
    return save_dir, eps, counts[:n_pos], counts[n_pos:]


if __name__ == '__main__':
    import yaml
    cli = parse_arguments()
    if cli.local_config is None:
        warnings.warn("No config file was provided. Using default parameters.")
    else:
        with open(str(cli.local_config)) as handle:
            update_args(cli, yaml.safe_load(handle))
    main(cli)
