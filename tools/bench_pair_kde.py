#!/usr/bin/env python3
"""Timing of the kernel-density (soft-min) sums on the float paths (gl_feat_kde_rows_h1_scaled, gl_l2_kde_rows_f32: the pair kernels with
EPI = 5) next to one counting pass with thresholds per query at the same T, shape and build (gl_feat_count_rows_h1_scaled,
gl_l2_count_rows_f32: EPI = 4, the same K loop with a cheaper epilogue -- the yardstick).  ONE process on the shipped library, rows resident:
    python tools/bench_pair_kde.py [--rounds 10] [--legs lpips,f32] [--queries 10000] [--bank 99968] [--res 64]
                                   [--f32_queries 10000] [--f32_bank 99968] [--f32_d 12288] [--quantile 0.5] [--out file.jsonl]
lpips leg (default shape: bench.py's `secondary` leg): lattice search rows of 3 x 64 x 64 images made and featurised on the device as
tools/bench_pair_kth.py makes them, half of the queries perturbed copies of bank images.  f32 leg: N(0, 1) rows made on the device, half of
the queries bank rows plus noise.
Per leg: one nearest-sample search for D0 (not timed), then for T = 1 and 16 coefficients, geometric from the one that puts x = 40 -- the
last weight that is not 0 -- at the --quantile of the pair distances above the median D0 (hit-dense: about that share of all pairs is
weighed under it) up to 64 times that.  Timed (every variant warmed up once, then the variants ALTERNATE inside every round; median,
smallest and largest reading, device events around the call):
  rows T           gl_counts_init + the per-query counting kernel, every query carrying the T radii D0 + 40 / coef[t]: the balls inside
                   which the kde kernel weighs, so both kernels see the same hit density
  kde T            gl_counts_init + the kde kernel (the call reads its flag back, which the events include)
One JSON line per leg, T and variant; `x_rows` is the ratio to the counting pass of the same leg and T."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--legs", default="lpips,f32")
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--bank", type=int, default=99968)
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--f32_queries", type=int, default=10000)
    ap.add_argument("--f32_bank", type=int, default=99968)
    ap.add_argument("--f32_d", type=int, default=12288)
    ap.add_argument("--quantile", type=float, default=0.5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import torch
    import ganleaks_amd as gl
    from ganleaks_amd import lpips as lp
    from ganleaks_amd import synth
    from ganleaks_amd._lib import DeviceArray, check
    from ganleaks_amd.attack import Bank, eps_rows_to_bits, kde_cut_bits_rows, kde_sums_f32, knn_keys, new_counts, pair_distance_quantiles
    ctx = gl.Context.get()
    lib = ctx.lib
    p = ctypes.c_void_p
    ev = [p(), p()]
    for e in ev:
        check(lib.gl_event_create(ctypes.byref(e)))
    device = torch.cuda.get_device_name(0)

    def timed(fn):
        check(lib.gl_event_record(ctx.handle, ev[0]))
        fn()
        check(lib.gl_event_record(ctx.handle, ev[1]))
        ctx.sync()
        ms = ctypes.c_float()
        check(lib.gl_event_elapsed_ms(ev[0], ev[1], ctypes.byref(ms)))
        return ms.value

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")

    def ladder(D0, q_pair, T):
        """T descending coefficients: the smallest puts x = 40 at q_pair - median(D0)"""
        span = max(float(q_pair) - float(np.median(D0)), 1e-30)
        lo = 40.0 / span
        return np.float32(np.geomspace(64.0 * lo, lo, T)) if T > 1 else np.float32([lo])

    def run_leg(leg, shape, Q, D0, q_pair, rows_call, kde_call):
        for T in (1, 16):
            coef = ladder(D0, q_pair, T)
            bound = kde_cut_bits_rows(D0, coef[-1])
            radii = D0[:, None].astype(np.float64) + 40.0 / coef[::-1].astype(np.float64)[None, :]          # ascending per query
            thr_dev, d0_dev, bound_dev = ctx.to_device(eps_rows_to_bits(radii)), ctx.to_device(D0), ctx.to_device(bound)
            out = new_counts(ctx, Q, T)

            def rows_pass():
                check(lib.gl_counts_init(ctx.handle, p(out.ptr), Q, T))
                rows_call(thr_dev, T, out)

            def kde_pass():
                check(lib.gl_counts_init(ctx.handle, p(out.ptr), Q, T))
                kde_call(d0_dev, bound_dev, coef, out)

            variants = [("rows T=%d" % T, rows_pass), ("kde T=%d" % T, kde_pass)]
            extra = {}
            for label, fn in variants:                   # warm-up: code object load, first touch
                fn()
                ctx.sync()
                c = out.numpy()[:Q]
                extra[label] = {"pairs_in_largest_ball": int(c[:, -1].astype(np.int64).sum())} if label.startswith("rows") else \
                               {"mean_weight_sum_smallest_coef": float(c[:, -1].astype(np.float64).mean() * 2.0 ** -40)}
            times = {label: [] for label, _ in variants}
            for _ in range(args.rounds):
                for label, fn in variants:
                    times[label].append(timed(fn))
            base = float(np.median(times["rows T=%d" % T]))
            for label, t in times.items():
                line = dict(shape, leg=leg, variant=label, T=T, median_ms=round(float(np.median(t)), 3), min_ms=round(min(t), 3), max_ms=round(max(t), 3),
                            x_rows=round(float(np.median(t)) / base, 4), rounds=len(t), device=device, date=time.strftime("%Y-%m-%d"))
                line.update(extra[label])
                emit(line)

    g = torch.Generator(device="cuda").manual_seed(1)

    if "lpips" in args.legs.split(","):
        Q, N, res = args.queries, args.bank, args.res
        lin = np.load(os.path.join(ROOT, "tests", "golden", "lpips_lin_v0.1.npz"))
        model = lp.LpipsModel(ctx).load_state_dicts(synth.vgg16_state_dict(7), {"lin%d" % i: lin["lin%d" % i] for i in range(5)})
        K1 = int(lib.gl_lpips_lattice_dim(res, res))
        K_lp = K1 - 3 * res * res
        scale = float(lib.gl_lpips_lattice_scale(res, res))
        step = 4096                                                  # images per featurisation pass

        def prepare(n, role, like=None):
            cap = int(lib.gl_lpips_search_rows_capacity(n, K1))
            V, norms = ctx.empty((cap, K1), np.float16), ctx.empty((cap,), np.float32)
            keep = None
            for lo in range(0, n, step):
                hi = min(n, lo + step)
                img = torch.randint(0, 256, (hi - lo, 3, res, res), dtype=torch.uint8, device="cuda", generator=g)
                if like is not None and lo == 0:                       # the first pass of the queries: perturbed copies of the first bank images
                    m = min(len(like), hi - lo)
                    noise = torch.randint(-12, 13, (m, 3, res, res), dtype=torch.int16, device="cuda", generator=g)
                    img[:m] = (like[:m].to(torch.int16) + noise).clamp_(0, 255).to(torch.uint8)
                if like is None and lo == 0:
                    keep = img.clone()
                torch.cuda.synchronize()
                part = lp.FeatureBank(ctx, V.view((hi - lo, K1), offset_bytes=lo * K1 * 2), norms.view((hi - lo,), offset_bytes=lo * 4), hi - lo, K1,
                                      K_lp, 0, role, "lattice", scale)
                model.features(img, role=role, fmt="lattice", out=part)
                ctx.sync()
            return lp.FeatureBank(ctx, V, norms, n, K1, K_lp, 0, role, "lattice", scale), keep

        fb, first = prepare(N, "bank")
        fq, _ = prepare(Q, "query", like=first[:Q // 2])
        del first
        torch.cuda.empty_cache()
        assert not fb.blocked or N <= 256, "K-blocked rows are prepared in whole blocks; use --res <= 80 here"
        D0 = (lp.feat_knn_keys(fb, fq).numpy()[:Q] >> np.uint64(32)).astype(np.uint32).view(np.float32)
        q_pair = pair_distance_quantiles(fq, fb, [args.quantile], batch_size=1)[0][0]
        run_leg("lpips", {"queries": Q, "bank": N, "res": res, "K1": K1, "rows": "lattice"}, Q, D0, q_pair,
                lambda thr, T, out: lp.feat_count_rows(fb, fq, thr, counts=out),
                lambda d0, bound, coef, out: lp.feat_kde_rows(fb, fq, d0, bound, coef, sums=out))
        del fb, fq
        ctx.trim()
        torch.cuda.empty_cache()

    if "f32" in args.legs.split(","):
        Q, N, d = args.f32_queries, args.f32_bank, args.f32_d
        bank = torch.randn((N, d), dtype=torch.float32, device="cuda", generator=g)
        query = torch.randn((Q, d), dtype=torch.float32, device="cuda", generator=g)
        m = min(Q // 2, N)
        query[:m] = bank[:m] + 0.05 * torch.randn((m, d), dtype=torch.float32, device="cuda", generator=g)
        sample = ((query[-32:, None, :] - bank[None, :512, :]) ** 2).mean(dim=2).reshape(-1).cpu().numpy()
        torch.cuda.synchronize()
        # (views of torch's memory: nothing is freed through them)
        b = Bank(ctx, "f32", N, d, rows_f32=DeviceArray(ctx, (N, d), np.float32, ptr=bank.data_ptr(), owner=bank))
        f = Bank(ctx, "f32", Q, d, rows_f32=DeviceArray(ctx, (Q, d), np.float32, ptr=query.data_ptr(), owner=query))
        D0 = (knn_keys(b, f, fpath="exact")[0].numpy()[:Q] >> np.uint64(32)).astype(np.uint32).view(np.float32)

        def rows_call(thr, T, out):
            check(lib.gl_l2_count_rows_f32(ctx.handle, p(bank.data_ptr()), N, p(query.data_ptr()), Q, d, p(thr.ptr), T, p(out.ptr)))

        run_leg("f32", {"queries": Q, "bank": N, "d": d}, Q, D0, float(np.quantile(sample, args.quantile)), rows_call,
                lambda d0, bound, coef, out: kde_sums_f32(b, f, d0, bound, coef, sums=out))


if __name__ == "__main__":
    main()
