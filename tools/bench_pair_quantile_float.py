#!/usr/bin/env python3
"""Timing of the pair-distance histogram on the two float paths and of the exact quantiles built on it, next to what a user had before: the
eps-ball count pass with 16 radii and a bisection on its counts.  ONE process on the shipped library, prepared rows resident:
    python tools/bench_pair_quantile_float.py [--rounds 7] [--paths lpips,f32] [--out profiles/...jsonl]
`lpips` (bench_count_lpips.py's shape and data: 10 000 queries x 99 968 bank rows of 3 x 64 x 64 images as lattice search rows, BASELINE
configs[2]): gl_feat_hist_h1_scaled against gl_feat_count_h1_scaled, the same main loop.
`f32` (8 192 x 262 144 rows of 1 071 floats, N(0, 1.5^2), half of the queries noisy bank rows): gl_l2_hist_f32 against gl_l2_count_f32.
Timed per path (every variant warmed up once, then the variants ALTERNATE inside every round; median, smallest and largest reading):
  hist level1      one first-level pass, gl_hist_init + the histogram over [0, 2^31) in 2048 bins of the top 11 bits              (device events)
  hist refined     one pass of the last level (shift 0, 512 bins) around the median: almost every workgroup leaves early          (device events)
  count T=16       gl_counts_init + the count with 16 radii at the 0.40 .. 0.60 quantiles of the PAIR distances                    (device events)
  quantiles        attack.pair_distance_quantiles([0.001, 0.5]) complete: passes, host radix-select, copies       (wall clock; lpips only)
  bisection        the same two radii by bisection on the counts over the bit patterns, 16 radii per pass          (wall clock; lpips only)
One JSON line per path and variant; `x_count` is the ratio to the count pass of the same path."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INF_BITS = 0x7F800000


def as_float(bits):
    return np.asarray(bits, np.int64).astype(np.uint32).view(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--paths", default="lpips,f32")
    ap.add_argument("--queries", type=int, default=None)
    ap.add_argument("--bank", type=int, default=None)
    ap.add_argument("--out", default=None, help="also append the lines to this JSONL file")
    args = ap.parse_args()
    import torch
    import ganleaks_amd as gl
    from ganleaks_amd import lpips as lp, synth
    from ganleaks_amd._lib import DeviceArray, check
    from ganleaks_amd.attack import Bank, count_balls_f32, new_counts, new_hist, pair_distance_quantiles, pair_histogram_f32, quantile_ranks, select_ranks
    ctx = gl.Context.get()
    lib = ctx.lib
    p = ctypes.c_void_p
    ev = [p(), p()]
    for e in ev:
        check(lib.gl_event_create(ctypes.byref(e)))
    device = {"device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
              "date": time.strftime("%Y-%m-%d")}

    def timed(fn):
        check(lib.gl_event_record(ctx.handle, ev[0]))
        fn()
        check(lib.gl_event_record(ctx.handle, ev[1]))
        ms = ctypes.c_float()
        check(lib.gl_event_elapsed_ms(ev[0], ev[1], ctypes.byref(ms)))
        return ms.value

    def wall(fn):
        ctx.sync()
        t0 = time.perf_counter()
        out = fn()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3, out

    g = torch.Generator(device="cuda").manual_seed(1)

    def lpips_rows(Q, N, res=64):
        lin = np.load(os.path.join(ROOT, "tests", "golden", "lpips_lin_v0.1.npz"))
        model = lp.LpipsModel(ctx).load_state_dicts(synth.vgg16_state_dict(7), {"lin%d" % i: lin["lin%d" % i] for i in range(5)})
        K1 = int(lib.gl_lpips_lattice_dim(res, res))
        K_lp, scale = K1 - 3 * res * res, float(lib.gl_lpips_lattice_scale(res, res))

        def prepare(n, role, like=None):
            cap = int(lib.gl_lpips_search_rows_capacity(n, K1))
            V, norms = ctx.empty((cap, K1), np.float16), ctx.empty((cap,), np.float32)
            keep = None
            for lo in range(0, n, 4096):
                hi = min(n, lo + 4096)
                img = torch.randint(0, 256, (hi - lo, 3, res, res), dtype=torch.uint8, device="cuda", generator=g)
                if like is not None and lo == 0:                       # perturbed copies of the first bank images
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
        return fb, fq

    def f32_rows(Q, N, d=1071):
        bank = torch.randn((N, d), device="cuda", generator=g) * 1.5
        q = torch.randn((Q, d), device="cuda", generator=g) * 1.5
        q[:Q // 2] = bank[:Q // 2] + 0.3 * torch.randn((Q // 2, d), device="cuda", generator=g)
        torch.cuda.synchronize()
        # (the library's view of the tensors' own memory: DeviceArray with an owner)
        out = [Bank(ctx, "f32", len(t), d, rows_f32=DeviceArray(ctx, tuple(t.shape), np.float32, ptr=t.data_ptr(), owner=t)) for t in (bank, q)]
        return out[0], out[1]

    lines = []
    for path in args.paths.split(","):
        if path == "lpips":
            Q, N = args.queries or 10000, args.bank or 99968
            bank, q = lpips_rows(Q, N)
            hist_fn = lambda lo, shift, n_bins, h: lp.feat_hist(bank, q, lo, shift, n_bins, hist=h)                                   # noqa: E731
            count_fn = lambda thr, c: lp.feat_count(bank, q, thr, counts=c)                                                         # noqa: E731
            shape = {"path": path, "queries": Q, "bank": N, "res": 64, "K1": bank.K, "rows": "lattice"}
        else:
            Q, N = args.queries or 8192, args.bank or 262144
            bank, q = f32_rows(Q, N)
            hist_fn = lambda lo, shift, n_bins, h: pair_histogram_f32(bank, q, lo, shift, n_bins, hist=h)                            # noqa: E731
            count_fn = lambda thr, c: count_balls_f32(bank, q, thr, counts=c)                                                       # noqa: E731
            shape = {"path": path, "queries": Q, "bank": N, "d": bank.d}
        hists = {n: new_hist(ctx, n) for n in (2048, 512)}
        counts = new_counts(ctx, Q, 16)

        def one_pass(lo, shift, n_bins):
            h = new_hist(ctx, n_bins)
            hist_fn(lo, shift, n_bins, h)
            return h.numpy().reshape(-1).astype(np.int64)

        # the radii of the count pass and the window of the refined pass come from the exact quantiles themselves
        pairs = Q * N
        keys16, _ = select_ranks(one_pass, quantile_ranks(np.linspace(0.40, 0.60, 16).tolist(), pairs), INF_BITS)
        thr = np.sort(as_float(keys16))
        med = int(select_ranks(one_pass, quantile_ranks([0.5], pairs), INF_BITS)[0][0])

        def hist_pass(lo, shift, n_bins):
            def run():
                check(lib.gl_hist_init(ctx.handle, p(hists[n_bins].ptr), n_bins))
                hist_fn(lo, shift, n_bins, hists[n_bins])
            return run

        def count_pass():
            check(lib.gl_counts_init(ctx.handle, p(counts.ptr), Q, 16))
            count_fn(thr, counts)

        targets = [0.001, 0.5]

        def quantiles():
            calls = []
            real = lp.feat_hist

            def counting(*a, **kw):
                calls.append(1)
                return real(*a, **kw)

            lp.feat_hist = counting
            try:
                _, key, _ = pair_distance_quantiles(q, bank, targets, batch_size=1)
            finally:
                lp.feat_hist = real
            return [int(v) for v in key], len(calls)

        def bisection():
            """per quantile: the smallest pattern with #{pairs <= it} >= rank + 1, 16 radii per pass inside the bracket (lo, hi]"""
            out, passes = [], 0
            for r in quantile_ranks(targets, pairs):
                lo, hi = -1, INF_BITS
                while hi - lo > 1:
                    t = np.unique(np.linspace(lo + 1, hi, 17)[:16].astype(np.int64) if hi - lo > 16 else np.arange(lo + 1, hi + 1, dtype=np.int64))
                    c = new_counts(ctx, Q, len(t))
                    count_fn(as_float(t), c)
                    c = c.numpy()[:Q].astype(np.int64).sum(axis=0)
                    passes += 1
                    ok = np.flatnonzero(c >= r + 1)
                    if len(ok):
                        hi = int(t[ok[0]])
                        lo = int(t[ok[0] - 1]) if ok[0] else lo
                    else:
                        lo = int(t[-1])
                out.append(hi)
            return out, passes

        event_variants = [("hist level1", hist_pass(0, 20, 2048)), ("hist refined", hist_pass(med >> 9 << 9, 0, 512)), ("count T=16", count_pass)]
        wall_variants = [("quantiles", quantiles), ("bisection", bisection)] if path == "lpips" else []
        extra = {}
        for label, fn in event_variants:            # warm-up: code object load, first touch
            fn()
            ctx.sync()
            if label.endswith("level1"):
                h = hists[2048].numpy().reshape(-1)
                assert int(h.sum()) == pairs, "the first-level window holds every pair"
                extra[label] = {"bins_in_use": int(np.count_nonzero(h)), "largest_bin_share": round(float(h.max()) / float(pairs), 4)}
            if label == "hist refined":
                extra[label] = {"pairs_in_window": int(hists[512].numpy().sum())}
            if label == "count T=16":
                extra[label] = {"pairs_in_largest_ball": int(counts.numpy()[:Q, -1].sum())}
        answers = {}
        for label, fn in wall_variants:
            _, (key, passes) = wall(fn)
            answers[label] = key
            extra[label] = {"passes": passes, "eps": [float(v) for v in as_float(key)]}
        if answers:
            assert answers["quantiles"] == answers["bisection"], answers
        times = {label: [] for label, _ in event_variants + wall_variants}
        for _ in range(args.rounds):
            for label, fn in event_variants:
                times[label].append(timed(fn))
            for label, fn in wall_variants:
                times[label].append(wall(fn)[0])
        base = float(np.median(times["count T=16"]))
        for label, _ in event_variants + wall_variants:
            t = times[label]
            line = dict(shape, variant=label, median_ms=round(float(np.median(t)), 3), min_ms=round(min(t), 3), max_ms=round(max(t), 3),
                        x_count=round(float(np.median(t)) / base, 3), rounds=args.rounds, **device)
            line.update(extra.get(label, {}))
            lines.append(line)
            print(json.dumps(line), flush=True)
        del bank, q, hists, counts
        ctx.trim()
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
