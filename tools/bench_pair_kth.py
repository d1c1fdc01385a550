#!/usr/bin/env python3
"""Timing of the counting kernels with thresholds PER QUERY on the float paths (gl_feat_count_rows_h1_scaled, gl_l2_count_rows_f32) next to
the count passes with thresholds shared by all queries (gl_feat_count_h1_scaled, gl_l2_count_f32), and of the exact k-th neighbour distance
built on them.  ONE process on the shipped library, rows resident:
    python tools/bench_pair_kth.py [--rounds 10] [--legs lpips,f32] [--queries 10000] [--bank 99968] [--res 64] [--k 316]
                                   [--f32_queries 10000] [--f32_bank 99968] [--f32_d 12288] [--out file.jsonl]
lpips leg (default shape: bench.py's `secondary` leg, BASELINE configs[2]): lattice search rows of 3 x 64 x 64 images made and featurised
on the device as tools/bench_count_lpips.py makes them.  f32 leg: N(0, 1) rows made on the device.
Timed (every variant warmed up once, then the variants ALTERNATE inside every round; median, smallest and largest reading):
  count T=16       gl_counts_init + the shared-threshold kernel with 16 radii spread evenly between the 0.40 and the 0.60 quantile of the
                   PAIR distances (hit-dense: about half of all pairs lie inside)                                                  (device events)
  rows same T=16   gl_counts_init + the per-query kernel, every row carrying the patterns of those same 16 radii: equal counts,
                   equal hit density                                                                                              (device events)
  rows first pass  (lpips) the first pass of the search: 15 thresholds spread evenly over the patterns and +inf itself             (device events)
  rows last pass   (lpips) the thresholds of the search's last pass for k: around every query's own k-th neighbour                 (device events)
  kth              (lpips) attack.pair_kth_distances(k) on the resident FeatureBanks, complete: 8 passes, host search, copies      (wall clock)
One JSON line per leg and variant; `x_count` is the ratio to the shared-threshold count pass of the same leg."""
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
    ap.add_argument("--k", type=int, default=316)
    ap.add_argument("--kth_rounds", type=int, default=3)
    ap.add_argument("--f32_queries", type=int, default=10000)
    ap.add_argument("--f32_bank", type=int, default=99968)
    ap.add_argument("--f32_d", type=int, default=12288)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import torch
    import ganleaks_amd as gl
    from ganleaks_amd import lpips as lp
    from ganleaks_amd import synth
    from ganleaks_amd._lib import check
    from ganleaks_amd.attack import eps_rows_to_bits, new_counts, pair_distance_quantiles, pair_kth_distances
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
        ms = ctypes.c_float()
        check(lib.gl_event_elapsed_ms(ev[0], ev[1], ctypes.byref(ms)))
        return ms.value

    def wall(fn):
        ctx.sync()
        t0 = time.perf_counter()
        out = fn()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3, out

    def report(leg, shape, times, extra, rounds):
        base = float(np.median(times["count T=16"]))
        for label, t in times.items():
            if not t:
                continue
            line = dict(shape, leg=leg, variant=label, median_ms=round(float(np.median(t)), 3), min_ms=round(min(t), 3), max_ms=round(max(t), 3),
                        x_count=round(float(np.median(t)) / base, 4), rounds=len(t), device=device, date=time.strftime("%Y-%m-%d"))
            line.update(extra.get(label, {}))
            text = json.dumps(line)
            print(text, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(text + "\n")

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
        counts = new_counts(ctx, Q, 16)
        lo_hi = pair_distance_quantiles(fq, fb, [0.40, 0.60], batch_size=1)[0]            # (two exact quantiles; the 16 radii lie evenly between them)
        radii = np.linspace(float(lo_hi[0]), float(lo_hi[1]), 16).astype(np.float32)

        # the thresholds the search itself uses: its first and its last pass for k, recorded from one run
        seen = []
        real = lp.feat_count_rows

        def recording(b, f, t, *a, **kw):
            seen.append(t.numpy().copy())
            return real(b, f, t, *a, **kw)

        lp.feat_count_rows = recording
        try:
            _, key_k, passes = pair_kth_distances(fq, fb, args.k, batch_size=1)
        finally:
            lp.feat_count_rows = real
        assert len(seen) == passes
        rows_thr = {"rows same T=16": ctx.to_device(np.repeat(eps_rows_to_bits(radii[None, :]), Q, axis=0)),
                    "rows first pass": ctx.to_device(seen[0]), "rows last pass": ctx.to_device(seen[-1])}

        def count_pass():
            check(lib.gl_counts_init(ctx.handle, p(counts.ptr), Q, 16))
            lp.feat_count(fb, fq, radii, counts=counts)

        def rows_pass(t_dev):
            def run():
                check(lib.gl_counts_init(ctx.handle, p(counts.ptr), Q, 16))
                lp.feat_count_rows(fb, fq, t_dev, counts=counts)
            return run

        def kth():
            _, key, n_pass = pair_kth_distances(fq, fb, args.k, batch_size=1)
            return key, n_pass

        event_variants = [("count T=16", count_pass)] + [(label, rows_pass(t)) for label, t in rows_thr.items()]
        extra, shared = {}, None
        for label, fn in event_variants:            # warm-up: code object load, first touch
            fn()
            ctx.sync()
            c = counts.numpy()[:Q].astype(np.int64)
            extra[label] = {"pairs_in_largest_ball": int(c[:, -1].sum())}
            if label == "count T=16":
                shared = c
            if label == "rows same T=16":
                assert np.array_equal(c, shared), "the same radii in every row give the counts of the shared-threshold kernel"
            if label == "rows first pass":
                assert np.all(c[:, -1] == N), "the first pass carries +inf: the total"
        times = {label: [] for label, _ in event_variants}
        times["kth"] = []
        for _ in range(args.rounds):
            for label, fn in event_variants:
                times[label].append(timed(fn))
        for _ in range(args.kth_rounds):
            ms, (key, n_pass) = wall(kth)
            assert np.array_equal(key, key_k)
            times["kth"].append(ms)
            extra["kth"] = {"passes": n_pass, "k": args.k}
        report("lpips", {"queries": Q, "bank": N, "res": res, "K1": K1, "rows": "lattice"}, times, extra, args.rounds)
        del fb, fq, counts, rows_thr, seen
        ctx.trim()
        torch.cuda.empty_cache()

    if "f32" in args.legs.split(","):
        Q, N, d = args.f32_queries, args.f32_bank, args.f32_d
        bank = torch.randn((N, d), dtype=torch.float32, device="cuda", generator=g)
        query = torch.randn((Q, d), dtype=torch.float32, device="cuda", generator=g)
        sample = ((query[:32, None, :] - bank[None, :512, :]) ** 2).mean(dim=2).reshape(-1).cpu().numpy()
        radii = np.linspace(np.quantile(sample, 0.40), np.quantile(sample, 0.60), 16).astype(np.float32)
        thr_dev = ctx.to_device(np.repeat(eps_rows_to_bits(radii[None, :]), Q, axis=0))
        torch.cuda.synchronize()
        counts = new_counts(ctx, Q, 16)

        def count_pass():
            check(lib.gl_counts_init(ctx.handle, p(counts.ptr), Q, 16))
            check(lib.gl_l2_count_f32(ctx.handle, p(bank.data_ptr()), N, p(query.data_ptr()), Q, d, radii.ctypes.data_as(p), 16, p(counts.ptr)))

        def rows_pass():
            check(lib.gl_counts_init(ctx.handle, p(counts.ptr), Q, 16))
            check(lib.gl_l2_count_rows_f32(ctx.handle, p(bank.data_ptr()), N, p(query.data_ptr()), Q, d, p(thr_dev.ptr), 16, p(counts.ptr)))

        variants = [("count T=16", count_pass), ("rows same T=16", rows_pass)]
        extra, shared = {}, None
        for label, fn in variants:
            fn()
            ctx.sync()
            c = counts.numpy()[:Q].astype(np.int64)
            extra[label] = {"pairs_in_largest_ball": int(c[:, -1].sum())}
            if shared is None:
                shared = c
            else:
                assert np.array_equal(c, shared), "the same radii in every row give the counts of the shared-threshold kernel"
        times = {label: [] for label, _ in variants}
        for _ in range(args.rounds):
            for label, fn in variants:
                times[label].append(timed(fn))
        report("f32", {"queries": Q, "bank": N, "d": d}, times, extra, args.rounds)


if __name__ == "__main__":
    main()
