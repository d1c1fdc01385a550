#!/usr/bin/env python3
"""Timing of the kernel-density pass (gl_l2_kde_rows_i8) next to the counting pass with thresholds per query (gl_l2_count_rows_i8) on the
same rows: the same K loops, another epilogue.  ONE process on the shipped library, prepared banks resident:
    python tools/bench_kde.py [--rounds 7] [--data spread] [--queries 10000] [--bank 99968] [--res 64] [--bandwidths 16]
Data, made on the device, as tools/bench_kth.py makes it (`spread` / `uniform`).  The bandwidths are a geometric ladder from 1/8 to 8 times
the median nearest-sample distance (the median heuristic); the counting pass gets, per query, the thresholds S0 + gl_kde_cut(coef[t]) - 1:
the very balls whose pairs the density pass weighs, so both epilogues enter their slow path for the same pairs.
Timed with device events, every variant warmed up once, then the variants ALTERNATE inside every round (median, smallest, largest):
  count rows      gl_counts_init + gl_l2_count_rows_i8 with those thresholds
  kde             gl_counts_init + gl_l2_kde_rows_i8 with the T coefficients
  kde T=1         the same with the median-heuristic bandwidth alone
One JSON line per data set and variant; `x_count_rows` is the ratio to the counting pass of the same data."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kde_cut(c):
    """gl_kde_cut (csrc/gl_kde_epi.h): the smallest delta with fl32(fl32(delta) c) >= 41, or 2^62 when there is none below it"""
    c = np.float32(c)
    lo, hi = 0, 1 << 62
    with np.errstate(over="ignore"):
        if np.float32(hi) * c < np.float32(41.0):
            return hi
        while hi - lo > 1:
            mid = lo + (hi - lo) // 2
            if np.float32(np.int64(mid)) * c < np.float32(41.0):
                lo = mid
            else:
                hi = mid
    return hi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--data", default="spread")
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--bank", type=int, default=99968)
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--bandwidths", type=int, default=16)
    args = ap.parse_args()
    import torch
    import ganleaks_amd as gl
    from ganleaks_amd._lib import check
    from ganleaks_amd.attack import Bank, kde_coef, kde_scores, new_counts
    ctx = gl.Context.get()
    lib = ctx.lib
    p = ctypes.c_void_p
    ev = [p(), p()]
    for e in ev:
        check(lib.gl_event_create(ctypes.byref(e)))

    def timed(fn):
        check(lib.gl_event_record(ctx.handle, ev[0]))
        fn()
        check(lib.gl_event_record(ctx.handle, ev[1]))
        ms = ctypes.c_float()
        check(lib.gl_event_elapsed_ms(ev[0], ev[1], ctypes.byref(ms)))
        return ms.value

    Q, N, d, T = args.queries, args.bank, 3 * args.res * args.res, args.bandwidths
    stride = int(lib.gl_l2_row_stride(d))
    g = torch.Generator(device="cuda").manual_seed(1)

    def make(n, kind):
        rows_i8, norms = ctx.empty((n, stride), np.int8), ctx.empty((n,), np.int32)
        step = max(1, min(n, (1 << 30) // d))
        for lo in range(0, n, step):
            hi = min(n, lo + step)
            if kind == "uniform":
                u8 = torch.randint(0, 256, (hi - lo, d), dtype=torch.uint8, device="cuda", generator=g)
            else:
                m = 40.0 + 175.0 * torch.rand((hi - lo, 1), device="cuda", generator=g)
                s = 5.0 + 55.0 * torch.rand((hi - lo, 1), device="cuda", generator=g)
                u8 = (m + s * torch.randn((hi - lo, d), device="cuda", generator=g)).clamp_(0, 255).to(torch.uint8)
            torch.cuda.synchronize()
            check(lib.gl_l2_prepare(ctx.handle, p(u8.data_ptr()), hi - lo, d, p(rows_i8.ptr + lo * stride), p(norms.ptr + lo * 4)))
            ctx.sync()
            del u8
        return Bank(ctx, "u8", n, d, rows_i8=rows_i8, norms=norms)

    for kind in args.data.split(","):
        bank, q = make(N, kind), make(Q, kind)
        unit = 65025.0 * d / 4.0
        _, _, S0 = kde_scores(q, bank, 1.0, batch_size=1)
        h_med = float(np.median(S0[S0 > 0])) / unit
        ladder = h_med * np.geomspace(1.0 / 8.0, 8.0, T) if T > 1 else np.asarray([h_med])
        coef = np.sort(kde_coef(ladder, d, "u8")[0])[::-1].copy()
        one = kde_coef([h_med], d, "u8")[0]
        thr = np.sort(S0[:, None] + np.asarray([kde_cut(c) for c in coef], np.int64)[None, :] - 1, axis=1)
        thr_dev, s0_dev = ctx.to_device(thr), ctx.to_device(S0)
        counts, sums, sums1 = new_counts(ctx, Q, T), new_counts(ctx, Q, T), new_counts(ctx, Q, 1)
        rows = (p(bank.rows_i8.ptr), p(bank.norms.ptr), N, p(q.rows_i8.ptr), p(q.norms.ptr), Q, d)

        def count_rows():
            check(lib.gl_counts_init(ctx.handle, p(counts.ptr), Q, T))
            check(lib.gl_l2_count_rows_i8(ctx.handle, *rows, p(thr_dev.ptr), T, p(counts.ptr)))

        def kde():
            check(lib.gl_counts_init(ctx.handle, p(sums.ptr), Q, T))
            check(lib.gl_l2_kde_rows_i8(ctx.handle, *rows, p(s0_dev.ptr), coef.ctypes.data_as(p), T, p(sums.ptr)))

        def kde_one():
            check(lib.gl_counts_init(ctx.handle, p(sums1.ptr), Q, 1))
            check(lib.gl_l2_kde_rows_i8(ctx.handle, *rows, p(s0_dev.ptr), one.ctypes.data_as(p), 1, p(sums1.ptr)))

        variants = [("count rows", count_rows), ("kde", kde), ("kde T=1", kde_one)]
        for _, fn in variants:                   # warm-up: code object load, first touch
            fn()
            ctx.sync()
        inside = int(counts.numpy()[:Q, -1].astype(np.int64).sum())
        W = sums.numpy()[:Q]
        assert np.all(W[:, 0] >= np.uint64(1 << 40)), "every query's nearest weighs 2^40"
        times = {label: [] for label, _ in variants}
        for _ in range(args.rounds):
            for label, fn in variants:
                times[label].append(timed(fn))
        base = float(np.median(times["count rows"]))
        for label in times:
            t = times[label]
            print(json.dumps({"data": kind, "queries": Q, "bank": N, "d": d, "T": 1 if label == "kde T=1" else T, "variant": label,
                              "median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3),
                              "x_count_rows": round(float(np.median(t)) / base, 3), "rounds": args.rounds, "pairs_in_largest_ball": inside,
                              "h_median": h_med}), flush=True)
        del bank, q, counts, sums, sums1, thr_dev, s0_dev
        ctx.trim()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
