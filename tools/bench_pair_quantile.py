#!/usr/bin/env python3
"""Timing of the pair-distance histogram (gl_l2_hist_i8: the int8 pair loop with the binning epilogue) and of the exact quantiles built
on it, next to what a user had before: the eps-ball count pass (gl_l2_count_i8, 16 thresholds) and a bisection on its counts.  ONE process
on the shipped library, prepared banks resident:
    python tools/bench_pair_quantile.py [--rounds 7] [--data spread,uniform] [--queries 10000] [--bank 99968] [--res 64]
Data, made on the device:  `uniform` = every byte uniform-random (tests/test_gpu_count.py::test_large_tile at this size): all pair
distances crowd into a narrow band of the first-level bins, the worst case for bin contention;  `spread` = every row has its own brightness
and contrast, u = clamp(m_i + s_i * noise): the pair distances spread over hundreds of bins, as those of images do.
Timed per data set (every variant warmed up once, then the variants ALTERNATE inside every round; median, smallest and largest reading):
  hist level1      one first-level histogram pass, gl_hist_init + gl_l2_hist_i8 over [0, 2^bitlen(65025 d)) in 2048 bins      (device events)
  hist refined     one pass of the last level (shift 0) around the median: almost every workgroup leaves early               (device events)
  count T=16       gl_counts_init + gl_l2_count_i8 with 16 thresholds at the 0.40 .. 0.60 quantiles of the PAIR distances, where its
                   sparse shortcut does not help                                                                             (device events)
  quantiles        attack.distance_quantiles([0.001, 0.5]) complete: passes, host radix-select, copies                        (wall clock)
  bisection        the same two S by bisection on count_balls, 16 thresholds per pass and quantile until S is pinned         (wall clock)
One JSON line per data set and variant; `x_count` is the ratio to the count pass of the same data.  Another build of the library (an epilogue
variant) is timed by a second run with $GANLEAKS_LIB set: both runs carry the count pass as their common reference."""
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--data", default="spread,uniform")
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--bank", type=int, default=99968)
    ap.add_argument("--res", type=int, default=64)
    args = ap.parse_args()
    import importlib
    import torch
    import ganleaks_amd as gl
    from ganleaks_amd._lib import check
    from ganleaks_amd.attack import Bank, count_balls, distance_quantiles, new_counts, new_hist, quantile_ranks
    attack_mod = importlib.import_module("ganleaks_amd.attack")
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

    def wall(fn):
        ctx.sync()
        t0 = time.perf_counter()
        out = fn()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3, out

    Q, N, d = args.queries, args.bank, 3 * args.res * args.res
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
        bits = int(65025 * d).bit_length()
        hist = new_hist(ctx, 2048)
        counts = new_counts(ctx, Q, 16)
        # the thresholds of the count pass and the window of the refined pass come from the exact quantiles themselves
        qs = np.linspace(0.40, 0.60, 16).tolist()
        _, S16, pairs = distance_quantiles(q, bank, qs, batch_size=1)
        thr = np.sort(S16).astype(np.int64)
        arr = (ctypes.c_int64 * 16)(*[int(v) for v in thr])
        med = int(distance_quantiles(q, bank, [0.5], batch_size=1)[1][0])

        def hist_pass(lo, shift):
            def run():
                check(lib.gl_hist_init(ctx.handle, p(hist.ptr), 2048))
                check(lib.gl_l2_hist_i8(ctx.handle, p(bank.rows_i8.ptr), p(bank.norms.ptr), N, p(q.rows_i8.ptr), p(q.norms.ptr), Q, d, lo, shift,
                                          2048, p(hist.ptr)))
            return run

        def count_pass():
            check(lib.gl_counts_init(ctx.handle, p(counts.ptr), Q, 16))
            check(lib.gl_l2_count_i8(ctx.handle, p(bank.rows_i8.ptr), p(bank.norms.ptr), N, p(q.rows_i8.ptr), p(q.norms.ptr), Q, d, ctypes.cast(arr, p),
                                     16, p(counts.ptr)))

        targets = [0.001, 0.5]

        def quantiles():
            calls = []
            real = attack_mod.pair_histogram

            def counting(*a, **kw):
                calls.append(1)
                return real(*a, **kw)

            attack_mod.pair_histogram = counting
            try:
                _, S, _ = distance_quantiles(q, bank, targets, batch_size=1)
            finally:
                attack_mod.pair_histogram = real
            return [int(v) for v in S], len(calls)

        def bisection():
            """per quantile: the smallest S with #{pairs <= S} >= rank + 1, 16 thresholds per pass inside the bracket (lo, hi]"""
            out, passes = [], 0
            for r in quantile_ranks(targets, pairs):
                lo, hi = -1, 65025 * d                       # the answer lies in (lo, hi]
                while hi - lo > 1:
                    t = np.unique(np.linspace(lo + 1, hi, 17)[:16].astype(np.int64) if hi - lo > 16 else np.arange(lo + 1, hi + 1, dtype=np.int64))
                    c = count_balls(bank, q, t)[0].numpy()[:Q].astype(np.int64).sum(axis=0)
                    passes += 1
                    ok = np.flatnonzero(c >= r + 1)
                    if len(ok):
                        hi = int(t[ok[0]])
                        lo = int(t[ok[0] - 1]) if ok[0] else lo
                    else:
                        lo = int(t[-1])
                out.append(hi)
            return out, passes

        event_variants = [("hist level1", hist_pass(0, bits - 11)), ("hist refined", hist_pass(max(med - 1024, 0), 0)), ("count T=16", count_pass)]
        wall_variants = [("quantiles", quantiles), ("bisection", bisection)]
        extra = {}
        for label, fn in event_variants:            # warm-up: code object load, first touch
            fn()
            ctx.sync()
            if label.endswith("level1"):
                h = hist.numpy().reshape(-1)
                assert int(h.sum()) == Q * N, "the first-level window holds every pair"
                extra[label] = {"bins_in_use": int(np.count_nonzero(h)), "largest_bin_share": round(float(h.max()) / float(Q * N), 4)}
            if label == "hist refined":
                extra[label] = {"pairs_in_window": int(hist.numpy().sum())}
            if label == "count T=16":
                extra[label] = {"pairs_in_largest_ball": int(counts.numpy()[:Q, -1].sum())}
        answers = {}
        for label, fn in wall_variants:
            _, (S, passes) = wall(fn)
            answers[label] = S
            extra[label] = {"passes": passes, "S": S}
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
            line = {"data": kind, "queries": Q, "bank": N, "d": d, "variant": label, "median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3),
                    "max_ms": round(max(t), 3), "x_count": round(float(np.median(t)) / base, 3), "rounds": args.rounds}
            line.update(extra.get(label, {}))
            print(json.dumps(line), flush=True)
        del bank, q, hist, counts
        ctx.trim()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
