#!/usr/bin/env python3
"""Timing of the counting kernels with thresholds PER QUERY (gl_l2_count_rows_i8) and of the exact k-th neighbour distance built on them,
next to the count pass with thresholds shared by all queries (gl_l2_count_i8).  ONE process on the shipped library, prepared banks resident:
    python tools/bench_kth.py [--rounds 7] [--data spread] [--queries 10000] [--bank 99968] [--res 64] [--k 316]
Data, made on the device, as tools/bench_pair_quantile.py makes it: `spread` = every row has its own brightness and contrast, so the pair
distances spread as those of images do; `uniform` = every byte uniform-random.
Timed (every variant warmed up once, then the variants ALTERNATE inside every round; median, smallest and largest reading):
  count T=16       gl_counts_init + gl_l2_count_i8 with 16 thresholds at the 0.40 .. 0.60 quantiles of the PAIR distances      (device events)
  rows same T=16   gl_counts_init + gl_l2_count_rows_i8, every row carrying those same 16 thresholds                           (device events)
  rows first pass  the first pass of the search: 15 thresholds spread evenly over [0, 65025 d) and 65025 d itself -- hit-dense by
                   construction, every workgroup counts for every threshold                                                   (device events)
  rows last pass   the thresholds of the search's last pass for k: around every query's own k-th neighbour                     (device events)
  kth              attack.kth_distances(k) complete: passes, host search, copies                                              (wall clock)
One JSON line per data set and variant; `x_count` is the ratio to the shared-threshold count pass of the same data."""
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
    ap.add_argument("--data", default="spread")
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--bank", type=int, default=99968)
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--k", type=int, default=316)
    args = ap.parse_args()
    import importlib
    import torch
    import ganleaks_amd as gl
    from ganleaks_amd._lib import check
    from ganleaks_amd.attack import Bank, distance_quantiles, kth_distances, new_counts
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
    s_max = 65025 * d
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
        counts = new_counts(ctx, Q, 16)
        qs = np.linspace(0.40, 0.60, 16).tolist()
        thr = np.sort(distance_quantiles(q, bank, qs, batch_size=1)[1]).astype(np.int64)
        arr = (ctypes.c_int64 * 16)(*[int(v) for v in thr])

        # the thresholds the search itself uses: its first and its last pass for k, recorded from one run
        seen = []
        real = attack_mod.count_balls_rows

        def recording(b, f, t, *a, **kw):
            seen.append(t.numpy().copy())
            return real(b, f, t, *a, **kw)

        attack_mod.count_balls_rows = recording
        try:
            _, S_k, passes = kth_distances(q, bank, args.k, batch_size=1)
        finally:
            attack_mod.count_balls_rows = real
        assert len(seen) == passes
        rows_thr = {"rows same T=16": ctx.to_device(np.repeat(thr[None, :], Q, axis=0)), "rows first pass": ctx.to_device(seen[0]),
                    "rows last pass": ctx.to_device(seen[-1])}

        def count_pass():
            check(lib.gl_counts_init(ctx.handle, p(counts.ptr), Q, 16))
            check(lib.gl_l2_count_i8(ctx.handle, p(bank.rows_i8.ptr), p(bank.norms.ptr), N, p(q.rows_i8.ptr), p(q.norms.ptr), Q, d, ctypes.cast(arr, p),
                                     16, p(counts.ptr)))

        def rows_pass(t_dev):
            def run():
                check(lib.gl_counts_init(ctx.handle, p(counts.ptr), Q, 16))
                check(lib.gl_l2_count_rows_i8(ctx.handle, p(bank.rows_i8.ptr), p(bank.norms.ptr), N, p(q.rows_i8.ptr), p(q.norms.ptr), Q, d, p(t_dev.ptr),
                                              16, p(counts.ptr)))
            return run

        def kth():
            _, S, n_pass = kth_distances(q, bank, args.k, batch_size=1)
            return S, n_pass

        event_variants = [("count T=16", count_pass)] + [(label, rows_pass(t)) for label, t in rows_thr.items()]
        extra = {}
        shared = None
        for label, fn in event_variants:            # warm-up: code object load, first touch
            fn()
            ctx.sync()
            c = counts.numpy()[:Q].astype(np.int64)
            extra[label] = {"pairs_in_largest_ball": int(c[:, -1].sum())}
            if label == "count T=16":
                shared = c
            if label == "rows same T=16":
                assert np.array_equal(c, shared), "the same thresholds in every row give the counts of gl_l2_count_i8"
            if label == "rows first pass":
                assert np.all(c[:, -1] == N), "the first pass carries 65025 d: the total"
        _, (S, n_pass) = wall(kth)
        assert np.array_equal(S, S_k)
        extra["kth"] = {"passes": n_pass, "k": args.k, "S_median": int(np.median(S)), "pass_bound": attack_mod.kth_pass_bound(s_max)}
        times = {label: [] for label, _ in event_variants}
        times["kth"] = []
        for _ in range(args.rounds):
            for label, fn in event_variants:
                times[label].append(timed(fn))
            times["kth"].append(wall(kth)[0])
        base = float(np.median(times["count T=16"]))
        for label in times:
            t = times[label]
            line = {"data": kind, "queries": Q, "bank": N, "d": d, "variant": label, "median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3),
                    "max_ms": round(max(t), 3), "x_count": round(float(np.median(t)) / base, 3), "rounds": args.rounds}
            line.update(extra.get(label, {}))
            print(json.dumps(line), flush=True)
        del bank, q, counts, rows_thr
        ctx.trim()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
