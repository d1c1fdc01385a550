#!/usr/bin/env python3
"""Timing of the top-K search (gl_l2_topk_i8*: pairwise kernel that stores S, selection, list merge -- the whole call) next to the top-1
search (gl_l2_knn_i8*) on the same operands, in ONE process on the shipped library:
    python tools/bench_l2_topk.py [--rounds 10] [--shapes headline,big,wide] [--ks 1,2,5,16,32]
Shapes: headline = 10 000 queries x 99 968 rows of 3 x 64 x 64 (the 256 x 256 tile); big = 3 x 256 x 256 (64-bit totals) and wide =
3 x 512 x 512 (int64 norms), both 4 096 queries x 32 768 rows as in tools/bench_l2_wide.py.  Random operands are made on the device; every variant is warmed up once, then the variants ALTERNATE inside every round
and each launch is timed with device events (median over --rounds, with the smallest and largest reading).  One JSON line per shape and
variant; `x_top1` is the ratio to the top-1 median of the same shape -- a top-K search that needed k floor-filtered passes of the top-1
kernel would sit at x_top1 = k."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# name: (queries, bank rows, square image size)
SHAPES = {"headline": (10000, 99968, 64), "big": (4096, 32768, 256), "wide": (4096, 32768, 512)}      # big / wide: the shapes of tools/bench_l2_wide.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--shapes", default="headline,big,wide")
    ap.add_argument("--ks", default="1,2,5,16,32")
    args = ap.parse_args()
    import torch
    import ganleaks_amd as gl
    from ganleaks_amd._lib import check
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

    ks = [int(k) for k in args.ks.split(",")]
    g = torch.Generator(device="cuda").manual_seed(1)
    for name in args.shapes.split(","):
        Q, N, res = SHAPES[name]
        d = 3 * res * res
        wide = d > int(lib.gl_l2_max_d(0))
        stride = int(lib.gl_l2_row_stride(d))
        nt = torch.int64 if wide else torch.int32
        prepare = lib.gl_l2_prepare_wide if wide else lib.gl_l2_prepare
        knn = lib.gl_l2_knn_i8_wide if wide else lib.gl_l2_knn_i8
        topk = lib.gl_l2_topk_i8_wide if wide else lib.gl_l2_topk_i8
        rows = {}
        for side, count in (("bank", N), ("query", Q)):
            i8 = torch.empty((count, stride), dtype=torch.int8, device="cuda")
            nrm = torch.empty((count,), dtype=nt, device="cuda")
            step = max(1, min(count, (4 << 30) // d))
            for lo in range(0, count, step):
                hi = min(count, lo + step)
                u8 = torch.randint(0, 256, (hi - lo, d), dtype=torch.uint8, device="cuda", generator=g)
                torch.cuda.synchronize()
                check(prepare(ctx.handle, p(u8.data_ptr()), hi - lo, d, p(i8[lo].data_ptr()), p(nrm[lo].data_ptr())))
                ctx.sync()
                del u8
            rows[side] = (i8, nrm)
        (bank_i8, bank_n), (q_i8, q_n) = rows["bank"], rows["query"]
        keys = torch.empty((Q, max(ks)), dtype=torch.int64, device="cuda")

        def top1():
            check(lib.gl_keys_init(ctx.handle, p(keys.data_ptr()), Q))
            check(knn(ctx.handle, p(bank_i8.data_ptr()), p(bank_n.data_ptr()), N, 0, p(q_i8.data_ptr()), p(q_n.data_ptr()), Q, d, p(keys.data_ptr())))

        def topk_of(k):
            def run():
                check(lib.gl_topk_init(ctx.handle, p(keys.data_ptr()), Q, k))
                check(topk(ctx.handle, p(bank_i8.data_ptr()), p(bank_n.data_ptr()), N, 0, p(q_i8.data_ptr()), p(q_n.data_ptr()), Q, d, k,
                           p(keys.data_ptr())))
            return run

        variants = [("top1", top1)] + [("k=%d" % k, topk_of(k)) for k in ks]
        for _, fn in variants:                  # warm-up: code object load, first touch, the workspace enters the arena
            fn()
        ctx.sync()
        times = {label: [] for label, _ in variants}
        for _ in range(args.rounds):
            for label, fn in variants:
                times[label].append(timed(fn))
        base = float(np.median(times["top1"]))
        for label, _ in variants:
            t = times[label]
            print(json.dumps({"shape": name, "queries": Q, "bank": N, "d": d, "variant": label, "median_ms": round(float(np.median(t)), 3),
                              "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "x_top1": round(float(np.median(t)) / base, 3),
                              "rounds": args.rounds}), flush=True)
        del bank_i8, bank_n, q_i8, q_n, keys, rows
        ctx.trim()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
