#!/usr/bin/env python3
"""Timing of the eps-ball count (gl_l2_count_i8*: pairwise kernel with the counting epilogue -- the whole call) next to the top-1 search
(gl_l2_knn_i8*) and the top-K search at k = 2 (gl_l2_topk_i8*: pairwise kernel that stores S, selection, list merge) on the same
operands, in ONE process on the shipped library:
    python tools/bench_ball_counts.py [--rounds 10] [--shapes headline,big,wide] [--ts 1,8,16]
Shapes as tools/bench_l2_topk.py: headline = 10 000 queries x 99 968 rows of 3 x 64 x 64 (the 256 x 256 tile); big = 3 x 256 x 256 (64-bit
totals) and wide = 3 x 512 x 512 (int64 norms), both 4 096 queries x 32 768 rows.  Random operands are made on the device.  Thresholds:
`median` = T quantiles of the top-1 distances of this very search, spread evenly over [0.1, 0.9] with the median among them (T = 1: the
median heuristic itself), so about half of the queries have a sample inside the largest ball; `inf` = every pair inside every ball, every
counter of every tile non-zero: the worst case for the epilogue and for the atomic adds.  Every variant is warmed up once, then the variants
ALTERNATE inside every round and each call is timed with device events (median over --rounds, with the smallest and largest reading).  One JSON
line per shape and variant; `x_top1` is the ratio to the top-1 median of the same shape, `x_k2` the ratio to k = 2."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# name: (queries, bank rows, square image size)
SHAPES = {"headline": (10000, 99968, 64), "big": (4096, 32768, 256), "wide": (4096, 32768, 512)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--shapes", default="headline,big,wide")
    ap.add_argument("--ts", default="1,8,16")
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

    ts = [int(t) for t in args.ts.split(",")]
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
        count = lib.gl_l2_count_i8_wide if wide else lib.gl_l2_count_i8
        rows = {}
        for side, n in (("bank", N), ("query", Q)):
            i8 = torch.empty((n, stride), dtype=torch.int8, device="cuda")
            nrm = torch.empty((n,), dtype=nt, device="cuda")
            step = max(1, min(n, (4 << 30) // d))
            for lo in range(0, n, step):
                hi = min(n, lo + step)
                u8 = torch.randint(0, 256, (hi - lo, d), dtype=torch.uint8, device="cuda", generator=g)
                torch.cuda.synchronize()
                check(prepare(ctx.handle, p(u8.data_ptr()), hi - lo, d, p(i8[lo].data_ptr()), p(nrm[lo].data_ptr())))
                ctx.sync()
                del u8
            rows[side] = (i8, nrm)
        (bank_i8, bank_n), (q_i8, q_n) = rows["bank"], rows["query"]
        keys = torch.empty((Q, 2), dtype=torch.int64, device="cuda")
        counts = torch.empty((Q, max(ts)), dtype=torch.int64, device="cuda")

        def top1():
            check(lib.gl_keys_init(ctx.handle, p(keys.data_ptr()), Q))
            check(knn(ctx.handle, p(bank_i8.data_ptr()), p(bank_n.data_ptr()), N, 0, p(q_i8.data_ptr()), p(q_n.data_ptr()), Q, d, p(keys.data_ptr())))

        def k2():
            check(lib.gl_topk_init(ctx.handle, p(keys.data_ptr()), Q, 2))
            check(topk(ctx.handle, p(bank_i8.data_ptr()), p(bank_n.data_ptr()), N, 0, p(q_i8.data_ptr()), p(q_n.data_ptr()), Q, d, 2, p(keys.data_ptr())))

        # the thresholds of the median heuristic come from the top-1 search itself
        top1()
        ctx.sync()
        shift = min(32, 63 - int(65025 * d).bit_length())     # gl_l2_key_shift: keys are S << shift | index, below 2^63
        S1 = np.sort(keys.view(-1)[:Q].cpu().numpy().astype(np.uint64) >> np.uint64(shift)).astype(np.int64)

        def count_of(thr):
            arr = (ctypes.c_int64 * len(thr))(*[int(v) for v in thr])

            def run():
                check(lib.gl_counts_init(ctx.handle, p(counts.data_ptr()), Q, len(thr)))
                check(count(ctx.handle, p(bank_i8.data_ptr()), p(bank_n.data_ptr()), N, p(q_i8.data_ptr()), p(q_n.data_ptr()), Q, d,
                            ctypes.cast(arr, p), len(thr), p(counts.data_ptr())))
            return run

        variants = [("top1", top1), ("k=2", k2)]
        for T in ts:
            quantiles = [0.5] if T == 1 else sorted(set(np.linspace(0.1, 0.9, T - 1).tolist() + [0.5]))[:T]
            thr = sorted(int(S1[min(len(S1) - 1, int(v * len(S1)))]) for v in quantiles)
            while len(thr) < T:
                thr.append(thr[-1])
            variants.append(("count T=%d median" % T, count_of(thr)))
            variants.append(("count T=%d inf" % T, count_of([65025 * d] * T)))
        hits = {}
        for label, fn in variants:              # warm-up: code object load, first touch, the workspace enters the arena
            fn()
            ctx.sync()
            if label.startswith("count"):
                T = int(label.split("=")[1].split()[0])
                c = counts.view(-1)[:Q * T].view(Q, T).cpu().numpy()
                hits[label] = int(c[:, -1].sum())
                if label.endswith("inf"):
                    assert np.all(c == N), "eps = inf must count every row"
        times = {label: [] for label, _ in variants}
        for _ in range(args.rounds):
            for label, fn in variants:
                times[label].append(timed(fn))
        base, base2 = float(np.median(times["top1"])), float(np.median(times["k=2"]))
        for label, _ in variants:
            t = times[label]
            line = {"shape": name, "queries": Q, "bank": N, "d": d, "variant": label, "median_ms": round(float(np.median(t)), 3),
                    "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "x_top1": round(float(np.median(t)) / base, 3),
                    "x_k2": round(float(np.median(t)) / base2, 3), "rounds": args.rounds}
            if label in hits:
                line["pairs_in_largest_ball"] = hits[label]
            print(json.dumps(line), flush=True)
        del bank_i8, bank_n, q_i8, q_n, keys, counts, rows
        ctx.trim()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
