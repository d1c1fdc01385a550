#!/usr/bin/env python3
"""Timing of the three reductions over the fixed-order float32 distance of off-lattice rows (csrc/gl_l2f32.hip), on the same operands, in ONE
process on the shipped library:
    python tools/bench_l2_f32_rows.py [--rounds 7] [--shapes tabular,pca] [--k 5] [--t 16]
  top1   gl_l2_knn_f32    (atomicMin epilogue; gl_keys_init inside the bracket)
  count  gl_l2_count_f32  (T radii spread evenly up to the 1 % quantile of the pair distances, estimated on a sample of pairs; gl_counts_init inside)
  topk   gl_l2_topk_f32   (pieces, selection and list merge: the whole call; gl_topk_init inside)
Shapes: tabular = 8 192 queries x 262 144 rows of 1 071 columns (DESIGN's tabular shape), pca = the same rows of 40 columns, where the
epilogue and the selection are expected to dominate.  Rows are N(0, 1), made on the device.  Every variant is warmed up once, then the
variants ALTERNATE inside every round and each call is timed with device events (median over --rounds, with the smallest and the largest
reading).  One JSON line per shape and variant; `x_top1` is the ratio to the top-1 median of the same shape."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# name: (queries, bank rows, columns)
SHAPES = {"tabular": (8192, 262144, 1071), "pca": (8192, 262144, 40)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default="tabular,pca")
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--t", type=int, default=16)
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

    g = torch.Generator(device="cuda").manual_seed(1)
    k, T = args.k, args.t
    for name in args.shapes.split(","):
        Q, N, d = SHAPES[name]
        bank = torch.randn((N, d), dtype=torch.float32, device="cuda", generator=g)
        query = torch.randn((Q, d), dtype=torch.float32, device="cuda", generator=g)
        sample = ((query[:64, None, :] - bank[None, :4096, :]) ** 2).mean(dim=2).reshape(-1).cpu().numpy()
        thr = np.asarray([np.quantile(sample, 0.01 * (t + 1) / T) for t in range(T)], np.float32)
        torch.cuda.synchronize()
        keys = torch.empty((Q,), dtype=torch.int64, device="cuda")
        lists = torch.empty((Q, k), dtype=torch.int64, device="cuda")
        counts = torch.empty((Q, T), dtype=torch.int64, device="cuda")

        def top1():
            check(lib.gl_keys_init(ctx.handle, p(keys.data_ptr()), Q))
            check(lib.gl_l2_knn_f32(ctx.handle, p(bank.data_ptr()), N, 0, p(query.data_ptr()), Q, d, p(keys.data_ptr())))

        def count():
            check(lib.gl_counts_init(ctx.handle, p(counts.data_ptr()), Q, T))
            check(lib.gl_l2_count_f32(ctx.handle, p(bank.data_ptr()), N, p(query.data_ptr()), Q, d, thr.ctypes.data_as(p), T, p(counts.data_ptr())))

        def topk():
            check(lib.gl_topk_init(ctx.handle, p(lists.data_ptr()), Q, k))
            check(lib.gl_l2_topk_f32(ctx.handle, p(bank.data_ptr()), N, 0, p(query.data_ptr()), Q, d, k, p(lists.data_ptr())))

        variants = [("top1", top1), ("count_T%d" % T, count), ("topk_k%d" % k, topk)]
        for _, fn in variants:
            fn()
        ctx.sync()
        # the three must agree with each other before their times mean anything
        assert torch.equal(lists[:, 0], keys), "column 0 of the lists is not the top-1 key"
        inside = float((counts[:, -1] > 0).float().mean())
        times = {n: [] for n, _ in variants}
        for _ in range(args.rounds):
            for n, fn in variants:
                times[n].append(timed(fn))
        base = float(np.median(times["top1"]))
        for n, _ in variants:
            t = np.asarray(times[n])
            print(json.dumps({"shape": name, "queries": Q, "rows": N, "d": d, "variant": n, "ms_median": round(float(np.median(t)), 3),
                              "ms_min": round(float(t.min()), 3), "ms_max": round(float(t.max()), 3), "x_top1": round(float(np.median(t)) / base, 3),
                              "rounds": args.rounds, "queries_with_a_hit": round(inside, 3)}), flush=True)
        del bank, query


if __name__ == "__main__":
    main()
