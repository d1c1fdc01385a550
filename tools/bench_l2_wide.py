#!/usr/bin/env python3
"""Timing of the exact-L2 search beyond the int32-norm limit, in ONE process on the shipped library:
    python tools/bench_l2_wide.py [--queries 4096] [--bank 32768] [--rounds 5] [--res 256,512,1024]
3 x 256 x 256 runs on the existing 128-tile kernel with 64-bit totals (gl_l2_knn_i8 -> l2_knn_i8_kernel<true>), larger images on the wide
kernel (gl_l2_knn_i8_wide).  Random operands are made on the device; each case is warmed up once, then timed with device events over
--rounds launches (median).  One JSON line per case: ms, 2 Q N d / t in POP/s and its share of the 5 POP/s int8 dense peak; and one per
row-preparation kernel (gl_l2_prepare / gl_l2_prepare_wide) in TB/s of bytes read and written."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INT8_PEAK_POPS = 5.0        # dense int8 MFMA, 2x the fp16 rate (MI355X)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--bank", type=int, default=32768)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--res", default="256,512,1024", help="square image sizes, 3 channels each")
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

    def median_ms(fn):
        fn()                                    # warm-up: code object load, first-touch of the operands
        ctx.sync()
        return float(np.median([timed(fn) for _ in range(args.rounds)]))

    Q, N = args.queries, args.bank
    g = torch.Generator(device="cuda").manual_seed(1)
    for res in (int(r) for r in args.res.split(",")):
        d = 3 * res * res
        wide = d > int(lib.gl_l2_max_d(0))
        stride = int(lib.gl_l2_row_stride(d))
        nt = torch.int64 if wide else torch.int32
        prepare = lib.gl_l2_prepare_wide if wide else lib.gl_l2_prepare
        knn = lib.gl_l2_knn_i8_wide if wide else lib.gl_l2_knn_i8
        bank_i8 = torch.empty((N, stride), dtype=torch.int8, device="cuda")
        bank_n = torch.empty((N,), dtype=nt, device="cuda")
        q_i8 = torch.empty((Q, stride), dtype=torch.int8, device="cuda")
        q_n = torch.empty((Q,), dtype=nt, device="cuda")
        step = max(1, min(N, (8 << 30) // d))   # u8 rows made and prepared in slices of <= 8 GiB
        for lo in range(0, N, step):
            hi = min(N, lo + step)
            u8 = torch.randint(0, 256, (hi - lo, d), dtype=torch.uint8, device="cuda", generator=g)
            torch.cuda.synchronize()
            check(prepare(ctx.handle, p(u8.data_ptr()), hi - lo, d, p(bank_i8[lo].data_ptr()), p(bank_n[lo].data_ptr())))
            ctx.sync()
        u8 = torch.randint(0, 256, (Q, d), dtype=torch.uint8, device="cuda", generator=g)
        torch.cuda.synchronize()
        check(prepare(ctx.handle, p(u8.data_ptr()), Q, d, p(q_i8.data_ptr()), p(q_n.data_ptr())))
        ctx.sync()
        ms = median_ms(lambda: check(prepare(ctx.handle, p(u8.data_ptr()), Q, d, p(q_i8.data_ptr()), p(q_n.data_ptr()))))
        moved = Q * (d + stride + (8 if wide else 4))
        print(json.dumps({"kernel": "l2_prepare_wide" if wide else "l2_prepare", "res": res, "d": d, "rows": Q, "median_ms": round(ms, 4),
                          "TB/s": round(moved / (ms * 1e-3) / 1e12, 2), "rounds": args.rounds}), flush=True)
        del u8
        keys = torch.empty((Q,), dtype=torch.int64, device="cuda")

        def search():
            check(lib.gl_keys_init(ctx.handle, p(keys.data_ptr()), Q))
            check(knn(ctx.handle, p(bank_i8.data_ptr()), p(bank_n.data_ptr()), N, 0, p(q_i8.data_ptr()), p(q_n.data_ptr()), Q, d,
                      p(keys.data_ptr())))
        ms = median_ms(search)
        pops = 2.0 * Q * N * d / (ms * 1e-3) / 1e15
        print(json.dumps({"kernel": "l2_knn_i8_wide" if wide else "l2_knn_i8<BIG>", "res": res, "d": d, "queries": Q, "bank": N,
                          "median_ms": round(ms, 3), "POP/s": round(pops, 3), "share_of_int8_peak": round(pops / INT8_PEAK_POPS, 3),
                          "rounds": args.rounds}), flush=True)
        del bank_i8, bank_n, q_i8, q_n, keys
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
