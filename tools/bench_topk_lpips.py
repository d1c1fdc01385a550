#!/usr/bin/env python3
"""Timing of the K nearest samples under 'l2-lpips' (gl_feat_topk_h1_scaled: the persistent search kernel with the piece-storing epilogue,
then the selection of the exact-integer top-k) next to the shipped top-1 search (gl_feat_knn_h1_scaled) on the same prepared rows, in ONE
process on the shipped library:
    timeout -k 10 900 python tools/bench_topk_lpips.py [--rounds 7] [--queries 10000] [--bank 99968] [--res 64] [--ks 1,5,32] [--out profiles/...json]
(a GPU step of its own: run it under a time limit sized to it, as above).
Default shape: bench.py's `secondary` leg (BASELINE configs[2]): 10 000 queries x 99 968 bank rows of 3 x 64 x 64 images as lattice search
rows (512 000 halves each, 102 GB + 10 GB).  Images are made on the device (uniform noise; half of the queries are perturbed bank images so
that the nearest distances spread), featurised ONCE with seeded synthetic VGG16 weights and the reference's lin weights.  Every variant is
warmed up once -- and column 0 of every list is then compared with the key of the top-1 search --, then the variants ALTERNATE inside
every round and each call is timed with device events (median over --rounds, with the smallest and largest reading).  One JSON line per
variant; `x_top1` is the ratio to the top-1 median of the same run; `pairs_ms` / `select_ms` are the library's own split of one profiled call
(GL_PROF_FEAT_COUNT, GL_PROF_TOPK_SELECT) taken after the timed rounds.
The yardstick: k = 5 at <= 1.10 x top-1 -- 4 GB of pieces written and read back, and the last round of every slice partly empty."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--bank", type=int, default=99968)
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--ks", default="1,5,32")
    ap.add_argument("--out", default=None, help="also write the lines as one JSON document to this file")
    args = ap.parse_args()
    import torch
    import ganleaks_amd as gl
    from ganleaks_amd import synth
    from ganleaks_amd._lib import check
    from ganleaks_amd.lpips import FeatureBank, LpipsModel, feat_knn_keys, feat_topk_keys
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

    Q, N, res = args.queries, args.bank, args.res
    lin = np.load(os.path.join(ROOT, "tests", "golden", "lpips_lin_v0.1.npz"))
    model = LpipsModel(ctx).load_state_dicts(synth.vgg16_state_dict(7), {"lin%d" % i: lin["lin%d" % i] for i in range(5)})
    K1 = int(lib.gl_lpips_lattice_dim(res, res))
    K_lp = K1 - 3 * res * res
    scale = float(lib.gl_lpips_lattice_scale(res, res))
    g = torch.Generator(device="cuda").manual_seed(1)
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
            part = FeatureBank(ctx, V.view((hi - lo, K1), offset_bytes=lo * K1 * 2), norms.view((hi - lo,), offset_bytes=lo * 4), hi - lo, K1, K_lp,
                               0, role, "lattice", scale)
            model.features(img, role=role, fmt="lattice", out=part)
            ctx.sync()
        return FeatureBank(ctx, V, norms, n, K1, K_lp, 0, role, "lattice", scale), keep

    fb, first = prepare(N, "bank")
    fq, _ = prepare(Q, "query", like=first[:Q // 2])
    del first
    torch.cuda.empty_cache()
    assert not fb.blocked or N <= 256, "K-blocked rows are prepared in whole blocks; use --res <= 80 here"

    keys = ctx.empty((Q,), np.uint64)

    def top1():
        check(lib.gl_keys_init(ctx.handle, p(keys.ptr), Q))
        feat_knn_keys(fb, fq, keys=keys)

    ks = [int(k) for k in args.ks.split(",")]
    lists = {k: ctx.empty((Q, k), np.uint64) for k in ks}

    def topk_of(k):
        def run():
            check(lib.gl_topk_init(ctx.handle, p(lists[k].ptr), Q, k))
            feat_topk_keys(fb, fq, k, keys=lists[k])
        return run

    variants = [("top1", top1)] + [("topk k=%d" % k, topk_of(k)) for k in ks]
    for label, fn in variants:              # warm-up: code object load, first touch, the workspace enters the arena
        fn()
        ctx.sync()
        if label.startswith("topk"):
            got = lists[int(label.split("=")[1])].numpy()
            assert np.array_equal(got[:, 0], keys.numpy()), "column 0 disagrees with the top-1 search"
            assert np.all(got[:, :-1] < got[:, 1:]), "lists are not strictly ascending"
    times = {label: [] for label, _ in variants}
    for _ in range(args.rounds):
        for label, fn in variants:
            times[label].append(timed(fn))
    base = float(np.median(times["top1"]))
    split = {}
    for label, fn in variants[1:]:          # one profiled call per k: the library's own tags
        ctx.prof_enable(True)
        ctx.prof_reset()
        fn()
        ctx.sync()
        prof = ctx.prof_read()
        split[label] = (prof["feat_count"][0], prof["topk_select"][0])
        ctx.prof_enable(False)
    lines = []
    for label, _ in variants:
        t = times[label]
        line = {"queries": Q, "bank": N, "res": res, "K1": K1, "rows": "lattice", "variant": label, "median_ms": round(float(np.median(t)), 3),
                "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "x_top1": round(float(np.median(t)) / base, 4), "rounds": args.rounds,
                "tflops": round(2.0 * Q * N * K1 / (float(np.median(t)) * 1e-3) / 1e12, 1)}
        if label in split:
            line["pairs_ms"], line["select_ms"] = round(split[label][0], 3), round(split[label][1], 3)
        lines.append(line)
        print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/bench_topk_lpips.py", "device": torch.cuda.get_device_name(0),
                       "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "lines": lines}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
