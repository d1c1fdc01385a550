#!/usr/bin/env python3
"""Timing of the VAEGAN encoder and of the reconstruction attack (ganleaks_amd.recon) next to one round of the partial-black-box search on the
same box.  ONE process on the shipped library, run it under the caller's `timeout`:
    python tools/bench_recon.py [--rounds 7] [--images 4096] [--queries 1000] [--samples 16] [--population 16]
VAEGAN (d = 64, z = 100) with synthetic weights, Generator.frozen(1); the queries are images of other latents.  Every variant is warmed up
once, then the variants ALTERNATE inside every round (median, smallest, largest), wall clock around a synchronised call:
  encode        Encoder.encode_device on `images` resident u8 images -> images_per_s
  recon_attack  recon_attack(queries, samples=16) end to end, host work included -> s_per_1000_queries
  pbb round     pbb_attack(rounds=1, population=16) from z_mu minus pbb_attack(rounds=0): one round of the search on the same queries
One JSON line per variant."""
import argparse
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
    ap.add_argument("--images", type=int, default=4096)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--population", type=int, default=16)
    args = ap.parse_args()
    import ganleaks_amd as gl
    from ganleaks_amd.gan_models.vaegan.train import Encoder, Generator
    if gl.device_count() < 1:
        raise SystemExit("bench_recon.py needs a GPU")
    ctx = gl.Context.get()
    nz = 100
    parent = Generator(nz, d=64)
    parent.load_state_dict(gl.synth.vaegan_state_dict(z_dim=nz, d=64))
    view = parent.frozen(1)
    enc = Encoder(nz)
    enc.load_state_dict(gl.synth.vaegan_encoder_state_dict(778, nz))
    n = max(args.images, args.queries)
    images = view.generate_u8(gl.synth.latent(2, n, nz).reshape(n, nz))
    bank = images.view((args.images, 3, 64, 64))
    queries = images.view((args.queries, 3, 64, 64))
    z_mu = gl.recon_attack(queries, enc, view, samples=0)[3]

    def wall(fn):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        return time.perf_counter() - t0

    variants = [("encode", lambda: enc.encode_device(bank)),
                ("recon_attack", lambda: gl.recon_attack(queries, enc, view, samples=args.samples)),
                ("pbb rounds=0", lambda: gl.pbb_attack(queries, view, z_mu, rounds=0, population=args.population)),
                ("pbb rounds=1", lambda: gl.pbb_attack(queries, view, z_mu, rounds=1, population=args.population))]
    for _, fn in variants:
        fn()
    s = {label: [] for label, _ in variants}
    for _ in range(args.rounds):
        for label, fn in variants:
            s[label].append(wall(fn))
    med = {k: float(np.median(v)) for k, v in s.items()}
    rows = [{"variant": "encode", "images": args.images, "median_s": med["encode"], "images_per_s": round(args.images / med["encode"], 1)},
            {"variant": "recon_attack", "queries": args.queries, "samples": args.samples, "median_s": med["recon_attack"],
             "s_per_1000_queries": round(med["recon_attack"] * 1000.0 / args.queries, 4)},
            {"variant": "pbb round", "queries": args.queries, "population": args.population, "median_s": med["pbb rounds=1"] - med["pbb rounds=0"],
             "s_per_1000_queries": round((med["pbb rounds=1"] - med["pbb rounds=0"]) * 1000.0 / args.queries, 4)}]
    for row, key in zip(rows, ("encode", "recon_attack", "pbb rounds=1")):
        row.update(min_s=round(min(s[key]), 5), max_s=round(max(s[key]), 5), rounds=args.rounds, median_s=round(row["median_s"], 5))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
