#!/usr/bin/env python3
"""Powell's method against the evolution strategy in the partial-black-box attack, at the nearest equal budget and from the same start.  ONE
process on the shipped library, run it under the caller's `timeout`:
    python tools/bench_pbb_powell.py [--queries 256] [--ngf 64] [--sweeps 2] [--ladder 8] [--rounds 25] [--population 64] [--repeat 3]
                                     [--only {both,powell,es}]
DCGAN-64 with synthetic weights; a bank of `queries` latents; half the queries are images of latents 0.5 N(0, 1) away from a bank latent, half
images of unrelated latents (the inputs of tools/bench_wb.py's comparison); the start is pbb_init_from_bank.  Every variant runs once to warm
up, then `repeat` times alternating; the time is the wall time of the whole call (uploads, every launch, the downloads that end it).
A forward-equivalent is one generator forward of one latent: (nz + 1) * ladder + 1 per sweep and query, plus the start; population per
round and query, plus the start.  One JSON line per variant.  --only powell is for a run under a profiler's kernel trace: the share of the
gl_pbb_powell kernels is read from its statistics."""
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
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--ngf", type=int, default=64)
    ap.add_argument("--sweeps", type=int, default=2)
    ap.add_argument("--ladder", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--population", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--only", choices=["both", "powell", "es"], default="both")
    args = ap.parse_args()
    import ganleaks_amd as gl
    from ganleaks_amd.gan_models.dcgan.model_torch import Generator
    if gl.device_count() < 1:
        raise SystemExit("bench_pbb_powell.py needs a GPU")
    n, nz = args.queries, 100
    gen = Generator(nz, 3, args.ngf)
    gen.load_state_dict(gl.synth.dcgan_state_dict(1234, features_g=args.ngf))
    z_bank = gl.synth.latent(11, n, nz).reshape(n, nz)
    z_img = gl.synth.latent(12, n, nz).reshape(n, nz)
    z_img[: n // 2] = z_bank[: n // 2] + np.float32(0.5) * gl.synth.latent(13, n // 2, nz).reshape(n // 2, nz)
    q = gen.generate_u8(z_img).numpy()
    z_init, _ = gl.pbb_init_from_bank(q, gen, z_bank, batch_size=64)
    variants = []
    if args.only in ("both", "powell"):
        variants.append(("powell", dict(optimizer="powell", sweeps=args.sweeps, ladder=args.ladder), args.sweeps, ((nz + 1) * args.ladder + 1) * args.sweeps + 1))
    if args.only in ("both", "es"):
        variants.append(("es", dict(rounds=args.rounds, population=args.population), args.rounds, args.population * args.rounds + 1))
    results, wall = {}, {label: [] for label, _, _, _ in variants}
    for label, kw, _, _ in variants:                                     # warm-up: code objects, the generator's workspaces
        results[label] = gl.pbb_attack(q, gen, z_init, history=True, **kw)
    for _ in range(args.repeat):
        for label, kw, _, _ in variants:
            t0 = time.perf_counter()
            gl.pbb_attack(q, gen, z_init, history=True, **kw)
            wall[label].append(time.perf_counter() - t0)
    half = n // 2
    for label, kw, units, forwards in variants:
        _, _, S, trace = results[label]
        t = wall[label]
        med = float(np.median(t)) if t else None
        row = {"variant": label, "queries": n, "ngf": args.ngf, **{k: v for k, v in kw.items() if k != "optimizer"}, "forwards_per_query": forwards,
               "mean_S_start": float(trace[0].mean()), "median_S_start": float(np.median(trace[0])), "mean_S": float(S.mean()),
               "median_S": float(np.median(S)), "median_S_near": float(np.median(S[:half])), "median_S_far": float(np.median(S[half:])),
               "trace_mean": [float(r.mean()) for r in trace] if label == "powell" else None}
        if med is not None:
            row.update({"wall_s_median": round(med, 4), "wall_s_min": round(min(t), 4), "wall_s_max": round(max(t), 4),
                        "ms_per_sweep_or_round": round(1e3 * med / units, 3), "us_per_forward_equivalent": round(1e6 * med / (n * forwards), 4)})
        print(json.dumps(row), flush=True)
    if len(variants) == 2:
        Sp, Se = results["powell"][2], results["es"][2]
        print(json.dumps({"comparison": "final S, powell against es at the nearest equal budget", "queries": n, "powell_lower": int((Sp < Se).sum()),
                          "es_lower": int((Se < Sp).sum()), "equal": int((Sp == Se).sum()),
                          "median_ratio_powell_over_es": float(np.median(Sp[Se > 0] / Se[Se > 0])) if (Se > 0).any() else None}), flush=True)


if __name__ == "__main__":
    main()
