#!/usr/bin/env python3
"""Timing of one round of the partial-black-box search (ganleaks_amd.pbb) next to the generator alone on the same latents.  ONE process on
the shipped library, run it under the caller's `timeout`:
    python tools/bench_pbb.py [--rounds 7] [--queries 1024] [--population 64] [--ngf 64] [--repeat 20]
DCGAN-64 with synthetic weights; the queries are images of other latents.  Timed with device events, every variant warmed up once, then the
variants ALTERNATE inside every round (median, smallest, largest):
  generate only   generate_u8 on the Q * lambda candidate latents of a round -- what the parent commit could already do
  round           gl_pbb_candidates + generate_u8 + gl_pbb_group_min + gl_pbb_accept: one round of pbb_attack
  candidates      gl_pbb_candidates alone, `repeat` launches per window
  group_min       gl_pbb_group_min alone on the candidate images, `repeat` launches per window; bytes_per_s counts what the algorithm has
                  to read, Q * lambda * d candidate bytes + Q * d query bytes, once
  accept          gl_pbb_accept alone, `repeat` launches per window
One JSON line per variant; `x_generate` is the ratio to `generate only`, `generate_share` of `round` the inverse."""
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
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--population", type=int, default=64)
    ap.add_argument("--ngf", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=20)
    args = ap.parse_args()
    import ganleaks_amd as gl
    from ganleaks_amd._lib import check
    from ganleaks_amd.gan_models.dcgan.model_torch import Generator
    from ganleaks_amd.pbb import GL_PBB_GROUP, GL_PBB_PARTIAL_BYTES
    if gl.device_count() < 1:
        raise SystemExit("bench_pbb.py needs a GPU")
    ctx = gl.Context.get()
    lib = ctx.lib
    p, f = ctypes.c_void_p, ctypes.c_float
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

    Q, lam, nz, d, rep = args.queries, args.population, 100, 3 * 64 * 64, args.repeat
    gen = Generator(nz, 3, args.ngf)
    gen.load_state_dict(gl.synth.dcgan_state_dict(1234, features_g=args.ngf))
    queries = gen.generate_u8(gl.synth.latent(2, Q))
    z = ctx.to_device(gl.synth.latent(1, Q).reshape(Q, nz))
    sigma = ctx.to_device(np.full((Q,), 0.5, np.float32))
    cand = ctx.empty((Q * lam, nz), np.float32)
    S_cur, S_new = ctx.to_device(np.full((Q,), np.iinfo(np.int64).max, np.uint64)), ctx.empty((Q,), np.uint64)
    j_new, accepted = ctx.empty((Q,), np.int32), ctx.empty((Q,), np.uint8)
    work = ctx.empty((GL_PBB_PARTIAL_BYTES * Q * ((lam + GL_PBB_GROUP - 1) // GL_PBB_GROUP),), np.uint8)
    state = {"round": 0, "images": None}

    def candidates():
        state["round"] += 1
        check(lib.gl_pbb_candidates(ctx.handle, p(z.ptr), p(sigma.ptr), Q, nz, lam, ctypes.c_uint64(7), ctypes.c_uint32(state["round"]), 0, f(4.0),
                                    p(cand.ptr)))

    def generate():
        state["images"] = gen.generate_u8(cand)

    def group_min():
        check(lib.gl_pbb_group_min(ctx.handle, p(queries.ptr), p(state["images"].ptr), Q, lam, d, p(S_new.ptr), p(j_new.ptr), p(work.ptr)))

    def accept():
        check(lib.gl_pbb_accept(ctx.handle, p(z.ptr), p(sigma.ptr), p(S_cur.ptr), p(cand.ptr), p(S_new.ptr), p(j_new.ptr), Q, nz, lam, f(1.5),
                                f(1.5 ** -0.25), f(1e-4), f(4.0), p(accepted.ptr)))

    def one_round():
        candidates()
        generate()
        group_min()
        accept()

    def times(fn):
        return lambda: [fn() for _ in range(rep)]

    variants = [("generate only", generate, 1), ("round", one_round, 1), ("candidates", times(candidates), rep), ("group_min", times(group_min), rep),
                ("accept", times(accept), rep)]
    candidates()
    for _, fn, _ in variants:                    # warm-up: code object load, first touch, the generator's workspaces
        fn()
        ctx.sync()
    ms = {label: [] for label, _, _ in variants}
    for _ in range(args.rounds):
        for label, fn, n in variants:
            ms[label].append(timed(fn) / n)
    base = float(np.median(ms["generate only"]))
    for label, _, n in variants:
        t = ms[label]
        row = {"variant": label, "queries": Q, "population": lam, "d": d, "ngf": args.ngf, "launches_per_window": n,
               "median_ms": round(float(np.median(t)), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
               "x_generate": round(float(np.median(t)) / base, 4), "rounds": args.rounds}
        if label == "round":
            row["generate_share"] = round(base / float(np.median(t)), 4)
        if label == "group_min":
            row["bytes"] = Q * lam * d + Q * d
            row["bytes_per_s"] = round(row["bytes"] / (float(np.median(t)) * 1e-3), 1)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
