#!/usr/bin/env python3
"""Timing of the white-box attack's gradient and step (ganleaks_amd.wb), and its result next to the partial-black-box search from the same
start.  ONE process on the shipped library, run it under the caller's `timeout`:
    python tools/bench_wb.py [--rounds 7] [--queries 4096] [--ngf 64] [--compare_queries 1024] [--steps 64]
    python tools/bench_wb.py --gan pggan [--in_channels 256] [--pg_steps 4] [--alpha 1.0] [--nz 256] --queries 1024 --compare_queries 256
    python tools/bench_wb.py --optimizer lbfgs [--memory 8] [--ladder 8] ...
DCGAN-64, or with --gan pggan PGGAN at a fixed depth (gl_pggan_forward / gl_pggan_l2_grad_z, Generator.at), with synthetic weights.  Timed with device events on the context's stream, every variant warmed up once, then the variants
ALTERNATE inside every round (median, smallest, largest):
  forward fp32    gl_dcgan_forward (gl_pggan_forward) at precision 0, fp32 output: the forward half of the gradient call
  l2_grad_z       gl_dcgan_l2_grad_z: that forward, the cotangent and the backward pass; x_forward is its ratio to `forward fp32`
  scoring         generate_u8 at the generator's own precision (split-fp16), the extra forward of a step
  step            l2_grad_z + gl_wb_adam_step + generate_u8 + gl_pbb_group_min + gl_pbb_accept: one step of wb_attack; scoring_share is
                  `scoring` / `step`, steps_per_s the inverse of the median
Then, on --compare_queries queries (half images of latents 0.5 away from a bank latent, half images of unrelated latents) started from
pbb_init_from_bank: the final S of wb_attack(steps) beside pbb_attack(rounds=32, population=64) -- `steps` gradient passes against 2048
forwards per query.  One JSON line per variant and one for the comparison.
With --optimizer lbfgs `step` is one step of wb_attack(optimizer='lbfgs') -- l2_grad_z + gl_wb_lbfgs_push + gl_wb_lbfgs_direction +
gl_wb_lbfgs_candidates + generate_u8 on Q * ladder candidates + gl_pbb_group_min + gl_pbb_accept + gl_wb_lbfgs_advance, in blocks of
pbb.POPULATION_IMAGES // ladder queries as wb_attack runs them -- and two variants are added: `ladder scoring`, generate_u8 on the Q * ladder
candidates, and `lbfgs kernels`, the four gl_wb_lbfgs_* calls alone (kernels_share is their ratio to `step`).  The comparison then also runs
wb_attack(optimizer='lbfgs') at the same --steps and reports the median of S_lbfgs / S_adam over the queries and who ends lower."""
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
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--ngf", type=int, default=64)
    ap.add_argument("--compare_queries", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--gan", choices=["dcgan", "pggan"], default="dcgan")
    ap.add_argument("--in_channels", type=int, default=256, help="pggan: channel count of the first block")
    ap.add_argument("--pg_steps", type=int, default=4, help="pggan: resolution steps (4 * 2^pg_steps pixels)")
    ap.add_argument("--alpha", type=float, default=1.0, help="pggan: fade-in weight of the last block")
    ap.add_argument("--nz", type=int, default=None, help="latent length (default 100; 256 for pggan)")
    ap.add_argument("--optimizer", choices=["adam", "lbfgs"], default="adam")
    ap.add_argument("--memory", type=int, default=8, help="lbfgs: pairs kept per query")
    ap.add_argument("--ladder", type=int, default=8, help="lbfgs: step widths scored per step")
    args = ap.parse_args()
    import ganleaks_amd as gl
    from ganleaks_amd._lib import check
    from ganleaks_amd.gan_models.dcgan.model_torch import Generator
    if gl.device_count() < 1:
        raise SystemExit("bench_wb.py needs a GPU")
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

    pg = args.gan == "pggan"
    Q, nz = args.queries, args.nz if args.nz is not None else (256 if pg else 100)
    if pg:
        from ganleaks_amd.gan_models.pggan.model_torch import Generator as PgganGenerator
        R, pgs, alpha = 4 * 2 ** args.pg_steps, int(args.pg_steps), f(args.alpha)
        sd = gl.synth.pggan_state_dict(1234, nz, args.in_channels)
        full, full0 = PgganGenerator(nz, args.in_channels, 3), PgganGenerator(nz, args.in_channels, 3)
        full.load_state_dict(sd)
        full0.load_state_dict(sd)
        full0.set_precision(0)
        gen = full.at(pgs, args.alpha)               # what the attacks are handed
        tag = {"gan": "pggan", "in_channels": args.in_channels, "pg_steps": pgs, "alpha": args.alpha}
    else:
        R = 64
        sd = gl.synth.dcgan_state_dict(1234, features_g=args.ngf)
        gen, gen0 = Generator(nz, 3, args.ngf), Generator(nz, 3, args.ngf)
        gen.load_state_dict(sd)
        gen0.load_state_dict(sd)
        gen0.set_precision(0)
        tag = {"ngf": args.ngf}
    d = 3 * R * R
    queries = gen.generate_u8(gl.synth.latent(2, Q, nz))
    z = ctx.to_device(gl.synth.latent(1, Q, nz).reshape(Q, nz))
    z_best = ctx.to_device(gl.synth.latent(1, Q, nz).reshape(Q, nz))
    m, v = ctx.zeros((Q, nz), np.float32), ctx.zeros((Q, nz), np.float32)
    grad, loss, out = ctx.empty((Q, nz), np.float32), ctx.empty((Q,), np.float32), ctx.empty((Q, 3, R, R), np.float32)
    one = ctx.to_device(np.ones((Q,), np.float32))
    S_best, S_new = ctx.to_device(np.full((Q,), np.iinfo(np.int64).max, np.uint64)), ctx.empty((Q,), np.uint64)
    j_new, accepted, work = ctx.empty((Q,), np.int32), ctx.empty((Q,), np.uint8), ctx.empty((16 * Q,), np.uint8)
    state = {"t": 0, "images": None}

    def forward32():
        if pg:
            check(lib.gl_pggan_forward(full0._handle, p(z.ptr), Q, pgs, alpha, p(out.ptr), p(0)))
        else:
            check(lib.gl_dcgan_forward(gen0._handle, p(z.ptr), Q, p(out.ptr), p(0)))

    def l2_grad():
        if pg:
            check(lib.gl_pggan_l2_grad_z(full._handle, p(z.ptr), p(queries.ptr), Q, pgs, alpha, p(grad.ptr), p(loss.ptr)))
        else:
            check(lib.gl_dcgan_l2_grad_z(gen._handle, p(z.ptr), p(queries.ptr), Q, p(grad.ptr), p(loss.ptr)))

    def scoring():
        if pg:
            state["images"] = full.forward_device(z, pgs, args.alpha, False, True, check_range=False)[1]
        else:
            state["images"] = gen.forward_device(z, False, True, check_range=False)[1]

    def step():
        state["t"] += 1
        t = state["t"]
        l2_grad()
        check(lib.gl_wb_adam_step(ctx.handle, p(z.ptr), p(m.ptr), p(v.ptr), p(grad.ptr), Q, nz, f(0.05), f(0.9), f(0.999), f(1e-8),
                                  f(1.0 / (1.0 - 0.9 ** t)), f(1.0 / (1.0 - 0.999 ** t)), f(4.0)))
        scoring()
        check(lib.gl_pbb_group_min(ctx.handle, p(queries.ptr), p(state["images"].ptr), Q, 1, d, p(S_new.ptr), p(j_new.ptr), p(work.ptr)))
        check(lib.gl_pbb_accept(ctx.handle, p(z_best.ptr), p(one.ptr), p(S_best.ptr), p(z.ptr), p(S_new.ptr), p(j_new.ptr), Q, nz, 1, f(1.0), f(1.0),
                                f(1.0), f(1.0), p(accepted.ptr)))

    variants = [("forward fp32", forward32), ("l2_grad_z", l2_grad), ("scoring", scoring), ("step", step)]
    lbfgs = args.optimizer == "lbfgs"
    if lbfgs:
        from ganleaks_amd.pbb import POPULATION_IMAGES
        mem, L = args.memory, args.ladder
        nb = min(Q, max(1, POPULATION_IMAGES // L))                     # the block wb_attack runs
        z_prev, g_prev = ctx.zeros((Q, nz), np.float32), ctx.zeros((Q, nz), np.float32)
        S_hist, Y_hist = ctx.zeros((Q, mem, nz), np.float32), ctx.zeros((Q, mem, nz), np.float32)
        count, head, flag = ctx.zeros((Q,), np.int32), ctx.zeros((Q,), np.int32), ctx.zeros((Q,), np.uint8)
        t_w = ctx.to_device(np.ones((Q,), np.float32))
        moved = ctx.zeros((Q,), np.uint8)
        direc, cand = ctx.empty((Q, nz), np.float32), ctx.empty((nb * L, nz), np.float32)
        work_l = ctx.empty((16 * nb * ((L + 15) // 16),), np.uint8)
        S_cur = ctx.to_device(np.full((Q,), np.iinfo(np.int64).max, np.uint64))

        def before_scoring(lo, n):
            o4, o1 = lo * nz * 4, lo
            check(lib.gl_wb_lbfgs_push(ctx.handle, p(z.ptr + o4), p(grad.ptr + o4), p(z_prev.ptr + o4), p(g_prev.ptr + o4), p(S_hist.ptr + o4 * mem),
                                       p(Y_hist.ptr + o4 * mem), p(count.ptr + 4 * o1), p(head.ptr + 4 * o1), p(moved.ptr + o1), n, nz, mem))
            check(lib.gl_wb_lbfgs_direction(ctx.handle, p(grad.ptr + o4), p(S_hist.ptr + o4 * mem), p(Y_hist.ptr + o4 * mem), p(count.ptr + 4 * o1),
                                            p(head.ptr + 4 * o1), p(t_w.ptr + 4 * o1), p(flag.ptr + o1), n, nz, mem, f(1.0), p(direc.ptr + o4)))
            check(lib.gl_wb_lbfgs_candidates(ctx.handle, p(z.ptr + o4), p(direc.ptr + o4), p(t_w.ptr + 4 * o1), n, nz, L, f(4.0), p(cand.ptr)))

        def after_scoring(lo, n):
            check(lib.gl_wb_lbfgs_advance(ctx.handle, p(t_w.ptr + 4 * lo), p(count.ptr + 4 * lo), p(head.ptr + 4 * lo), p(flag.ptr + lo),
                                          p(moved.ptr + lo), p(j_new.ptr + 4 * lo), n, L))

        def ladder_images(n):
            c = cand.view((n * L, nz))
            if pg:
                return full.forward_device(c, pgs, args.alpha, False, True, check_range=False)[1]
            return gen.forward_device(c, False, True, check_range=False)[1]

        def ladder_scoring():
            for lo in range(0, Q, nb):
                state["images"] = ladder_images(min(nb, Q - lo))

        def lbfgs_kernels():
            for lo in range(0, Q, nb):
                before_scoring(lo, min(nb, Q - lo))
                after_scoring(lo, min(nb, Q - lo))

        def lbfgs_step():
            l2_grad()
            for lo in range(0, Q, nb):
                n = min(nb, Q - lo)
                before_scoring(lo, n)
                images = ladder_images(n)
                check(lib.gl_pbb_group_min(ctx.handle, p(queries.ptr + lo * d), p(images.ptr), n, L, d, p(S_new.ptr + 8 * lo), p(j_new.ptr + 4 * lo),
                                           p(work_l.ptr)))
                check(lib.gl_pbb_accept(ctx.handle, p(z.ptr + lo * nz * 4), p(one.ptr + 4 * lo), p(S_cur.ptr + 8 * lo), p(cand.ptr), p(S_new.ptr + 8 * lo),
                                        p(j_new.ptr + 4 * lo), n, nz, L, f(1.0), f(1.0), f(1.0), f(1.0), p(moved.ptr + lo)))
                after_scoring(lo, n)
                state["images"] = images

        variants = variants[:3] + [("ladder scoring", ladder_scoring), ("lbfgs kernels", lbfgs_kernels), ("step", lbfgs_step)]
        tag = dict(tag, optimizer="lbfgs", memory=mem, ladder=L)
    for _, fn in variants:                       # warm-up: code object load, first touch, the workspaces and the transposed packs
        fn()
        ctx.sync()
    ms = {label: [] for label, _ in variants}
    for _ in range(args.rounds):
        for label, fn in variants:
            ms[label].append(timed(fn))
    med = {label: float(np.median(t)) for label, t in ms.items()}
    for label, _ in variants:
        t = ms[label]
        row = {"variant": label, "queries": Q, **tag, "median_ms": round(med[label], 4), "min_ms": round(min(t), 4),
               "max_ms": round(max(t), 4), "x_forward": round(med[label] / med["forward fp32"], 4), "rounds": args.rounds}
        if label == "step":
            row["scoring_share"] = round(med["ladder scoring" if lbfgs else "scoring"] / med[label], 4)
            if lbfgs:
                row["kernels_share"] = round(med["lbfgs kernels"] / med[label], 5)
            row["steps_per_s"] = round(1e3 / med[label], 3)
        print(json.dumps(row), flush=True)

    # ---- the result: gradient descent against the gradient-free search, same start
    n = args.compare_queries
    if n > 0:
        z_bank = gl.synth.latent(11, n, nz).reshape(n, nz)
        z_img = gl.synth.latent(12, n, nz).reshape(n, nz)
        z_img[: n // 2] = z_bank[: n // 2] + np.float32(0.5) * gl.synth.latent(13, n // 2, nz).reshape(n // 2, nz)
        q = gen.generate_u8(z_img).numpy()
        z_init, _ = gl.pbb_init_from_bank(q, gen, z_bank, batch_size=64)
        t0 = time.perf_counter()
        _, _, S_wb, tr = gl.wb_attack(q, gen, z_init, steps=args.steps, history=True)
        t_wb = time.perf_counter() - t0
        t0 = time.perf_counter()
        _, _, S_pbb = gl.pbb_attack(q, gen, z_init, rounds=32, population=64)
        t_pbb = time.perf_counter() - t0
        half = n // 2
        if lbfgs:
            t0 = time.perf_counter()
            _, _, S_lb = gl.wb_attack(q, gen, z_init, steps=args.steps, optimizer="lbfgs", memory=args.memory, ladder=args.ladder)
            t_lb = time.perf_counter() - t0
            both = (S_lb > 0) & (S_wb > 0)
            print(json.dumps({"comparison": "final S, lbfgs against adam at equal steps", "queries": n, **tag, "steps": args.steps,
                              "median_ratio_lbfgs_over_adam": float(np.median(S_lb[both] / S_wb[both])) if both.any() else None,
                              "median_S_lbfgs_near": float(np.median(S_lb[:half])), "median_S_adam_near": float(np.median(S_wb[:half])),
                              "median_S_lbfgs_far": float(np.median(S_lb[half:])), "median_S_adam_far": float(np.median(S_wb[half:])),
                              "lbfgs_lower": int((S_lb < S_wb).sum()), "adam_lower": int((S_wb < S_lb).sum()), "equal": int((S_lb == S_wb).sum()),
                              "lbfgs_wall_s": round(t_lb, 3), "adam_wall_s": round(t_wb, 3)}), flush=True)
        print(json.dumps({"comparison": "final S from the same start", "queries": n, **tag, "wb_steps": args.steps, "pbb_rounds": 32,
                          "pbb_population": 64, "median_S_start_near": float(np.median(tr[0][:half])), "median_S_wb_near": float(np.median(S_wb[:half])),
                          "median_S_pbb_near": float(np.median(S_pbb[:half])), "median_S_start_far": float(np.median(tr[0][half:])),
                          "median_S_wb_far": float(np.median(S_wb[half:])), "median_S_pbb_far": float(np.median(S_pbb[half:])),
                          "wb_below_pbb": int((S_wb < S_pbb).sum()), "wb_wall_s": round(t_wb, 3), "pbb_wall_s": round(t_pbb, 3)}), flush=True)


if __name__ == "__main__":
    main()
