#!/usr/bin/env python3
"""Where a round of the partial-black-box search under 0.2 * LPIPS + L2 (ganleaks_amd.pbb.pair_pbb_attack) spends its time, next to the
same search on exact L2 (pbb_attack).  ONE process on the shipped library, run it under the caller's `timeout`:
    python tools/time_pair_pbb.py [--queries 256] [--population 64] [--rounds 8] [--ngf 64]
DCGAN-64 with synthetic weights and synthetic VGG16 / lin weights (times do not depend on the values); the queries are images of other
latents.  A round is restated here from the calls pair_pbb_attack makes, with a device event between the steps; one round warms up, then
`rounds` rounds are timed (median, smallest, largest per share):
  generator   gl_pbb_candidates + generate_u8 on the Q * lambda candidate latents
  features    LpipsModel.features(role='bank', out=...) on the candidate images: VGG16 and the search rows
  pair        gl_feat_pair_dist_h1_scaled per tile of 256 queries against the tile's 256 * lambda candidate rows
  min+accept  gl_pbb_group_min_keys per tile + gl_pbb_accept
and pair_pbb_attack / pbb_attack themselves for `rounds` rounds by the host clock around a synchronised call (warmed by a call of one
round).  One JSON line per row; `share` is the part of the sum of the four medians, `x_l2` the ratio of the two attacks."""
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
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--population", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--ngf", type=int, default=64)
    args = ap.parse_args()
    import ganleaks_amd as gl
    from ganleaks_amd._lib import check
    from ganleaks_amd.gan_models.dcgan.model_torch import Generator
    from ganleaks_amd.lpips import LpipsModel
    if gl.device_count() < 1:
        raise SystemExit("time_pair_pbb.py needs a GPU")
    ctx = gl.Context.get()
    lib = ctx.lib
    p, f = ctypes.c_void_p, ctypes.c_float
    Q, lam, nz, tile = args.queries, args.population, 100, 256
    gen = Generator(nz, 3, args.ngf)
    gen.load_state_dict(gl.synth.dcgan_state_dict(1234, features_g=args.ngf))
    lin = {"lin%d" % i: np.abs(np.random.default_rng(i).standard_normal(c)).astype(np.float32) for i, c in enumerate((64, 128, 256, 512, 512))}
    model = LpipsModel().load_state_dicts(gl.synth.vgg16_state_dict(7), lin)
    queries = gen.generate_u8(gl.synth.latent(2, Q)).view((Q, 3, 64, 64))
    z_init = gl.synth.latent(1, Q).reshape(Q, nz)

    fq = model.features(queries, role="query")
    z = ctx.to_device(z_init)
    sigma = ctx.to_device(np.full((Q,), 0.5, np.float32))
    cand = ctx.empty((Q * lam, nz), np.float32)
    S_cur, S_new = ctx.to_device(np.full((Q,), 0x7F800000, np.uint64)), ctx.empty((Q,), np.uint64)
    j_new, accepted = ctx.empty((Q,), np.int32), ctx.empty((Q,), np.uint8)
    M = ctx.empty((min(tile, Q), min(tile, Q) * lam), np.float32)
    ld = min(tile, Q) * lam
    ev = [ctx.event() for _ in range(5)]
    state = {"fb": None}

    def one_round(r):
        ev[0].record()
        check(lib.gl_pbb_candidates(ctx.handle, p(z.ptr), p(sigma.ptr), Q, nz, lam, ctypes.c_uint64(7), ctypes.c_uint32(r), 0, f(4.0), p(cand.ptr)))
        u8 = gen.generate_u8(cand).view((Q * lam, 3, 64, 64))
        ev[1].record()
        fb = state["fb"] = model.features(u8, role="bank", fmt=fq.fmt, out=state["fb"])
        ev[2].record()
        for b0 in range(0, Q, tile):
            m = min(tile, Q - b0)
            check(lib.gl_feat_pair_dist_h1_scaled(ctx.handle, p(fb.V.ptr + b0 * lam * fb.K * 2), p(fb.norms.ptr + b0 * lam * 4), m * lam,
                                                  p(fq.V.ptr + b0 * fq.K * 2), p(fq.norms.ptr + b0 * 4), m, fb.K, f(fb.scale), p(M.ptr), ld))
        ev[3].record()
        for b0 in range(0, Q, tile):                     # with more than one tile M holds the last one: the time is what counts here
            m = min(tile, Q - b0)
            check(lib.gl_pbb_group_min_keys(ctx.handle, p(M.ptr), m, lam, ld, p(S_new.ptr + b0 * 8), p(j_new.ptr + b0 * 4)))
        check(lib.gl_pbb_accept(ctx.handle, p(z.ptr), p(sigma.ptr), p(S_cur.ptr), p(cand.ptr), p(S_new.ptr), p(j_new.ptr), Q, nz, lam, f(1.5),
                                f(1.5 ** -0.25), f(1e-4), f(4.0), p(accepted.ptr)))
        ev[4].record()
        ctx.sync()
        return [ev[i].elapsed_ms_until(ev[i + 1]) for i in range(4)]

    one_round(1)                                         # warm-up: code objects, first touch, the workspaces of generator and VGG16
    ms = np.array([one_round(r) for r in range(2, 2 + args.rounds)])
    med = np.median(ms, axis=0)
    common = {"queries": Q, "population": lam, "ngf": args.ngf, "rounds": args.rounds}
    for i, label in enumerate(("generator", "features", "pair", "min+accept")):
        print(json.dumps(dict(common, share_of=label, median_ms=round(float(med[i]), 4), min_ms=round(float(ms[:, i].min()), 4),
                              max_ms=round(float(ms[:, i].max()), 4), share=round(float(med[i] / med.sum()), 4))), flush=True)
    print(json.dumps(dict(common, share_of="round", median_ms=round(float(np.median(ms.sum(axis=1))), 4))), flush=True)
    state["fb"] = None                                   # the attack below allocates its own rows

    def wall(fn):
        ctx.sync()
        t = time.perf_counter()
        fn()
        ctx.sync()
        return (time.perf_counter() - t) * 1e3

    q_host = queries.numpy()
    kw = dict(population=lam, sigma=0.5, seed=7, block_images=Q * lam)
    pair = lambda rounds: gl.pair_pbb_attack(q_host, gen, z_init, rounds=rounds, lpips=model, **kw)     # noqa: E731
    l2 = lambda rounds: gl.pbb_attack(q_host, gen, z_init, rounds=rounds, **kw)                         # noqa: E731
    pair(1)
    l2(1)
    t_pair = [wall(lambda: pair(args.rounds)) for _ in range(3)]
    t_l2 = [wall(lambda: l2(args.rounds)) for _ in range(3)]
    t0_pair, t0_l2 = wall(lambda: pair(0)), wall(lambda: l2(0))       # round 0 and the queries' rows: not part of a round
    per_pair, per_l2 = (float(np.median(t_pair)) - t0_pair) / args.rounds, (float(np.median(t_l2)) - t0_l2) / args.rounds
    print(json.dumps(dict(common, attack="pair_pbb_attack", call_ms=[round(v, 2) for v in t_pair], rounds0_ms=round(t0_pair, 2),
                          ms_per_round=round(per_pair, 3))), flush=True)
    print(json.dumps(dict(common, attack="pbb_attack", call_ms=[round(v, 2) for v in t_l2], rounds0_ms=round(t0_l2, 2),
                          ms_per_round=round(per_l2, 3), x_l2=round(per_pair / per_l2, 2))), flush=True)


if __name__ == "__main__":
    main()
