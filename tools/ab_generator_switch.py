#!/usr/bin/env python3
"""In-process A/B of one tuning switch on the DCGAN-64 generator: the values of an environment variable that the tuning build reads on
every call (csrc/gl_common.h gl_tuning_int) alternate inside ONE process on one device, un-profiled, after a warm-up of every arm:

    GANLEAKS_LIB=gan-leaks_amd/libganleaks_hip_tuning.so python tools/ab_generator_switch.py --var GL_H3_EPI16 [--arms 0,1] [--rounds 7] [--images 16384]

Timed: the generator with u8 output, passes of 4096 images as in the headline step.  The first arm is the baseline.  One JSON line: every
round's ms per arm, the medians, the gain over the first arm, and the spread (max - min) inside each arm.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ganleaks_amd as gl  # noqa: E402
from ganleaks_amd import _lib  # noqa: E402
from ganleaks_amd.gan_models.dcgan.model_torch import Generator  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--var", required=True, help="the tuning variable, e.g. GL_H3_EPI16, GL_H3_XONCE, GL_H3_T4")
    ap.add_argument("--arms", default="0,1", help="values of the variable to alternate; the first is the baseline")
    ap.add_argument("--reps", type=int, default=20, help="generator calls per timed sample")
    ap.add_argument("--images", type=int, default=16384)
    args = ap.parse_args()
    assert _lib.LIB_PATH.endswith("libganleaks_hip_tuning.so"), "load the tuning build through $GANLEAKS_LIB"
    ctx = gl.Context.get()
    g = Generator(100, 3, 64, ctx)
    g.load_state_dict(gl.synth.dcgan_state_dict(1234))
    z = ctx.to_device(gl.synth.latent(1, args.images).reshape(args.images, 100))
    fn = lambda: g.forward_device(z, False, True, check_range=False)
    arms = args.arms.split(",")

    def select(a):
        os.environ[args.var] = a
    ms = {a: [] for a in arms}
    for a in arms:                                     # warm-up of every arm
        select(a)
        fn()
        fn()
    ctx.sync()
    for _ in range(args.rounds):
        for a in arms:
            select(a)
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                fn()
            ctx.sync()
            ms[a].append((time.perf_counter() - t0) / args.reps * 1e3)
    base = ms[arms[0]]
    out = {"workload": "dcgan64_forward_u8", "images": args.images, "var": args.var, "baseline_arm": arms[0]}
    for a in arms:
        out["arm" + a] = {"ms": [round(x, 3) for x in ms[a]], "median": round(float(np.median(ms[a])), 3),
                          "spread": round(max(ms[a]) - min(ms[a]), 3), "gain_ms": round(float(np.median(base) - np.median(ms[a])), 3),
                          "every_run_below_baseline": bool(max(ms[a]) < min(base))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
