#!/usr/bin/env python3
"""A/B of gather_conv_h3's staged-once input (GL_H3_XONCE=1: each 32-channel input chunk staged once per tile in padded coordinates, taps
read as shifted LDS rows) against the form that stages every tap's rows again (0).  The arms alternate inside ONE process on one device,
un-profiled, after warm-up; needs the tuning build:

    GANLEAKS_LIB=gan-leaks_amd/libganleaks_hip_tuning.so python tools/ab_conv_xonce.py [--rounds 7] [--images 16384]

Timed: the DCGAN-64 generator (u8 output, passes of 4096 images as in the headline step) and, as a control the switch does not reach, VGG16
features at 64 x 64.  The switch changes only the tile of 8 rows of a 16 x 16 image (DCGAN's last hidden layer with the fused RGB tail), so
the difference to arm 0 is that kernel's.  One JSON line per workload: every round's ms per arm, the medians, the gain over the first arm,
and the spread (max - min) inside each arm.
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
from ganleaks_amd.lpips import LpipsModel  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--arms", default="0,1", help="values of GL_H3_XONCE to alternate; the first is the baseline")
    ap.add_argument("--reps", type=int, default=20, help="generator calls per timed sample")
    ap.add_argument("--images", type=int, default=16384)
    ap.add_argument("--vgg-images", type=int, default=4096)
    args = ap.parse_args()
    assert _lib.LIB_PATH.endswith("libganleaks_hip_tuning.so"), "load the tuning build through $GANLEAKS_LIB"
    ctx = gl.Context.get()
    g = Generator(100, 3, 64, ctx)
    g.load_state_dict(gl.synth.dcgan_state_dict(1234))
    z = ctx.to_device(gl.synth.latent(1, args.images).reshape(args.images, 100))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lin = np.load(os.path.join(root, "tests", "golden", "lpips_lin_v0.1.npz"))
    m = LpipsModel(ctx).load_state_dicts(gl.synth.vgg16_state_dict(7), {"lin%d" % i: lin["lin%d" % i] for i in range(5)})
    imgs = np.random.default_rng(5).integers(0, 256, size=(args.vgg_images, 3, 64, 64), dtype=np.uint8)
    work = {"dcgan64_forward_u8": (lambda: g.forward_device(z, False, True, check_range=False), args.reps),
            "vgg16_features_64": (lambda: m.features(imgs, role="bank"), max(1, args.reps // 4))}
    arms = [int(v) for v in args.arms.split(",")]
    for name, (fn, reps) in work.items():
        ms = {v: [] for v in arms}
        for v in arms:                                 # warm-up of every arm
            os.environ["GL_H3_XONCE"] = str(v)
            fn()
            fn()
        ctx.sync()
        for _ in range(args.rounds):
            for v in arms:
                os.environ["GL_H3_XONCE"] = str(v)
                ctx.sync()
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                ctx.sync()
                ms[v].append((time.perf_counter() - t0) / reps * 1e3)
        base = ms[arms[0]]
        out = {"workload": name, "baseline_arm": arms[0]}
        for v in arms:
            out["arm%d" % v] = {"ms": [round(x, 3) for x in ms[v]], "median": round(float(np.median(ms[v])), 3),
                                "spread": round(max(ms[v]) - min(ms[v]), 3), "gain_ms": round(float(np.median(base) - np.median(ms[v])), 3),
                                "every_run_below_baseline": bool(max(ms[v]) < min(base))}
        print(json.dumps(out))


if __name__ == "__main__":
    main()
