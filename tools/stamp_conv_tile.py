#!/usr/bin/env python3
"""Where a 256 x 256 tile of gather_conv_h3 spends its cycles: s_memtime stamps of the tuning build's STAMP instantiation (csrc/gl_conv_h3.hip),
taken by wave 0 of every workgroup at kernel entry, before the input pieces of slice 0, after the K loop, after the last conversion of the
epilogue and after its last store has landed (the stamped build alone waits for that).  Needs the tuning build:

    GANLEAKS_LIB=gan-leaks_amd/libganleaks_hip_tuning.so python tools/stamp_conv_tile.py [--images 4096] [--arms 0,1] [--warm-seconds 2]

Per arm (the value of GL_H3_EPI16: 8-byte or 16-byte split stores): the DCGAN-64 generator runs back to back on random latents for --warm-seconds (the clock
the chip holds depends on load and data), then ONE forward of --images images is stamped.  Printed per layer that runs on this tile (layer 0:
1 x 1 grid, layer 1: 4 x 4, layer 2: 8 x 8): the median over workgroups of the cycles per phase, the phase's share of the tile, and the cycles
per K slice; one JSON line per arm and layer at the end.  The stamped kernel waits where the real one does not, so read the SHARES and the
differences between arms, never its run time.  Two stamps back to back are about 40 cycles apart.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ganleaks_amd as gl  # noqa: E402
from ganleaks_amd import _lib  # noqa: E402
from ganleaks_amd.gan_models.dcgan.model_torch import Generator  # noqa: E402

PHASES = ["prologue", "k_loop", "convert_and_issue", "store_drain"]      # stamp k + 1 minus stamp k
MAX_TILES = 1 << 16
LAYER_OF_H = {1: 0, 4: 1, 8: 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4096)
    ap.add_argument("--arms", default="0,1", help="values of GL_H3_EPI16")
    ap.add_argument("--warm-seconds", type=float, default=2.0)
    args = ap.parse_args()
    assert _lib.LIB_PATH.endswith("libganleaks_hip_tuning.so"), "load the tuning build through $GANLEAKS_LIB"
    ctx = gl.Context.get()
    lib = ctx.lib
    lib.gl_tune_h3_stamp_begin.restype = ctypes.c_int
    lib.gl_tune_h3_stamp_begin.argtypes = [ctypes.c_void_p, ctypes.c_longlong]
    lib.gl_tune_h3_stamp_end.restype = ctypes.c_int
    lib.gl_tune_h3_stamp_end.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    g = Generator(100, 3, 64, ctx)
    g.load_state_dict(gl.synth.dcgan_state_dict(1234))
    z = ctx.to_device(gl.synth.latent(1, args.images).reshape(args.images, 100))
    run = lambda: g.forward_device(z, False, True, check_range=False)
    rows = []
    for arm in args.arms.split(","):
        os.environ["GL_H3_EPI16"] = arm
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < args.warm_seconds:
            for _ in range(8):
                run()
            ctx.sync()
        assert lib.gl_tune_h3_stamp_begin(ctx.handle, MAX_TILES) == 0
        run()
        ctx.sync()
        stamps = np.zeros((MAX_TILES, 8), np.uint64)
        info = np.zeros((256, 8), np.int64)
        n = lib.gl_tune_h3_stamp_end(ctx.handle, stamps.ctypes.data, info.ctypes.data)
        assert n > 0, "no launch was stamped"
        for first, wgs, H, W, nk, t4, epi16, _ in info[:n]:
            s = stamps[first:first + wgs, :5].astype(np.int64)
            d = np.diff(s, axis=1)
            total = s[:, 4] - s[:, 0]
            med = [float(np.median(d[:, k])) for k in range(4)]
            rows.append({"arm": arm, "layer": LAYER_OF_H.get(int(H), -1), "grid": "%dx%d" % (H, W), "k_slices": int(nk), "workgroups": int(wgs),
                         "t4": int(t4), "epi16": int(epi16), "median_cycles": dict(zip(PHASES, med)),
                         "median_tile_cycles": float(np.median(total)), "cycles_per_slice": med[1] / float(nk),
                         "fixed_cycles": float(np.median(total - d[:, 1]))})
    print("%-4s %-6s %-5s %6s | %10s %10s %18s %12s | %10s %9s %9s" % (("arm", "layer", "grid", "slices") + tuple(PHASES) + ("tile", "per slice", "fixed")))
    for r in rows:
        m = r["median_cycles"]
        share = lambda v: "%7.0f %2.0f%%" % (v, 100.0 * v / r["median_tile_cycles"])
        print("%-4s %-6d %-5s %6d | %10s %10s %18s %12s | %10.0f %9.1f %9.0f" % (r["arm"], r["layer"], r["grid"], r["k_slices"], share(m["prologue"]),
              share(m["k_loop"]), share(m["convert_and_issue"]), share(m["store_drain"]), r["median_tile_cycles"], r["cycles_per_slice"], r["fixed_cycles"]))
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
