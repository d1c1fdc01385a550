#!/usr/bin/env python3
"""Generate tests/golden/knn_res512.npz by running the REFERENCE's custom_knn (attack_models/fbb.py:73-88) with the L2 lambda of
attack_models/utils.py:163 on synth.attack_case(..., res=512): images of 3 x 512 x 512 = 786432 values, beyond the int32-norm limit of
the exact path (262143), searched on its wide form.

Run where the reference tree exists, never on the GPU machine:   python tests/golden/make_golden_wide.py
The reference is imported in place (tests/golden/_refimport.py).  Only the seed, the sizes and the reference's distances and indices are
stored (the images are re-derived from the seed), so the file is a few KB.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refimport  # noqa: E402
from make_golden import ref_l2_loss, synth, to_ref_tensor  # noqa: E402

# name: (seed, n_bank, n_pos, n_neg, res, batch_size)
CASES = {"knn_res512": (15, 70, 6, 6, 512, 32)}          # 70 -> 64 rows used


def make_knn_wide(fbb):
    for name, (seed, nb, npos, nneg, res, bs) in CASES.items():
        case = synth.attack_case(seed, nb, npos, nneg, res)
        bank = to_ref_tensor(case["bank"])
        args = types.SimpleNamespace(BATCH_SIZE=bs)
        out = {}
        for kind in ("pos", "neg"):
            d, i = [], []
            for sample in to_ref_tensor(case[kind]):
                dd, ii = fbb.custom_knn(bank, sample, ref_l2_loss, args)
                d.append(dd)
                i.append(ii)
            out[kind + "_dist"] = np.array(d, np.float64)
            out[kind + "_idx"] = np.array(i, np.int64)
        np.savez(os.path.join(HERE, name + ".npz"), seed=seed, n_bank=nb, n_pos=npos, n_neg=nneg, res=res, batch_size=bs, **out)
        print(name, "pos idx == src:", np.mean(out["pos_idx"] == case["pos_src"]))


if __name__ == "__main__":
    torch.set_num_threads(8)
    make_knn_wide(_refimport.load("attack_models/fbb.py", "ref_fbb"))
