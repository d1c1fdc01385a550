#!/usr/bin/env python3
"""Generate tests/golden/knn_topk.npz: the reference's first 8 nearest neighbours per query.  The reference keeps one (torch.min at
attack_models/fbb.py:86), but its custom_knn (fbb.py:73-88) evaluates the loss of every batch on the way.  The script runs the REFERENCE's
custom_knn, imported in place (tests/golden/_refimport.py), with a loss callable that is the L2 lambda of attack_models/utils.py:163 and
also records what it returns for every batch; a stable sort of the recorded distances is what "the K nearest samples" (fbb.py:35) means
in the reference's arithmetic.  custom_knn's own result must equal the first entry.

Run where the reference tree exists, never on the GPU machine:   python tests/golden/make_golden_topk.py
Only seeds, sizes and the reference's distances and indices are stored (the images are re-derived from the seed): a few KB.

Condition: the reference's fp32 order of the first 9 neighbours must equal the exact-integer order (S, index) for EVERY query of a case --
then a test may compare all queries and skip none.  The script asserts it and writes nothing otherwise.
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

KEEP = 8
# (seed, n_bank, n_pos, n_neg, res, batch_size)
CASES = [(21, 700, 8, 8, 16, 64), (22, 330, 6, 6, 64, 30), (23, 1100, 8, 8, 32, 64)]


def ref_sorted_distances(fbb, bank, sample, batch_size):
    """one call of the reference's custom_knn; the loss records its per-batch results, which are then sorted (stable)"""
    recorded = []

    def recording_loss(x_hat, x_gt):
        recorded.append(ref_l2_loss(x_hat, x_gt))
        return recorded[-1]

    d_min, i_min = fbb.custom_knn(bank, sample, recording_loss, types.SimpleNamespace(BATCH_SIZE=batch_size))
    d, order = torch.sort(torch.cat(recorded), stable=True)
    assert int(order[0]) == i_min and float(d[0]) == d_min, "custom_knn's own result is not the first of the sorted distances"
    return d.numpy(), order.numpy()


def main(fbb):
    out = {"n_cases": len(CASES), "keep": KEEP}
    for c, (seed, nb, npos, nneg, res, bs) in enumerate(CASES):
        case = synth.attack_case(seed, nb, npos, nneg, res)
        bank_u8 = case["bank"]
        q_u8 = np.concatenate([case["pos"], case["neg"]])
        bank, queries = to_ref_tensor(bank_u8), to_ref_tensor(q_u8)
        n_eff = (nb // bs) * bs
        dist = np.empty((len(q_u8), KEEP), np.float32)
        idx = np.empty((len(q_u8), KEEP), np.int64)
        d_vals = res * res * 3
        worst_gap, worst_err = np.inf, 0.0
        for qi, sample in enumerate(queries):
            d, i = ref_sorted_distances(fbb, bank, sample, bs)
            diff = bank_u8[:n_eff].astype(np.int64) - q_u8[qi].astype(np.int64)
            S = (diff * diff).reshape(n_eff, -1).sum(axis=1)
            exact = np.argsort(S, kind="stable")
            assert np.array_equal(i[:KEEP + 1], exact[:KEEP + 1]), "case %d query %d: the fp32 order differs from the exact one" % (c, qi)
            s = S[exact[:KEEP + 1]].astype(np.float64)
            assert np.all(np.diff(s) > 0), "case %d query %d: exact tie among the first %d" % (c, qi, KEEP + 1)
            worst_gap = min(worst_gap, float(np.min(np.diff(s) / s[1:])))
            worst_err = max(worst_err, float(np.max(np.abs(d[:KEEP].astype(np.float64) - np.float32(s[:KEEP] * 4.0 / (65025.0 * d_vals))))))
            dist[qi], idx[qi] = d[:KEEP], i[:KEEP]
        print("case %d: %d queries, smallest relative gap %.2e, largest |ref - fl32(S*4/(65025 D))| %.2e" % (c, len(q_u8), worst_gap, worst_err))
        out["case%d" % c] = np.array([seed, nb, npos, nneg, res, bs], np.int64)
        out["dist%d" % c] = dist
        out["idx%d" % c] = idx
    np.savez(os.path.join(HERE, "knn_topk.npz"), **out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    main(_refimport.load("attack_models/fbb.py", "ref_fbb"))
