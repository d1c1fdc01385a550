#!/usr/bin/env python3
"""Generate tests/golden/knn_float_rows.npz: the reference's first 8 nearest neighbours per query for rows OFF the 8-bit and the integer
lattice (float images, continuous tables) -- the sibling of make_golden_topk.py.  The same recording-loss run of the REFERENCE's custom_knn
(attack_models/fbb.py:73-88, imported in place through tests/golden/_refimport.py) under the L2 lambda of attack_models/utils.py:163;
tables go in shaped [N, F, 1, 1], as a caller of custom_knn would hand them over.

Run where the reference tree exists, never on the GPU machine:   python tests/golden/make_golden_float_rows.py
Only seeds, sizes, the reference's distances and indices and the per-case error are stored; the rows are re-derived from the seeds
(tests/float_rows_common.py).

The reference sums in whatever order its torch build takes; the product fixes one order (the chain D32 of csrc/gl_l2f32.hip, restated on the
CPU by oracle/fbb_oracle.c).  Condition, for every query of a case: the reference's order of the first 9 neighbours equals the chain's
stable order, and the smallest gap between consecutive chain distances among them exceeds 4 x the largest |reference - chain| of the case --
then a test may compare every slot of every query.  The script asserts it and writes nothing otherwise.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refimport  # noqa: E402
import float_rows_common as common  # noqa: E402
from make_golden import synth  # noqa: E402
from make_golden_topk import ref_sorted_distances  # noqa: E402

KEEP = common.KEEP


def main(fbb):
    cases = common.golden_cases()
    out = {"n_cases": len(cases), "keep": KEEP}
    for c, (name, kind, params) in enumerate(cases):
        bank, queries, bs = common.derive(synth, kind, params)
        n_eff = (len(bank) // bs) * bs
        as4d = lambda x: torch.from_numpy(x.reshape(x.shape + (1, 1)) if x.ndim == 2 else x)      # noqa: E731
        tb, tq = as4d(bank), as4d(queries)
        M = common.chain_matrix(queries, bank[:n_eff])
        dist = np.empty((len(queries), KEEP), np.float32)
        idx = np.empty((len(queries), KEEP), np.int64)
        gap, err, mismatches = np.inf, 0.0, 0
        for qi, sample in enumerate(tq):
            d, i = ref_sorted_distances(fbb, tb, sample, bs)
            order = np.argsort(M[qi], kind="stable")
            mismatches += int(not np.array_equal(i[:KEEP + 1], order[:KEEP + 1]))
            chain = M[qi, order[:KEEP + 1]].astype(np.float64)
            gap = min(gap, float(np.min(np.diff(chain))))
            err = max(err, float(np.max(np.abs(d[:KEEP + 1].astype(np.float64) - chain))))
            dist[qi], idx[qi] = d[:KEEP], i[:KEEP]
        print("%s: %d queries, %d order mismatches, smallest gap %.2e, largest |ref - chain| %.2e" % (name, len(queries), mismatches, gap, err))
        assert mismatches == 0, "%s: the reference's order differs from the chain's" % name
        assert gap > 4.0 * err, "%s: a gap of %.2e is within 4 x the error %.2e" % (name, gap, err)
        out["name%d" % c] = np.array(name)
        out["kind%d" % c] = np.array(kind)
        out["params%d" % c] = np.array(params, np.int64)          # seed and sizes: float_rows_common.derive re-derives the rows
        out["dist%d" % c] = dist
        out["idx%d" % c] = idx
        out["err%d" % c] = np.float64(err)
    np.savez(os.path.join(HERE, "knn_float_rows.npz"), **out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    main(_refimport.load("attack_models/fbb.py", "ref_fbb"))
