"""Shared by the float-row tests and tests/golden/make_golden_float_rows.py: the off-lattice inputs re-derived from seeds, and the CPU chain
matrix every device result is compared with (oracle/fbb_oracle.c gl_oracle_l2_pair_f32: the fixed-order float32 distance D32)."""
import ctypes

import numpy as np

import gpu_common  # noqa: F401  (puts oracle/ on the path)

KEEP = 8
# (seed, n_bank, n_pos, n_neg, res, batch_size): synth.attack_case images, decoded and moved off the 8-bit lattice
IMAGE_CASES = [(31, 330, 6, 6, 16, 30), (32, 700, 8, 8, 8, 64)]
# (seed, n_bank, columns, batch_size, n_pos, n_neg): continuous tables (medGAN with Autoencoder(binary=False), PCA-projected rows)
TABLE_CASES = [(41, 300, 37, 30, 8, 8), (42, 520, 1071, 64, 8, 8)]


def decode_u8(codes):
    """what read_image yields for 8-bit codes (attack_models/utils.py:82) as float32: gl_decode_u8"""
    return (2.0 * (codes.astype(np.float64) / 255.0) - 1.0).astype(np.float32)


def image_case(synth, seed, nb, npos, nneg, res):
    """(bank, queries) float32 [N,3,res,res]: the codes of synth.attack_case decoded, plus float32 noise within +-0.4 / 255 (less than half
    a code step: no row lands back on the lattice, neighbours keep their order by and large)"""
    case = synth.attack_case(seed, nb, npos, nneg, res)
    rng = np.random.default_rng(seed + 1000)
    out = []
    for codes in (case["bank"], np.concatenate([case["pos"], case["neg"]])):
        noise = (rng.uniform(-0.4, 0.4, codes.shape) / 255.0).astype(np.float32)
        out.append(decode_u8(codes) + noise)
    return out[0], out[1]


def table_case(seed, nb, cols, npos, nneg):
    """(bank, queries) float32 [N,cols]: bank N(0, 1.5^2); positives = bank rows + N(0, 0.3^2), negatives fresh N(0, 1.5^2)"""
    rng = np.random.default_rng(seed)
    bank = rng.normal(0.0, 1.5, (nb, cols)).astype(np.float32)
    members = rng.choice(nb, npos, replace=False)
    pos = bank[members] + rng.normal(0.0, 0.3, (npos, cols)).astype(np.float32)
    neg = rng.normal(0.0, 1.5, (nneg, cols)).astype(np.float32)
    return bank, np.concatenate([pos, neg])


def derive(synth, kind, params):
    """(bank, queries, batch_size) of one stored case: kind 'image' with IMAGE_CASES' tuple, 'table' with TABLE_CASES'"""
    params = [int(v) for v in params]
    if kind == "image":
        seed, nb, npos, nneg, res, bs = params
        return image_case(synth, seed, nb, npos, nneg, res) + (bs,)
    seed, nb, cols, bs, npos, nneg = params
    return table_case(seed, nb, cols, npos, nneg) + (bs,)


def golden_cases():
    """[(name, kind, params)] in the order of knn_float_rows.npz"""
    return ([("seed%d" % c[0], "image", c) for c in IMAGE_CASES] + [("table%dx%d" % (c[1], c[2]), "table", c) for c in TABLE_CASES])


def chain_matrix(queries, bank):
    """M[q, n] = c_oracle.l2_pair_f32(queries[q], bank[n]), float32 [Q, N] (one C call per pair)"""
    import c_oracle
    fn = c_oracle.lib().gl_oracle_l2_pair_f32
    fn.restype = ctypes.c_float
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    q = np.ascontiguousarray(queries, np.float32).reshape(len(queries), -1)
    b = np.ascontiguousarray(bank, np.float32).reshape(len(bank), -1)
    d = q.shape[1]
    assert b.shape[1] == d
    out = np.empty((len(q), len(b)), np.float32)
    qp, bp = q.ctypes.data, b.ctypes.data
    for i in range(len(q)):
        for n in range(len(b)):
            out[i, n] = fn(qp + i * d * 4, bp + n * d * 4, d)
    return out
