"""Host restatements for the partial-black-box attack under 0.2 * LPIPS + L2 (csrc/gl_pbb.hip gl_pbb_group_min_keys, ganleaks_amd/pbb.py
pair_pbb_attack): the grouped minimum over a block of pair distances on the uint32 patterns, the search on the host under the float64
distance of wb_lpips_common (the precondition of the GPU search test), and a search driven from the host that takes its images and its
distance matrix through two callables -- on the GPU, parts that existed before pair_pbb_attack.  Nothing here imports the product."""
import numpy as np

import pbb_common as pc
import wb_lpips_common as wl

# the search test: the 16 x 16 PGGAN view and the latents of wb_lpips_common's (own start / near start / displaced start).  lambda = 5 is
# no power of two and no divisor of 64; 16 rounds of 5 candidates are the work of 80 images per query
SEARCH_ROUNDS, SEARCH_LAMBDA, SEARCH_SIGMA, SEARCH_SEED = 16, 5, 0.0625, 7
UP, DOWN, SIGMA_MIN, SIGMA_MAX, Z_MAX = 1.5, 1.5 ** -0.25, 1e-4, 4.0, 4.0


def bits32(x):
    """the uint32 patterns of float32 values, as int64"""
    return np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.int64)


def group_min_keys(M, lam):
    """M float32 [nq, ld >= nq * lam]: (keys int64 [nq], j int32 [nq]) -- keys[i] the smallest uint32 pattern among M[i, i * lam : (i + 1) * lam],
    compared as unsigned integers, j[i] the first column (relative to i * lam) that holds it"""
    M = np.ascontiguousarray(M, np.float32)
    nq = M.shape[0]
    assert M.ndim == 2 and lam >= 1 and M.shape[1] >= nq * lam
    pat = M.view(np.uint32).astype(np.int64)
    own = np.stack([pat[i, i * lam:(i + 1) * lam] for i in range(nq)]) if nq else np.zeros((0, lam), np.int64)
    j = own.argmin(axis=1)                               # numpy's argmin returns the first minimum
    return own[np.arange(nq), j], j.astype(np.int32)


def group_min_keys_brute(M, lam):
    """the same by two plain loops: strict < in ascending j"""
    M = np.ascontiguousarray(M, np.float32)
    keys, js = [], []
    for i in range(M.shape[0]):
        best, bj = None, None
        for j in range(lam):
            v = int(M[i:i + 1, i * lam + j].view(np.uint32)[0])
            if best is None or v < best:
                best, bj = v, j
        keys.append(best)
        js.append(bj)
    return np.array(keys, np.int64), np.array(js, np.int32)


def key64(d):
    """float64 distances >= +0 as int64 keys: for non-negative IEEE values the order of the patterns is the order of the numbers, 0.0 is key 0"""
    d = np.ascontiguousarray(d, np.float64)
    assert (d >= 0).all()
    return (d + 0.0).view(np.int64).copy()               # -0.0 + 0.0 = +0.0


def host_search(queries_u8, net64, z_init, rounds, lam, sigma, seed, query_base=0):
    """the whole attack on the host: pbb_common's candidates and accept rule, the 8-bit images of the host module, the float64 distance
    -> (z_star float32, dist float64 [Q], trace float64 [rounds + 1, Q])"""
    Q = len(queries_u8)
    z = np.array(z_init, np.float32).reshape(Q, -1)
    sig = np.full(Q, sigma, np.float32)
    image = lambda zz: net64.quantize(net64.forward(zz))                                    # noqa: E731
    S = key64(wl.distance64(net64.vgg, queries_u8, image(z)))
    trace = [S.copy()]
    for r in range(1, rounds + 1):
        cz = pc.candidates(z, sig, lam, seed, r, query_base, Z_MAX)
        d = wl.distance64(net64.vgg, np.repeat(queries_u8, lam, axis=0), image(cz)).reshape(Q, lam)
        j_new = d.argmin(axis=1).astype(np.int32)
        S_new = key64(d[np.arange(Q), j_new])
        z, sig, S, _ = pc.accept(z, sig, S, cz, S_new, j_new, lam, UP, DOWN, SIGMA_MIN, SIGMA_MAX)
        trace.append(S.copy())
    trace = np.stack(trace)
    return z, S.view(np.float64), trace.view(np.float64)


def driven_search(queries_u8, generate, matrix, z_init, rounds, lam, sigma, seed, query_base=0):
    """the attack with its two device steps handed in: generate(z [n, nz]) -> u8 images [n,3,H,W], matrix(queries, images) -> float32
    [Q, n] of pair distances (one call per round on all Q * lam candidates; entry [q, q * lam + j] is used).  Candidates, the grouped
    minimum and the accept step are the host's -> (z_star float32, key int64 [Q], trace int64 [rounds + 1, Q])"""
    Q = len(queries_u8)
    z = np.array(z_init, np.float32).reshape(Q, -1)
    sig = np.full(Q, sigma, np.float32)
    S, _ = group_min_keys(matrix(queries_u8, generate(z)), 1)
    trace = [S.copy()]
    for r in range(1, rounds + 1):
        cz = pc.candidates(z, sig, lam, seed, r, query_base, Z_MAX)
        S_new, j_new = group_min_keys(matrix(queries_u8, generate(cz)), lam)
        z, sig, S, _ = pc.accept(z, sig, S, cz, S_new, j_new, lam, UP, DOWN, SIGMA_MIN, SIGMA_MAX)
        trace.append(S.copy())
    return z, S, np.stack(trace)
