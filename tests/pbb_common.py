"""Host restatements for the partial-black-box attack (csrc/gl_pbb.hip, ganleaks_amd/pbb.py): Philox4x32-10 on uint64 lanes, the
Irwin-Hall noise, the candidates, the grouped exact distance and the (1 + lambda) accept rule, in numpy.  Nothing here imports the product;
the constants are written out again on purpose."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
SH = np.uint64(32)
# float32(1 / (65536 sqrt(8/3))): t = 2 sum(h) - 524280 has variance (8/3) 65536^2 (eight uniform 16-bit halves, doubled)
C = np.float32(1.0 / (65536.0 * np.sqrt(8.0 / 3.0)))


def philox4x32_10(counter, key):
    """counter: 4 arrays (broadcastable) of 32-bit values, key: 2 -> 4 uint64 arrays holding the 32-bit output words"""
    c = [np.asarray(v, np.uint64) & MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.asarray(v, np.uint64) & MASK for v in key)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                     # 32 x 32 -> 64 bits: no overflow on uint64 lanes
        c = [((p1 >> SH) ^ c[1] ^ k0) & MASK, p1 & MASK, ((p0 >> SH) ^ c[3] ^ k1) & MASK, p0 & MASK]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def noise_t(seed, rnd, query, j, c):
    """the integer t = 2 sum(h0..h7) - 524280 behind eps, int32, any broadcastable index arrays"""
    seed = int(seed)
    w = philox4x32_10((c, j, np.asarray(query, np.uint64) & MASK, rnd), (seed & 0xFFFFFFFF, seed >> 32))
    total = np.zeros(w[0].shape, np.int64)
    for x in w:
        total += (x & np.uint64(0xFFFF)).astype(np.int64) + (x >> np.uint64(16)).astype(np.int64)
    return (2 * total - 524280).astype(np.int32)


def noise(seed, rnd, query, j, c):
    """eps = fl32(float(t) * C)"""
    return noise_t(seed, rnd, query, j, c).astype(np.float32) * C


def candidates(z, sigma, lam, seed, rnd, query_base, z_max):
    """[nq * lam, nz] float32: clamp(fl32(z + fl32(sigma * eps)), -z_max, z_max), every operation a float32 one"""
    z = np.asarray(z, np.float32)
    nq, nz = z.shape
    q = (query_base + np.arange(nq, dtype=np.uint64))[:, None, None]
    eps = noise(seed, rnd, q, np.arange(lam, dtype=np.uint64)[None, :, None], np.arange(nz, dtype=np.uint64)[None, None, :])
    step = np.asarray(sigma, np.float32)[:, None, None] * eps
    assert step.dtype == np.float32
    out = z[:, None, :] + step
    assert out.dtype == np.float32
    zm = np.float32(z_max)
    return np.minimum(np.maximum(out, -zm), zm).reshape(nq * lam, nz)


def group_min(queries, cand, lam):
    """exact S = sum (a - b)^2 of every query against its own lam rows: (S int64 [nq], j int32 [nq], all S [nq, lam]); first minimum"""
    q = np.asarray(queries).reshape(len(queries), -1).astype(np.int64)
    c = np.asarray(cand).reshape(len(q), lam, -1).astype(np.int64)
    S = ((c - q[:, None, :]) ** 2).sum(axis=2)
    j = S.argmin(axis=1)
    return S[np.arange(len(q)), j], j.astype(np.int32), S


def accept(z, sigma, S_cur, cand_z, S_new, j_new, lam, up, down, sigma_min, sigma_max):
    """the elitist step: strict <, float32 sigma updates and clamps -> (z, sigma, S_cur, accepted), new arrays"""
    z, sigma, S_cur = np.array(z, np.float32), np.array(sigma, np.float32), np.array(S_cur, np.int64)
    take = np.asarray(S_new, np.int64) < S_cur
    rows = np.asarray(cand_z, np.float32).reshape(len(z), lam, -1)[np.arange(len(z)), j_new]
    z[take] = rows[take]
    S_cur[take] = np.asarray(S_new, np.int64)[take]
    s = sigma * np.where(take, np.float32(up), np.float32(down)).astype(np.float32)
    assert s.dtype == np.float32
    return z, np.minimum(np.maximum(s, np.float32(sigma_min)), np.float32(sigma_max)), S_cur, take


def search(queries, generate, z_init, rounds, lam, sigma, seed, up, down, sigma_min, sigma_max, z_max, query_base=0):
    """the whole attack on the host, `generate(z [n, nz]) -> u8 images` being the only outside call (one per round, all candidates):
    (z_star, S int64, trace int64 [rounds + 1, Q], sigma)"""
    z = np.array(z_init, np.float32).reshape(len(queries), -1)
    sig = np.full(len(z), sigma, np.float32)
    S, _, _ = group_min(queries, generate(z), 1)
    trace = [S.copy()]
    for r in range(1, rounds + 1):
        cz = candidates(z, sig, lam, seed, r, query_base, z_max)
        S_new, j_new, _ = group_min(queries, generate(cz), lam)
        z, sig, S, _ = accept(z, sig, S, cz, S_new, j_new, lam, up, down, sigma_min, sigma_max)
        trace.append(S.copy())
    return z, S, np.stack(trace), sig
