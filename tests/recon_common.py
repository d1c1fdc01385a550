"""Host restatements for the reconstruction attack (csrc/gl_pbb.hip gl_recon_latents / gl_pbb_group_S, ganleaks_amd/recon.py) in numpy, on
top of the partial-black-box restatement of the noise.  Nothing here imports the product."""
import numpy as np

import pbb_common as pc


def recon_latents(mu, std, lam, seed, query_base, z_max):
    """[nq * lam, nz] float32: clamp(fl32(mu + fl32(std * eps)), -z_max, z_max); eps = 0 for j = 0, else the round-0 noise of
    (seed, query_base + q, j, c); every operation a float32 one"""
    mu, std = np.asarray(mu, np.float32), np.asarray(std, np.float32)
    nq, nz = mu.shape
    q = (query_base + np.arange(nq, dtype=np.uint64))[:, None, None]
    eps = pc.noise(seed, 0, q, np.arange(lam, dtype=np.uint64)[None, :, None], np.arange(nz, dtype=np.uint64)[None, None, :])
    eps = np.array(eps, np.float32)
    eps[:, 0, :] = 0.0
    step = std[:, None, :] * eps
    assert step.dtype == np.float32
    out = mu[:, None, :] + step
    assert out.dtype == np.float32
    zm = np.float32(z_max)
    return np.minimum(np.maximum(out, -zm), zm).reshape(nq * lam, nz)


def group_S(queries, cand, lam):
    """exact S = sum (a - b)^2 of every query against its own lam rows, int64 [nq, lam]"""
    return pc.group_min(queries, cand, lam)[2]


def lattice(u8):
    """the float32 values the library reads bytes as: 2 * (u / 255.) - 1 in float64, rounded to float32"""
    return (2.0 * (np.asarray(u8).astype(np.float64) / 255.0) - 1.0).astype(np.float32)
