"""Cases, host references and the GPU entry of the per-kernel tests of the attention backward (csrc/gl_attention_grad.hip: attention_grad_rows_kernel<C>
then attention_grad_cols_kernel<C>, one launch sequence through gl_tune_attention_grad of the tuning build).  No GPU needed to import.

Per image of T = 256 positions, from fp32 rows [position][q | k | v] (q, k: DK = C / 8 channels, v: C) and dY [position][C], the gradient with respect
to y = gamma * out + x of the forward (tests/attention_common.py):
    P = softmax_j(q_i . k_j),  dO = gamma dY,  dV_j = sum_i P_ij dO_i,  dP_ij = dO_i . v_j,  D_i = sum_j P_ij dP_ij,  dE_ij = P_ij (dP_ij - D_i),
    dq_i = sum_j dE_ij k_j,  dk_j = sum_i dE_ij q_i
The kernels write rows [dq | dk | dv | zero columns up to a multiple of 32] and the statistics (m_i, 1 / l_i, D_i).

Every case has n = 3 images, image 2 equal to image 0 (equal outputs bit for bit, and equal to the n = 1 run of image 0).  Exact cases are built
so that every value the kernels can form, in any order, is exactly representable (tests/test_attention_grad_cpu.py asserts the preconditions);
real-valued cases come with the float64 formulas, a float32 torch autograd evaluation of the same graph and a host-side allowance for the hardware
exponential.
"""
import ctypes
import zlib

import numpy as np

import attention_common as ac

T, N_IMG, GUARD, SENTINEL, POISON, SLACK = ac.T, ac.N_IMG, ac.GUARD, ac.SENTINEL, ac.POISON, ac.SLACK
PARTS = ("dq", "dk", "dv")


class Case:
    def __init__(self, kind, C, gamma, temp=None):
        self.kind, self.C, self.gamma, self.temp = kind, C, float(gamma), temp
        self.DK = C // 8
        self.cols = -(-(2 * self.DK + C) // 32) * 32
        self.base = kind + ("_%s" % temp if temp else "")
        self.name = "%s_c%d" % (self.base, C)
        self.exact = kind != "real"

    def __repr__(self):
        return self.name


ALL_CASES = []
for _C in (64, 128):
    ALL_CASES += [Case("uniform", _C, 0.5), Case("onehot", _C, 2.0), Case("gamma0", _C, 0.0, temp="mild"),
                  Case("real", _C, 0.7, temp="mild"), Case("real", _C, 0.7, temp="peaked")]
EXACT_CASES = [c for c in ALL_CASES if c.exact]
REAL_CASES = [c for c in ALL_CASES if not c.exact]
BY_NAME = {c.name: c for c in ALL_CASES}


def _small_ints(rng, shape):
    return rng.integers(1, 9, shape).astype(np.float32) * rng.choice([-1.0, 1.0], shape).astype(np.float32)


def make_inputs(c):
    """dict(q [n][T][DK], k, v [n][T][C], dY [n][T][C]) float32"""
    rng = np.random.default_rng(zlib.crc32(("grad_" + c.base).encode()) + c.C)
    n, C, DK = N_IMG, c.C, c.DK
    if c.kind in ("uniform", "onehot"):
        q, k = np.zeros((n, T, DK), np.float32), np.zeros((n, T, DK), np.float32)
        v, dY = _small_ints(rng, (n, T, C)), _small_ints(rng, (n, T, C))
        if c.kind == "onehot":
            for img in range(n):
                k[img, :, :8] = 8 * ac.code(np.arange(T))
                q[img, :, :8] = 8 * ac.code(ac.perm(img))
    else:
        s = np.sqrt(ac.TEMPS[c.temp] / np.sqrt(DK))
        q = (rng.standard_normal((n, T, DK)) * s).astype(np.float32)
        k = (rng.standard_normal((n, T, DK)) * s).astype(np.float32)
        v = rng.standard_normal((n, T, C)).astype(np.float32)
        dY = rng.standard_normal((n, T, C)).astype(np.float32)
    d = {"q": q, "k": k, "v": v, "dY": dY}
    for a in d.values():
        a[2] = a[0]
    return d


def backward64(c, d, full=False):
    """the hand-written formulas in float64 -> dict(dq, dk, dv) (and, with full, P, t = energy - row max, dP, D, dE)"""
    q, k, v, dY = (d[n].astype(np.float64) for n in ("q", "k", "v", "dY"))
    e = np.einsum("nid,njd->nij", q, k)
    t = e - e.max(axis=2, keepdims=True)
    P = np.exp(t)
    P /= P.sum(axis=2, keepdims=True)
    dO = c.gamma * dY
    dv = np.einsum("nij,nic->njc", P, dO)
    dP = np.einsum("nic,njc->nij", dO, v)
    D = (P * dP).sum(axis=2, keepdims=True)
    dE = P * (dP - D)
    out = {"dq": np.einsum("nij,njd->nid", dE, k), "dk": np.einsum("nij,nid->njd", dE, q), "dv": dv}
    if full:
        out.update(P=P, t=t, dP=dP, D=D, dE=dE, dO=dO)
    return out


def autograd(c, d, dtype):
    """torch autograd of y = gamma * softmax(q k^T) v (+ x, which has no part in these gradients) in `dtype` -> dict(dq, dk, dv) as float64 arrays"""
    import torch
    q, k, v = (torch.from_numpy(np.array(d[n])).to(dtype).requires_grad_(True) for n in ("q", "k", "v"))
    y = torch.tensor(c.gamma, dtype=dtype) * torch.bmm(torch.softmax(torch.bmm(q, k.transpose(1, 2)), dim=-1), v)
    g = torch.autograd.grad(y, (q, k, v), torch.from_numpy(np.array(d["dY"])).to(dtype))
    return {n: a.numpy().astype(np.float64) for n, a in zip(PARTS, g)}


def closed_form(c, d):
    """what an exact case must give, written without a softmax (float64)"""
    dY = d["dY"].astype(np.float64)
    out = {"dq": np.zeros((N_IMG, T, c.DK)), "dk": np.zeros((N_IMG, T, c.DK)), "dv": np.zeros((N_IMG, T, c.C))}
    if c.kind == "uniform":
        out["dv"][:] = c.gamma / 256.0 * dY.sum(axis=1, keepdims=True)
    elif c.kind == "onehot":
        for img in range(N_IMG):
            out["dv"][img, ac.perm(img)] = c.gamma * dY[img]
    return out


def exactness_problems(c, d):
    """why an exact case might not be exact on the device: empty list = every intermediate value is a float32 in any order of summation"""
    bad = []
    if c.kind == "gamma0":
        return bad if c.gamma == 0.0 and all(np.isfinite(a).all() for a in d.values()) else ["gamma0 needs gamma = 0 and finite inputs"]
    q, k, v, dY = (d[n].astype(np.float64) for n in ("q", "k", "v", "dY"))
    for name, a in (("q", q), ("k", k), ("v", v), ("dY", dY)):
        if not np.array_equal(a, np.round(a)):
            bad.append(name + " is not integer")
    if np.frexp(abs(c.gamma))[0] != 0.5:
        bad.append("gamma is no power of two")
    if not np.einsum("nid,njd->nij", np.abs(q), np.abs(k)).max() < 2.0 ** 24:
        bad.append("sum of absolute q k products not below 2^24")
    dO = np.abs(c.gamma * dY)
    # dP: sums of integer (or half-integer) products; D and dV: sums of 256 of those, scaled by 1 / 256 or picked out by a one-hot row
    if not 2 * np.einsum("nic,njc->nij", dO, np.abs(v)).max() * 256 < 2.0 ** 24:
        bad.append("256 x the sum of absolute dO v products (in halves) not below 2^24")
    if not 2 * dO.sum(axis=1).max() < 2.0 ** 24:
        bad.append("sum of |dO| over i (in halves) not below 2^24")
    f = backward64(c, d, full=True)
    if c.kind == "uniform":
        if not (np.array_equal(q, np.zeros_like(q)) and np.array_equal(k, np.zeros_like(k)) and np.array_equal(f["P"], np.full_like(f["P"], 1.0 / 256))):
            bad.append("attention not uniform")
    else:
        e = np.einsum("nid,njd->nij", q, k)
        top2 = np.sort(e, axis=2)[:, :, -2:]
        if not ((top2[:, :, 1] - top2[:, :, 0]) >= ac.EXP_ZERO_GAP).all():
            bad.append("runner-up energy within %d of the maximum: its weight is not 0 in float32" % ac.EXP_ZERO_GAP)
        for img in range(N_IMG):
            if not np.array_equal(e[img].argmax(axis=1), ac.perm(img)):
                bad.append("the maximum of row i is not at perm(i)")
    want = closed_form(c, d)
    for n in PARTS:
        if not np.allclose(f[n], want[n], rtol=0, atol=1e-9):
            bad.append(n + ": closed form and float64 formulas disagree")
        if not np.array_equal(want[n].astype(np.float32).astype(np.float64), want[n]):
            bad.append(n + ": result not a float32")
    return bad


def exp_allowance(c, d, f=None, per_position=False):
    """The allowance for the hardware exponential, derived as attention_common.exp_allowance derives the forward's: a weight formed as
    exp2(fl32(t log2 e)), t = e - max <= 0, has relative error at most eps_ij = (|t_ij| + 1) 2^-23.  After the normalisation the probability moves by
    dP'_ij = P_ij (delta_ij - sum_k P_ik delta_ik), |dP'_ij| <= W_ij = P_ij (eps_ij + sum_k P_ik eps_ik), and to first order
        |d dv_jc| <= sum_i W_ij |dO_ic|,   |d D_i| <= B_i = sum_k W_ik |dP_ik - D_i|,   |d dE_ij| <= A_ij = W_ij |dP_ij - D_i| + P_ij B_i,
        |d dq_id| <= sum_j A_ij |k_jd|,    |d dk_jd| <= sum_i A_ij |q_id|
    -> dict(dq, dk, dv) of per-image values in the row metric, |bound|_2 / |reference|_2; per_position: the largest such value over the positions,
    each with the norms over its own channels"""
    f = f if f is not None else backward64(c, d, full=True)
    q, k = np.abs(d["q"].astype(np.float64)), np.abs(d["k"].astype(np.float64))
    eps = (np.abs(f["t"]) + 1.0) * 2.0 ** -23
    W = f["P"] * (eps + (f["P"] * eps).sum(axis=2, keepdims=True))
    dev = np.abs(f["dP"] - f["D"])
    A = W * dev + f["P"] * (W * dev).sum(axis=2, keepdims=True)
    bound = {"dv": np.einsum("nij,nic->njc", W, np.abs(f["dO"])), "dq": np.einsum("nij,njd->nid", A, k), "dk": np.einsum("nij,nid->njd", A, q)}
    if per_position:
        return {n: float((np.linalg.norm(bound[n], axis=2) / np.linalg.norm(f[n], axis=2)).max()) for n in PARTS}
    return {n: np.linalg.norm(bound[n].reshape(N_IMG, -1), axis=1) / np.linalg.norm(f[n].reshape(N_IMG, -1), axis=1) for n in PARTS}


def row_errors(got, want64):
    return ac.row_errors(got, want64)


def position_error(got, want64):
    """the same metric position by position, |g_i - g64_i|_2 / |g64_i|_2 over the channels of one query / key position: the largest of all positions"""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    return float((np.linalg.norm(got - want64, axis=2) / np.linalg.norm(want64, axis=2)).max())


# ------------------------------------------------------------------------------------------------------------ the GPU entry
class TuneAttentionGrad(ctypes.Structure):          # csrc/gl_tune.hip GlTuneAttentionGrad
    _fields_ = [("C", ctypes.c_int32), ("cols", ctypes.c_int32), ("n_img", ctypes.c_int64),
                ("gamma", ctypes.c_float), ("poison", ctypes.c_float), ("sentinel", ctypes.c_int32), ("reserved_i", ctypes.c_int32),
                ("qkv", ctypes.c_void_p), ("dY", ctypes.c_void_p), ("dqkv", ctypes.c_void_p), ("stats", ctypes.c_void_p),
                ("out_guards", ctypes.c_void_p)]


def run_attention_grad(lib, ctx_handle, c, d, imgs):
    """one launch sequence through gl_tune_attention_grad on the images `imgs`
    -> dict(dqkv float32 [n][T][cols], stats float32 [n][3][T], guards = 4 x bytes)"""
    imgs = list(imgs)
    n = len(imgs)
    qkv = np.ascontiguousarray(np.concatenate([d["q"][imgs], d["k"][imgs], d["v"][imgs]], axis=2), np.float32)
    dY = np.ascontiguousarray(d["dY"][imgs], np.float32)
    assert qkv.shape == (n, T, 2 * c.DK + c.C) and dY.shape == (n, T, c.C)
    dqkv = np.empty((n, T, c.cols), np.float32)
    stats = np.empty((n, 3, T), np.float32)
    og = np.empty(4 * GUARD, np.uint8)
    a = TuneAttentionGrad()
    a.C, a.cols, a.n_img, a.gamma, a.poison, a.sentinel = c.C, 0, n, c.gamma, POISON, SENTINEL
    a.qkv, a.dY, a.dqkv, a.stats, a.out_guards = qkv.ctypes.data, dY.ctypes.data, dqkv.ctypes.data, stats.ctypes.data, og.ctypes.data
    lib.gl_tune_attention_grad.restype = ctypes.c_int
    lib.gl_tune_attention_grad.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    rc = lib.gl_tune_attention_grad(ctx_handle, ctypes.byref(a))
    if rc != 0:
        lib.gl_last_error.restype = ctypes.c_char_p
        raise RuntimeError("gl_tune_attention_grad(%s): %s" % (c.name, lib.gl_last_error().decode()))
    assert a.cols == c.cols, (a.cols, c.cols)
    return {"dqkv": dqkv, "stats": stats, "guards": tuple(og[i * GUARD:(i + 1) * GUARD].tobytes() for i in range(4))}


def split(c, dqkv):
    """rows [dq | dk | dv | pad] -> dict(dq, dk, dv, pad)"""
    DK, C = c.DK, c.C
    return {"dq": dqkv[..., :DK], "dk": dqkv[..., DK:2 * DK], "dv": dqkv[..., 2 * DK:2 * DK + C], "pad": dqkv[..., 2 * DK + C:]}
