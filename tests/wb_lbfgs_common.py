"""Host restatements for L-BFGS in the white-box attack (csrc/gl_wb_lbfgs.hip, ganleaks_amd/wb.py optimizer='lbfgs'): push, direction, ladder
and advance in numpy float32 with every operation rounded on its own and the device's summation order, a textbook two-loop recursion in
float64, and a host search built on wb_common's torch module.  Nothing here imports the product."""
import numpy as np

import wb_common as wc

f32 = np.float32
STEEPEST, DROPPED = 1, 2                                 # the flag bits of include/ganleaks.h
FLT_MAX = f32(3.4028234663852886e38)

# the host search reaches a quarter of the starting S on the 2::3 queries of wb_common.search_latents() within wb_common.SEARCH_STEPS = 16
# gradient evaluations (tests/test_wb_lbfgs_cpu.py asserts it), so the step count of the Adam search test is kept
SEARCH_STEPS = wc.SEARCH_STEPS
MEMORY, LADDER, STEP0 = 8, 8, 1.0                        # wb_attack's defaults


def dot32(a, b):
    """the device's dot product: lane l adds fl(a[c] b[c]) for c = l, l + 64, ... in ascending order into a sum that starts at +0, then
    the 64 sums go through the butterfly v = fl(v + v[lane ^ o]), o = 32, 16, 8, 4, 2, 1"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    with np.errstate(all="ignore"):
        prod = a * b
        pad = (-len(prod)) % 64
        rows = np.concatenate([prod, np.zeros(pad, f32)]).reshape(-1, 64)      # x + (+0) = x for every x a sum that starts at +0 can hold
        acc = np.zeros(64, f32)
        for row in rows:
            acc = acc + row
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[lanes ^ o]
    assert acc.dtype == f32
    return acc[0]


def live(t):
    return bool(t > 0 and t <= FLT_MAX)


def pow2_neg(j):
    return f32(2.0 ** -int(j))


class State:
    """the per-query state of a block, as numpy arrays in the device's layout"""

    def __init__(self, z, m):
        nq, nz = z.shape
        self.m = m
        self.z = np.array(z, f32)
        self.z_prev, self.g_prev = np.zeros((nq, nz), f32), np.zeros((nq, nz), f32)
        self.S, self.Y = np.zeros((nq, m, nz), f32), np.zeros((nq, m, nz), f32)
        self.count, self.head = np.zeros(nq, np.int32), np.zeros(nq, np.int32)
        self.t = np.ones(nq, f32)
        self.flag = np.zeros(nq, np.uint8)

    def copy(self):
        other = State(self.z, self.m)
        for k, v in vars(self).items():
            setattr(other, k, v.copy() if isinstance(v, np.ndarray) else v)
        return other


def push(st, g, moved):
    """gl_wb_lbfgs_push, in place"""
    g = np.asarray(g, f32)
    with np.errstate(all="ignore"):
        for q in range(len(st.z)):
            if moved[q]:
                s, y = st.z[q] - st.z_prev[q], g[q] - st.g_prev[q]
                sy = dot32(s, y)
                rho = f32(1.0) / sy
                if sy > 0 and np.isfinite(rho):
                    h = int(st.head[q])
                    st.S[q, h], st.Y[q, h] = s, y
                    st.head[q] = (h + 1) % st.m
                    st.count[q] = min(int(st.count[q]) + 1, st.m)
            st.z_prev[q], st.g_prev[q] = st.z[q], g[q]


def direction(st, g, step0):
    """gl_wb_lbfgs_direction: -> p [nq, nz]; count, head, t and flag of st in place"""
    g = np.asarray(g, f32)
    p = np.zeros_like(g)
    with np.errstate(all="ignore"):
        for q in range(len(g)):
            if not live(st.t[q]):
                continue
            k, h, m = int(st.count[q]), int(st.head[q]), st.m
            was_steepest = bool(st.flag[q] & STEEPEST)
            two_loop, dropped = k > 0, False
            if two_loop:
                v = g[q].copy()
                rho, alpha = [None] * k, [None] * k
                gamma = None
                for i in range(k):
                    s, y = st.S[q, (h - 1 - i) % m], st.Y[q, (h - 1 - i) % m]
                    sy, sq = dot32(s, y), dot32(s, v)
                    if i == 0:
                        gamma = sy / dot32(y, y)
                    rho[i] = f32(1.0) / sy
                    alpha[i] = rho[i] * sq
                    v = v - alpha[i] * y
                v = gamma * v
                for i in range(k - 1, -1, -1):
                    s, y = st.S[q, (h - 1 - i) % m], st.Y[q, (h - 1 - i) % m]
                    beta = rho[i] * dot32(y, v)
                    v = v + s * (alpha[i] - beta)
                v = -v
                assert v.dtype == f32
                gp = dot32(g[q], v)
                if not np.isfinite(v).all() or not gp < 0 or not np.isfinite(gp):
                    two_loop, dropped = False, True
                p[q] = v
            if two_loop:
                st.t[q], st.flag[q] = f32(1.0), 0
            else:
                p[q] = -g[q]
                if not was_steepest:
                    st.t[q] = f32(step0) / np.sqrt(dot32(g[q], g[q]))
                st.flag[q] = STEEPEST | (DROPPED if dropped else 0)
                if dropped:
                    st.count[q] = st.head[q] = 0
    return p


def candidates(z, p, t, L, z_max):
    """gl_wb_lbfgs_candidates -> [nq * L, nz]"""
    z, p, zm = np.asarray(z, f32), np.asarray(p, f32), f32(z_max)
    out = np.empty((len(z), L, z.shape[1]), f32)
    with np.errstate(all="ignore"):
        for q in range(len(z)):
            for j in range(L):
                if not live(t[q]):
                    out[q, j] = z[q]
                    continue
                w = f32(t[q]) * pow2_neg(j)
                v = z[q] + w * p[q]
                out[q, j] = np.minimum(np.maximum(v, -zm), zm)
    return out.reshape(len(z) * L, -1)


def advance(st, accepted, j_new, L):
    """gl_wb_lbfgs_advance, in place"""
    with np.errstate(all="ignore"):
        for q in range(len(st.t)):
            if not live(st.t[q]):
                continue
            steepest = bool(st.flag[q] & STEEPEST)
            if accepted[q]:
                if steepest and 0 <= j_new[q] < L:
                    st.t[q] = (f32(2.0) * st.t[q]) * pow2_neg(j_new[q])
            elif steepest:
                st.t[q] = st.t[q] * pow2_neg(L)
            else:
                st.count[q] = st.head[q] = 0


def two_loop64(S, Y, g):
    """the textbook two-loop recursion in float64: S, Y [k, nz] with the NEWEST pair first -> -H g"""
    S, Y, v = np.asarray(S, np.float64), np.asarray(Y, np.float64), np.array(g, np.float64)
    rho = [1.0 / (s @ y) for s, y in zip(S, Y)]
    alpha = []
    for i in range(len(S)):
        alpha.append(rho[i] * (S[i] @ v))
        v = v - alpha[i] * Y[i]
    v = (S[0] @ Y[0]) / (Y[0] @ Y[0]) * v
    for i in range(len(S) - 1, -1, -1):
        v = v + S[i] * (alpha[i] - rho[i] * (Y[i] @ v))
    return -v


def ring_rows(st, q):
    """(S, Y) of query q, newest pair first"""
    k, h, m = int(st.count[q]), int(st.head[q]), st.m
    slots = [(h - 1 - i) % m for i in range(k)]
    return st.S[q, slots], st.Y[q, slots]


def quadratic(seed, nz, nq=4):
    """nq problems f(z) = z'Az / 2 - b'z: A with eigenvalues linspace(1, 10, nz) in a random orthogonal basis; -> (A [nq,nz,nz], b, z0) float64"""
    rng = np.random.default_rng(seed)
    A = np.empty((nq, nz, nz))
    for q in range(nq):
        basis, _ = np.linalg.qr(rng.standard_normal((nz, nz)))
        A[q] = (basis * np.linspace(1.0, 10.0, nz)) @ basis.T
    return A, rng.standard_normal((nq, nz)), rng.standard_normal((nq, nz))


def quadratic_run(A, b, z0, m, steps, push_fn, direction_fn, candidates_fn):
    """the protocol of the finite-termination test: g = Az - b in float64 from the float32 iterate, handed over as float32; push and
    direction by the functions given; the exact step t = -g.p / p'Ap through candidates_fn with L = 1; every step moves.
    push_fn(z, g, moved), direction_fn(g) -> p, candidates_fn(z, p, t) -> the new z, all float32 arrays.  -> |g_steps| / |g_0| per query"""
    z = np.asarray(z0, f32)
    grad = lambda z: np.einsum("qij,qj->qi", A, z.astype(np.float64)) - b          # noqa: E731
    g0 = np.linalg.norm(grad(z), axis=1)
    moved = np.zeros(len(z), np.uint8)
    for _ in range(steps):
        g = grad(z)
        g32 = g.astype(f32)
        push_fn(z, g32, moved)
        p = direction_fn(g32).astype(np.float64)
        t = -(g * p).sum(axis=1) / np.einsum("qi,qij,qj->q", p, A, p)
        z = candidates_fn(z, p.astype(f32), t.astype(f32))
        moved[:] = 1
    return np.linalg.norm(grad(z), axis=1) / g0


def quadratic_host(A, b, z0, m, steps):
    """quadratic_run on the float32 restatement"""
    st = State(np.asarray(z0, f32), m)

    def push_fn(z, g, moved):
        st.z = z
        push(st, g, moved)

    return quadratic_run(A, b, z0, m, steps, push_fn, lambda g: direction(st, g, 1.0),
                         lambda z, p, t: candidates(z, p, t, 1, 1e6))


def search(queries_u8, net, z_init, steps, memory=MEMORY, ladder=LADDER, step0=STEP0, z_max=4.0):
    """the whole attack on the host, mirroring wb_common.search: float64 autograd gradients, the float32 restatement above, 8-bit images of
    the host module, exact S; the iterate is itself the best so far -> (z float32, S int64, trace int64 [steps + 1, Q])"""
    q = np.asarray(queries_u8).reshape(len(queries_u8), -1)
    st = State(np.array(z_init, f32).reshape(len(q), -1), memory)
    S = wc.ssd(wc.quantize_u8(wc.forward(net, st.z)), q)
    trace = [S.copy()]
    accepted = np.zeros(len(q), np.uint8)
    for _ in range(steps):
        g, _ = wc.l2_grad_z(net, st.z, q)
        g = g.astype(f32)
        push(st, g, accepted)
        p = direction(st, g, step0)
        cand = candidates(st.z, p, st.t, ladder, z_max)
        S_all = wc.ssd(wc.quantize_u8(wc.forward(net, cand)), np.repeat(q, ladder, axis=0)).reshape(len(q), ladder)
        j_new = S_all.argmin(axis=1)                                               # the smallest j that attains the minimum
        S_new = S_all[np.arange(len(q)), j_new]
        accepted = (S_new < S).astype(np.uint8)
        take = accepted.astype(bool)
        st.z[take] = cand.reshape(len(q), ladder, -1)[take, j_new[take]]
        S = np.where(take, S_new, S)
        advance(st, accepted, j_new, ladder)
        trace.append(S.copy())
    return st.z.copy(), S, np.stack(trace)
