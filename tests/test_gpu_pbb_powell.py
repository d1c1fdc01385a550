"""GPU: Powell's method in the partial-black-box attack (csrc/gl_pbb_powell.hip, ganleaks_amd/pbb.py optimizer='powell') -- the seven
entry points bit for bit against the numpy restatement of tests/pbb_powell_common.py with every array inside sentinel guards, the refusals
of the C ABI, and pbb_attack on the suite's small DCGAN against the restatement driven from the host, which scores with the device's own
generate_u8 and gl_pbb_group_min.  The evolution strategy must be what it was."""
import ctypes

import numpy as np
import pytest

import gpu_common  # noqa: F401
import pbb_powell_common as pc
import wb_common as wc

pytestmark = pytest.mark.gpu
_p = ctypes.c_void_p
_f = ctypes.c_float
f32 = np.float32
GUARD = 4096                     # bytes of sentinel on each side of a guarded device buffer
SENT8 = 0xA5
T_MIN, T_MAX, Z_MAX = 1e-4, 4.0, 4.0


@pytest.fixture(scope="module")
def gl():
    import ganleaks_amd
    return ganleaks_amd


@pytest.fixture(scope="module")
def small(gl):
    from ganleaks_amd.gan_models.dcgan.model_torch import Generator
    gen = Generator(100, 3, 16)
    gen.load_state_dict(gl.synth.dcgan_state_dict(1234, z_dim=100, features_g=16))
    return gen


class Guarded:
    """a host array on the device between two sentinel guards; numpy() reads it back and checks the guards"""

    def __init__(self, ctx, host):
        host = np.ascontiguousarray(host)
        self.shape, self.dtype, self.count = host.shape, host.dtype, host.nbytes
        raw = np.full(2 * GUARD + self.count, SENT8, np.uint8)
        raw[GUARD:GUARD + self.count] = host.reshape(-1).view(np.uint8)
        self.buf = ctx.to_device(raw)
        self.ptr = self.buf.ptr + GUARD

    def numpy(self):
        raw = self.buf.numpy()
        assert (raw[:GUARD] == SENT8).all() and (raw[GUARD + self.count:] == SENT8).all() and len(raw) == 2 * GUARD + self.count, "a guard was written"
        return raw[GUARD:GUARD + self.count].view(self.dtype).reshape(self.shape).copy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == f32 else (a.view(np.uint64) if a.dtype == np.float64 else a)


class Dev:
    """the state of pc.State on the device, every array guarded, and the calls on it"""

    def __init__(self, gl, st):
        from ganleaks_amd._lib import check
        self.check = check
        self.ctx = gl.Context.get()
        self.lib, self.h = self.ctx.lib, self.ctx.handle
        self.nq, self.nz = st.z.shape
        for name in pc.State.NAMES:
            setattr(self, name, Guarded(self.ctx, getattr(st, name)))
        self.one = Guarded(self.ctx, np.ones(self.nq, f32))

    def same(self, st, where):
        for name in pc.State.NAMES:
            assert np.array_equal(_bits(getattr(self, name).numpy()), _bits(getattr(st, name))), (name, where)
        assert np.array_equal(self.one.numpy(), np.ones(self.nq, f32)), where

    def begin(self):
        self.check(self.lib.gl_pbb_powell_begin(self.h, _p(self.z.ptr), _p(self.S_cur.ptr), _p(self.z0.ptr), _p(self.f0.ptr), _p(self.S_prev.ptr),
                                                _p(self.drop_best.ptr), _p(self.i_best.ptr), self.nq, self.nz))

    def candidates(self, line, L):
        self.cand = Guarded(self.ctx, np.full((self.nq * L, self.nz), np.nan, f32))
        self.check(self.lib.gl_pbb_powell_candidates(self.h, _p(self.z.ptr), _p(self.U.ptr), _p(self.t.ptr), self.nq, self.nz, line, L, _f(Z_MAX),
                                                     _p(self.cand.ptr)))
        return self.cand.numpy()

    def accept_and_advance(self, S_new, j_new, line, L, kind):
        """gl_pbb_accept as _powell_block calls it, then gl_pbb_powell_advance -> accepted"""
        S_new, j_new = Guarded(self.ctx, np.asarray(S_new, np.uint64)), Guarded(self.ctx, np.asarray(j_new, np.int32))
        accepted = Guarded(self.ctx, np.full(self.nq, 7, np.uint8))
        self.check(self.lib.gl_pbb_accept(self.h, _p(self.z.ptr), _p(self.one.ptr), _p(self.S_cur.ptr), _p(self.cand.ptr), _p(S_new.ptr), _p(j_new.ptr),
                                          self.nq, self.nz, L, _f(1.0), _f(1.0), _f(1.0), _f(1.0), _p(accepted.ptr)))
        took = accepted.numpy()
        self.check(self.lib.gl_pbb_powell_advance(self.h, _p(self.t.ptr), _p(accepted.ptr), _p(j_new.ptr), _p(self.S_cur.ptr), _p(self.S_prev.ptr),
                                                  _p(self.drop_best.ptr), _p(self.i_best.ptr), self.nq, self.nz, line, L, kind, _f(T_MIN), _f(T_MAX)))
        assert np.array_equal(accepted.numpy(), took)                    # advance reads them
        return took

    def extrapolate(self):
        z_e = Guarded(self.ctx, np.full((self.nq, self.nz), np.nan, f32))
        self.check(self.lib.gl_pbb_powell_extrapolate(self.h, _p(self.z.ptr), _p(self.z0.ptr), _p(self.U.ptr), self.nq, self.nz, _f(Z_MAX), _p(z_e.ptr)))
        return z_e.numpy()

    def decide(self, kind):
        self.check(self.lib.gl_pbb_powell_decide(self.h, _p(self.U.ptr), _p(self.t.ptr), _p(self.f0.ptr), _p(self.S_cur.ptr), _p(self.S_e.ptr),
                                                 _p(self.drop_best.ptr), _p(self.flag.ptr), self.nq, self.nz, kind))

    def replace(self):
        self.check(self.lib.gl_pbb_powell_replace(self.h, _p(self.U.ptr), _p(self.t.ptr), _p(self.flag.ptr), _p(self.i_best.ptr), self.nq, self.nz))


def _keys(values, kind):
    """the keys of these scores: the integers themselves, or the patterns of the float32 values / 8"""
    values = np.asarray(values, np.int64)
    if kind:
        return (values.astype(f32) / f32(8.0)).view(np.uint32).astype(np.uint64)
    return values.astype(np.uint64)


# one element, fewer than a wave, exactly one wave, one past it, ragged tails of 36 and 44 with several elements per lane
@pytest.mark.parametrize("nq,nz", [(1, 1), (3, 3), (5, 64), (4, 65), (2, 100), (2, 300)])
@pytest.mark.parametrize("L", [2, 8, 32])
def test_bit_for_bit(gl, nq, nz, L):
    from ganleaks_amd._lib import check
    ctx = gl.Context.get()
    kind = 1 if L == 32 else 0                                           # float32 patterns as keys on one ladder, exact integers on the others
    rng = np.random.default_rng(1000 * nz + 10 * nq + L)
    # init, over garbage
    U, t = Guarded(ctx, np.full((nq, nz + 1, nz), np.nan, f32)), Guarded(ctx, np.full((nq, nz + 1), np.nan, f32))
    check(ctx.lib.gl_pbb_powell_init(ctx.handle, _p(U.ptr), _p(t.ptr), nq, nz, _f(0.75)))
    U0, t0 = pc.init(nq, nz, 0.75)
    assert np.array_equal(_bits(U.numpy()), _bits(U0)) and np.array_equal(_bits(t.numpy()), _bits(t0))
    # a state in the middle of a search: directions that are no unit vectors, widths that are no powers of two
    st = pc.State(rng.uniform(-1.0, 1.0, (nq, nz)).astype(f32))
    st.U = rng.standard_normal((nq, nz + 1, nz)).astype(f32)
    st.U[rng.random(st.U.shape) < 0.2] = 0.0
    st.t = rng.uniform(0.01, 3.0, (nq, nz + 1)).astype(f32)
    st.U[:, 0, 0] = f32(1.0)                                             # whoever is accepted on line 0 moves
    st.z[0, 0], st.t[0, 0] = f32(3.9), f32(3.5)                          # the clamp of the candidates, and t_max after an accepted rung 0
    if nq > 1:
        st.t[1, 0] = f32(1.5e-4)                                         # t_min after a rejected ladder: query 1 is rejected on line 0
    vals = np.full(nq, 1000, np.int64)
    st.S_cur = _keys(vals, kind)
    st.z0[:], st.f0[:], st.S_prev[:], st.S_e[:], st.drop_best[:], st.i_best[:], st.flag[:] = 9.0, 9, 9, 9, 9.0, 9, 9
    dev = Dev(gl, st)
    pc.begin(st)
    dev.begin()
    dev.same(st, "begin")
    q = np.arange(nq)
    clamped = False

    def line(i, take, drop):
        nonlocal vals, clamped
        cand = pc.candidates(st.z, st.U, st.t, i, L, Z_MAX)
        assert np.array_equal(_bits(dev.candidates(i, L)), _bits(cand)), ("candidates", i)
        clamped |= bool((np.abs(cand) == f32(Z_MAX)).any())
        assert np.abs(cand).max() <= Z_MAX
        j_new = rng.integers(0, L, size=nq).astype(np.int32)
        j_new[0] = 0
        new = np.where(take, vals - drop, vals + (q % 2))                # the rejected: equal (never strictly closer) or worse
        S_new = _keys(new, kind)
        accepted = pc.accept(st, cand, S_new, j_new, L)
        assert np.array_equal(accepted, take.astype(np.uint8))
        vals = np.where(take, new, vals)
        pc.advance(st, accepted, j_new, i, L, kind, T_MIN, T_MAX)
        assert np.array_equal(dev.accept_and_advance(S_new, j_new, i, L, kind), accepted)
        dev.same(st, ("line", i))

    line(0, q % 2 == 0, 300)
    assert st.t[0, 0] == f32(T_MAX) and clamped and (nq == 1 or st.t[1, 0] == f32(T_MIN))
    if nz > 1:
        line(nz - 1, q % 3 != 0, 400)
    z_e = pc.extrapolate(st, Z_MAX)
    assert np.array_equal(_bits(dev.extrapolate()), _bits(z_e))
    dev.same(st, "extrapolate")
    st.S_e = _keys(np.where(q % 2 == 0, 100, 2000), kind)
    dev.S_e = Guarded(ctx, st.S_e)
    pc.decide(st, kind)
    dev.decide(kind)
    dev.same(st, "decide")
    # the even queries moved on line 0 and their extrapolated point is closer: the test holds for them; the odd ones' fE is above f0
    assert st.flag.tolist() == [1 - (i % 2) for i in range(nq)] and st.t[:, nz].tolist() == [2.0 * (1 - (i % 2)) for i in range(nq)]
    assert st.i_best[0] == 0
    if nq >= 3 and nz > 1:
        assert st.i_best[2] == nz - 1 and st.flag[2] == 1               # the last line had the largest decrease, and the flag is set
    before = st.z.copy()
    line(nz, q % 3 != 2, 50)
    assert np.array_equal(st.z[st.flag == 0], before[st.flag == 0])      # a width of 0: whatever was accepted is the latent itself
    old_U, old_t = st.U.copy(), st.t.copy()
    pc.replace(st)
    dev.replace()
    dev.same(st, "replace")
    for i in range(nq):
        if st.flag[i]:
            assert np.array_equal(st.U[i, nz - 1], old_U[i, nz]) and st.t[i, nz - 1] == old_t[i, nz]
            if st.i_best[i] < nz - 1:
                assert np.array_equal(st.U[i, st.i_best[i]], old_U[i, nz - 1]) and st.t[i, st.i_best[i]] == old_t[i, nz - 1]
        else:
            assert np.array_equal(st.U[i], old_U[i]) and np.array_equal(st.t[i], old_t[i])


def test_abi_refusals(gl):
    from ganleaks_amd._lib import check
    ctx = gl.Context.get()
    lib, h = ctx.lib, ctx.handle
    nq, nz, L = 2, 5, 4
    a = ctx.zeros((nq * 8 * (nz + 1), nz), f32)
    k, dd = ctx.zeros((nq + 1,), np.uint64), ctx.zeros((nq + 1,), np.float64)
    i4, u1 = ctx.zeros((nq + 1,), np.int32), ctx.zeros((nq,), np.uint8)
    A, K, D, I, B, N = _p(a.ptr), _p(k.ptr), _p(dd.ptr), _p(i4.ptr), _p(u1.ptr), _p(0)
    A1, K4, D4, I1 = _p(a.ptr + 1), _p(k.ptr + 4), _p(dd.ptr + 4), _p(i4.ptr + 2)       # misaligned for their types
    one, lo, hi = _f(1.0), _f(1e-4), _f(4.0)
    nan, inf = _f(float("nan")), _f(float("inf"))
    big = 1 << 31
    # nothing to do: no pointer is touched
    check(lib.gl_pbb_powell_init(h, N, N, 0, nz, one))
    check(lib.gl_pbb_powell_begin(h, N, N, N, N, N, N, N, 0, nz))
    check(lib.gl_pbb_powell_candidates(h, N, N, N, 0, nz, 0, L, one, N))
    check(lib.gl_pbb_powell_advance(h, N, N, N, N, N, N, N, 0, nz, 0, L, 0, lo, hi))
    check(lib.gl_pbb_powell_extrapolate(h, N, N, N, 0, nz, one, N))
    check(lib.gl_pbb_powell_decide(h, N, N, N, N, N, N, N, 0, nz, 0))
    check(lib.gl_pbb_powell_replace(h, N, N, N, N, 0, nz))
    # and what the arguments allow runs
    check(lib.gl_pbb_powell_init(h, A, _p(a.ptr + 1024), nq, 1, one))
    ctx.sync()
    assert a.numpy().reshape(-1)[:4].tolist() == [1.0, 0.0, 1.0, 0.0] and a.numpy().reshape(-1)[256:260].tolist() == [1.0, 0.0, 1.0, 0.0]
    for call in (lambda: lib.gl_pbb_powell_init(None, A, A, nq, nz, one),
                 lambda: lib.gl_pbb_powell_init(h, A, A, -1, nz, one),
                 lambda: lib.gl_pbb_powell_init(h, A, A, big, nz, one),
                 lambda: lib.gl_pbb_powell_init(h, A, A, nq, 0, one),
                 lambda: lib.gl_pbb_powell_init(h, A, A, nq, big - 1, one),
                 lambda: lib.gl_pbb_powell_init(h, A, A, big - 1, big - 2, one),          # nq (nz + 1) nz overflows
                 lambda: lib.gl_pbb_powell_init(h, A, A, nq, nz, _f(0.0)),
                 lambda: lib.gl_pbb_powell_init(h, A, A, nq, nz, _f(-1.0)),
                 lambda: lib.gl_pbb_powell_init(h, A, A, nq, nz, nan),
                 lambda: lib.gl_pbb_powell_init(h, A, A, nq, nz, inf),
                 lambda: lib.gl_pbb_powell_init(h, N, A, nq, nz, one),
                 lambda: lib.gl_pbb_powell_init(h, A, N, nq, nz, one),
                 lambda: lib.gl_pbb_powell_init(h, A1, A, nq, nz, one),
                 lambda: lib.gl_pbb_powell_begin(None, A, K, A, K, K, D, I, nq, nz),
                 lambda: lib.gl_pbb_powell_begin(h, A, K, A, K, K, D, I, nq, 0),
                 lambda: lib.gl_pbb_powell_begin(h, A, K, A, K, K, D, I, big - 1, big - 2),
                 lambda: lib.gl_pbb_powell_begin(h, N, K, A, K, K, D, I, nq, nz),
                 lambda: lib.gl_pbb_powell_begin(h, A, K, A, K, K, N, I, nq, nz),
                 lambda: lib.gl_pbb_powell_begin(h, A, K4, A, K, K, D, I, nq, nz),
                 lambda: lib.gl_pbb_powell_begin(h, A, K, A, K, K, D4, I, nq, nz),
                 lambda: lib.gl_pbb_powell_begin(h, A, K, A, K, K, D, I1, nq, nz),
                 lambda: lib.gl_pbb_powell_candidates(None, A, A, A, nq, nz, 0, L, one, A),
                 lambda: lib.gl_pbb_powell_candidates(h, A, A, A, nq, nz, 0, 0, one, A),
                 lambda: lib.gl_pbb_powell_candidates(h, A, A, A, nq, nz, 0, 1, one, A),
                 lambda: lib.gl_pbb_powell_candidates(h, A, A, A, nq, nz, 0, 3, one, A),
                 lambda: lib.gl_pbb_powell_candidates(h, A, A, A, nq, nz, 0, 34, one, A),
                 lambda: lib.gl_pbb_powell_candidates(h, A, A, A, nq, nz, -1, L, one, A),
                 lambda: lib.gl_pbb_powell_candidates(h, A, A, A, nq, nz, nz + 1, L, one, A),
                 lambda: lib.gl_pbb_powell_candidates(h, A, A, A, nq, nz, 0, L, _f(0.0), A),
                 lambda: lib.gl_pbb_powell_candidates(h, A, A, A, nq, nz, 0, L, inf, A),
                 lambda: lib.gl_pbb_powell_candidates(h, A, A, A, nq, nz, 0, L, nan, A),
                 lambda: lib.gl_pbb_powell_candidates(h, A, A, N, nq, nz, 0, L, one, A),
                 lambda: lib.gl_pbb_powell_candidates(h, A, A, A, nq, nz, 0, L, one, N),
                 lambda: lib.gl_pbb_powell_candidates(h, A, A1, A, nq, nz, 0, L, one, A),
                 lambda: lib.gl_pbb_powell_candidates(h, A, A, A, big - 1, big - 2, 0, 32, one, A),
                 lambda: lib.gl_pbb_powell_advance(None, A, B, I, K, K, D, I, nq, nz, 0, L, 0, lo, hi),
                 lambda: lib.gl_pbb_powell_advance(h, A, B, I, K, K, D, I, nq, nz, 0, 5, 0, lo, hi),
                 lambda: lib.gl_pbb_powell_advance(h, A, B, I, K, K, D, I, nq, nz, 0, 34, 0, lo, hi),
                 lambda: lib.gl_pbb_powell_advance(h, A, B, I, K, K, D, I, nq, nz, nz + 1, L, 0, lo, hi),
                 lambda: lib.gl_pbb_powell_advance(h, A, B, I, K, K, D, I, nq, nz, 0, L, 2, lo, hi),
                 lambda: lib.gl_pbb_powell_advance(h, A, B, I, K, K, D, I, nq, nz, 0, L, -1, lo, hi),
                 lambda: lib.gl_pbb_powell_advance(h, A, B, I, K, K, D, I, nq, nz, 0, L, 0, _f(0.0), hi),
                 lambda: lib.gl_pbb_powell_advance(h, A, B, I, K, K, D, I, nq, nz, 0, L, 0, hi, lo),
                 lambda: lib.gl_pbb_powell_advance(h, A, B, I, K, K, D, I, nq, nz, 0, L, 0, lo, inf),
                 lambda: lib.gl_pbb_powell_advance(h, A, B, I, K, K, D, I, nq, nz, 0, L, 0, nan, hi),
                 lambda: lib.gl_pbb_powell_advance(h, A, N, I, K, K, D, I, nq, nz, 0, L, 0, lo, hi),
                 lambda: lib.gl_pbb_powell_advance(h, A, B, I, K, K, D, N, nq, nz, 0, L, 0, lo, hi),
                 lambda: lib.gl_pbb_powell_advance(h, A, B, I, K, K4, D, I, nq, nz, 0, L, 0, lo, hi),
                 lambda: lib.gl_pbb_powell_advance(h, A, B, I, K, K, D4, I, nq, nz, 0, L, 0, lo, hi),
                 lambda: lib.gl_pbb_powell_extrapolate(None, A, A, A, nq, nz, one, A),
                 lambda: lib.gl_pbb_powell_extrapolate(h, A, A, A, nq, 0, one, A),
                 lambda: lib.gl_pbb_powell_extrapolate(h, A, A, A, nq, nz, _f(0.0), A),
                 lambda: lib.gl_pbb_powell_extrapolate(h, A, A, A, nq, nz, inf, A),
                 lambda: lib.gl_pbb_powell_extrapolate(h, A, A, N, nq, nz, one, A),
                 lambda: lib.gl_pbb_powell_extrapolate(h, A, A, A, nq, nz, one, A1),
                 lambda: lib.gl_pbb_powell_extrapolate(h, A, A, A, big - 1, big - 2, one, A),
                 lambda: lib.gl_pbb_powell_decide(None, A, A, K, K, K, D, B, nq, nz, 0),
                 lambda: lib.gl_pbb_powell_decide(h, A, A, K, K, K, D, B, nq, nz, 2),
                 lambda: lib.gl_pbb_powell_decide(h, A, A, K, K, K, D, B, nq, 0, 0),
                 lambda: lib.gl_pbb_powell_decide(h, A, A, K, K, K, D, N, nq, nz, 0),
                 lambda: lib.gl_pbb_powell_decide(h, A, A, N, K, K, D, B, nq, nz, 0),
                 lambda: lib.gl_pbb_powell_decide(h, A, A, K, K, K4, D, B, nq, nz, 0),
                 lambda: lib.gl_pbb_powell_decide(h, A, A, K, K, K, D4, B, nq, nz, 0),
                 lambda: lib.gl_pbb_powell_decide(h, A, A, K, K, K, D, B, big - 1, big - 2, 0),
                 lambda: lib.gl_pbb_powell_replace(None, A, A, B, I, nq, nz),
                 lambda: lib.gl_pbb_powell_replace(h, A, A, B, I, nq, 0),
                 lambda: lib.gl_pbb_powell_replace(h, A, A, B, I, -1, nz),
                 lambda: lib.gl_pbb_powell_replace(h, N, A, B, I, nq, nz),
                 lambda: lib.gl_pbb_powell_replace(h, A, A, N, I, nq, nz),
                 lambda: lib.gl_pbb_powell_replace(h, A, A, B, I1, nq, nz),
                 lambda: lib.gl_pbb_powell_replace(h, A, A, B, I, big - 1, big - 2)):
        with pytest.raises(gl.GanLeaksError) as e:
            check(call())
        assert e.value.code == -1


Q, SWEEPS = 9, 2


def _driven(gl, gen, queries, z_init, sweeps, ladder, step0=1.0):
    """the restatement's search, scored by the device: generate_u8 on the uploaded candidates and gl_pbb_group_min on the result"""
    from ganleaks_amd._lib import check
    ctx = gen.ctx
    n = len(queries)
    q_dev = ctx.to_device(np.ascontiguousarray(queries).reshape(n, -1))
    d = q_dev.shape[1]
    S, j = ctx.empty((n,), np.uint64), ctx.empty((n,), np.int32)
    work = ctx.empty((16 * n * (-(-ladder // 16)),), np.uint8)

    def score(q, images, lam):
        assert images.dtype == np.uint8 and images.nbytes == n * lam * d
        check(ctx.lib.gl_pbb_group_min(ctx.handle, _p(q.ptr), _p(images.ptr), n, lam, d, _p(S.ptr), _p(j.ptr), _p(work.ptr)))
        return S.numpy(), j.numpy()

    return pc.search(q_dev, lambda lat: gen.generate_u8(np.ascontiguousarray(lat, f32)), score, z_init, sweeps=sweeps, ladder=ladder, step0=step0,
                     t_min=T_MIN, t_max=T_MAX, z_max=Z_MAX, kind=0)


@pytest.fixture(scope="module")
def attack_case(gl, small):
    """nine queries from the nearest of 128 bank latents: the attack's answer and the host-driven restatement's"""
    gen = small
    queries = gen.generate_u8(gl.synth.latent(81, Q)).numpy()
    z_bank = gl.synth.latent(82, 130).reshape(130, 100)
    z_init, _ = gl.pbb_init_from_bank(queries, gen, z_bank, batch_size=64)
    fbb_dist, _ = gl.attack(queries, gl.GeneratedBank(gen, z_bank), distance="l2", batch_size=64)
    got = gl.pbb_attack(queries, gen, z_init, optimizer="powell", sweeps=SWEEPS, history=True)
    want = _driven(gl, gen, queries, z_init, SWEEPS, 8)
    return gen, queries, z_init, fbb_dist, got, want


def test_attack_against_the_host_driven_restatement(attack_case):
    _, _, _, _, (dist, z_star, S, trace), (want_z, want_S, want_trace, st) = attack_case
    print("start", trace[0].tolist(), "final", S.tolist(), "flags of the last sweep", st.flag.tolist())
    assert np.array_equal(z_star.view(np.uint32), want_z.view(np.uint32)) and np.array_equal(S, want_S) and np.array_equal(trace, want_trace)


def test_attack_properties(gl, attack_case):
    from ganleaks_amd.attack import _dist32
    gen, queries, z_init, fbb_dist, (dist, z_star, S, trace), _ = attack_case
    assert trace.dtype == np.int64 and trace.shape == (SWEEPS + 1, Q) and S.dtype == np.int64 and S.shape == (Q,)
    assert dist.dtype == np.float32 and dist.shape == (Q,) and z_star.dtype == np.float32 and z_star.shape == (Q, 100)
    assert (np.diff(trace, axis=0) <= 0).all() and np.array_equal(trace[-1], S)
    assert np.array_equal(trace[0], wc.ssd(gen.generate_u8(z_init).numpy(), queries))
    assert np.array_equal(S, wc.ssd(gen.generate_u8(z_star).numpy(), queries)) and np.abs(z_star).max() <= Z_MAX
    assert np.array_equal(dist, _dist32(S, 12288, "u8")) and np.array_equal(_dist32(trace[0], 12288, "u8"), fbb_dist)
    assert (dist <= fbb_dist).all() and (dist < fbb_dist).any()
    # no sweeps: the start; history off: three values; seed and query_base have no effect
    d0, z0, S0, t0 = gl.pbb_attack(queries, gen, z_init.reshape(Q, 100, 1, 1), optimizer="powell", sweeps=0, history=True)
    assert np.array_equal(S0, trace[0]) and np.array_equal(z0, z_init) and np.array_equal(t0, trace[:1]) and np.array_equal(d0, fbb_dist)
    short = gl.pbb_attack(queries[:2], gen, z_init[:2], optimizer="powell", sweeps=1, ladder=2, step0=0.5, seed=5, query_base=77)
    assert len(short) == 3
    for a, b in zip(short, gl.pbb_attack(queries[:2], gen, z_init[:2], optimizer="powell", sweeps=1, ladder=2, step0=0.5)):
        assert np.array_equal(a, b)
    want = _driven(gl, gen, queries[:2], z_init[:2], 1, 2, 0.5)
    assert np.array_equal(short[1].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(short[2], want[1])
    # direction sets that cannot fit the device are refused before anything is allocated for them
    with pytest.raises(ValueError, match="block_images"):
        gl.pbb.pbb_attack(np.zeros((8192, 3, 2, 2), np.uint8), _Wide(gen.ctx), np.zeros((8192, 4096), f32), optimizer="powell",
                          block_images=1 << 30)                          # 8192 x 4097 x 4096 floats: 550 GB


class _Wide:
    """a generator of 4096-value latents that must not be reached"""
    def __init__(self, ctx):
        self.ctx = ctx

    def generate_u8(self, z):
        raise AssertionError("the memory check must come first")


def test_attack_does_not_depend_on_the_blocks(gl, attack_case):
    gen, queries, z_init, _, got, _ = attack_case
    # one query per block against all nine in one
    for a, b in zip(gl.pbb_attack(queries, gen, z_init, optimizer="powell", sweeps=SWEEPS, history=True, block_images=8), got):
        assert np.array_equal(a, b)


def test_es_untouched(gl, small):
    gen = small
    z_init, z_image = wc.search_latents()
    queries = gen.generate_u8(z_image).numpy()
    kw = dict(rounds=3, population=8, sigma=0.25, seed=9, history=True)
    plain = gl.pbb_attack(queries, gen, z_init, **kw)
    named = gl.pbb_attack(queries, gen, z_init, optimizer="es", sweeps=2, ladder=8, step0=1.0, **kw)
    for a, b in zip(plain, named):
        assert np.array_equal(a, b)
    assert plain[3].shape == (4, 12) and (plain[3][-1] < plain[3][0]).any()
