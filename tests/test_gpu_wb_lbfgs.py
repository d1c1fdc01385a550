"""GPU: L-BFGS in the white-box attack (csrc/gl_wb_lbfgs.hip, ganleaks_amd/wb.py optimizer='lbfgs') -- push, direction, candidates and
advance bit for bit against the numpy float32 restatement of tests/wb_lbfgs_common.py, finite termination on a quadratic (the check that does
not rest on the restatement: steepest descent with exact steps cannot get below ((kappa - 1) / (kappa + 1))^8 = 0.2 at kappa = 10, the
gate is 1e-4 and the restatement reaches 2e-8, tests/test_wb_lbfgs_cpu.py), and wb_attack on the inputs at which the host search works."""
import ctypes

import numpy as np
import pytest

import gpu_common  # noqa: F401
import wb_common as wc
import wb_lbfgs_common as lc

pytestmark = pytest.mark.gpu
_p = ctypes.c_void_p
_f = ctypes.c_float
f32 = np.float32


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


class Dev:
    """the state of lc.State on the device and the four calls on it"""
    NAMES = ("z", "z_prev", "g_prev", "S", "Y", "count", "head", "t", "flag")

    def __init__(self, gl, st):
        self.ctx = gl.Context.get()
        self.lib = self.ctx.lib
        self.m = st.m
        self.nq, self.nz = st.z.shape
        for name in self.NAMES:
            setattr(self, name, self.ctx.to_device(getattr(st, name)))
        self.p = self.ctx.zeros((self.nq, self.nz), f32)

    def host(self):
        st = lc.State(self.z.numpy(), self.m)
        for name in self.NAMES:
            setattr(st, name, getattr(self, name).numpy())
        return st

    def push(self, g, moved):
        from ganleaks_amd._lib import check
        g, moved = self.ctx.to_device(np.asarray(g, f32)), self.ctx.to_device(np.asarray(moved, np.uint8))
        check(self.lib.gl_wb_lbfgs_push(self.ctx.handle, _p(self.z.ptr), _p(g.ptr), _p(self.z_prev.ptr), _p(self.g_prev.ptr), _p(self.S.ptr),
                                        _p(self.Y.ptr), _p(self.count.ptr), _p(self.head.ptr), _p(moved.ptr), self.nq, self.nz, self.m))
        self.ctx.sync()

    def direction(self, g, step0):
        from ganleaks_amd._lib import check
        g = self.ctx.to_device(np.asarray(g, f32))
        check(self.lib.gl_wb_lbfgs_direction(self.ctx.handle, _p(g.ptr), _p(self.S.ptr), _p(self.Y.ptr), _p(self.count.ptr), _p(self.head.ptr),
                                             _p(self.t.ptr), _p(self.flag.ptr), self.nq, self.nz, self.m, _f(step0), _p(self.p.ptr)))
        return self.p.numpy()

    def candidates(self, L, z_max):
        from ganleaks_amd._lib import check
        self.cand = self.ctx.empty((self.nq * L, self.nz), f32)
        check(self.lib.gl_wb_lbfgs_candidates(self.ctx.handle, _p(self.z.ptr), _p(self.p.ptr), _p(self.t.ptr), self.nq, self.nz, L, _f(z_max),
                                              _p(self.cand.ptr)))
        return self.cand.numpy()

    def accept_and_advance(self, take, j_new, L):
        """gl_pbb_accept on scores made up so that exactly the queries of `take` are strictly closer, then gl_wb_lbfgs_advance"""
        from ganleaks_amd._lib import check
        ctx = self.ctx
        S_cur, S_new = ctx.to_device(np.full(self.nq, 10, np.uint64)), ctx.to_device(np.where(take, 5, 10).astype(np.uint64))
        j, one = ctx.to_device(np.asarray(j_new, np.int32)), ctx.to_device(np.ones(self.nq, f32))
        accepted = ctx.zeros((self.nq,), np.uint8)
        check(self.lib.gl_pbb_accept(ctx.handle, _p(self.z.ptr), _p(one.ptr), _p(S_cur.ptr), _p(self.cand.ptr), _p(S_new.ptr), _p(j.ptr), self.nq,
                                     self.nz, L, _f(1.0), _f(1.0), _f(1.0), _f(1.0), _p(accepted.ptr)))
        check(self.lib.gl_wb_lbfgs_advance(ctx.handle, _p(self.t.ptr), _p(self.count.ptr), _p(self.head.ptr), _p(self.flag.ptr), _p(accepted.ptr),
                                           _p(j.ptr), self.nq, L))
        return accepted.numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == f32 else a


def _same(dev_state, st, names, where):
    for name in names:
        assert np.array_equal(_bits(getattr(dev_state, name)), _bits(getattr(st, name))), (name, where)


def _start_state(rng, nq, nz, m):
    """rings that differ per query: 0 empty, 1 one pair, 2 about half, 3 full, 4 and 5 wrapped past m, 6 one pair with s.y < 0 (uploaded by
    the caller: no push makes it), whose -H g is no descent direction"""
    st = lc.State(rng.standard_normal((nq, nz)).astype(f32), m)
    fills = [0, 1, m // 2 + 1, m, m + 2, 2 * m + 1, 0]
    g = rng.standard_normal((nq, nz)).astype(f32)
    g[:, 1] = 0.0                                                       # column 1 has no gradient, here and in the test's steps
    lc.push(st, g, np.zeros(nq, np.uint8))
    scale = (1.0 + rng.random((nq, nz)) * 9.0).astype(f32)              # y = scale * s + noise: s.y > 0
    for k in range(max(fills)):
        moved = np.array([k < n for n in fills], np.uint8)
        step = rng.standard_normal((nq, nz)).astype(f32) * f32(0.2) * moved[:, None]
        st.z = (st.z + step).astype(f32)
        g = (g + scale * step + f32(0.01) * rng.standard_normal((nq, nz)).astype(f32) * moved[:, None]).astype(f32)
        g[:, 1] = 0.0
        lc.push(st, g, moved)
    assert st.count.tolist()[:6] == [min(n, m) for n in fills[:6]] and st.head.tolist()[:6] == [n % m for n in fills[:6]]
    s = rng.standard_normal(nz).astype(f32)
    st.S[6, 0], st.Y[6, 0] = s, -(scale[6] * s)
    st.count[6], st.head[6] = 1, 1 % m
    return st, g, scale


@pytest.mark.parametrize("nz", [3, 64, 100, 130])                       # below one wave, exactly one wave, the tails 36 and 2
@pytest.mark.parametrize("m", [1, 3, 8])
def test_bit_for_bit(gl, nz, m):
    nq, z_max, step0 = 7, 4.0, 1.0
    for L in (1, 8):
        rng = np.random.default_rng(1000 * nz + 10 * m + L)
        st, g, scale = _start_state(rng, nq, nz, m)
        st.z[0, 2] = f32(3.99)
        st.z_prev[0, 2] = f32(3.99)
        dev = Dev(gl, st)
        moved = np.array([0, 1, 1, 1, 1, 1, 0], np.uint8)
        flags = []
        for step in (1, 2, 3):
            # the queries that moved took a step; query 5's first pair is rejected (y = -s: s.y < 0)
            delta = rng.standard_normal((nq, nz)).astype(f32) * f32(0.1) * moved[:, None]
            st.z = (st.z + delta).astype(f32)
            dev.z = dev.ctx.to_device(st.z)
            g = (g + scale * delta).astype(f32)
            if step > 1:                                                 # gradients of other magnitudes: pairs with s.y of either sign
                g = g * f32(10.0) ** rng.integers(-1, 2, size=(nq, 1)).astype(f32)
            if step == 1:
                g[5] = st.g_prev[5] - delta[5]
                g[0, 2] = f32(-1e15)                                     # empty ring: t = step0 / 1e15, t p = 1 on that element, 3.99 + 1 > z_max
            g[:, 1] = 0.0                                                # a column without gradient
            if step == 2:
                g[3] = 0.0                                               # a zero gradient finishes the query: step 3 leaves it alone
            before = st.count.copy()
            lc.push(st, g, moved)
            dev.push(g, moved)
            _same(dev.host(), st, ("z_prev", "g_prev", "S", "Y", "count", "head"), ("push", L, step))
            if step == 1:
                assert st.count[5] == before[5] and (st.count[1:5] == np.minimum(before[1:5] + 1, m)).all()
            p = lc.direction(st, g, step0)
            p_dev = dev.direction(g, step0)
            assert np.array_equal(_bits(p_dev), _bits(p)), ("p", L, step)
            _same(dev.host(), st, ("count", "head", "t", "flag"), ("direction", L, step))
            flags.append(st.flag.copy())
            cand = lc.candidates(st.z, p, st.t, L, z_max)
            cand_dev = dev.candidates(L, z_max)
            assert np.array_equal(_bits(cand_dev), _bits(cand)), ("cand", L, step)
            steepest = (st.flag & lc.STEEPEST) != 0                       # -g leaves the column without gradient where it is
            assert np.abs(cand).max() <= z_max and np.array_equal(cand.reshape(nq, L, nz)[steepest, :, 1], np.repeat(st.z[steepest, 1:2], L, axis=1))
            if step == 1:
                assert cand[0, 2] == f32(z_max)
            take = rng.random(nq) < 0.6
            take[1], take[2] = step != 2, step == 2
            j_new = rng.integers(0, L, size=nq).astype(np.int32)
            live = np.array([lc.live(t) for t in st.t])
            picked = cand.reshape(nq, L, nz)[np.arange(nq), j_new]
            changes = take & (picked != st.z).any(axis=1)
            st.z[take] = picked[take]
            lc.advance(st, take.astype(np.uint8), j_new, L)
            accepted = dev.accept_and_advance(take, j_new, L)
            assert np.array_equal(accepted, take.astype(np.uint8))
            _same(dev.host(), st, ("z", "t", "count", "head", "flag"), ("advance", L, step))
            assert not (changes & ~live).any()                           # a finished query's candidates are its iterate
            moved = take.astype(np.uint8)
        flags = np.stack(flags)
        assert flags[0, 0] == lc.STEEPEST and flags[0, 6] == (lc.STEEPEST | lc.DROPPED) and (flags[0, 1:5] == 0).all()
        assert not lc.live(st.t[3])


def _device_quadratic(gl, A, b, z0, m, steps):
    st = lc.State(np.asarray(z0, f32), m)
    dev = Dev(gl, st)

    def push_fn(z, g, moved):
        dev.z = dev.ctx.to_device(z)
        dev.push(g, moved)

    def candidates_fn(z, p, t):
        dev.t = dev.ctx.to_device(t)                                     # the exact step, from a device array; p is the device's own
        return dev.candidates(1, 1e6)

    ratio = lc.quadratic_run(A, b, z0, m, steps, push_fn, lambda g: dev.direction(g, 1.0), candidates_fn)
    return ratio, dev.host()


@pytest.mark.parametrize("nz,steps", [(8, 8), (100, 24)])
def test_finite_termination_on_a_quadratic(gl, nz, steps):
    """f(z) = z'Az / 2 - b'z, eigenvalues linspace(1, 10, nz) in a random orthogonal basis, m = 8, four problems; g = Az - b on the host in
    float64 from the device's float32 z, the exact step t = -g.p / p'Ap through the candidates call with L = 1, push and direction on the
    device.  Gate: |g_steps| <= 1e-4 |g_0| for every query"""
    A, b, z0 = lc.quadratic(0, nz)
    ratio, st = _device_quadratic(gl, A, b, z0, 8, steps)
    print("nz=%d: |g_%d| / |g_0| per query %s; the float32 restatement %s" % (nz, steps, ratio, lc.quadratic_host(A, b, z0, 8, steps)))
    assert (st.count >= 1).all()                                         # the ring was in use
    assert (ratio <= 1e-4).all()


def test_search(gl, small):
    from ganleaks_amd.attack import _dist32
    gen = small
    z_init, z_image = wc.search_latents()
    queries = gen.generate_u8(z_image).numpy()
    start = wc.ssd(gen.generate_u8(z_init).numpy(), queries)
    kw = dict(steps=lc.SEARCH_STEPS, optimizer="lbfgs", history=True)
    dist, z_star, S, trace = gl.wb_attack(queries, gen, z_init, **kw)
    print("start", start.tolist(), "final", S.tolist())
    assert trace.dtype == np.int64 and trace.shape == (lc.SEARCH_STEPS + 1, 12) and S.dtype == np.int64 and S.shape == (12,)
    assert dist.dtype == np.float32 and dist.shape == (12,) and z_star.dtype == np.float32 and z_star.shape == (12, 100)
    assert (np.diff(trace, axis=0) <= 0).all() and np.array_equal(trace[0], start) and np.array_equal(trace[-1], S)
    assert np.array_equal(S, wc.ssd(gen.generate_u8(z_star).numpy(), queries))
    assert np.array_equal(dist, _dist32(S, 12288, "u8"))
    # the queries that are the image of their own start: S = 0 from the start, nothing is accepted
    assert (trace[:, 0::3] == 0).all() and np.array_equal(z_star[0::3], z_init[0::3])
    # half the margin of the host precondition (a quarter, tests/test_wb_lbfgs_cpu.py), as the Adam test does
    assert (start[2::3] > 0).all() and (2 * S[2::3] <= start[2::3]).all()
    assert (S[1::3] < start[1::3]).all()
    # 12 queries as 5 + 5 + 2
    for a, b in zip(gl.wb_attack(queries, gen, z_init, block_images=5, **kw), (dist, z_star, S, trace)):
        assert np.array_equal(a, b)
    # steps = 0 returns the start; history off returns three values
    d0, z0, S0 = gl.wb_attack(queries, gen, z_init.reshape(12, 100, 1, 1), steps=0, optimizer="lbfgs")
    assert np.array_equal(S0, start) and np.array_equal(z0, z_init) and np.array_equal(d0, _dist32(start, 12288, "u8"))
    # the other keywords change the path, not the contract
    d1, z1, S1 = gl.wb_attack(queries, gen, z_init, steps=4, optimizer="lbfgs", memory=1, ladder=1, step0=0.5)
    assert np.array_equal(S1, wc.ssd(gen.generate_u8(z1).numpy(), queries)) and (S1 <= start).all() and np.abs(z1).max() <= 4.0


def test_never_above_the_full_black_box_score(gl, small):
    gen = small
    queries = gen.generate_u8(gl.synth.latent(71, 6)).numpy()
    z_bank = gl.synth.latent(72, 130).reshape(130, 100)
    z_init, _ = gl.pbb_init_from_bank(queries, gen, z_bank, batch_size=64)
    fbb_dist, _ = gl.attack(queries, gl.GeneratedBank(gen, z_bank), distance="l2", batch_size=64)
    dist, _, _ = gl.wb_attack(queries, gen, z_init, steps=4, optimizer="lbfgs")
    assert (dist <= fbb_dist).all() and (dist < fbb_dist).any()


def test_adam_untouched(gl, small):
    gen = small
    z_init, z_image = wc.search_latents()
    queries = gen.generate_u8(z_image).numpy()
    kw = dict(steps=3, lr=wc.SEARCH_LR, history=True)
    plain = gl.wb_attack(queries, gen, z_init, **kw)
    named = gl.wb_attack(queries, gen, z_init, optimizer="adam", memory=3, ladder=5, step0=0.25, **kw)
    for a, b in zip(plain, named):
        assert np.array_equal(a, b)
    assert (plain[3][-1] < plain[3][0]).any()


def test_abi_refusals(gl):
    from ganleaks_amd._lib import check
    ctx = gl.Context.get()
    lib, h = ctx.lib, ctx.handle
    nq, nz, m, L = 2, 5, 2, 4
    bufs = [ctx.zeros((nq * max(m, L), nz), f32) for _ in range(8)]
    Z, G, ZP, GP, S, Y, P, C = (_p(b.ptr) for b in bufs)
    a = bufs[0]
    i1, i2, u1, u2 = ctx.zeros((nq,), np.int32), ctx.zeros((nq,), np.int32), ctx.zeros((nq,), np.uint8), ctx.zeros((nq,), np.uint8)
    t = ctx.to_device(np.ones(nq, f32))
    A, I1, I2, U1, U2, T, N = _p(a.ptr), _p(i1.ptr), _p(i2.ptr), _p(u1.ptr), _p(u2.ptr), _p(t.ptr), _p(0)
    one = _f(1.0)
    # nothing to do: no pointer is touched
    check(lib.gl_wb_lbfgs_push(h, N, N, N, N, N, N, N, N, N, 0, nz, m))
    check(lib.gl_wb_lbfgs_direction(h, N, N, N, N, N, N, N, 0, nz, m, one, N))
    check(lib.gl_wb_lbfgs_candidates(h, N, N, N, 0, nz, L, one, N))
    check(lib.gl_wb_lbfgs_advance(h, N, N, N, N, N, N, 0, L))
    # and what the arguments allow runs
    j = ctx.zeros((nq,), np.int32)
    check(lib.gl_wb_lbfgs_push(h, Z, G, ZP, GP, S, Y, I1, I2, U1, nq, nz, m))
    check(lib.gl_wb_lbfgs_direction(h, G, S, Y, I1, I2, T, U1, nq, nz, m, one, P))
    check(lib.gl_wb_lbfgs_candidates(h, Z, P, T, nq, nz, L, one, C))
    check(lib.gl_wb_lbfgs_advance(h, T, I1, I2, U1, U2, _p(j.ptr), nq, L))
    ctx.sync()
    assert not np.isfinite(t.numpy()).any()                              # a zero gradient finished both queries
    big = 1 << 31
    for call in (lambda: lib.gl_wb_lbfgs_push(h, A, A, A, A, A, A, I1, I2, U1, nq, nz, 0),
                 lambda: lib.gl_wb_lbfgs_push(h, A, A, A, A, A, A, I1, I2, U1, nq, nz, 17),
                 lambda: lib.gl_wb_lbfgs_push(h, A, A, A, A, A, A, I1, I2, U1, nq, 0, m),
                 lambda: lib.gl_wb_lbfgs_push(h, A, A, A, A, A, A, I1, I2, U1, nq, big, m),
                 lambda: lib.gl_wb_lbfgs_push(h, A, A, A, A, A, A, I1, I2, U1, -1, nz, m),
                 lambda: lib.gl_wb_lbfgs_push(h, A, A, A, A, N, A, I1, I2, U1, nq, nz, m),
                 lambda: lib.gl_wb_lbfgs_push(h, A, A, A, A, A, A, I1, I2, N, nq, nz, m),
                 lambda: lib.gl_wb_lbfgs_push(None, A, A, A, A, A, A, I1, I2, U1, nq, nz, m),
                 lambda: lib.gl_wb_lbfgs_direction(h, A, A, A, I1, I2, T, U1, nq, nz, 0, one, A),
                 lambda: lib.gl_wb_lbfgs_direction(h, A, A, A, I1, I2, T, U1, nq, nz, 17, one, A),
                 lambda: lib.gl_wb_lbfgs_direction(h, A, A, A, I1, I2, T, U1, nq, nz, m, _f(0.0), A),
                 lambda: lib.gl_wb_lbfgs_direction(h, A, A, A, I1, I2, T, U1, nq, nz, m, _f(float("nan")), A),
                 lambda: lib.gl_wb_lbfgs_direction(h, A, A, A, I1, I2, T, U1, nq, nz, m, _f(float("inf")), A),
                 lambda: lib.gl_wb_lbfgs_direction(h, A, A, A, I1, I2, T, U1, big - 1, big - 1, 16, one, A),
                 lambda: lib.gl_wb_lbfgs_direction(h, N, A, A, I1, I2, T, U1, nq, nz, m, one, A),
                 lambda: lib.gl_wb_lbfgs_direction(h, A, A, A, I1, I2, T, U1, nq, nz, m, one, N),
                 lambda: lib.gl_wb_lbfgs_candidates(h, A, A, T, nq, nz, 0, one, A),
                 lambda: lib.gl_wb_lbfgs_candidates(h, A, A, T, nq, nz, 33, one, A),
                 lambda: lib.gl_wb_lbfgs_candidates(h, A, A, T, nq, nz, L, _f(0.0), A),
                 lambda: lib.gl_wb_lbfgs_candidates(h, A, A, T, nq, nz, L, _f(float("inf")), A),
                 lambda: lib.gl_wb_lbfgs_candidates(h, A, A, N, nq, nz, L, one, A),
                 lambda: lib.gl_wb_lbfgs_candidates(h, A, A, T, big - 1, big - 1, 32, one, A),
                 lambda: lib.gl_wb_lbfgs_advance(h, T, I1, I2, U1, U2, I1, nq, 33),
                 lambda: lib.gl_wb_lbfgs_advance(h, T, I1, I2, U1, U2, I1, nq, 0),
                 lambda: lib.gl_wb_lbfgs_advance(h, T, I1, I2, U1, N, I1, nq, L),
                 lambda: lib.gl_wb_lbfgs_advance(None, T, I1, I2, U1, U2, I1, nq, L)):
        with pytest.raises(gl.GanLeaksError) as e:
            check(call())
        assert e.value.code == -1
