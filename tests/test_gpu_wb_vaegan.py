"""GPU: VAEGAN under the attacks that hold the generator -- Generator.frozen(k) (gan_models/vaegan/train.py: gl_dcgan_advance_spectral, then the state
held) bit for bit against the parent's k-th next forward, its latent gradient (csrc/gl_dcgan_grad.hip with the attention backward of
csrc/gl_attention_grad.hip) against float64 autograd of the host restatement of tests/vaegan_wb_common.py, and wb_attack, pbb_attack,
GeneratedBank and the two l2-lpips attacks on the view.

The bound on a gradient row is tests/test_gpu_wb.py's, unchanged: the same metric, |g - g64|_2 / |g64|_2, is measured for float32 torch autograd of
the graph on the CPU on the test's own inputs, its maximum over the rows is taken, and the device may be SLACK = 4 times that.  Every row is counted.
Both attention widths run: d = 32 (width 64, z_dim 100) and d = 64 (width 128, z_dim 64).  Measured figures: DESIGN.md section 5 and what each
test prints."""
import ctypes

import numpy as np
import pytest
import torch

import gpu_common  # noqa: F401
import vaegan_wb_common as vw
import wb_common as wc
import wb_lpips_common as wl

pytestmark = pytest.mark.gpu
_p = ctypes.c_void_p
SLACK = 4.0


@pytest.fixture(scope="module")
def gl():
    import ganleaks_amd
    return ganleaks_amd


def _parent(gl, d, nz, precision=1):
    from ganleaks_amd.gan_models.vaegan.train import Generator
    g = Generator(nz, d=d)
    g.load_state_dict(gl.synth.vaegan_state_dict(z_dim=nz, d=d))
    g.set_precision(precision)
    return g


def _make(gl, d, nz):
    sd = gl.synth.vaegan_state_dict(z_dim=nz, d=d)
    assert float(sd["sa1.gamma"][0]) == np.float32(vw.GAMMA)
    view, view0 = _parent(gl, d, nz).frozen(1), _parent(gl, d, nz, 0).frozen(1)
    assert view._precision == 1 and view0._precision == 0
    return view, view0, vw.HeldVaegan(sd, 1), vw.HeldVaegan(sd, 1, torch.float32)


@pytest.fixture(scope="module")
def small(gl):
    """d = 32: (the view under test with the default split-fp16 precision, one at precision 0, the float64 and the float32 host modules)"""
    return _make(gl, *vw.SMALL)


@pytest.fixture(scope="module")
def wide(gl):
    return _make(gl, *vw.WIDE)


@pytest.fixture(scope="module")
def model(gl, synth):
    from ganleaks_amd.lpips import LpipsModel
    return LpipsModel().load_state_dicts(synth.vgg16_state_dict(7), wl.lin_weights())


def _bits(a):
    a = a.numpy() if hasattr(a, "numpy") else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("d,nz,precision", [(32, 100, 0), (32, 100, 1), (64, 64, 0), (64, 64, 1)])
def test_frozen_view_is_the_parents_kth_next_forward(gl, d, nz, precision):
    parent, control = _parent(gl, d, nz, precision), _parent(gl, d, nz, precision)
    z = gl.synth.latent(31, 5).reshape(5, -1)[:, :nz].copy()
    views = [parent.frozen(1), parent.frozen(2)]
    got = [[_bits(a) for a in v.forward_device(z, True, True)] for v in views]
    for v in views:
        assert not hasattr(v, "power_iterations") and v.image_shape == (3, 64, 64) and v.z_dim == nz and v.ctx is parent.ctx
        assert v._precision == precision and v._handle.value != parent._handle.value
    # the parent has not moved: its next two forwards are the control's, and they are what the views gave
    for k in range(2):
        mine, ctrl = [_bits(a) for a in parent.forward_device(z, True, True)], [_bits(a) for a in control.forward_device(z, True, True)]
        state, cstate, held = parent.state_dict(), control.state_dict(), views[k].state_dict()
        for a, b, c in zip(mine, ctrl, got[k]):
            assert np.array_equal(a, b) and np.array_equal(a, c), k
        for key in state:
            assert np.array_equal(_bits(state[key]), _bits(cstate[key])) and np.array_equal(_bits(state[key]), _bits(held[key])), (k, key)
    assert not np.array_equal(got[0][0], got[1][0])
    # the views stay where they are, whatever ran in between, and whatever the batch
    for v, first in zip(views, got):
        again = [_bits(a) for a in v.forward_device(z, True, True)]
        assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])
        assert np.array_equal(_bits(v.generate_u8(z[3:])), first[1][3:])
        assert np.array_equal(v.forward(z.reshape(5, nz, 1, 1)).view(np.uint32), first[0])
    assert parent._precision == precision
    with pytest.raises(ValueError, match="forwards"):
        parent.frozen(0)


_REFS = {}


def _references(which, models):
    """the host side of the gradient cases of one generator, computed once and left unchanged"""
    if which not in _REFS:
        _REFS[which] = vw.gradient_references(which, models[2], models[3], models[0].z_dim)
    return _REFS[which]


def _check_gradients(gl, models, which, n, chunk):
    """The inputs are vaegan_wb_common.GRADIENT_CASES': latents at which no ReLU input is within float32's reach of zero (asserted in
    tests/test_vaegan_wb_cpu.py; a unit that is decides its mask by the arithmetic, and one unit is up to 1 % of a row).  Gradient rows: the
    bound of tests/test_gpu_wb.py, 4 x the float32-autograd maximum over the rows of the case.  Loss: 4 x the float32 maximum over all nine rows
    of the generator's three cases (vaegan_wb_common.gradient_references says why one to five samples of a single float32 number are no
    yardstick); SLACK stays 4 and nothing is added to it."""
    view, view0, net64, net32 = models
    nz = view.z_dim
    cases, yard_l = _references(which, models)
    c = cases[(n, chunk)]
    z, cot, targets, g64, l64g, l64 = c["z"], c["cot"], c["targets"], c["g64"], c["lg64"], c["l64"]
    ref, ref_g, ref_l = c["ref_vjp"], c["ref_grad"], c["ref_loss"]
    before = view.generate_u8(z).numpy()
    try:
        if chunk:
            view.set_chunk(chunk)
            view0.set_chunk(chunk)
        grad, out = view.vjp_z(z, cot, want_output=True)
        grad, out = grad.numpy(), out.numpy()
        lgrad, loss = (a.numpy() for a in view.l2_grad_z(z, targets))
        after = view.generate_u8(z).numpy()
        out0 = view0.forward(z.reshape(n, nz, 1, 1))
    finally:
        view.set_chunk(0)
        view0.set_chunk(0)
    err, err_g, err_l = wc.row_errors(grad, g64), wc.row_errors(lgrad, l64g), np.abs(loss.astype(np.float64) - l64) / l64
    print("FIG %s n=%d chunk=%d | vjp_z float32 max %.3e device max %.3e ratio %.2f | l2_grad_z float32 max %.3e device max %.3e ratio %.2f | "
          "loss float32 max of the case %.3e, of the generator's nine rows %.3e, device max %.3e ratio %.2f"
          % (which, n, chunk, ref.max(), err.max(), err.max() / ref.max(), ref_g.max(), err_g.max(), err_g.max() / ref_g.max(), ref_l.max(), yard_l,
             err_l.max(), err_l.max() / yard_l))
    assert grad.shape == (n, nz) and grad.dtype == np.float32 and np.isfinite(grad).all() and np.isfinite(lgrad).all() and loss.shape == (n,)
    assert (err <= SLACK * ref.max()).all()
    assert (err_g <= SLACK * ref_g.max()).all()
    assert (err_l <= SLACK * yard_l).all()
    assert np.array_equal(out, out0)                       # the fp32-product forward's output
    assert view._precision == 1 and np.array_equal(after, before)          # precision and chunk are as they were
    assert np.array_equal(view.generate_u8(z).numpy(), before)


@pytest.mark.parametrize("n,chunk", [(1, 0), (3, 0), (5, 2)])
def test_gradients_against_autograd(gl, small, n, chunk):
    _check_gradients(gl, small, "small", n, chunk)


@pytest.mark.parametrize("n,chunk", [(1, 0), (3, 0), (5, 2)])
def test_gradients_against_autograd_wide(gl, wide, n, chunk):
    _check_gradients(gl, wide, "wide", n, chunk)


@pytest.mark.parametrize("which", ["small", "wide"])
def test_gradient_rows_do_not_depend_on_the_batch(gl, small, wide, which):
    view = (small if which == "small" else wide)[0]
    nz = view.z_dim
    z = gl.synth.latent(64, 5).reshape(5, -1)[:, :nz].copy()
    targets = view.generate_u8(gl.synth.latent(65, 5).reshape(5, -1)[:, :nz].copy()).numpy()
    cot = np.random.default_rng(66).standard_normal((5, 3, 64, 64)).astype(np.float32)
    bits = lambda pair: [a.numpy().view(np.uint32) for a in pair]        # noqa: E731
    together = bits(view.l2_grad_z(z, targets))
    parts = [bits(view.l2_grad_z(z[:2], targets[:2])), bits(view.l2_grad_z(z[2:], targets[2:]))]
    vjp = view.vjp_z(z, cot).numpy().view(np.uint32)
    try:
        view.set_chunk(2)
        chunked = bits(view.l2_grad_z(z, targets))
        vjp_chunked = view.vjp_z(z, cot).numpy().view(np.uint32)
    finally:
        view.set_chunk(0)
    for k in (0, 1):
        assert np.array_equal(np.concatenate([parts[0][k], parts[1][k]]), together[k])
        assert np.array_equal(chunked[k], together[k])
    assert np.array_equal(vjp_chunked, vjp) and np.array_equal(view.vjp_z(z[3:], cot[3:]).numpy().view(np.uint32), vjp[3:])


def test_an_unheld_generator_is_still_refused(gl):
    from ganleaks_amd._lib import check
    parent = _parent(gl, 32, 100)
    ctx = parent.ctx
    z, t = ctx.to_device(np.zeros((2, 100), np.float32)), ctx.to_device(np.zeros((2, 3, 64, 64), np.uint8))
    cot, grad, loss = ctx.zeros((2, 3, 64, 64), np.float32), ctx.empty((2, 100), np.float32), ctx.empty((2,), np.float32)
    for call in (lambda: ctx.lib.gl_dcgan_vjp_z(parent._handle, _p(z.ptr), 2, _p(cot.ptr), _p(grad.ptr), _p(0)),
                 lambda: ctx.lib.gl_dcgan_l2_grad_z(parent._handle, _p(z.ptr), _p(t.ptr), 2, _p(grad.ptr), _p(loss.ptr))):
        with pytest.raises(gl.GanLeaksError, match="self-attention or spectral normalisation") as e:
            check(call())
        assert e.value.code == -4
    for attack in (gl.wb_attack, gl.pbb_attack):
        with pytest.raises(NotImplementedError):
            attack(np.zeros((2, 3, 64, 64), np.uint8), parent, np.zeros((2, 100), np.float32))
    with pytest.raises(gl.GanLeaksError, match="bad argument"):
        check(ctx.lib.gl_dcgan_advance_spectral(parent._handle, -1))


@pytest.fixture(scope="module")
def attack_case(gl, small):
    view, _, net64, _ = small
    z_bank, z_query = vw.attack_latents()
    queries = wc.quantize_u8(vw.forward(net64, z_query))
    z_init, _ = gl.pbb_init_from_bank(queries, view, z_bank, batch_size=64)
    return view, queries, z_bank, z_init


def test_wb_attack(gl, attack_case):
    from ganleaks_amd.attack import _dist32
    view, queries, z_bank, z_init = attack_case
    assert np.array_equal(z_init, z_bank[list(vw.ATTACK_PICK)])            # the start tests/test_vaegan_wb_cpu.py descends from
    kw = dict(steps=vw.ATTACK_STEPS, lr=vw.ATTACK_LR, history=True)
    dist, z_star, S, trace = gl.wb_attack(queries, view, z_init, **kw)
    print("start", trace[0].tolist(), "final", S.tolist())
    assert trace.shape == (vw.ATTACK_STEPS + 1, vw.ATTACK_Q) and np.array_equal(trace[-1], S)
    assert np.array_equal(S, wc.ssd(view.generate_u8(z_star).numpy(), queries))
    assert np.array_equal(trace[0], wc.ssd(view.generate_u8(z_init).numpy(), queries))
    assert np.array_equal(dist, _dist32(S, 12288, "u8"))
    assert (np.diff(trace, axis=0) <= 0).all()
    assert (trace[-1] < trace[0]).all()
    for a, b in zip(gl.wb_attack(queries, view, z_init, block_images=3, **kw), (dist, z_star, S, trace)):
        assert np.array_equal(a, b)
    for a, b in zip(gl.wb_attack(queries, view, z_init, block_images=4096, **kw), (dist, z_star, S, trace)):
        assert np.array_equal(a, b)


def test_pbb_attack(gl, attack_case):
    view, queries, z_bank, z_init = attack_case
    kw = dict(rounds=4, population=8, history=True)
    dist, z_star, S, trace = gl.pbb_attack(queries, view, z_init, **kw)
    print("start", trace[0].tolist(), "final", S.tolist())
    assert trace.shape == (5, vw.ATTACK_Q) and np.array_equal(trace[-1], S)
    assert np.array_equal(S, wc.ssd(view.generate_u8(z_star).numpy(), queries))
    assert np.array_equal(trace[0], wc.ssd(view.generate_u8(z_init).numpy(), queries))
    assert (np.diff(trace, axis=0) <= 0).all() and (S <= trace[0]).all()
    for blocks in (3 * 8, 4096):
        for a, b in zip(gl.pbb_attack(queries, view, z_init, block_images=blocks, **kw), (dist, z_star, S, trace)):
            assert np.array_equal(a, b)


def test_generated_bank_equals_the_materialised_bank(gl, attack_case):
    view, queries, z_bank, _ = attack_case
    try:
        view.set_chunk(3)
        streamed = gl.attack(queries, gl.GeneratedBank(view, z_bank), distance="l2", batch_size=16)
        resident = gl.attack(queries, view.generate_u8(z_bank), distance="l2", batch_size=16)
    finally:
        view.set_chunk(0)
    assert np.array_equal(_bits(streamed[0]), _bits(resident[0])) and np.array_equal(streamed[1], resident[1])
    assert np.array_equal(_bits(gl.attack(queries, view.generate_u8(z_bank), distance="l2", batch_size=16)[0]), _bits(resident[0]))


def _pattern(dist):
    return np.asarray(dist, np.float32).view(np.uint32).astype(np.int64)


def _recount(gl, model, view, queries, z_star):
    images = view.generate_u8(z_star).numpy()
    return np.array([gl.attack(queries[q:q + 1], images[q:q + 1], distance="l2-lpips", batch_size=1, lpips=model)[0][0] for q in range(len(queries))],
                    np.float32)


def test_pair_wb_attack(gl, model, attack_case):
    view, queries, _, z_init = attack_case
    dist, z_star, key, trace = gl.pair_wb_attack(queries[:4], view, z_init[:4], steps=2, lr=vw.ATTACK_LR, history=True, lpips=model)
    assert trace.shape == (3, 4) and (np.diff(trace, axis=0) <= 0).all() and np.array_equal(trace[-1], key)
    assert np.array_equal(_pattern(dist), key) and np.array_equal(_pattern(_recount(gl, model, view, queries[:4], z_star)), key)
    assert view._precision == 1


def test_pair_pbb_attack(gl, model, attack_case):
    view, queries, _, z_init = attack_case
    dist, z_star, key, trace = gl.pair_pbb_attack(queries[:4], view, z_init[:4], rounds=2, population=8, history=True, lpips=model)
    assert trace.shape == (3, 4) and (np.diff(trace, axis=0) <= 0).all() and np.array_equal(trace[-1], key)
    assert np.array_equal(_pattern(dist), key) and np.array_equal(_pattern(_recount(gl, model, view, queries[:4], z_star)), key)
