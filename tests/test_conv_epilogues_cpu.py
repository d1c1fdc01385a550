"""No GPU: what tests/test_gpu_conv_epilogues.py rests on (second half of tests/conv_layer_common.py).

(a) the decoders of the V row layouts (split rows, fp16 rows row-major and K-blocked) and of the split layout's halves, on addresses
    written out by hand from the layouts' descriptions in csrc/gl_conv.h;
(b) the float64 references on a hand-computed position;
(c) every case compared bit for bit meets the oracle's preconditions, asserted from the reference alone: the convolution's own (as in
    tests/test_conv_layers_cpu.py), stored activations integer multiples of one power of two, sum of squares / unit^2 < 2^24, the split
    representation exact;
(d) the exact host oracle stays within the derived bounds of the float64 references (so a device that equals the oracle meets them too, and the
    bounds are not vacuous: the largest error / bound is printed);
(e) the inputs of the stand-alone kernels meet the same preconditions at every C;
(f) the case table covers what the epilogue can get wrong.
"""
import ctypes

import numpy as np
import pytest

import conv_layer_common as cl

EXACT_KEYS = sorted(set(c.key for c in cl.EPI_CASES if cl.epi_exact(c)))
_cache = {}


def key_data(key):
    """inputs and float64 reference of a key, computed once and left unchanged"""
    if key not in _cache:
        if len(_cache) >= 2:
            _cache.pop(next(iter(_cache)))
        c = [c for c in cl.EPI_CASES if c.key == key][0]
        d = cl.make_epi_inputs(c)
        ref = cl.reference(c, d)
        ref.setflags(write=False)
        _cache[key] = (c, d, ref)
    return _cache[key]


# ---------------------------------------------------------------------------------------------------------------- (a) layouts
def test_split_row_addresses_by_hand():
    # split row of 1024 bytes: half k sits in chunk k / 32 of 128 bytes, hi at (k % 32) * 2, lo 64 bytes further
    idx = cl.vrow_half_index(0, 1024, [3], [70])
    assert idx[0, 0] * 2 == 3 * 1024 + 2 * 128 + 6 * 2
    buf = np.full(4 * 1024, cl.SENTINEL, np.uint8)
    h = buf.view(np.float16)
    h[idx[0, 0]], h[idx[0, 0] + 32] = 1.5, 0.25
    hi, lo, rest = cl.decode_vrows(buf, 0, 1024, 3, 1, 70, 1)
    assert hi[0, 0] == 1.5 and lo[0, 0] == 0.25 and rest
    h[5] = 2.0                                                              # a stray store outside the written range shows
    assert not cl.decode_vrows(buf, 0, 1024, 3, 1, 70, 1)[2]


def test_fp16_row_addresses_by_hand():
    assert cl.vrow_half_index(1, 512, [3], [70])[0, 0] * 2 == 3 * 512 + 70 * 2
    # K-blocked, 5 cells per row: [row / 256][cell = k / 64][row % 256][64 halves]: row 259, half 200 -> block 1, cell 3, row 3, half 8
    assert cl.vrow_half_index(1, -5, [259], [200])[0, 0] * 2 == (1 * 5 + 3) * 32768 + 3 * 128 + 8 * 2
    # rows 250 ... 260 of a tap case cross the block boundary
    idx = cl.vrow_half_index(1, -5, np.arange(250, 261), np.arange(0, 320))
    assert len(np.unique(idx)) == idx.size and idx.max() < 2 * 5 * 16384
    assert (idx[:6] < 5 * 16384).all() and (idx[6:] >= 5 * 16384).all()


def test_v_geometry():
    c = cl.EPI_BY_NAME["tap_t1_w16_cols64_f16_blocked"]
    ldv, vb = cl.v_geometry(c)
    K = cl.TAP_OFF + 96 * 64
    assert ldv == -((K + 63) // 64) and vb == 2 * (-ldv) * 32768 and c.tap_row0 + c.n > 256 > c.tap_row0 == 255
    c = cl.EPI_BY_NAME["tap_t1_w16_cols64_split"]
    ldv, vb = cl.v_geometry(c)
    assert ldv == K * 4 + 128 and ldv % 128 == 0 and vb == (c.tap_row0 + c.n + 1) * ldv
    c = cl.EPI_BY_NAME["tap_t1_w16_cols64_f16"]
    assert cl.v_geometry(c)[0] == K * 2 + 64
    for c in cl.TAP_CASES:
        assert c.tap_off % 64 == 0 and c.tap_off > 0 and cl.v_geometry(c)[1] <= 256 << 20


def test_split_halves_by_hand():
    v = np.arange(2 * 64, dtype=np.float32).reshape(2, 64) + np.float32(2.0 ** -12)
    hi, lo = cl.split_halves(cl.encode_split(v), 2, 64)
    assert hi[1, 40] == np.float16(104.0) and lo[1, 40] == np.float16(2.0 ** -12)
    assert np.array_equal(cl.halves_value(hi, lo), v.astype(np.float64))


def test_struct_mirrors_have_the_size_of_the_c_structs():
    # GlTuneConvLayer: 200 bytes up to `form` (as before), 7 ints, 8 pointers, 4 int64;  GlTuneSplitPost: by hand from its fields
    assert cl.TuneConvLayer.form.offset + 4 + 7 * 4 == cl.TuneConvLayer.rgb_w.offset and cl.TuneConvLayer.rgb_w.offset % 8 == 0
    assert ctypes.sizeof(cl.TuneConvLayer) == cl.TuneConvLayer.rgb_w.offset + 8 * 8 + 4 * 8
    assert ctypes.sizeof(cl.TuneSplitPost) == 16 + 8 + 8 + 32 + 8 + 6 * 8


# ------------------------------------------------------------------------------------------------------------- (b) references
def test_references_by_hand():
    v = np.array([[3.0, -4.0, 0.0, 12.0]])
    assert np.allclose(cl.ref_pixelnorm(v), v / np.sqrt(169.0 / 4 + 1e-8), rtol=0, atol=0)
    assert cl.ref_tap(v, [1.0, 0.5, 1.0, 0.25])[0, 1] == -4.0 / (13.0 + 1e-10) * 0.5 * 16384.0
    out, S = cl.ref_rgb(v, [[0.25, -0.125, 1.0, 0.0]], [2.0])
    assert out[0, 0] == 2.0 + 0.75 + 0.5 and S[0, 0] == 0.75 + 0.5
    img = np.arange(2 * 4 * 4 * 1, dtype=np.float64).reshape(2, 4, 4, 1)
    assert cl.pool2(img)[1, 1, 0, 0] == 16 + 13 and cl.pool2(img).shape == (2, 2, 2, 1)


def test_oracle_steps_by_hand():
    """one position, every step spelled out in Python floats rounded with numpy's float32"""
    f = np.float32
    stored = np.zeros((1, 32), f)
    stored[0, :3] = [12.0, -20.0, 2052.0]
    ss = f(12.0 * 12 + 20 * 20 + 2052.0 * 2052)
    inv = f(16.0) / f(np.sqrt(f(f(ss / f(32.0)) + f(f(f(1e-8) * f(16.0)) * f(16.0)))))
    hi, lo = cl.oracle_pixelnorm(stored)
    p = float(stored[0, 2]) * float(inv)
    assert hi[0, 2] == np.float16(f(p)) and lo[0, 2] == np.float16(f(p - float(hi[0, 2]))) and lo[0, 2] != 0
    coef = np.full(32, 0.3, f)
    tinv = f(16384.0) / f(f(np.sqrt(ss)) + f(f(1e-10) * f(16.0)))
    t = f(f(stored[0, 1] * tinv) * coef[1])
    th, tl = cl.oracle_tap(stored, coef)
    assert th[0, 1] == np.float16(t) and tl[0, 1] == np.float16(f(t - f(th[0, 1])))


# ---------------------------------------------------------------------------------------- (c), (d) preconditions and bounds
@pytest.mark.parametrize("key", EXACT_KEYS)
def test_exact_cases_meet_the_oracles_preconditions_and_the_oracle_the_bounds(key):
    c, d, ref = key_data(key)
    assert cl.exactness_problems(c, d, ref) == []
    assert d["x"].min() != 0 and np.abs(d["w"]).min() != 0
    stored = (ref * cl.ACT_SCALE).reshape(-1, c.cols)
    unit = cl.stored_unit(c, d)
    print("%s: largest sum of squares %.3g unit^2 (unit %g)" % (key, np.sum(stored * stored, axis=-1).max() / unit ** 2, unit))
    assert cl.sumsq_problems(stored, unit) == []
    modes = set(k.fuse for k in cl.EPI_CASES if k.key == key and cl.epi_exact(k))
    if 1 in modes:
        want = cl.ref_pixelnorm(ref).reshape(-1, c.cols) * cl.ACT_SCALE
        got = cl.halves_value(*cl.oracle_pixelnorm(stored))
        r = float((np.abs(got - want) / cl.bound_split(want)).max())
        print("  PixelNorm oracle: largest error / bound %.3f" % r)
        assert r <= 1.0
    if 3 in modes:
        assert d["tap_coef"].min() >= 0.01 and d["tap_coef"].max() <= 1.0
        want = cl.ref_tap(ref, d["tap_coef"]).reshape(-1, c.cols)
        hi, lo = cl.oracle_tap(stored, d["tap_coef"])
        r = float((np.abs(cl.halves_value(hi, lo) - want) / cl.bound_split(want)).max())
        r16 = float((np.abs(hi.astype(np.float64) - want) / cl.bound_f16(want)).max())
        print("  tap oracle: largest error / bound %.3f (split rows), %.3f (fp16 rows)" % (r, r16))
        assert r <= 1.0 and r16 <= 1.0
        ph, pl = cl.oracle_pool(stored.reshape(c.n, c.Ho, c.Wo, c.cols))
        assert np.array_equal(cl.halves_value(ph, pl), cl.pool2(ref * cl.ACT_SCALE).reshape(-1, c.cols))        # the pool of exact values is exact


def test_saturation_pair_differs_in_one_value():
    lo_c, hi_c = cl.EPI_BY_NAME["pn_sat_below"], cl.EPI_BY_NAME["pn_sat_above"]
    for c, top in ((lo_c, 65488.0), (hi_c, 65520.0)):
        d = cl.make_epi_inputs(c)
        ref = cl.reference(c, d)
        s = np.sort(np.abs(ref).ravel()) * cl.ACT_SCALE
        assert s[-1] == top and s[-2] < cl.F16_MAX                          # one value at the limit, every other inside the fp16 range
        assert (np.abs(cl.ref_clamped(c, ref) - ref) > 0).sum() == (1 if top > cl.F16_MAX else 0)


# ------------------------------------------------------------------------------------------------ (e) the stand-alone kernels
@pytest.mark.parametrize("c", [c for c in cl.POST_CASES if c.inputs == "exact" and c.tap_fmt == 0 and c.tap_layout == "row"], ids=repr)
def test_stand_alone_inputs_meet_the_preconditions(c):
    d = cl.make_post_inputs(c)
    stored = d["stored"].astype(np.float64)
    assert cl.sumsq_problems(stored, 1.0) == []
    hi, lo = cl.split_halves(cl.encode_split(d["stored"]), c.positions, c.C)
    assert (lo != 0).any(axis=1).all()                                      # every position has a value that needs its low half
    if c.op == 0:
        want = cl.ref_pixelnorm(stored / cl.ACT_SCALE) * cl.ACT_SCALE
        r = float((np.abs(cl.halves_value(*cl.oracle_pixelnorm(d["stored"])) - want) / cl.bound_split(want)).max())
    else:
        want = cl.ref_tap(stored / cl.ACT_SCALE, d["tap_coef"])
        r = float((np.abs(cl.halves_value(*cl.oracle_tap(d["stored"], d["tap_coef"])) - want) / cl.bound_split(want)).max())
    print("%s: oracle error / bound %.3f" % (c.name, r))
    assert r <= 1.0


def test_real_stand_alone_inputs_are_what_the_split_layout_holds():
    c = cl.POST_BY_NAME["post_pn_real_C512"]
    s = cl.make_post_inputs(c)["stored"]
    assert np.array_equal(cl.decode_split(cl.encode_split(s), c.positions, c.C), s.astype(np.float64)) and np.abs(s).max() < cl.F16_MAX


# ------------------------------------------------------------------------------------------------------------ (f) the table
def test_case_table_covers_the_epilogues_edges():
    forms = lambda cases: set(c.form for c in cases)
    want = {cl.H3 | 0, cl.H3 | 1, cl.H3 | 0 | cl.UP, cl.H3 | 1 | cl.UP, cl.HALO | 1, cl.HALO | 2}
    assert forms(cl.PN_CASES) == want
    assert forms(cl.RGB_CASES) == {cl.H3 | 0, cl.H3 | 1, cl.HALO | 1, cl.HALO | 2} == forms(cl.TAP_CASES)
    assert set(c.rgb_n for c in cl.RGB_CASES) == {1, 3}
    for c in cl.EPI_CASES:
        assert c.Cin == 32 and c.out == "split" and c.kind == "c3"
    # ragged position tiles (128 positions per tile 0, 256 per tile 1), cols below the tile's channels
    assert any(c.positions % 128 and c.cols == 96 for c in cl.PN_CASES) and any(c.positions % 256 and c.cols == 32 for c in cl.PN_CASES)
    # the tap: an image boundary inside a wave's 64 positions; W = 32; every format / layout / pool combination for every shape
    assert any(c.W == 16 and (c.H * c.W) % 64 and c.n > 1 for c in cl.TAP_CASES) and any(c.W == 32 for c in cl.TAP_CASES)
    shapes = set(c.key for c in cl.TAP_CASES)
    for key in shapes:
        assert sorted((c.tap_pool, c.tap_fmt, c.tap_layout) for c in cl.TAP_CASES if c.key == key) == sorted(cl.TAP_VARIANTS)
    for c in cl.TAP_CASES:
        if c.tap_layout == "blocked":
            assert c.tap_row0 + c.n > 256 and (c.n == 1 or c.tap_row0 < 256)   # the images cross the 256-row block boundary
    assert len(cl.REFUSE_CASES) == 5 and all(c.refused for c in cl.REFUSE_CASES)
    assert sorted(set(c.C for c in cl.POST_CASES if c.op == 0)) == [32, 64, 96, 128, 256, 512]
    assert sorted(set(c.C for c in cl.POST_CASES if c.op)) == [64, 128, 256, 512]
