"""No GPU: the float64 reference, the layout codecs and the case table that tests/test_gpu_conv_layers.py rests on (tests/conv_layer_common.py).

(a) the reference's tap / phase gather is right: the four sub-pixel phases of ConvTranspose2d k4 s2 p1 against oracle.conv_transpose2d, and the
    nine-tap form against a direct conv2d with padding=1;
(b) every case that is compared with zero tolerance meets the exactness preconditions (sum of absolute products < 2^24 units,
    float32(ref) == ref, split output below the fp16 limit and representable as hi + lo), asserted from the reference alone;
(c) the float64 reference of every big case takes a few seconds at the most;
(d) the split layout's encoder and decoder round-trip, on the layout written out by hand.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_layer_common as cl

EXACT = sorted([c for c in cl.ALL_CASES if c.atol is None and c.inputs != "real"], key=lambda c: c.key)
BIG = sorted(set(c.key for c in cl.ALL_CASES if c.big))
REF_SECONDS = 8.0
_cache, _seconds = {}, {}


def case_data(c):
    """inputs, reference and its wall time, computed once per key (cases a tuning switch apart share them) and left unchanged"""
    if c.key not in _cache:
        if len(_cache) >= 2:                       # the big ones are a few hundred MB each
            _cache.pop(next(iter(_cache)))
        d = cl.make_inputs(c)
        ref, dt = cl.timed_reference(c, d)
        ref.setflags(write=False)
        _cache[c.key] = (d, ref, dt)
        _seconds[c.key] = dt
    return _cache[c.key]


def test_phase_gather_matches_conv_transpose(oracle):
    """weights gathered as w[phase][co][tap][ci] = Wt[ci][co][KY[py][ty]][KY[px][tx]] make the four phases ConvTranspose2d k4 s2 p1"""
    rng = np.random.default_rng(1)
    c = cl.Case("ct_check", "h3", "ct", 2, 5, 7, 32, 8, 0)
    x = rng.standard_normal((c.n, c.H, c.W, c.Cin)).astype(np.float32)
    wt = rng.standard_normal((c.Cin, c.cols, 4, 4)).astype(np.float32)
    w = np.empty((4, c.cols, 4, c.Cin), np.float32)
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                for tx in range(2):
                    w[py * 2 + px, :, ty * 2 + tx, :] = wt[:, :, cl.KY[py][ty], cl.KY[px][tx]].T
    got = cl.accumulate(c, x, w).numpy()
    want = oracle.conv_transpose2d(x.transpose(0, 3, 1, 2), wt, 2, 1).transpose(0, 2, 3, 1)
    assert got.shape == want.shape == (2, 10, 14, 8)
    assert np.abs(got - want).max() < 1e-12


@pytest.mark.parametrize("up", [0, 1])
def test_nine_tap_gather_matches_conv2d_padding_1(up):
    rng = np.random.default_rng(2)
    c = cl.Case("c3_check", "h3", "c3", 2, 6, 10, 32, 8, 0, up=up)
    x = rng.standard_normal((c.n, c.H >> up, c.W >> up, c.Cin)).astype(np.float32)
    k = rng.standard_normal((c.cols, c.Cin, 3, 3)).astype(np.float32)
    w = k.reshape(c.cols, c.Cin, 9).transpose(0, 2, 1)[None]               # [1][cols][tap = ky * 3 + kx][ci]
    xt = torch.from_numpy(x).double().permute(0, 3, 1, 2)
    if up:
        xt = F.interpolate(xt, scale_factor=2, mode="nearest")
    want = F.conv2d(xt, torch.from_numpy(k).double(), padding=1).permute(0, 2, 3, 1).numpy()
    assert np.abs(cl.accumulate(c, x, w).numpy() - want).max() < 1e-12


def test_epilogue_of_the_reference():
    """act(acc * scale[c % cmod] + shift[c % cmod]) + residual, written out by hand for one element per channel"""
    c = cl.Case("epi_check", "f32", "one", 1, 2, 2, 32, 8, 0, cmod=4, act=2, residual=True)
    d = cl.make_inputs(c)
    ref = cl.reference(c, d)
    for ch in range(8):
        acc = float(np.dot(d["x"][0, 1, 0].astype(np.float64), d["w"][0, ch, 0].astype(np.float64)))
        v = acc * float(d["scale"][ch % 4]) + float(d["shift"][ch % 4])
        v = v if v >= 0 else float(np.float32(np.float32(0.2) * np.float32(v)))
        assert ref[0, 1, 0, ch] == v + float(d["residual"][0, 1, 0, ch])


def test_tail_of_the_reference():
    c = cl.Case("tail_check", "h3", "ct", 1, 2, 2, 32, 64, 0, act=1, tail=True, out="split")
    d = cl.make_inputs(c)
    hid = cl.reference(c, d, hidden=True)
    ref = cl.reference(c, d)
    assert ref.shape == (48, 16) and hid.min() >= 0
    assert ref[5, 7] == float(np.dot(hid.reshape(16, 64)[7], d["tail_w"][5].astype(np.float64)))


@pytest.mark.parametrize("c", EXACT, ids=repr)
def test_exactness_preconditions(c):
    d, ref, _ = case_data(c)
    assert cl.exactness_problems(c, d, ref) == []
    assert d["x"].min() != 0 and np.abs(d["w"]).min() != 0                  # no zeros: a missing zero fill must show
    if c.sat == "below":
        assert ref.max() * cl.ACT_SCALE == 65488.0
    if c.sat == "above":
        assert ref.max() * cl.ACT_SCALE == 65520.0 and np.sort(np.abs(ref).ravel())[-2] * cl.ACT_SCALE < cl.F16_MAX
    if c.inputs == "arith_w":                                              # one operand only carries a low half (lo * lo is dropped by design)
        assert np.array_equal(d["x"], np.round(d["x"])) and not np.array_equal(d["w"], np.round(d["w"]))
    if c.inputs == "arith_x":
        assert np.array_equal(d["w"], np.round(d["w"])) and not np.array_equal(d["x"], np.round(d["x"]))


@pytest.mark.parametrize("key", BIG)
def test_big_reference_is_quick(key):
    """the GPU test computes every reference in its child process: a few seconds each at the most (16 threads there)"""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    if key not in _seconds:
        case_data(cl.BY_NAME[key])
    print("%s: float64 reference %.2f s" % (key, _seconds[key]))
    assert _seconds[key] < REF_SECONDS


def test_forms_cover_every_instantiation():
    forms = set(c.form for c in cl.ALL_CASES)
    for f in (cl.FP32_WIDE, cl.FP32_NARROW, cl.H3 | 0, cl.H3 | 1, cl.H3 | 2, cl.H3 | 5, cl.H3 | 3, cl.H3 | 4, cl.HALO | 1, cl.HALO | 2):
        assert f in forms
    for flag in (cl.UP, cl.T4, cl.XONCE):
        assert any(f & cl.H3 and f & flag for f in forms)


def test_split_layout_round_trip():
    rng = np.random.default_rng(3)
    v = (rng.standard_normal((5, 96)) * 1000).astype(np.float32)
    v[0, :4] = [65504.0, -65504.0, 1.0 + 2.0 ** -12, 4093.0 * 16]
    buf = cl.encode_split(v)
    assert len(buf) == 5 * 96 * 4
    raw = np.frombuffer(buf, np.float16)
    # by hand: value (row 3, channel 70) = chunk 2, element 6: hi at half 3 * 192 + 2 * 64 + 6, lo 32 halves further
    hi, lo = raw[3 * 192 + 2 * 64 + 6], raw[3 * 192 + 2 * 64 + 32 + 6]
    assert hi == np.float16(v[3, 70]) and lo == np.float16(v[3, 70] - np.float32(hi))
    back = cl.decode_split(buf, 5, 96)
    assert np.abs(back - v).max() <= np.abs(v).max() * 2.0 ** -21          # ~22 mantissa bits
    assert np.array_equal(back[0, :4], v[0, :4].astype(np.float64))
    q = back.astype(np.float32)                                            # values that ARE hi + lo survive exactly
    assert np.array_equal(cl.decode_split(cl.encode_split(q), 5, 96), back)


def test_planar_decoder():
    c = cl.Case("planar_check", "f32", "one", 2, 2, 2, 32, 8, 0, out="planar")
    a = np.arange(8 * 8, dtype=np.float32).reshape(8, 8)                    # [col][position]
    out = cl.decode_output(c, a.tobytes())
    assert out.shape == (2, 2, 2, 8) and out[1, 0, 1, 3] == a[3, 5]
