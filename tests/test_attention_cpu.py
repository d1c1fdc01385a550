"""No GPU: the cases and host references that tests/test_gpu_attention.py rests on (tests/attention_common.py).

(a) every case compared with zero tolerance meets its exactness preconditions, asserted from the inputs and the closed forms alone: integer
    q, k, v and 16 x, sums of absolute products below 2^24, gamma a power of two, the result a float32 and (split) hi + lo of two halves;
(b) the constructions do what they claim in float32: energies all zero (uniform), the row maximum at j = pi(i) with every other energy at
    least 104 below, so that every other float32 weight is exactly 0 (one-hot), two weights of exactly 1 with the third energy 256 below
    (two-hot), and the largest |16 y| exactly 65504 / 65520 at the planted elements only (clamp);
(c) the closed forms agree with the float64 softmax reference;
(d) the real-valued cases are in the regimes they are named after, and the split layout is the one written out by hand.
"""
import ctypes

import numpy as np
import pytest

import attention_common as ac

_cache = {}


def data(c):
    if c.name not in _cache:
        d = ac.make_inputs(c)
        for a in d.values():
            a.setflags(write=False)
        _cache[c.name] = d
    return _cache[c.name]


def test_case_grid():
    names = [c.name for c in ac.ALL_CASES]
    assert len(set(names)) == len(names)
    for C in (64, 128):
        for split in (False, True):
            kinds = sorted(c.base for c in ac.ALL_CASES if c.C == C and c.split == split)
            want = ["onehot", "twohot_b2", "twohot_b5", "uniform", "uniform_lo"] + ["real_%s%s" % (t, z) for t in ac.TEMPS for z in ("", "_x0")]
            assert kinds == sorted(want + (["clamp_at", "clamp_over"] if split else []))
    assert ctypes.sizeof(ac.TuneAttention) == 72
    for img in (0, 1):
        p = ac.perm(img)
        assert sorted(p) == list(range(ac.T)) and not (p == np.arange(ac.T)).any()
        assert ((p // 32) != (np.arange(ac.T) // 32)).mean() > 0.8 and (((p >> 2) & 1) != ((np.arange(ac.T) >> 2) & 1)).any()


@pytest.mark.parametrize("c", ac.ALL_CASES, ids=repr)
def test_images_0_and_2_are_equal_and_image_1_differs(c):
    d = data(c)
    for n, a in d.items():
        assert a.dtype == np.float32 and np.array_equal(a[0], a[2])
        if not ((n == "x" and c.x_zero) or (n == "q" and c.kind.startswith("uniform")) or (n == "k" and c.exact and not c.kind.startswith("uniform"))):
            assert not np.array_equal(a[0], a[1]), n
    if c.split:
        assert np.array_equal(ac.split_round(d["x"]), d["x"].astype(np.float64))


@pytest.mark.parametrize("c", ac.EXACT_CASES, ids=repr)
def test_exactness_preconditions(c):
    d = data(c)
    assert ac.exactness_problems(c, d) == []
    assert np.abs(d["v"]).min() >= 1 and np.abs(d["x"]).min() > 0            # no zeros: a dropped term must show
    y64 = ac.reference64(c, d)[0]
    assert np.abs(ac.closed_form(c, d) - y64).max() <= 1e-12 * np.abs(y64).max()
    w, es = ac.weights32(d)
    idx = np.arange(ac.T)
    if c.kind.startswith("uniform"):
        assert not d["q"].any() and d["k"].any() and np.array_equal(w, np.ones_like(w))
        assert w.sum(axis=2, dtype=np.float32).max() == 256.0 == w.sum(axis=2, dtype=np.float32).min()
    elif c.kind == "twohot":
        assert (es[:, :, -1] == es[:, :, -2]).all() and (es[:, :, -2] - es[:, :, -3] >= 256).all() and 256 >= ac.EXP_ZERO_GAP
        for img in range(ac.N_IMG):
            a = ac.perm(img)
            want = np.zeros((ac.T, ac.T), np.float32)
            want[idx, a] = 1
            want[idx, a ^ (1 << c.b)] = 1
            assert np.array_equal(w[img], want)
        assert (w.sum(axis=2) == 2.0).all()
        a = ac.perm(0)
        if c.b == 2:        # the partner: same 32-row block, other lane half (bit 2 of j is the lane half)
            assert ((a ^ 4) // 32 == a // 32).all()
        else:
            assert ((a ^ 32) // 32 != a // 32).all()
    else:                   # one-hot (the clamp cases are one-hot too)
        assert es.max() == 512.0 and (es[:, :, -1] - es[:, :, -2] >= ac.EXP_ZERO_GAP).all()
        for img in range(ac.N_IMG):
            want = np.zeros((ac.T, ac.T), np.float32)
            want[idx, ac.perm(img)] = 1
            assert np.array_equal(w[img], want)
    if c.kind == "uniform_lo":                                               # some stored x carry a non-zero lo half
        s = d["x"].astype(np.float64) * ac.ACT_SCALE
        assert (s != s.astype(np.float16).astype(np.float64)).mean() > 0.05
    elif c.split and not c.kind.startswith("clamp"):
        s = d["x"].astype(np.float64) * ac.ACT_SCALE
        assert np.array_equal(s, s.astype(np.float16).astype(np.float64))


@pytest.mark.parametrize("c", [c for c in ac.EXACT_CASES if c.kind.startswith("clamp")], ids=repr)
def test_clamp_cases_sit_at_the_fp16_limit(c):
    d = data(c)
    t = ac.closed_form(c, d) * ac.ACT_SCALE
    top = 65504.0 if c.kind == "clamp_at" else 65520.0
    assert t.max() == top and t.min() == -top
    sites = np.zeros(t.shape, bool)
    for img in range(ac.N_IMG):
        for (i, ch, s) in ac.clamp_sites(img):
            sites[img, i, ch] = True
            assert t[img, i, ch] == s * top
    assert np.abs(t[~sites]).max() < 4096                                    # everything else far inside
    assert np.array_equal(ac.expected_exact(c, d) * ac.ACT_SCALE != t, sites if c.kind == "clamp_over" else np.zeros_like(sites))


@pytest.mark.parametrize("c", [c for c in ac.REAL_CASES if not c.split], ids=repr)
def test_real_cases_are_in_their_regime(c):
    d = data(c)
    y, p, t, out = ac.reference64(c, d)
    e = np.einsum("nid,njd->nij", d["q"].astype(np.float64), d["k"].astype(np.float64))
    pmax = p.max(axis=2)
    if c.temp == "mild":
        assert np.abs(e).max() < 7 and pmax.max() < 0.3
    if c.temp == "peaked":
        assert (pmax > 0.5).mean() > 0.75
    if c.temp == "extreme":
        assert np.abs(e).max() > 3000 and np.median(np.abs(e)) > 500
        e32 = np.sort(np.einsum("nid,njd->nij", d["q"], d["k"]), axis=2)
        assert (e32[:, :, -1] > e32[:, :, -2]).all()                         # no exact ties, in float32 either
    a, b = ac.row_errors(ac.reference32(c, d), y), ac.exp_allowance(c, d, (y, p, t, out))
    print("%s: float32 CPU error %s, exponential allowance %s" % (c.name, a, b))
    assert (a > 0).all() and (a < 1e-4).all() and (b > 0).all() and (b < 1e-4).all()
    assert (d["x"] == 0).all() == c.x_zero


def test_split_layout_by_hand():
    """value (position, channel c): hi half at byte position * 4 C + (c >> 5) * 128 + (c & 31) * 2, lo half 64 bytes on, both of value * 16"""
    c = ac.BY_NAME["uniform_lo_c128_split"]
    d = data(c)
    buf = ac.x_bytes(c, d, [0, 1, 2])
    assert len(buf) == 3 * ac.T * c.C * 4
    raw = np.frombuffer(buf, np.uint8)
    for (img, i, ch) in ((0, 0, 0), (1, 3, 1), (1, 255, 127), (2, 77, 33), (1, 9, 95)):
        off = (img * ac.T + i) * c.C * 4 + (ch >> 5) * 128 + (ch & 31) * 2
        hi, lo = raw[off:off + 2].view(np.float16)[0], raw[off + 64:off + 66].view(np.float16)[0]
        s = np.float32(d["x"][img, i, ch]) * np.float32(16)
        assert hi == np.float16(s) and lo == np.float16(s - np.float32(hi)) and float(hi) + float(lo) == float(s)
    assert np.array_equal(ac.decode_y(c, buf, 3), d["x"].astype(np.float64))
    f = ac.BY_NAME["uniform_lo_c128_f32"]
    assert ac.x_bytes(f, data(f), [1]) == data(f)["x"][1].tobytes()
    assert ac.pack_qkv(d, [1]).shape == (1, ac.T, 16 + 16 + 128) and np.array_equal(ac.pack_qkv(d, [1])[0, :, 32:], d["v"][1])
