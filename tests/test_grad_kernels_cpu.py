"""No GPU: the host side of tests/test_gpu_grad_kernels.py.

  * the float64 restatements of tests/grad_kernels_common.py agree with torch float64 autograd on the edge inputs -- so "the first maximum in row-major
    order", "slope 0.2 at exactly zero" and "taps mirrored" are torch's rules, not this project's reading of them;
  * every exactness precondition holds and no case passes vacuously (all 81 tie patterns, zero positions, tied cells, sums below 2^24);
  * the comparison itself works: with the float32 restatement standing in for the device every case passes, and with any of the named wrong variants
    standing in for it the case's own comparison, on its own inputs, fails;
  * the ctypes struct has the layout of the C struct.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import grad_kernels_common as gk

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def inputs():
    return {c.name: c.make() for c in gk.ALL_CASES}


# ------------------------------------------------------------------------------------------------------------ a stand-in device
def index_maps(c, d, imgs, variant=None):
    """per output name, where in the raw buffers (buffer, flat index) the kernel's layout puts every value: unpack() applied to index arrays"""
    _, _, _, shapes, _ = c.launch(d, imgs)
    raws, base = [], 0
    for s in shapes:
        if s is None:
            raws.append(None)
            continue
        size = int(np.prod(s))
        raws.append((np.arange(size, dtype=F64) + base).reshape(s))
        base += size
    raws += [None] * (2 - len(raws))
    out, _ = c.unpack(d, raws, len(imgs), variant)
    return out, shapes, base


def fake_run(c, d, imgs, values, layout_variant=None):
    """what run_case would return if the device wrote `values` (dict name -> [len(imgs)][P][C]) in the kernel's layout (or a wrong variant of it)"""
    maps, shapes, total = index_maps(c, d, imgs, layout_variant)
    flat = np.frombuffer(bytes([gk.SENTINEL]) * (4 * total), F32).copy()
    for k, idx in maps.items():
        flat[idx.astype(np.int64).reshape(-1)] = np.asarray(values[k], F32).reshape(-1)
    raws, base = [], 0
    for s in shapes:
        if s is None:
            raws.append(None)
            continue
        size = int(np.prod(s))
        raws.append(flat[base:base + size].reshape(s))
        base += size
    raws += [None] * (2 - len(raws))
    out, rest = c.unpack(d, raws, len(imgs))
    return out, rest


LAYOUT_VARIANTS = ("not_chunked", "phase_swapped")


def simulate(c, d, variant=None):
    if variant in LAYOUT_VARIANTS:
        want = c.expect(d, F32)
        dev3, rest3 = fake_run(c, d, [0, 1, 2], want, variant)
        dev1, _ = fake_run(c, d, [0], {k: v[:1] for k, v in want.items()}, variant)
    else:
        want = c.expect(d, F32, variant)
        dev3, rest3 = fake_run(c, d, [0, 1, 2], want)
        dev1, _ = fake_run(c, d, [0], {k: v[:1] for k, v in want.items()})
    r = gk.evaluate(c, d, dev3, rest3, dev1, True)
    return gk.verdict(c, r), r


@pytest.mark.parametrize("c", gk.ALL_CASES, ids=repr)
def test_float32_restatement_passes_its_own_case(c, inputs):
    bad, r = simulate(c, inputs[c.name])
    assert bad == [], (bad, r)
    if not c.exact:
        for k, e in r["err_f32"].items():
            assert 0 < max(e) < 1e-5 or (max(e) == 0 and c.name.endswith("_notanh")), (k, e)      # a float32 evaluation, and a real-valued one
        assert all(v == 0 for v in r["ulp"].values())
        # positions at which the formula cancels beyond float32: the one-hot position of the tap cases with nothing arriving from above, nowhere else
        one_hot_mode0 = isinstance(c, gk.ActGrad) and c.kind == "tap" and c.mode == 0
        assert r["ill"] == ({"out": gk.N_IMG, "part": 0} if one_hot_mode0 else {k: 0 for k in r["ill"]}), r["ill"]
        assert all(v < 1e-4 for v in r["pos_f32"].values()), r["pos_f32"]      # the largest: 1 - y^2 of tanh's gradient at |y| = 0.9999


VARIANT_CASES = [(c, v) for c in gk.ALL_CASES for v in c.variants]


@pytest.mark.parametrize("c,variant", VARIANT_CASES, ids=lambda x: x if isinstance(x, str) else repr(x))
def test_wrong_variant_is_detected(c, variant, inputs):
    bad, r = simulate(c, inputs[c.name], variant)
    assert bad != [], (variant, r)


def test_every_named_variant_has_a_case():
    named = {v for _, v in VARIANT_CASES}
    # last maximum; >= where the kernel has > (pool ties: tie_all, ReLU: relu_ge); taps not mirrored; y / x swapped on 4 x 2; output not chunked;
    # py / px swapped; slope 0 at zero.  "The projection term kept at r == 0" is test_projection_term_at_zero_norm below.
    assert named >= {"last_max", "tie_all", "relu_ge", "not_mirrored", "transposed", "swap_yx", "not_chunked", "phase_swapped", "slope0"}
    for kind, v in (("act_grad_ties", "swap_yx"), ("maxpool", "swap_yx"), ("conv1_grad", "swap_yx"), ("act_grad_ties", "not_chunked"),
                    ("pg_pn_grad", "not_chunked"), ("pg_leaky", "not_chunked"), ("relu_bn_grad_rows", "not_chunked"), ("pg_pn_grad", "slope0"),
                    ("pg_leaky", "slope0")):
        assert any(c.name.startswith(kind) and x == v for c, x in VARIANT_CASES), (kind, v)


def test_every_kernel_and_template_arm_has_a_case():
    names = " ".join(c.name for c in gk.ALL_CASES)
    for C in gk.J_WIDTHS:
        for stem in ("act_grad_ties_c%d_mode2", "act_grad_mask_c%d_mode1", "act_grad_tap_c%d_mode0", "act_grad_tap_c%d_mode1", "act_grad_tap_c%d_mode2",
                     "ref_rows_c%d"):
            assert stem % C in names
    for stem in ("conv1_f32", "conv1_u8", "maxpool_", "conv1_grad_4x2", "conv1_grad_4x4", "lpips_loss_", "tanh_grad_cot", "tanh_grad_l2", "patch_rgb",
                 "relu_bn_grad_planar_c32", "relu_bn_grad_planar_c64", "relu_bn_grad_rows_kc64", "pg_out_grad_cot", "pg_out_grad_l2", "_notanh",
                 "pg_rgb_grad_plain_nc1", "pg_rgb_grad_plain_nc3", "pg_rgb_grad_pool_nc1", "pg_rgb_grad_pool_nc3", "pg_leaky_grad", "pg_rowpn_grad_d64",
                 "pg_rowpn_grad_d100"):
        assert stem in names
    for C in (32, 64, 160):
        for p in ("plain", "pool"):
            for e in ("extra", "noextra"):
                assert "pg_pn_grad_c%d_%s_%s" % (C, p, e) in names


# ------------------------------------------------------------------------------------------------------------ preconditions
def test_tie_cases_hold_all_81_patterns_and_distinct_D(inputs):
    for c in gk.ALL_CASES:
        if not (isinstance(c, gk.ActGrad) and c.kind == "ties"):
            continue
        d = inputs[c.name]
        cl = gk.cells(d["a"]).transpose(0, 1, 2, 4, 3).reshape(gk.N_IMG, -1, 4)
        for img in range(gk.N_IMG):
            codes = set((cl[img] @ np.array([1, 3, 9, 27])).astype(int).tolist())
            assert codes == set(range(81)), (c.name, img)
            assert len(np.unique(d["D"][img])) == d["D"][img].size and (d["D"][img] > 0).all()
        assert set(np.unique(d["a"]).tolist()) == {0.0, 1.0, 2.0} and d["D"].max() < 2 ** 24
        tied = (gk.cells(d["a"]) == gk.cells(d["a"]).max(axis=3, keepdims=True)).sum(axis=3) > 1
        zero = gk.cells(d["a"]).max(axis=3) == 0
        assert tied.sum() > 0 and zero.sum() > 0
        want = c.expect(d)["out"].reshape(d["a"].shape)
        assert (gk.cells(want)[zero[:, :, :, None, :].repeat(4, axis=3)] == 0).all()            # all-zero cells give nothing
        assert ((gk.cells(want) != 0).sum(axis=3) == (~zero)).all()                              # one taker per cell with a positive maximum


def test_real_tap_cases_have_zero_positions_single_channels_and_ties(inputs):
    for c in gk.ALL_CASES:
        if not (isinstance(c, gk.ActGrad) and c.kind == "tap"):
            continue
        a = inputs[c.name]["a"]
        assert ((a == 0).all(axis=-1).sum(axis=(1, 2)) >= 2).all(), c.name
        assert (((a > 0).sum(axis=-1) == 1).sum(axis=(1, 2)) >= 1).all(), c.name
        cl = gk.cells(a)
        tied = ((cl == cl.max(axis=3, keepdims=True)).sum(axis=3) == 4)
        assert (tied & (cl.max(axis=3) > 0)).sum(axis=(1, 2, 3)).min() >= 1 and (tied & (cl.max(axis=3) == 0)).sum(axis=(1, 2, 3)).min() >= 1, c.name
        want = c.expect(inputs[c.name], F64)
        zero = (a == 0).all(axis=-1).reshape(gk.N_IMG, -1)
        assert (want["out"][zero] == 0).all()
        ref, lin = inputs[c.name]["ref"].astype(F64), inputs[c.name]["lin"].astype(F64)
        np.testing.assert_allclose(want["part"][..., 0][zero], (lin * ref * ref).sum(axis=-1).reshape(gk.N_IMG, -1)[zero], rtol=1e-12)


def test_mask_and_unit_zero_cases_hold_their_zeros(inputs):
    for c in gk.ALL_CASES:
        d = inputs[c.name]
        if isinstance(c, gk.ActGrad) and c.kind == "mask":
            a = d["a"]
            assert ((a == 0) & np.signbit(a)).any() and ((a == 0) & ~np.signbit(a)).any() and (a > 0).any()
        if isinstance(c, gk.PnGrad):
            a = d["a"]
            assert (a == 0).all(axis=-1).sum() >= gk.N_IMG and ((a == 0).sum(axis=-1) < c.C).any() and ((a == 0) & np.signbit(a)).any()
            assert np.isclose(d["inv"][(a == 0).all(axis=-1)], 1e4).all()
        if isinstance(c, (gk.LeakyGrad,)):
            assert (d["h"] == 0).any() and (d["h"] < 0).any() and (d["h"] > 0).any()
        if isinstance(c, gk.ReluBn):
            assert (d["a"] == 0).any() and (d["a"] > 0).any() and (np.frexp(d["scale"])[0] == 0.5).all()
        if isinstance(c, gk.MaxPool) and c.kind == "ties":
            cl = gk.cells(d["x"])
            assert ((cl == cl.max(axis=3, keepdims=True)).sum(axis=3) > 1).any() and (cl.max(axis=3) == 0).any()
        if isinstance(c, gk.RefRows):
            f = d["f"]
            assert ((f == 0).all(axis=-1).sum(axis=1) >= 2).all() and (((f != 0).sum(axis=-1) == 1).sum(axis=1) >= 1).all()
            want = c.expect(d)["out"]
            assert (want[(f == 0).all(axis=-1)] == 0).all()
            assert (want[(f != 0).sum(axis=-1) == 1].max(axis=-1) == 1).all()
        if isinstance(c, (gk.Conv1, gk.OutGrad)) and getattr(c, "u8", False) and c.h * c.w * 3 >= 256:
            assert set(np.unique(d["img"][0]).tolist()) == set(range(256))
        if isinstance(c, gk.OutGrad) and c.l2:
            assert all(set(np.unique(d["target"][i]).tolist()) == set(range(256)) for i in range(gk.N_IMG))
        if isinstance(c, gk.OutGrad) and not c.l2:
            assert set(np.unique(d["y"]).tolist()) == {-1.0, -0.5, 0.0, 0.5, 1.0}


def test_exact_cases_stay_below_2_to_24(inputs):
    """every sum an exact case forms, in any order, is an integer (or an integer times a power of two) below 2^24"""
    lim = 2.0 ** 24
    for c in gk.EXACT_CASES:
        d = inputs[c.name]
        if isinstance(c, gk.RefRows):
            assert np.array_equal(d["f"], np.round(d["f"])) and (d["f"].astype(F64) ** 2).sum(axis=-1).max() < lim
        elif isinstance(c, gk.Conv1Grad):
            assert np.array_equal(d["gpre"], np.round(d["gpre"])) and np.array_equal(d["w"], np.round(d["w"]))
            assert len(np.unique(d["w"])) == d["w"].size
            assert 9 * 64 * np.abs(d["gpre"]).max() * np.abs(d["w"]).max() < lim
            assert (d["y"][0] == gk.pixel_of_u8(d["target"][0])).sum() >= d["y"][0].size - 3 and (d["y"] != gk.pixel_of_u8(d["target"])).any()
        elif isinstance(c, gk.RgbGrad):
            assert np.array_equal(d["g"], np.round(d["g"])) and np.array_equal(d["w"], np.round(d["w"]))
            assert 4 * c.nc * np.abs(d["g"]).max() * np.abs(d["w"]).max() < lim
        elif isinstance(c, gk.OutGrad):
            assert np.array_equal(d["cot"], np.round(d["cot"])) and np.abs(d["cot"]).max() * 4 < lim         # cot * 3/4: quarters
        elif isinstance(c, gk.PatchRgb):
            assert len(np.unique(d["g4"][0])) == d["g4"][0].size and d["g4"].max() < lim
        elif isinstance(c, gk.ReluBn):
            assert len(np.unique(d["dA"][:2])) == d["dA"][:2].size and d["dA"].max() * 8 < lim
        elif isinstance(c, gk.LeakyGrad):
            assert np.array_equal(d["dA"], np.round(d["dA"]))
        want32, want64 = c.expect(d, F32), c.expect(d, F64)
        for k in want32:
            if isinstance(c, (gk.RefRows, gk.Conv1Grad, gk.LeakyGrad)):          # single rounded operations after exact sums: close, and met bit for bit
                np.testing.assert_allclose(want32[k], want64[k], rtol=3e-7, atol=0)
            else:
                assert np.array_equal(want32[k].astype(F64), want64[k]), (c.name, k)


# ------------------------------------------------------------------------------------------------------------ torch is the judge of the rules
def test_first_maximum_in_row_major_order_is_torchs_rule(inputs):
    for name in ("act_grad_ties_c64_mode2_4x4", "act_grad_ties_c64_mode2_4x2"):
        c, d = gk.BY_NAME[name], inputs[name]
        pre = torch.from_numpy(d["a"].astype(F64)).permute(0, 3, 1, 2).clone().requires_grad_(True)
        pooled = F.max_pool2d(F.relu(pre), 2)
        (g,) = torch.autograd.grad(pooled, pre, torch.from_numpy(d["D"].astype(F64)).permute(0, 3, 1, 2))
        want = c.expect(d, F64)["out"].reshape(d["a"].shape)
        assert np.array_equal(g.permute(0, 2, 3, 1).numpy(), want)
        assert not np.array_equal(want, c.expect(d, F64, "last_max")["out"].reshape(d["a"].shape))


def test_relu_mask_at_zero_is_torchs_rule(inputs):
    c, d = gk.BY_NAME["act_grad_mask_c64_mode1_4x2"], inputs["act_grad_mask_c64_mode1_4x2"]
    pre = torch.from_numpy(d["a"].astype(F64)).requires_grad_(True)
    (g,) = torch.autograd.grad(F.relu(pre), pre, torch.from_numpy(d["D"].astype(F64)))
    assert np.array_equal(g.numpy().reshape(gk.N_IMG, -1, 64), c.expect(d, F64)["out"])


def test_pixelnorm_leaky_formula_against_autograd_at_zero():
    rng = np.random.default_rng(5)
    n, H, C = 2, 4, 160
    pre = rng.standard_normal((n, H, H, C))
    pre[:, :, :, 3] = 0
    pre[0, 1, 2, 7] = -0.0
    dA = rng.standard_normal((n, H, H, C))
    h = torch.from_numpy(pre).requires_grad_(True)
    x = F.leaky_relu(h, 0.2)
    inv = torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + 1e-8)
    (g,) = torch.autograd.grad(x * inv, h, torch.from_numpy(dA))
    a, iv = (x * inv).detach().numpy(), inv.detach().numpy()[..., 0]
    got = gk.pn_grad(dA, a, iv, None, 0, F64).reshape(n, H, H, C)
    np.testing.assert_allclose(got, g.numpy(), rtol=1e-11, atol=1e-13)
    assert (a == 0).sum() >= n * H * H
    wrong = gk.pn_grad(dA, a, iv, None, 0, F64, "slope0").reshape(n, H, H, C)
    assert np.abs(wrong - g.numpy()).max() > 1e-3
    # with the 2 x 2 sums and the second toRGB branch's term
    dA2, extra = rng.standard_normal((n, 2 * H, 2 * H, C)), rng.standard_normal((n, H, H, C))
    h = torch.from_numpy(pre).requires_grad_(True)
    x = F.leaky_relu(h, 0.2)
    y = x * torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + 1e-8)
    up = y.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    (g,) = torch.autograd.grad((up * torch.from_numpy(dA2)).sum() + (y * torch.from_numpy(extra)).sum(), h)
    np.testing.assert_allclose(gk.pn_grad(dA2, a, iv, extra, 1, F64).reshape(n, H, H, C), g.numpy(), rtol=1e-11, atol=1e-13)


def test_tap_gradient_against_autograd_away_from_zero_norm():
    rng = np.random.default_rng(6)
    n, h, w, C = 2, 4, 2, 128
    f = np.abs(rng.standard_normal((n, h, w, C))) + 0.01
    ref = gk.ref_rows(np.abs(rng.standard_normal((n, h * w, C))), F64).reshape(n, h, w, C)
    lin = np.abs(rng.standard_normal(C))
    D = rng.standard_normal((n, h, w, C))
    ft = torch.from_numpy(f).requires_grad_(True)
    a = F.relu(ft)
    nrm = a / (torch.sqrt((a * a).sum(dim=-1, keepdim=True)) + 1e-10)
    loss = 0.2 * ((nrm - torch.from_numpy(ref)) ** 2 * torch.from_numpy(lin)).sum(dim=-1).mean(dim=(1, 2)).sum() + (a * torch.from_numpy(D)).sum()
    (g,) = torch.autograd.grad(loss, ft)
    out, part = gk.act_grad(f, D, 1, ref, lin, F64)
    np.testing.assert_allclose(out.reshape(n, h, w, C), g.numpy(), rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(part.reshape(n, h, w), ((nrm.detach().numpy() - ref) ** 2 * lin).sum(axis=-1), rtol=1e-12)


def test_projection_term_at_zero_norm(inputs):
    """Where r == 0 the formula takes the projection term as 0; torch's graph (the direction f / r) gives NaN there.  Every channel of such a position
    is 0, so the ReLU mask of the same kernel turns whatever the tap gradient is into 0: the two readings differ before the mask and cannot differ
    in `out` -- which is what the GPU cases assert at these positions (exactly 0), together with `part`."""
    c = gk.BY_NAME["act_grad_tap_c128_mode1_4x2"]
    d = inputs[c.name]
    zero = (d["a"] == 0).all(axis=-1)
    g, _ = gk.act_grad(d["a"], d["D"], c.mode, d["ref"], d["lin"], F64, before_mask=True)
    g_nan, _ = gk.act_grad(d["a"], d["D"], c.mode, d["ref"], d["lin"], F64, "proj_kept", before_mask=True)
    assert zero.sum() >= 2 * gk.N_IMG and np.isfinite(g).all() and np.isnan(g_nan[zero]).all() and np.allclose(g[~zero], g_nan[~zero], rtol=1e-8, atol=1e-12)
    g32, _ = gk.act_grad(d["a"], d["D"], c.mode, d["ref"], d["lin"], F32, before_mask=True)
    assert np.isfinite(g32).all()
    assert (c.expect(d, F32)["out"].reshape(d["a"].shape)[zero] == 0).all()


def test_conv1_and_its_mirrored_gradient_against_torch(inputs):
    for name in ("conv1_grad_4x2", "conv1_grad_4x4"):
        c, d = gk.BY_NAME[name], inputs[name]
        x = torch.zeros((gk.N_IMG, 3, c.h, c.w), dtype=torch.float64, requires_grad=True)
        out = F.conv2d(x, torch.from_numpy(d["w"].astype(F64)), padding=1)
        (g,) = torch.autograd.grad(out, x, torch.from_numpy(d["gpre"].astype(F64)).permute(0, 3, 1, 2))
        diff = (d["y"] - gk.pixel_of_u8(d["target"])).astype(F64)
        want = g.numpy() / gk.LP_SCALE.astype(F64).reshape(1, 3, 1, 1) + 2.0 / (3 * c.h * c.w) * diff
        np.testing.assert_allclose(c.expect(d, F64)["out"].reshape(want.shape), want, rtol=1e-12, atol=1e-12)
    c, d = gk.BY_NAME["conv1_f32_4x2"], inputs["conv1_f32_4x2"]
    v = (d["img"].astype(F64) - gk.LP_SHIFT.astype(F64).reshape(1, 3, 1, 1)) / gk.LP_SCALE.astype(F64).reshape(1, 3, 1, 1)
    out = F.relu(F.conv2d(torch.from_numpy(v), torch.from_numpy(d["w"].astype(F64)), torch.from_numpy(d["b"].astype(F64)), padding=1))
    np.testing.assert_allclose(c.expect(d, F64)["out"], out.permute(0, 2, 3, 1).reshape(gk.N_IMG, -1, 64).numpy(), rtol=1e-12, atol=1e-13)


def test_dcgan_layouts_against_torch(inputs):
    """patch rows x the layer's weights = the data gradient of ConvTranspose2d(k4 s2 p1); the phase-planar form holds position (2 y + py, 2 x + px)"""
    d = inputs["patch_rgb"]
    rng = np.random.default_rng(7)
    W4 = rng.integers(-3, 4, (5, 3, 4, 4)).astype(F64)                    # [ci][co][ky][kx]
    a3 = torch.zeros((1, 5, 32, 32), dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose2d(a3, torch.from_numpy(W4), stride=2, padding=1)
    (g,) = torch.autograd.grad(y, a3, torch.from_numpy(d["g4"][:1].astype(F64)))
    patch = gk.patch_rgb(d["g4"][:1]).astype(F64)[0, :, :48]              # [pos][(ky * 4 + kx) * 3 + co]
    pk = W4.transpose(0, 2, 3, 1).reshape(5, 48)
    assert np.array_equal(patch @ pk.T, g[0].permute(1, 2, 0).reshape(1024, 5).numpy())
    assert (gk.patch_rgb(d["g4"])[:, :, 48:] == 0).all()
    full = np.arange(2 * 4 * 4 * 8, dtype=F64).reshape(2, 4, 4, 8)
    planar = np.stack([full[:, py::2, px::2] for py in (0, 1) for px in (0, 1)])
    assert np.array_equal(gk.planar_unpack(planar, 2, 4, 4, 8), full)


# ------------------------------------------------------------------------------------------------------------ the ABI
def test_struct_layout():
    assert ctypes.sizeof(gk.TuneGradOp) == gk.STRUCT_LAYOUT["size"] == 224
    for f in ("ip", "in_", "in_bytes", "out", "out_bytes", "out_guards"):
        assert getattr(gk.TuneGradOp, f).offset == gk.STRUCT_LAYOUT[f], f
    assert gk.TuneGradOp.family.offset == 0 and gk.TuneGradOp.op.offset == 4 and gk.TuneGradOp.sentinel.offset == 8 and gk.TuneGradOp.copy_in.offset == 12
    assert gk.TuneGradOp.poison.offset == 16 and gk.TuneGradOp.f0.offset == 20
