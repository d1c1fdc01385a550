"""CPU: the host side of tests/test_gpu_attention_grad.py -- the hand-written backward formulas of the attention block against float64 autograd,
the exactness preconditions of the zero-tolerance cases, the allowance for the hardware exponential, and the mirrored structure."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import attention_grad_common as ag

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("c", [c for c in ag.ALL_CASES if c.kind != "uniform"], ids=repr)
def test_formulas_equal_float64_autograd(c):
    d = ag.make_inputs(c)
    f, g = ag.backward64(c, d), ag.autograd(c, d, torch.float64)
    for n in ag.PARTS:
        scale = max(np.abs(g[n]).max(), 1e-300)
        assert np.abs(f[n] - g[n]).max() <= 1e-12 * scale + (1e-9 if c.kind == "onehot" else 0.0), (n, np.abs(f[n] - g[n]).max(), scale)
        assert f[n].shape == d["q" if n != "dv" else "v"].shape


@pytest.mark.parametrize("c", ag.EXACT_CASES, ids=repr)
def test_exact_cases_satisfy_their_preconditions(c):
    d = ag.make_inputs(c)
    assert ag.exactness_problems(c, d) == []
    for name, a in d.items():
        assert np.array_equal(a[0], a[2])
        assert name in ("q", "k") or not np.array_equal(a[0], a[1])
    want = ag.closed_form(c, d)
    if c.kind == "gamma0":
        f = ag.backward64(c, d)
        assert all(not f[n].any() and not want[n].any() for n in ag.PARTS)
    else:
        assert want["dv"].any() and not want["dq"].any() and not want["dk"].any()
    if c.kind == "uniform":
        # dE itself is not zero in the uniform case: the zeros of dq and dk come from k = 0 and q = 0
        assert np.abs(ag.backward64(c, d, full=True)["dE"]).max() > 0


def test_a_broken_precondition_is_reported():
    c = ag.BY_NAME["onehot_c64"]
    d = ag.make_inputs(c)
    d["k"] = d["k"] / 8                              # energies 64 apart: the runner-up's weight is no longer 0 in float32
    assert any("runner-up" in p for p in ag.exactness_problems(c, d))
    d = ag.make_inputs(c)
    d["dY"][1, 3, 5] += 0.25
    assert "dY is not integer" in ag.exactness_problems(c, d)


@pytest.mark.parametrize("c", ag.REAL_CASES, ids=repr)
def test_float32_reference_and_allowance(c):
    d = ag.make_inputs(c)
    f = ag.backward64(c, d, full=True)
    g32 = ag.autograd(c, d, torch.float32)
    allow = ag.exp_allowance(c, d, f)
    for n in ag.PARTS:
        a = ag.row_errors(g32[n], f[n])
        assert a.shape == (3,) and (a > 0).all() and (a < 1e-4).all(), (n, a)
        assert allow[n].shape == (3,) and (allow[n] > 0).all() and (allow[n] < 1e-3).all(), (n, allow[n])
        assert a[0] == a[2] and allow[n][0] == allow[n][2]
        print("%s %s: float32 CPU %s  allowance %s" % (c.name, n, a, allow[n]))
    # a perturbation of the weights of the assumed size stays inside the allowance (first order: a factor 1.01 for the second)
    rng = np.random.default_rng(5)
    eps = (np.abs(f["t"]) + 1.0) * 2.0 ** -23
    P = f["P"] * (1.0 + eps * rng.choice([-1.0, 1.0], eps.shape))
    P /= P.sum(axis=2, keepdims=True)
    D = (P * f["dP"]).sum(axis=2, keepdims=True)
    dE = P * (f["dP"] - D)
    moved = {"dq": np.einsum("nij,njd->nid", dE, d["k"].astype(np.float64)), "dk": np.einsum("nij,nid->njd", dE, d["q"].astype(np.float64)),
             "dv": np.einsum("nij,nic->njc", P, f["dO"])}
    for n in ag.PARTS:
        assert (ag.row_errors(moved[n], f[n]) <= 1.01 * allow[n]).all(), n


def test_structure_mirrors_the_tuning_entry():
    src = open(os.path.join(ROOT, "gan-leaks_amd", "csrc", "gl_tune.hip")).read()
    body = re.search(r"struct GlTuneAttentionGrad \{(.*?)\n\};", src, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip().lstrip("*") for n in decl.split(None, 1)[1].replace("const ", "").split(",")] if not decl.startswith("const") else \
                     [n.strip().lstrip("*") for n in decl.split(None, 2)[2].split(",")]
    assert names == [n for n, _ in ag.TuneAttentionGrad._fields_], names
    assert ctypes.sizeof(ag.TuneAttentionGrad) == 72
    assert 'extern "C" int gl_tune_attention_grad(gl_ctx *ctx, GlTuneAttentionGrad *q)' in src
    for c in ag.ALL_CASES:
        assert c.cols % 32 == 0 and 0 <= c.cols - (2 * c.DK + c.C) < 32
