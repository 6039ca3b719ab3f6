"""The f32 and bf16 convolution planners and the two data-gradient entry points on a real MI355X: the recorded plans
(tests/golden/conv_plans_f32_bf16.json) replayed through the device library, and ds_conv_dgrad_f32 / ds_conv_dgrad_bf16 at
the kernel level on the emulator tests' own cases (conv_cases.py) against the oracle's conv2d_bwd in float64.

The cases are small (1x4 to 16x32 maps, batch 1 to 3): a 3x3 stride-1 gradient with a part-empty last row block and one
with whole-image segments, and 5x5 stride-2 gradients -- four parity-class launches whose outputs interleave -- with even
sizes, an odd height (the classes differ in size), a 7x8 map into multi-image tiles and a one-row map whose odd-row
classes are empty.  Every output starts as NaN: a pixel no class writes fails the comparison.

Bounds: those test_emul_kernels.py holds the same cases to, 2e-6 (exact f32 products) and 3e-5 (16 mantissa bits per
operand), on the max-norm relative error it uses and on the relative L2 error.
Measured on one MI355X (max-norm / L2): f32 6.3e-8 .. 4.6e-7 / 7.1e-8 .. 2.1e-7; bf16x3 3.9e-6 .. 5.4e-6 / 4.4e-6 .. 4.6e-6."""
import ctypes

import numpy as np
import pytest
import torch

import deepspeaker_oracle as O
from conftest import rel_err
from conv_cases import DGRAD_BF16_CASES, DGRAD_CASES
from conv_plan_cases import load_fixture, resolve_rows
from test_gpu_train_f16_kernels import dev, eng, full, host     # noqa: F401  (eng: the module-scoped engine fixture)

pytestmark = pytest.mark.gpu

_REFS = {}


def test_plans_on_the_device_library_are_the_recorded_ones():
    from deepspeaker_pytorch_amd import _native
    got, want = resolve_rows(_native.load()), load_fixture()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)


def _problem(case):
    """filter, output gradient and the float64 input gradient of a case (the emulator tests' data), computed once"""
    if case not in _REFS:
        b, ci, co, h, w, k, s = case
        rs = np.random.RandomState(abs(hash(case)) % 2**31)
        x = rs.randn(b, ci, h, w)
        wt = rs.randn(co, ci, k, k) / np.sqrt(ci * k * k)
        ho, wo = O.conv_out_size(h, k, s, k // 2), O.conv_out_size(w, k, s, k // 2)
        gy = rs.randn(b, co, ho, wo)
        gx_ref, _ = O.conv2d_bwd(x, wt, gy, s, k // 2)
        _REFS[case] = (wt, gy, gx_ref)
    return _REFS[case]


def _check(case, gx, bound, what):
    _, _, gx_ref = _problem(case)
    got = host(gx).transpose(0, 3, 1, 2).astype(np.float64)
    err = rel_err(got, gx_ref)                               # NaN anywhere: nan < bound is False
    l2 = float(np.linalg.norm(got - gx_ref) / np.linalg.norm(gx_ref))
    print(f"{what} {case}: max-norm relative {err:.2e}, relative L2 {l2:.2e} (bar {bound:.0e})")
    assert err < bound and l2 < bound, (err, l2)


@pytest.mark.parametrize("case", DGRAD_CASES)
def test_conv_dgrad_f32(eng, case):
    from deepspeaker_pytorch_amd._native import ConvShape
    b, ci, co, h, w, k, s = case
    wt, gy, _ = _problem(case)
    p = eng._p
    w_d, g_d = dev(wt, torch.float32), dev(gy.transpose(0, 2, 3, 1), torch.float32)
    wp, gx = full((wt.size,), torch.float32), full((b, h, w, ci), torch.float32)
    st = eng._stream(g_d)
    if s == 1:
        eng.lib.call("ds_pack_conv_weight_f32", p(w_d), p(wp), co, ci, k, 1, st)
    else:
        eng.lib.call("ds_pack_conv_dgrad_s2_f32", p(w_d), p(wp), co, ci, st)
    eng.lib.call("ds_conv_dgrad_f32", ctypes.byref(ConvShape(b, h, w, ci, co, k, s)), p(g_d), p(wp), p(gx), st)
    torch.cuda.synchronize()
    _check(case, gx, 2e-6, "dgrad f32")


@pytest.mark.parametrize("case", DGRAD_BF16_CASES)
def test_conv_dgrad_bf16x3(eng, case):
    from deepspeaker_pytorch_amd._native import ConvShape
    b, ci, co, h, w, k, s = case
    wt, gy, _ = _problem(case)
    p = eng._p
    w_d, g_d = dev(wt, torch.float32), dev(gy.transpose(0, 2, 3, 1), torch.float32)
    n = wt.size if s == 1 else 36 * co * ci
    whi, wlo = full((n,), torch.bfloat16), full((n,), torch.bfloat16)
    gx = full((b, h, w, ci), torch.float32)
    st = eng._stream(g_d)
    if s == 1:
        eng.lib.call("ds_pack_conv_weight_dgrad_bf16", p(w_d), p(whi), p(wlo), co, ci, k, st)
    else:
        eng.lib.call("ds_pack_conv_weight_dgrad_s2_bf16", p(w_d), p(whi), p(wlo), co, ci, st)
    eng.lib.call("ds_conv_dgrad_bf16", ctypes.byref(ConvShape(b, h, w, ci, co, k, s)), p(g_d), p(whi), p(wlo), p(gx), st)
    torch.cuda.synchronize()
    _check(case, gx, 3e-5, "dgrad bf16x3")
