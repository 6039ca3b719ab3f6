"""The fp16 convolution on a real MI355X after its plan resolution and the kernels' shared parts were written once:
the recorded plans (tests/golden/f16_conv_plans.json) replayed through the device library, every form a launch can take
(XCD queues / one queue / 64-wide / one tile per workgroup) bitwise equal on the emulator's cases, and the BasicBlock
kernel bitwise equal to two convolution calls.

Template instantiations these cases reach, read off the recorded plans (B, Cin, Cout, H, W, KS, stride):
  k3db    the NO_PERSIST run of every 3x3 case, (1, 32, 64, 12, 100) by default (13 items: not persistent), split-K
  k5db    the NO_PERSIST run of every 5x5 case, (1, 64, 128, 21, 64) by default (14 items)
  k5c16   the CHUNK16 | NO_PERSIST run of every 5x5 case
  k3sb / k5sb   not here: a plan is single-buffered only under the SINGLE_BUFFER hint at these sizes, which
          test_gpu_bench_size.py::test_conv_f16_kernel and test_gpu_f16_kernels.py (every configuration) run
  pk3     LIN at 16 items: (2, 64, 64, 11, 32), (3 / 96, 64, 64, 27, 32) (12 items); LIN at 8: (3 / 9, 32, 128, 20, 8),
          (2, 32, 128, 100, 4); without LIN: (5, 96, 128, 10, 4), (11, 64, 128, 10, 4), (1, 64, 64, 3, 5)
  pk5     without LIN: (3 / 7, 32, 256, 9, 8); LIN at 16 items: (3, 64, 128, 43, 16) (11 items)
  pk5c16  (2, 64, 128, 21, 16) by default (the 5x5 chunk-width switch), every 5x5 case under CHUNK16
  cfg 7   (7, 64, 256, 10, 4), (8, 32, 512, 10, 4), (40, 64, 256, 10, 4) -- and cfg 4 of the same layers under NO_WIDE
  block   both widths: <2, 1, 12> at (3, 11, 32, 64), <1, 2, 6> at (3, 11, 16, 128), and the MASKED form of each
All of these plan the two-wave configurations 3, 4 and 7.  The four-wave ones (1, 2, 5) are what the planner picks for the
network's layers at bench-size batches (rows of the golden file at batch 768), and configurations 0 and 6 win no recorded
shape (tools/f16_cfg_ab.py forces them): test_gpu_f16_kernels.py launches every kernel under each of 0 .. 6 forced in turn --
persistent and one tile per workgroup, single-buffered, 16-channel chunks, plane-major input and output, workgroups that walk
several tiles, split-K up to 8 ways, the block kernel's XCD-dealt order -- against float64 and bit for bit among them."""
import ctypes

import pytest
import torch

from f16_conv_cases import CASES, PERSIST_CASES
from f16_plan_cases import load_fixture, resolve_rows

pytestmark = pytest.mark.gpu

TOL = 20 * 2.0 ** -11 + 1e-5        # one fp16 rounding of a value in [0, 20] plus the f32 epilogue (test_gpu_parity.py)
EXTRA = [
    (96, 64, 64, 27, 32, 3, 1),     # 576 row-block tiles against 512 resident two-wave workgroups: the workgroups walk tiles
    (40, 64, 256, 10, 4, 3, 1),     # cfg 7, several tiles
]
RUNS = list(dict.fromkeys(CASES + PERSIST_CASES + EXTRA))


def test_plans_on_the_device_library_are_the_recorded_ones():
    from deepspeaker_pytorch_amd import _native
    got, want = resolve_rows(_native.load()), load_fixture()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)


def _operands(case, seed):
    from deepspeaker_pytorch_amd.model import get_engine
    eng = get_engine()
    b, ci, co, h, w, k, s = case
    g = torch.Generator(device="cpu").manual_seed(seed + sum(case))
    x = (torch.randn(b, h, w, ci, generator=g).abs() * 2).half().cuda()
    wt = (torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5).half().float().cuda()
    sc, sh = (torch.rand(co, generator=g) + 0.5).cuda(), torch.randn(co, generator=g).cuda()
    return eng, x, wt, eng._pack_f16(wt, k), sc, sh


def _reference(x, wt, sc, sh, k, s, nb):
    ref = torch.nn.functional.conv2d(x[:nb].permute(0, 3, 1, 2).double().cpu(), wt.double().cpu(), None, s, k // 2)
    return (ref * sc.double().cpu()[None, :, None, None] + sh.double().cpu()[None, :, None, None]).clamp(0, 20).permute(0, 2, 3, 1)


@pytest.mark.parametrize("case", RUNS)
def test_every_form_of_a_launch_is_bitwise_the_same(case):
    from deepspeaker_pytorch_amd._native import (ConvShape, DS_CONV_HINT_CHUNK16, DS_CONV_HINT_NO_PERSIST, DS_CONV_HINT_NO_WIDE,
                                                 DS_CONV_HINT_ONE_QUEUE, DS_EPI_AFFINE, DS_EPI_CLIP)
    eng, x, wt, wp, sc, sh = _operands(case, 41)
    b, ci, co, h, w, k, s = case
    ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
    shp, st = ConvShape(b, h, w, ci, co, k, s), eng._stream(x)
    outs = {}
    for name, hint in (("default", 0), ("one queue", DS_CONV_HINT_ONE_QUEUE), ("64-wide", DS_CONV_HINT_NO_WIDE),
                       ("one tile per workgroup", DS_CONV_HINT_NO_PERSIST)):
        y = torch.full((b, ho, wo, co), float("nan"), dtype=torch.float16, device="cuda")
        eng.lib.call("ds_conv_fwd_f16", ctypes.byref(shp), eng._p(x), eng._p(wp), eng._p(sc), eng._p(sh), None, eng._p(y),
                     DS_EPI_AFFINE | DS_EPI_CLIP | hint, st)
        outs[name] = y
    c16 = []
    if k == 5:                      # 16-channel chunks: the persistent kernel against the one-tile kernel
        for hint in (DS_CONV_HINT_CHUNK16, DS_CONV_HINT_CHUNK16 | DS_CONV_HINT_NO_PERSIST):
            c16.append(torch.full((b, ho, wo, co), float("nan"), dtype=torch.float16, device="cuda"))
            eng.lib.call("ds_conv_fwd_f16", ctypes.byref(shp), eng._p(x), eng._p(wp), eng._p(sc), eng._p(sh), None, eng._p(c16[-1]),
                         DS_EPI_AFFINE | DS_EPI_CLIP | hint, st)
    torch.cuda.synchronize()
    for name, y in outs.items():
        assert bool(torch.isfinite(y.float()).all()), name
        assert torch.equal(y, outs["default"]), name
    if c16:
        assert bool(torch.isfinite(c16[0].float()).all()) and torch.equal(c16[0], c16[1])
    if case == EXTRA[1]:
        out8 = (ctypes.c_int * 8)()
        eng.lib.call("ds_conv_f16_plan_describe", ctypes.byref(shp), out8)
        assert out8[7] >= 10000 and (out8[0], out8[1], out8[6]) == (128, 256, 128), list(out8)      # cfg 7
        eng.lib.call("ds_conv_f16_plan_describe_hinted", ctypes.byref(shp), DS_CONV_HINT_NO_WIDE, out8)
        assert out8[7] >= 10000 and (out8[0], out8[1], out8[6]) == (128, 128, 128), list(out8)      # cfg 4
    nb = min(b, 8)
    err = float((outs["default"][:nb].double().cpu() - _reference(x, wt, sc, sh, k, s, nb)).abs().max())
    print(case, "max |y - float64 reference| =", err)
    assert err <= TOL


def test_split_k_launch_with_its_workspace():
    """the contraction split over workgroups, then the reduce kernel with the epilogue"""
    from deepspeaker_pytorch_amd._native import ConvShape, DS_EPI_AFFINE, DS_EPI_CLIP
    case = (1, 64, 128, 10, 4, 3, 1)
    eng, x, wt, wp, sc, sh = _operands(case, 43)
    b, ci, co, h, w, k, s = case
    shp = ConvShape(b, h, w, ci, co, k, s)
    ws_bytes = eng.lib.raw("ds_conv_f16_splitk_workspace_bytes")(ctypes.byref(shp))
    assert ws_bytes == 2 * b * h * w * co * 4          # two chunks: two ways
    ws = torch.full((ws_bytes // 4,), float("nan"), device="cuda")
    y = torch.full((b, h, w, co), float("nan"), dtype=torch.float16, device="cuda")
    eng.lib.call("ds_conv_fwd_f16_splitk", ctypes.byref(shp), eng._p(x), eng._p(wp), eng._p(sc), eng._p(sh), None, eng._p(y),
                 DS_EPI_AFFINE | DS_EPI_CLIP, eng._p(ws), ws_bytes, eng._stream(x))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ws).all())               # every partial sum was written: the launch was split
    err = float((y.double().cpu() - _reference(x, wt, sc, sh, k, s, b)).abs().max())
    print(case, "split-K max |y - float64 reference| =", err)
    assert err <= TOL


@pytest.mark.parametrize("geom,lens", [((3, 11, 32, 64), None), ((3, 11, 16, 128), None), ((3, 11, 32, 64), (11, 5, 8)),
                                       ((3, 11, 16, 128), (11, 5, 8))])
def test_block_kernel_is_bitwise_two_convolutions(geom, lens):
    from deepspeaker_pytorch_amd._native import ConvShape, DS_EPI_AFFINE, DS_EPI_CLIP, DS_EPI_RESIDUAL
    from deepspeaker_pytorch_amd.model import get_engine
    eng = get_engine()
    b, h, w, c = geom
    g = torch.Generator(device="cpu").manual_seed(47 + sum(geom))
    x = (torch.randn(b, h, w, c, generator=g).abs() * 2).half().cuda()
    packs = [eng._pack_f16((torch.randn(c, c, 3, 3, generator=g) / (c * 9) ** 0.5).cuda(), 3) for _ in range(2)]
    folds = [((torch.rand(c, generator=g) + 0.5).cuda(), (torch.randn(c, generator=g) * 0.5).cuda()) for _ in range(2)]
    st, p = eng._stream(x), eng._p
    shp = ConvShape(b, h, w, c, c, 3, 1)
    lens_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")
    if lens is not None:        # the batch as the variable-length forward hands it over: zero past each extent
        eng.lib.call("ds_mask_rows", p(x), p(lens_d), b, h, w * c * 2, st)
    mid = torch.full((b, h, w, c), float("nan"), dtype=torch.float16, device="cuda")
    ref = torch.full_like(mid, float("nan"))
    got = torch.full_like(mid, float("nan"))
    eng.lib.call("ds_conv_fwd_f16", ctypes.byref(shp), p(x), p(packs[0]), p(folds[0][0]), p(folds[0][1]), None, p(mid),
                 DS_EPI_AFFINE | DS_EPI_CLIP, st)
    if lens is not None:
        eng.lib.call("ds_mask_rows", p(mid), p(lens_d), b, h, w * c * 2, st)
    eng.lib.call("ds_conv_fwd_f16", ctypes.byref(shp), p(mid), p(packs[1]), p(folds[1][0]), p(folds[1][1]), p(x), p(ref),
                 DS_EPI_AFFINE | DS_EPI_CLIP | DS_EPI_RESIDUAL, st)
    if lens is None:
        eng.lib.call("ds_conv_block_f16", p(x), p(packs[0]), p(packs[1]), p(folds[0][0]), p(folds[0][1]), p(folds[1][0]),
                     p(folds[1][1]), p(got), b, h, w, c, 0, st)
    else:
        eng.lib.call("ds_mask_rows", p(ref), p(lens_d), b, h, w * c * 2, st)
        eng.lib.call("ds_conv_block_f16_masked", p(x), p(packs[0]), p(packs[1]), p(folds[0][0]), p(folds[0][1]), p(folds[1][0]),
                     p(folds[1][1]), p(got), p(lens_d), b, h, w, c, 0, st)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got.float()).all()) and float(got.float().abs().max()) > 0
    assert torch.equal(got, ref)
    if lens is not None:
        for i, n in enumerate(lens):
            assert not bool(got[i, n:].any())
