"""The pipelined walk of the bf16x3 forward convolution (PIPE of conv_mfma_bf16_kernel.h; ds_conv_bf16_set_walk): case
lists and test bodies, written once against the backend adapter of bf16_train_cases.py and run by test_emul_bf16_walk.py
(host emulator) and test_gpu_bf16_walk.py (MI355X).

The pipelined walk accumulates every output element over the same k-steps in the same term order as the classic walk, so
pipelined against classic is an EQUALITY OF BITS on every output element.  So that "equal to a wrong classic walk" cannot
pass, every pipelined output is also held to the bf16x3 forward bar of bf16_train_cases.body_conv_fwd (2e-5, max-norm
relative) against the float64 convolution.

Shapes: the smallest at which the pipeline takes another path.  Cin = 16 (one chunk: the prologue's chunk is also the
last), 32 (one buffer swap), 48 (odd chunk count: the last chunk sits in buffer 0), 64 for the instances whose filter ring
holds a whole chunk's 25 taps (two chunks whose refills are not clamped).  3x3 stride 1 and 5x5 stride 2.  Cout: the
planner admits multiples of 64 that the row's N tile divides, so one N tile, two and three (64 / 128 / 192) for the
64-wide rows and one and two (128 / 256) for the 128-wide one; a ragged last N tile does not exist.  Maps: 3x5 (ragged
pixel tile), 10x4 with B = 3 (whole images in one tile), 8x8 with B = 1 (a single workgroup per N tile)."""
import contextlib
import ctypes

import numpy as np

import bf16_latency_cases as LC
import bf16_train_cases as BC
import deepspeaker_oracle as O
from conftest import rel_err
from deepspeaker_pytorch_amd._native import (ConvShape, DS_CONV_PLAN_LATENCY, DS_EPI_AFFINE, DS_EPI_CLIP, DS_EPI_RESIDUAL)

F32, F64 = np.float32, np.float64
CLASSIC, PIPELINED = 1, 2
AC = DS_EPI_AFFINE | DS_EPI_CLIP
FLAGS = (0, AC, AC | DS_EPI_RESIDUAL)
Y_BAR = 2e-5                                   # bf16_train_cases.body_conv_fwd, bf16x3

# forced configuration -> (M tile, N tile, threads): the rows with a pipelined instantiation (ds_bf16_has_pipe)
PIPE_ROWS = {0: (128, 64, 256), 9: (64, 64, 256), 10: (32, 128, 256)}
NO_PIPE_ROW = 1                                # 160 x 128: no pipelined instantiation
KERNELS = ((3, 1), (5, 2))                     # (KS, stride)
MAPS = ((1, 3, 5), (3, 10, 4), (1, 8, 8))      # (B, H, W)


def cins(cfg, k):
    return (16, 32, 48) + ((64,) if k == 5 and cfg in (9, 10) else ())


def couts(cfg):
    return (64, 128, 192) if PIPE_ROWS[cfg][1] == 64 else (128, 256)


@contextlib.contextmanager
def walk(lib, w):
    """a process-global hook, as bf16_train_cases.forced_cfg: it goes back to the planner's choice whatever happens"""
    try:
        lib.raw("ds_conv_bf16_set_walk")(w)
        yield
    finally:
        lib.raw("ds_conv_bf16_set_walk")(0)


def plan_walk(lib, shp, flags):
    return lib.raw("ds_conv_bf16_plan_walk")(ctypes.byref(shp), 1, flags)


def _reference(x, wt, scale, shift, res, k, s, flags):
    z = O.conv2d(BC.to_nchw(x).astype(F64), wt.astype(F64), s, k // 2)
    if flags & DS_EPI_AFFINE:
        z = z * scale[None, :, None, None] + shift[None, :, None, None]
    if flags & DS_EPI_RESIDUAL:
        z = z + BC.to_nchw(res)
    if flags & DS_EPI_CLIP:
        z = np.clip(z, 0.0, 20.0)
    return z


def body_walks_are_bit_identical(be, cfg, k, s, bhw):
    """row `cfg` forced, DS_CONV_PLAN_LATENCY set: the pipelined launch == the classic launch on every output element,
    for every Cin, Cout and epilogue of the lists above; the pipelined output within Y_BAR of float64"""
    b, h, w = bhw
    worst = 0.0
    for ci in cins(cfg, k):
        for co in couts(cfg):
            geom = (ci, co, h, w, k, s)
            shp = ConvShape(b, h, w, ci, co, k, s)
            x, wt, scale, shift, res, yshape = LC._inputs(geom, b)
            hi, lo = BC.pack_fwd_bank(be, wt, True)
            dev = (be.put(x), hi, lo, be.put(scale), be.put(shift), be.put(res))
            with BC.forced_cfg(be.lib, cfg):
                rc, out8 = LC.describe(be.lib, shp, DS_CONV_PLAN_LATENCY)
                assert rc == 0 and (out8[0], out8[1], out8[6]) == PIPE_ROWS[cfg], (cfg, geom, b, rc, out8)
                for flags in FLAGS:
                    fl = flags | DS_CONV_PLAN_LATENCY
                    with walk(be.lib, CLASSIC):
                        assert plan_walk(be.lib, shp, fl) == CLASSIC
                        y1 = LC._launch(be, shp, dev, fl, yshape)
                    with walk(be.lib, PIPELINED):
                        assert plan_walk(be.lib, shp, fl) == PIPELINED
                        y2 = LC._launch(be, shp, dev, fl, yshape)
                    got = be.get(y2)
                    assert np.isfinite(got).all(), f"{geom} B={b} cfg {cfg} flags {flags}: an output element was not written"
                    assert be.same(y1, y2), f"{geom} B={b} cfg {cfg} flags {flags}: pipelined != classic"
                    err = rel_err(BC.to_nchw(got), _reference(x, wt, scale, shift, res, k, s, flags))
                    worst = max(worst, err)
                    assert err < Y_BAR, (geom, b, cfg, flags, err)
    print(f"cfg {cfg} ({PIPE_ROWS[cfg][0]}x{PIPE_ROWS[cfg][1]}) {k}x{k} s{s} map {bhw}: Cin {cins(cfg, k)} x Cout {couts(cfg)} x "
          f"{len(FLAGS)} epilogues bit-identical; worst error against float64 {worst:.2e} (bar {Y_BAR:.0e})")


def body_selection(lib):
    """the planner's choice: classic without the flag and, with it, at a chip-filling batch; pipelined at B = 1 and 12
    with the flag, for all seven stage convolutions.  Forced: 1 is classic where the planner would pipeline; 2 on a row
    without a pipelined instantiation is DS_ERR_UNSUPPORTED from the plan and from the launch."""
    def shape(b, geom):
        ci, co, h, w, k, s = geom
        return ConvShape(b, h, w, ci, co, k, s)

    for geom in LC.GEOMETRIES:
        for b in (1, 12, 768):
            assert plan_walk(lib, shape(b, geom), 0) == CLASSIC, (geom, b)
        assert plan_walk(lib, shape(768, geom), DS_CONV_PLAN_LATENCY) == CLASSIC, geom
        for b in (1, 12):
            s = shape(b, geom)
            assert plan_walk(lib, s, DS_CONV_PLAN_LATENCY) == PIPELINED, (geom, b)
            rc0, piped = LC.describe(lib, s, DS_CONV_PLAN_LATENCY)
            with walk(lib, CLASSIC):
                assert plan_walk(lib, s, DS_CONV_PLAN_LATENCY) == CLASSIC
                rc1, classic = LC.describe(lib, s, DS_CONV_PLAN_LATENCY)
            # the same tile either way; only the LDS request differs (two pixel tiles)
            assert rc0 == 0 and rc1 == 0 and piped[:5] == classic[:5] and piped[6:] == classic[6:], (classic, piped)
            assert classic[5] <= piped[5] <= 160 * 1024, (classic, piped)
    s = shape(12, LC.GEOMETRIES[6])
    with BC.forced_cfg(lib, NO_PIPE_ROW), walk(lib, PIPELINED):
        assert plan_walk(lib, s, DS_CONV_PLAN_LATENCY) == BC.DS_ERR_UNSUPPORTED
        one = np.zeros(8, F32)
        p = (one.ctypes.data + 15) & ~15         # (an aligned non-null address: the call is refused before anything is read)
        rc = lib.raw("ds_conv_fwd_bf16")(ctypes.byref(s), p, p, p, None, None, None, p, None, DS_CONV_PLAN_LATENCY, None)
        assert rc == BC.DS_ERR_UNSUPPORTED, rc
    with BC.forced_cfg(lib, NO_PIPE_ROW):        # the planner's own choice never fails for want of an instantiation
        assert plan_walk(lib, s, DS_CONV_PLAN_LATENCY) == CLASSIC
    assert plan_walk(lib, s, DS_CONV_PLAN_LATENCY) == PIPELINED         # the hooks are back at their defaults


def body_forward_eval(make_engine, x, sd_torch, n_stages=4):
    """forward_eval_planned(precision="bf16x3", low_latency=True) under the classic and under the pipelined walk, bit
    for bit, and both equal to low_latency=False.  `make_engine()` -> a fresh Engine (each holds its own cached plans)."""
    import torch
    from deepspeaker_pytorch_amd.engine import BNParams
    out = {}
    for w in (CLASSIC, PIPELINED):
        eng = make_engine()
        pw = eng.pack_weights(sd_torch, n_stages, with_bf16=True)
        names = [n for i in range(1, n_stages + 1) for n in (f"model.bn{i}", f"model.layer{i}.0.bn1", f"model.layer{i}.0.bn2")]
        folded = {n: eng.bn_fold(BNParams(sd_torch[n + ".weight"], sd_torch[n + ".bias"], sd_torch[n + ".running_mean"],
                                          sd_torch[n + ".running_var"])) for n in names}
        with walk(eng.lib, w):
            out[w] = eng.forward_eval_planned(x, pw, folded, precision="bf16x3", low_latency=True).clone()
            if w == CLASSIC:
                out[0] = eng.forward_eval_planned(x, pw, folded, precision="bf16x3", low_latency=False).clone()
    assert bool(torch.isfinite(out[0]).all())
    for w in (CLASSIC, PIPELINED):
        assert torch.equal(out[0].view(torch.int32), out[w].view(torch.int32)), w
