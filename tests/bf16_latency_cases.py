"""The latency plan mode of the bf16x3 forward convolution (DS_CONV_PLAN_LATENCY; kCfgBLat of conv_mfma_bf16_kernel.h):
case lists and test bodies, written once against the backend adapter of bf16_train_cases.py and run by
test_emul_bf16_latency.py (host emulator) and test_gpu_bf16_latency.py (MI355X).

Every check here is an EQUALITY OF BITS: the mode picks another tile of the same kernel, and every tile accumulates an
output element over the same k-steps in the same order (hi*lo, lo*hi, hi*hi per step), so no tolerance is involved."""
import ctypes

import numpy as np

import bf16_train_cases as BC
from deepspeaker_pytorch_amd._native import (ConvShape, DS_CONV_PLAN_LATENCY, DS_EPI_AFFINE, DS_EPI_CLIP, DS_EPI_RESIDUAL,
                                             DS_EPI_STATS)

F32 = np.float32
AC = DS_EPI_AFFINE | DS_EPI_CLIP
LAT_ROWS = {9: (64, 64, 256), 10: (32, 128, 256)}        # forced configuration -> (M tile, N tile, threads): kCfgBLat

# the network's seven stage convolutions: (Cin, Cout, H, W, KS, stride) of the INPUT map
GEOMETRIES = [
    (64, 64, 80, 32, 3, 1),
    (64, 128, 80, 32, 5, 2),
    (128, 128, 40, 16, 3, 1),
    (128, 256, 40, 16, 5, 2),
    (256, 256, 20, 8, 3, 1),
    (256, 512, 20, 8, 5, 2),
    (512, 512, 10, 4, 3, 1),      # 40 pixels per image: ragged 32- and 64-pixel tiles, tiles that span images
]
BATCHES = (1, 3)
# (geometry, B) each forced latency row runs at: both kernel sizes, the 32 x 128 row needs Cout % 128 == 0; the 10 x 4
# maps for the ragged / image-spanning tiles
FORCED_CASES = [(GEOMETRIES[2], 1), (GEOMETRIES[1], 1), (GEOMETRIES[6], 1), (GEOMETRIES[6], 3), (GEOMETRIES[5], 1)]


def describe(lib, shp, flags):
    out8 = (ctypes.c_int * 8)()
    rc = lib.raw("ds_conv_bf16_plan_describe_hinted")(ctypes.byref(shp), 1, flags, out8)
    return rc, list(out8)


def _inputs(geom, b):
    ci, co, h, w, k, s = geom
    ho, wo = BC.out_dims(h, w, k, s)
    rs = np.random.RandomState(BC.seed_of(b, *geom))
    x = rs.randn(b, h, w, ci).astype(F32)
    wt = (rs.randn(co, ci, k, k) / np.sqrt(ci * k * k)).astype(F32)
    scale = rs.uniform(0.5, 1.5, co).astype(F32)
    shift = (10.0 + rs.randn(co)).astype(F32)                  # with the residual: both clip edges are reached
    res = (rs.randn(b, ho, wo, co) * 12.0).astype(F32)
    return x, wt, scale, shift, res, (b, ho, wo, co)


def _launch(be, shp, dev, flags, yshape):
    x_d, hi, lo, sc, sh, rs_d = dev
    y = be.nan(yshape, F32)
    be.lib.call("ds_conv_fwd_bf16", ctypes.byref(shp), be.p(x_d), be.p(hi), be.p(lo), be.p(sc), be.p(sh),
                be.p(rs_d) if flags & DS_EPI_RESIDUAL else None, be.p(y), None, flags, be.stream)
    return y


def _device_copies(be, geom, b):
    x, wt, scale, shift, res, yshape = _inputs(geom, b)
    hi, lo = BC.pack_fwd_bank(be, wt, True)
    return (be.put(x), hi, lo, be.put(scale), be.put(shift), be.put(res)), yshape


def body_flag_is_bit_identical(be, geom, b):
    """ds_conv_fwd_bf16 (x3, affine + clip; the 3x3 shapes also with a residual) with DS_CONV_PLAN_LATENCY == without"""
    ci, co, h, w, k, s = geom
    shp = ConvShape(b, h, w, ci, co, k, s)
    dev, yshape = _device_copies(be, geom, b)
    rc0, plan0 = describe(be.lib, shp, 0)
    rc1, plan1 = describe(be.lib, shp, DS_CONV_PLAN_LATENCY)
    assert rc0 == 0 and rc1 == 0, (rc0, rc1)
    print(f"{geom} B={b}: default plan {plan0[0]}x{plan0[1]} ({plan0[4]} workgroups), latency plan {plan1[0]}x{plan1[1]} "
          f"({plan1[4]} workgroups)")
    # one to three images leave the chip far short of a wave per SIMD: the mode must act, i.e. plan a latency row
    assert (plan1[0], plan1[1], plan1[6]) in LAT_ROWS.values() and plan1 != plan0, (geom, b, plan0, plan1)
    for flags in (AC,) + ((AC | DS_EPI_RESIDUAL,) if k == 3 else ()):
        y0 = _launch(be, shp, dev, flags, yshape)
        y1 = _launch(be, shp, dev, flags | DS_CONV_PLAN_LATENCY, yshape)
        got = be.get(y0)
        assert np.isfinite(got).all(), "an output element was not written"
        assert float((got == 0).mean()) < 0.9 and float((got == 20).mean()) < 0.9        # not clipped flat
        assert be.same(y0, y1), (geom, b, flags)


def body_forced_row_is_bit_identical(be, geom, b, cfg):
    """the launch through a forced latency row == the planner's own launch; the plan is that row's"""
    ci, co, h, w, k, s = geom
    shp = ConvShape(b, h, w, ci, co, k, s)
    dev, yshape = _device_copies(be, geom, b)
    flags = AC | (DS_EPI_RESIDUAL if k == 3 else 0)
    y0 = _launch(be, shp, dev, flags, yshape)
    with BC.forced_cfg(be.lib, cfg):
        rc, out8 = describe(be.lib, shp, 0)
        assert rc == 0 and (out8[0], out8[1], out8[6]) == LAT_ROWS[cfg], (cfg, rc, out8)
        y1 = _launch(be, shp, dev, flags, yshape)
    print(f"{geom} B={b} forced row {cfg}: {out8[0]}x{out8[1]}, {out8[3]} segments of {out8[2]} rows per tile, {out8[4]} workgroups")
    assert np.isfinite(be.get(y1)).all()
    assert be.same(y0, y1), (geom, b, cfg)


def body_plan_mode(lib):
    """with the flag, 12 rows of the 512-channel 3x3 layer plan onto a latency row and 768 rows onto today's tile; without
    it both are today's.  Also: every stage convolution of a 768-row batch keeps its plan under the flag, a forced
    latency row is refused to plain bf16, and the flag is refused together with the statistics epilogue."""
    def shape(b, geom=GEOMETRIES[6]):
        ci, co, h, w, k, s = geom
        return ConvShape(b, h, w, ci, co, k, s)

    old = (ctypes.c_int * 8)()
    for b in (12, 768):
        assert lib.raw("ds_conv_bf16_plan_describe")(ctypes.byref(shape(b)), 1, old) == 0
        rc, off = describe(lib, shape(b), 0)
        assert rc == 0 and off == list(old), (b, off, list(old))
        rc, on = describe(lib, shape(b), DS_CONV_PLAN_LATENCY)
        assert rc == 0
        print(f"512-channel 3x3, {b} rows: default {off[0]}x{off[1]} / {off[4]} workgroups, latency mode {on[0]}x{on[1]} / {on[4]}")
        if b == 12:
            assert (on[0], on[1], on[6]) in LAT_ROWS.values(), on
            assert (off[0], off[1]) == (128, 64), off
        else:
            assert on == off, (on, off)
    for geom in GEOMETRIES:
        rc0, off = describe(lib, shape(768, geom), 0)
        rc1, on = describe(lib, shape(768, geom), DS_CONV_PLAN_LATENCY)
        assert rc0 == 0 and rc1 == 0 and on == off, (geom, on, off)
    with BC.forced_cfg(lib, 9):
        assert BC.describe(lib, shape(12), False)[0] == BC.DS_ERR_UNSUPPORTED
    one = np.zeros(8, F32)
    p = (one.ctypes.data + 15) & ~15         # (an aligned non-null address: the call is refused before anything is read)
    rc = lib.raw("ds_conv_fwd_bf16")(ctypes.byref(shape(12)), p, p, p, None, None, None, p, p,
                                     DS_EPI_STATS | DS_CONV_PLAN_LATENCY, None)
    assert rc == BC.DS_ERR_UNSUPPORTED, rc


def body_forward_eval(eng, x, sd_torch, n_stages=4):
    """forward_eval_planned(precision="bf16x3") with low_latency=True == the same call with low_latency=False, bit for
    bit; the two are different cached plans"""
    import torch
    from deepspeaker_pytorch_amd.engine import BNParams
    pw = eng.pack_weights(sd_torch, n_stages, with_bf16=True)
    names = [n for i in range(1, n_stages + 1) for n in (f"model.bn{i}", f"model.layer{i}.0.bn1", f"model.layer{i}.0.bn2")]
    folded = {n: eng.bn_fold(BNParams(sd_torch[n + ".weight"], sd_torch[n + ".bias"], sd_torch[n + ".running_mean"],
                                      sd_torch[n + ".running_var"])) for n in names}
    e0 = eng.forward_eval_planned(x, pw, folded, precision="bf16x3", low_latency=False)
    e1 = eng.forward_eval_planned(x, pw, folded, precision="bf16x3", low_latency=True)
    assert len(eng._eval_plans) == 2
    assert bool(torch.isfinite(e0).all()) and torch.equal(e0.view(torch.int32), e1.view(torch.int32))
    return e0
