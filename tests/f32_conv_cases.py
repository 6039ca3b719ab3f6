"""The f32 convolution family (conv_mfma_f32.hip: forward and both data gradients; wgrad_mfma_f32.hip: the filter gradient),
one kernel at a time under EVERY tile configuration: case lists, float64 references and the test bodies, written once against
the backend adapter of bf16_train_cases.py and run by test_emul_f32_conv.py (host emulator, numpy memory) and
test_gpu_f32_conv_kernels.py (MI355X, torch device memory).

    a. ds_conv_fwd_f32 under configurations 0, 1, 2 of kCfg (ds_conv_f32_set_forced_cfg): the fused epilogue (affine +
       residual + clip on both edges + statistics) and the raw launch; the raw output of the three configurations bit for bit
    b. ds_conv_dgrad_f32 (stride 1: the flipped bank; stride 2: four parity classes on the table-driven tap schedule) under
       the three configurations, bit for bit among them
    c. ds_conv_wgrad_f32: its four instantiations, the split count and the tile shares of the restated plan, two launches bit
       for bit; the fc form and its feature permutation
    d. what a forced configuration must still refuse

Rules (bf16_train_cases.py): every output and workspace starts as NaN; a bar never comes from the kernel's output; every body
prints its errors and bars; the hook goes back to -1 whatever happens.

Bars.  y and gx: 2e-6 on the max-norm relative error (conftest.rel_err) and on the relative L2 error, the bar
test_emul_kernels.py and test_gpu_conv_plans.py hold this kernel to.  Statistics: rtol 1e-4 beyond the backend's atol (1e-4 on
the emulator, 1e-3 on the device: the bars of test_emul_kernels.py and test_gpu_parity.py).  Filter gradient: max(3e-6, 4 x the
error of torch's float32 convolution backward on the CPU against float64)."""
import contextlib
import ctypes
import functools

import numpy as np
import torch

import deepspeaker_oracle as O
import train_f16_cases as TC
from bf16_train_cases import (F32, F64, DS_ERR_UNSUPPORTED, bar_from_restatement, finite_rel_err, frozen, fwd_inputs,
                              out_dims, seed_of, to_nchw, to_nhwc, tol_err)
from conv_cases import CASES                                                            # noqa: F401  (re-exported)
from deepspeaker_pytorch_amd._native import (ConvShape, DS_EPI_AFFINE, DS_EPI_CLIP, DS_EPI_RESIDUAL, DS_EPI_STATS)

# kCfg of conv_mfma_f32.hip: (M tile, N tile); <KS,2,1,2,2>, <KS,5,1,1,4>, <KS,4,1,2,2>
CFG_TILES = [(128, 64), (160, 128), (256, 64)]
CFGS = (0, 1, 2)
Y_BAR = 2e-6
STATS_RTOL = 1e-4

# what the bodies of this process launched: forward (configuration, NIT, tap schedule 3 / 5 / "table"), data gradient
# (configuration, tap schedule), filter gradient (taps per workgroup, wide output-channel tile)
LAUNCHED, DGRAD_LAUNCHED, WGRAD_LAUNCHED = set(), set(), set()
_FWD_RAN = set()


@contextlib.contextmanager
def forced_cfg(lib, cfg):
    """plan every f32 convolution (forward and both data gradients) with tile configuration `cfg` (-1: the planner's
    choice) -- a process-global hook that later tests plan through, so it goes back to -1 whatever happens"""
    try:
        lib.raw("ds_conv_f32_set_forced_cfg")(cfg)
        yield
    finally:
        lib.raw("ds_conv_f32_set_forced_cfg")(-1)


def describe(lib, shp):
    out8 = (ctypes.c_int * 8)()
    rc = lib.raw("ds_conv_plan_describe")(ctypes.byref(shp), out8)
    return rc, list(out8)


def schedule_of(ks):
    """the tap schedule ds_conv_fwd_f32 launches: unrolled 3x3 / 5x5 with the filter ring, anything else the tap table"""
    return ks if ks in (3, 5) else "table"


def both_errs(got, ref):
    """(max-norm relative error, relative L2 error); inf when anything was left unwritten"""
    if not np.isfinite(got).all():
        return float("inf"), float("inf")
    return finite_rel_err(got, ref), TC.rel_l2(got, ref)


# ---------------------------------------------------------------------------------------------------------------------
# a. forward convolution, every tile configuration
# ---------------------------------------------------------------------------------------------------------------------
# (B, Cin, Cout, H, W, KS, stride) -> staging slots per thread (NIT) under configuration 0 / 1 / 2.  Together: the 19
# instantiations FWD_INSTANTIATIONS below
FWD_CFG_CASES = {
    (5, 8, 128, 10, 4, 3, 1): (2, 4, 4),        # several images per tile, ragged last tile
    (2, 8, 128, 9, 32, 3, 1): (2, 2, 4),        # part-empty last row block
    (3, 8, 128, 20, 8, 3, 1): (2, 2, 2),        # whole-image segments
    (1, 8, 128, 2, 128, 3, 1): (4, 4, 8),       # the widest row the kernels accept
    (3, 16, 128, 7, 8, 5, 2): (4, 4, 4),        # 5x5 stride 2, two channel chunks
    (2, 8, 128, 13, 16, 5, 2): (8, 8, 8),       # 5x5 stride 2, odd height
    (6, 8, 128, 1, 4, 5, 2): (2, 2, 2),         # a one-row map
    (70, 24, 128, 1, 1, 1, 1): (2, 2, 2),       # 1x1: table-driven taps
}
# 256 output channels: at least two N tiles under every configuration (the 160x128 tile has ONE at 128 channels).  Plans
# (M tile x N tile: rows per segment, segments per tile, workgroups = M tiles x N tiles, NIT):
#   (5, 8, 256, 10, 4, 3, 1)  128x64: 10, 3, 2 x 4, 2   160x128: 10, 4, 2 x 2, 4   256x64: 10, 5, 1 x 4, 4
#   (3, 16, 256, 7, 8, 5, 2)  128x64:  4, 3, 1 x 4, 4   160x128:  4, 3, 1 x 2, 4   256x64:  4, 3, 1 x 4, 4
FWD_WIDE_CASES = {(5, 8, 256, 10, 4, 3, 1): (2, 4, 4), (3, 16, 256, 7, 8, 5, 2): (4, 4, 4)}
FWD_WIDE_PLANS = {
    (5, 8, 256, 10, 4, 3, 1): [(10, 3, 8, 2), (10, 4, 4, 2), (10, 5, 4, 1)],       # (RT, NI, workgroups, M tiles)
    (3, 16, 256, 7, 8, 5, 2): [(4, 3, 4, 1), (4, 3, 2, 1), (4, 3, 4, 1)],
}

FWD_INSTANTIATIONS = (
    {(0, 2, 3), (0, 4, 3), (1, 2, 3), (1, 4, 3), (2, 2, 3), (2, 4, 3), (2, 8, 3)} |
    {(c, nit, 5) for c in CFGS for nit in (2, 4, 8)} | {(c, 2, "table") for c in CFGS})


def pack_fwd_bank(be, wt):
    co, ci, k, _ = wt.shape
    w_d, wp = be.put(wt), be.nan(wt.size, F32)
    be.lib.call("ds_pack_conv_weight_f32", be.p(w_d), be.p(wp), co, ci, k, 0, be.stream)
    return wp


def body_conv_fwd(be, case, cfgs, stats_atol, nits=None, min_ntiles=1):
    """ds_conv_fwd_f32 under each configuration of `cfgs` (-1: the planner's choice): the fused epilogue and the raw launch
    against float64; the statistics rows of both against the column sums of the un-affined convolution; the raw outputs of
    all configurations bit for bit (a pixel's contraction order -- chunks, taps, channel pairs -- does not depend on the tile)"""
    lib, p = be.lib, be.p
    b, ci, co, h, w, k, s = case
    ho, wo = out_dims(h, w, k, s)
    I = fwd_inputs(case)
    shp = ConvShape(b, h, w, ci, co, k, s)
    wp = pack_fwd_bank(be, I["wt"])
    x_d, sc, sh, rs_d = (be.put(I[n]) for n in ("x", "scale", "shift", "res"))
    first_raw = None
    for i, cfg in enumerate(cfgs):
        with forced_cfg(lib, cfg):
            rc, out8 = describe(lib, shp)
            assert rc == 0, f"{case}: configuration {cfg} is not feasible (code {rc})"
            if cfg >= 0:
                assert (out8[0], out8[1]) == CFG_TILES[cfg], (cfg, out8)
            if nits is not None:
                assert out8[6] == nits[i], f"{case} cfg {cfg}: NIT {out8[6]}, the case list says {nits[i]}"
            assert out8[4] % out8[7] == 0 and out8[4] // out8[7] >= min_ntiles, (case, cfg, out8)
            rows = lib.raw("ds_conv_stats_rows")(ctypes.byref(shp))
            assert rows == out8[7] and rows > 0, (rows, out8)
            y1, st1 = be.nan((b, ho, wo, co), F32), be.nan((rows, co, 2), F32)
            y2, st2 = be.nan((b, ho, wo, co), F32), be.nan((rows, co, 2), F32)
            lib.call("ds_conv_fwd_f32", ctypes.byref(shp), p(x_d), p(wp), p(sc), p(sh), p(rs_d), p(y1), p(st1),
                     DS_EPI_AFFINE | DS_EPI_RESIDUAL | DS_EPI_CLIP | DS_EPI_STATS, be.stream)
            lib.call("ds_conv_fwd_f32", ctypes.byref(shp), p(x_d), p(wp), None, None, None, p(y2), p(st2), DS_EPI_STATS,
                     be.stream)
        which = CFG_TILES.index((out8[0], out8[1]))
        LAUNCHED.add((which, out8[6], schedule_of(k)))
        e1, l1 = both_errs(to_nchw(be.get(y1)), I["ref"])
        e2, l2 = both_errs(to_nchw(be.get(y2)), I["z"])
        errs = []
        for st in (st1, st2):
            rows_h = be.get(st).astype(F64)
            assert rows_h.shape == (rows, co, 2) and np.isfinite(rows_h).all(), f"{case} cfg {cfg}: a statistics row holds a NaN"
            tot = rows_h.sum(axis=0)
            errs += [tol_err(tot[:, 0], I["s1"], stats_atol), tol_err(tot[:, 1], I["s2"], stats_atol)]
        tot = be.get(st2).astype(F64).sum(axis=0)
        abs1, rel2 = float(np.abs(tot[:, 0] - I["s1"]).max()), tol_err(tot[:, 1], I["s2"])
        print(f"conv fwd f32 {case} cfg {cfg} ({out8[0]}x{out8[1]}, RT {out8[2]} NI {out8[3]}, {out8[4]} workgroups, NIT "
              f"{out8[6]}, {rows} rows; clip edges {I['edges'][0]:.2f} / {I['edges'][1]:.2f}): fused {e1:.2e} / L2 {l1:.2e}, raw "
              f"{e2:.2e} / L2 {l2:.2e} (bar {Y_BAR:.0e}); sums {max(errs[0], errs[2]):.2e} (abs {abs1:.1e}) squares "
              f"{max(errs[1], errs[3]):.2e} (rel {rel2:.1e}) (rtol {STATS_RTOL:.0e} beyond atol {stats_atol:g})")
        assert max(e1, l1, e2, l2) < Y_BAR, (case, cfg, e1, l1, e2, l2)
        assert max(errs) <= STATS_RTOL, (case, cfg, errs)
        assert be.same(st1, st2), f"{case} cfg {cfg}: the statistics of the fused and the raw launch differ"
        if first_raw is None:
            first_raw = y2
        else:
            assert be.same(first_raw, y2), f"{case}: raw y under configuration {cfg} differs from configuration {cfgs[0]}"
    if tuple(cfgs) == CFGS:
        _FWD_RAN.add(case)


def body_fwd_wide(be, case, stats_atol):
    """two or more N tiles under every configuration, and the plans the case list records"""
    b, ci, co, h, w, k, s = case
    shp = ConvShape(b, h, w, ci, co, k, s)
    for cfg in CFGS:
        with forced_cfg(be.lib, cfg):
            rc, out8 = describe(be.lib, shp)
        assert rc == 0 and (out8[2], out8[3], out8[4], out8[7]) == FWD_WIDE_PLANS[case][cfg], (case, cfg, rc, out8)
    body_conv_fwd(be, case, CFGS, stats_atol, FWD_WIDE_CASES[case], min_ntiles=2)


def body_fwd_coverage(be, stats_atol):
    """the forward bodies launched all 19 instantiations (configuration, NIT, tap schedule); a case this process has not
    run yet (a selection, a worker of a parallel run) is run here"""
    for case, nits in FWD_CFG_CASES.items():
        if case not in _FWD_RAN:
            body_conv_fwd(be, case, CFGS, stats_atol, nits)
    for row in sorted(LAUNCHED, key=str):
        print("launched: configuration %d (%dx%d), NIT %d, tap schedule %s" % (row[0], *CFG_TILES[row[0]], row[1], row[2]))
    assert len(FWD_INSTANTIATIONS) == 19
    assert FWD_INSTANTIATIONS <= LAUNCHED, sorted(FWD_INSTANTIATIONS - LAUNCHED, key=str)


# ---------------------------------------------------------------------------------------------------------------------
# b. data gradient, every tile configuration
# ---------------------------------------------------------------------------------------------------------------------
# the FORWARD shape; 128 input channels: the swapped convolution's Cout, a multiple of every N tile
DGRAD_CFG_CASES = [(2, 128, 8, 9, 32, 3, 1), (2, 128, 8, 16, 32, 5, 2), (2, 128, 16, 13, 16, 5, 2), (3, 128, 8, 7, 8, 5, 2),
                   (1, 128, 8, 1, 4, 5, 2)]


@functools.lru_cache(maxsize=None)
def dgrad_inputs(case):
    b, ci, co, h, w, k, s = case
    rs = np.random.RandomState(seed_of(*case, 1))
    ho, wo = out_dims(h, w, k, s)
    wt = (rs.randn(co, ci, k, k) / np.sqrt(ci * k * k)).astype(F32)
    gy = rs.randn(b, co, ho, wo).astype(F32)
    gx = O.conv2d_bwd(np.zeros((b, ci, h, w)), wt.astype(F64), gy.astype(F64), s, k // 2)[0]
    return frozen(wt=wt, gy=to_nhwc(gy), gx=gx)


def body_conv_dgrad(be, case, cfgs):
    """ds_conv_dgrad_f32 under each configuration against float64, bit for bit among the configurations; every parity
    class of the stride-2 layer wrote (the output starts as NaN)"""
    lib, p = be.lib, be.p
    b, ci, co, h, w, k, s = case
    I = dgrad_inputs(case)
    w_d, wp = be.put(I["wt"]), be.nan(I["wt"].size, F32)
    if s == 1:
        lib.call("ds_pack_conv_weight_f32", p(w_d), p(wp), co, ci, k, 1, be.stream)
    else:
        lib.call("ds_pack_conv_dgrad_s2_f32", p(w_d), p(wp), co, ci, be.stream)
    assert np.isfinite(be.get(wp)).all()
    gy_d = be.put(I["gy"])
    shp = ConvShape(b, h, w, ci, co, k, s)
    # the plan of the (first) launch: a 3x3 stride-1 convolution over the dY grid with the channel roles swapped
    plan_shp = ConvShape(b, h, w, co, ci, 3, 1) if s == 1 else ConvShape(b, (h - 1) // 2 + 1, (w - 1) // 2 + 1, co, ci, 3, 1)
    classes = [(0, 0)] if s == 1 else [(0, 0), (0, 1), (1, 0), (1, 1)]
    first = None
    for cfg in cfgs:
        with forced_cfg(lib, cfg):
            rc, out8 = describe(lib, plan_shp)
            assert rc == 0, f"{case}: configuration {cfg} is not feasible (code {rc})"
            if cfg >= 0:
                assert (out8[0], out8[1]) == CFG_TILES[cfg], (cfg, out8)
            gx = be.nan((b, h, w, ci), F32)
            lib.call("ds_conv_dgrad_f32", ctypes.byref(shp), p(gy_d), p(wp), p(gx), be.stream)
        DGRAD_LAUNCHED.add((CFG_TILES.index((out8[0], out8[1])), 3 if s == 1 else "table"))
        got = be.get(gx)
        sizes = []
        for ph, pw in classes:
            part = got[:, ph::s, pw::s]
            sizes.append(part.shape[1] * part.shape[2])
            assert np.isfinite(part).all(), f"{case} cfg {cfg}: parity class ({ph}, {pw}) left output unwritten"
        e, l2 = both_errs(to_nchw(got), I["gx"])
        print(f"conv dgrad f32 {case} cfg {cfg} ({out8[0]}x{out8[1]}; pixels per image of the classes {sizes}): "
              f"{e:.2e} / L2 {l2:.2e} (bar {Y_BAR:.0e})")
        assert max(e, l2) < Y_BAR, (case, cfg, e, l2)
        if first is None:
            first = gx
        else:
            assert be.same(first, gx), f"{case}: gx under configuration {cfg} differs from configuration {cfgs[0]}"
    if h == 1:
        assert sizes[2] == 0 and sizes[3] == 0 and sizes[0] > 0 and sizes[1] > 0        # empty odd-row classes


def body_dgrad_coverage(be):
    """both tap schedules of the data gradient (unrolled 3x3 for stride 1, the tap table for the stride-2 classes) were
    launched under the three configurations; what this process has not run yet is run here"""
    want = {(c, sch) for c in CFGS for sch in (3, "table")}
    for case in DGRAD_CFG_CASES[:2]:
        if not want <= DGRAD_LAUNCHED:
            body_conv_dgrad(be, case, CFGS)
    for row in sorted(DGRAD_LAUNCHED, key=str):
        print("launched: data gradient, configuration %d (%dx%d), tap schedule %s" % (row[0], *CFG_TILES[row[0]], row[1]))
    assert want <= DGRAD_LAUNCHED, sorted(want - DGRAD_LAUNCHED, key=str)


# ---------------------------------------------------------------------------------------------------------------------
# c. filter gradient
# ---------------------------------------------------------------------------------------------------------------------
def plan_wgrad(case):
    """plan_wgrad of wgrad_mfma_f32.hip, restated: segments of RT output rows, NI segments per pixel tile, the tiles dealt
    round-robin to S pixel splits (split i owns tiles i, i + S, ...).  Nothing here depends on the device."""
    b, ci, co, h, w, k, s = case
    ho, wo = out_dims(h, w, k, s)
    wide = k == 5 and co % 128 == 0
    cot, cit = (128, 32) if wide else (64, 64)
    rt = 0
    for r in range(1, ho + 1):
        if r * wo > 64 or (s * (r - 1) + k) * (s * (wo - 1) + k) * cit * 4 > 40 * 1024:
            break
        rt = r
    rt = max(rt, 1)
    n_segs = b * -(-ho // rt)
    seg_pix = (s * (rt - 1) + k) * (s * (wo - 1) + k)
    ni = 1
    while (ni + 1) * rt * wo <= 64 and (ni + 1) * seg_pix * cit * 4 <= 40 * 1024 and ni + 1 <= n_segs:
        ni += 1
    n_tiles = -(-n_segs // ni)
    base = (5 if k == 5 else 1) * (co // cot) * (ci // cit)
    S = max(1, min(-(-1024 // base), n_tiles))
    return dict(inst=({3: 9, 5: 5, 1: 1}[k], wide), rt=rt, ni=ni, n_segs=n_segs, n_tiles=n_tiles, S=S,
                shares=[len(range(i, n_tiles, S)) for i in range(S)])


# case -> (instantiation <taps per workgroup, wide>, S, pixel tiles); both backends
WGRAD_CASES = {
    (2, 64, 64, 9, 32, 3, 1): ((9, False), 10, 10),
    (3, 128, 64, 20, 8, 3, 1): ((9, False), 9, 9),
    (5, 64, 128, 10, 4, 3, 1): ((9, False), 5, 5),
    (2, 64, 128, 16, 32, 5, 2): ((5, True), 6, 6),
    (3, 64, 64, 13, 16, 5, 2): ((5, False), 12, 12),
    (1, 128, 64, 70, 1, 1, 1): ((1, False), 2, 2),         # the fc layer as a 1x1 convolution over [1,B,1,K], fc_F = 0
    (7, 64, 64, 5, 4, 3, 1): ((9, False), 3, 3),           # three 20-pixel images per tile, the last tile one-third full
}
# slow on the emulator.  Three images per tile in both; 8 tiles over 7 splits (split 0 owns two); 52 images in 18 tiles over
# 16 splits (splits 0 and 1 own two), the last tile one-third full
WGRAD_CASES_DEVICE = {
    (24, 256, 512, 10, 4, 5, 2): ((5, True), 7, 8),
    (52, 512, 512, 5, 4, 3, 1): ((9, False), 16, 18),
}
WGRAD_INSTANTIATIONS = {(9, False), (5, True), (5, False), (1, False)}
WGRAD_MULTI_IMAGE = {(7, 64, 64, 5, 4, 3, 1), (24, 256, 512, 10, 4, 5, 2), (52, 512, 512, 5, 4, 3, 1)}       # NI = 3


def wgrad_launch_twice(be, shp, x_d, gy_d, n_ws, gw_shape, fc_F):
    lib, p = be.lib, be.p
    outs = []
    for _ in range(2):
        ws, gw = be.nan(n_ws, F32), be.nan(gw_shape, F32)
        lib.call("ds_conv_wgrad_f32", ctypes.byref(shp), p(x_d), p(gy_d), p(ws), p(gw), fc_F, be.stream)
        outs.append(gw)
    assert be.same(outs[0], outs[1]), "two launches differ: the fold of the splits is not in a fixed order"
    return be.get(outs[0])


def body_conv_wgrad(be, case, want):
    """ds_conv_wgrad_f32 against float64; the library's split count and the restated plan's tile shares"""
    b, ci, co, h, w, k, s = case
    inst, want_S, want_tiles = want
    ho, wo = out_dims(h, w, k, s)
    shp = ConvShape(b, h, w, ci, co, k, s)
    n_ws = be.lib.raw("ds_conv_wgrad_workspace_floats")(ctypes.byref(shp))
    assert n_ws > 0 and n_ws % (k * k * co * ci) == 0, n_ws
    S = n_ws // (k * k * co * ci)
    plan = plan_wgrad(case)
    assert (plan["inst"], plan["S"], plan["n_tiles"]) == (inst, want_S, want_tiles), plan
    assert S == plan["S"], (S, plan)
    assert plan["ni"] == (3 if case in WGRAD_MULTI_IMAGE else 1), plan
    rs = np.random.RandomState(seed_of(*case, 2))
    x, gy = rs.randn(b, ci, h, w).astype(F32), rs.randn(b, co, ho, wo).astype(F32)
    ref = TC.wgrad_ref(x, gy, k, s)
    restated = finite_rel_err(TC.wgrad_ref(x, gy, k, s, dtype=torch.float32), ref)
    bar = bar_from_restatement(3e-6, restated)
    got = wgrad_launch_twice(be, shp, be.put(to_nhwc(x)), be.put(to_nhwc(gy)), n_ws, (co, ci, k, k), 0)
    WGRAD_LAUNCHED.add(inst)
    err = finite_rel_err(got, ref)
    print(f"conv wgrad f32 {case} <{inst[0]},{str(inst[1]).lower()}>: RT {plan['rt']} NI {plan['ni']}, {plan['n_segs']} segments "
          f"in {plan['n_tiles']} tiles over S = {S} (tiles per split {min(plan['shares'])} .. {max(plan['shares'])}), "
          f"{b * ho * wo} pixels: f32-restated {restated:.2e} bar {bar:.2e} kernel {err:.2e}")
    assert err <= bar, (case, err, bar)
    return plan


def body_fc_wgrad_permutation(be):
    """fc_F > 0: the fc layer as a 1x1 convolution over [1,B,1,K] with the gradient written in the reference's [N, C*F]
    order (the kernels' feature order is k' = f*C + c)"""
    rs = np.random.RandomState(8)
    B, C, F, N = 40, 32, 4, 64                  # K = C*F = 128
    pooled = rs.randn(B, F * C).astype(F32)
    gf = rs.randn(B, N).astype(F32)
    ref_kp = gf.astype(F64).T @ pooled.astype(F64)                              # [N, f*C+c]
    ref = ref_kp.reshape(N, F, C).transpose(0, 2, 1).reshape(N, C * F)          # reference order c*F+f
    restated = finite_rel_err((gf.T @ pooled).reshape(N, F, C).transpose(0, 2, 1).reshape(N, C * F), ref)
    bar = bar_from_restatement(3e-6, restated)
    shp = ConvShape(1, B, 1, F * C, N, 1, 1)
    n_ws = be.lib.raw("ds_conv_wgrad_workspace_floats")(ctypes.byref(shp))
    assert n_ws > 0 and n_ws % (N * C * F) == 0
    got = wgrad_launch_twice(be, shp, be.put(pooled), be.put(gf), n_ws, (N, C * F), F)
    WGRAD_LAUNCHED.add((1, False))
    err, unpermuted = finite_rel_err(got, ref), finite_rel_err(got, ref_kp)
    print(f"fc wgrad, fc_F = {F}: S = {n_ws // (N * C * F)}, f32-restated {restated:.2e} bar {bar:.2e} kernel {err:.2e} "
          f"(against the unpermuted order: {unpermuted:.2e})")
    assert err <= bar, (err, bar)
    assert unpermuted > 0.1                                                     # the two orders really differ here


def body_wgrad_coverage(be):
    """the filter-gradient bodies launched all four instantiations; a case this process has not run yet is run here"""
    for case, want in WGRAD_CASES.items():
        if want[0] not in WGRAD_LAUNCHED:
            body_conv_wgrad(be, case, want)
    for inst in sorted(WGRAD_LAUNCHED):
        print("launched: wgrad_mfma_f32_kernel<%d, %s>" % (inst[0], str(inst[1]).lower()))
    assert WGRAD_INSTANTIATIONS <= WGRAD_LAUNCHED, WGRAD_INSTANTIATIONS - WGRAD_LAUNCHED


# ---------------------------------------------------------------------------------------------------------------------
# d. refusals
# ---------------------------------------------------------------------------------------------------------------------
REFUSED_NARROW = ((2, 8, 64, 9, 32, 3, 1), (1,))              # 64 output channels: the 160x128 tile does not divide them
REFUSED_ALWAYS = ((1, 16, 64, 8, 256, 5, 2), (-1, 0, 1, 2))   # a 259-pixel halo row: no configuration stages it


def body_refusals(be):
    """the hook does not turn an infeasible shape into a launch: a negative code from the describe, rows and launch entry
    points, and nothing written"""
    lib, p = be.lib, be.p
    for case, cfgs in (REFUSED_NARROW, REFUSED_ALWAYS):
        b, ci, co, h, w, k, s = case
        ho, wo = out_dims(h, w, k, s)
        shp = ConvShape(b, h, w, ci, co, k, s)
        rs = np.random.RandomState(seed_of(*case, 3))
        x_d = be.put(rs.randn(b, h, w, ci).astype(F32))
        wp = be.put(rs.randn(co * ci * k * k).astype(F32))
        for cfg in cfgs:
            y, st = be.nan((b, ho, wo, co), F32), be.nan((64, co, 2), F32)
            with forced_cfg(lib, cfg):
                rc_d, _ = describe(lib, shp)
                rows = lib.raw("ds_conv_stats_rows")(ctypes.byref(shp))
                rc = lib.raw("ds_conv_fwd_f32")(ctypes.byref(shp), p(x_d), p(wp), None, None, None, p(y), p(st), DS_EPI_STATS,
                                                be.stream)
            print(f"conv fwd f32 {case} cfg {cfg}: describe {rc_d}, rows {rows}, launch {rc}")
            assert rc_d == rows == rc == DS_ERR_UNSUPPORTED, (case, cfg, rc_d, rows, rc)
            assert np.isnan(be.get(y)).all() and np.isnan(be.get(st)).all()
    # ... and the first shape is planned again (128x64) once the hook is back at -1, also after a body that raised
    try:
        with forced_cfg(lib, 1):
            raise RuntimeError("a failing test body")
    except RuntimeError:
        pass
    b, ci, co, h, w, k, s = REFUSED_NARROW[0]
    rc, out8 = describe(lib, ConvShape(b, h, w, ci, co, k, s))
    assert rc == 0 and (out8[0], out8[1]) == (128, 64), (rc, out8)
    # values outside [0, 3) mean "the planner's choice"
    for bad in (3, 99, -7):
        with forced_cfg(lib, bad):
            assert describe(lib, ConvShape(b, h, w, ci, co, k, s)) == (rc, out8), bad
