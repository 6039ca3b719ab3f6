"""The kernels of the default (bf16x3) training step, one at a time: case lists, float64 references and the test bodies,
written once against a small backend adapter and run by test_emul_bf16_train.py (host emulator, numpy memory) and
test_gpu_bf16_train_kernels.py (MI355X, torch device memory).

    a. ds_conv_fwd_bf16 under EVERY tile configuration of kCfgB (ds_conv_bf16_set_forced_cfg), fused epilogue
       (affine + residual + clip + statistics) and raw; ds_pack_conv_weights_bf16_batch against single pack calls
    b. ds_conv_dgrad_bnbwd_bf16 / ds_conv_dgrad_s2_bnbwd_bf16 + ds_bn_bwd_group_finish_f32 (the fused instantiation of
       every tile configuration; members, parity classes, refusals)
    c. ds_conv5x5s2_c1_fwd_f32 / _bf16
    d. the f32 BatchNorm family: statistics -> tables -> normalise -> fold; backward in its one-call, split and grouped
       forms (G = 1 and 3) and the arguments its entry points refuse; ds_colsum_f32

The adapter (`be`):
    be.lib                      the NativeLib
    be.stream                   the stream argument of the entry points
    be.put(host_array)          -> handle of a copy in the backend's memory (16-byte aligned)
    be.nan(shape, dtype)        -> handle of an output prefilled with NaN (float32 / float64) or 0xFFFF (uint16: a bf16 NaN)
    be.p(handle)                pointer (None for None)
    be.get(handle)              -> host array (waits for the queued work)
    be.same(h1, h2)             bit-for-bit equality of two buffers

Rules: every output starts as NaN; a bar never comes from the kernel's output; every body prints its errors and bars.
Max-norm relative error = conftest.rel_err (max |got - ref| / max |ref|) unless said otherwise."""
import contextlib
import ctypes
import functools

import numpy as np
import torch

import deepspeaker_oracle as O
from conftest import rel_err
from conv_cases import BF16_CASES                                                       # noqa: F401  (re-exported)
from deepspeaker_pytorch_amd._native import (ConvShape, DS_EPI_AFFINE, DS_EPI_CLIP, DS_EPI_RESIDUAL, DS_EPI_STATS,
                                             PackJob)

F32, F64, U16 = np.float32, np.float64, np.uint16
EPS, MOMENTUM = 1e-5, 0.1
DS_ERR_UNSUPPORTED = -4

# kCfgB of conv_mfma_bf16_kernel.h: (M tile, N tile, threads per workgroup); 3 .. 8 exist for bf16x3 only
CFG_TILES = [(128, 64, 256), (160, 128, 256), (256, 64, 256), (160, 128, 128), (160, 256, 256), (320, 128, 256),
             (320, 64, 128), (128, 128, 128), (128, 256, 256)]
X3_CFGS, PLAIN_CFGS = tuple(range(9)), (0, 1, 2)

# every launch a body made: (kernel size, arithmetic, "plain" / "fused", configuration or "planner MxN/threads")
LAUNCHED = set()


@contextlib.contextmanager
def forced_cfg(lib, cfg):
    """plan every bf16 convolution with tile configuration `cfg` (-1: the planner's choice) -- a process-global hook
    that later tests plan through, so it goes back to -1 whatever happens"""
    try:
        lib.raw("ds_conv_bf16_set_forced_cfg")(cfg)
        yield
    finally:
        lib.raw("ds_conv_bf16_set_forced_cfg")(-1)


def seed_of(*vals):
    return int(sum((2 * i + 3) * 7919 ** (i % 3) * int(v) for i, v in enumerate(vals)) % (2 ** 31))


def frozen(**arrays):
    for a in arrays.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def to_nhwc(a):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1))


def to_nchw(a):
    return np.ascontiguousarray(a.transpose(0, 3, 1, 2))


def out_dims(h, w, k, s):
    return O.conv_out_size(h, k, s, k // 2), O.conv_out_size(w, k, s, k // 2)


def bar_from_restatement(floor, restated_err):
    """reductions: 4 x the error of a plain float32 restatement against float64 (equally valid summation orders differ
    by small factors), never below the emulator suite's bar"""
    return max(floor, 4.0 * restated_err)


def tol_err(got, ref, atol=0.0):
    """the smallest rtol with which np.testing.assert_allclose(got, ref, rtol, atol) passes"""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.clip(np.abs(got - ref) - atol, 0.0, None) / np.maximum(np.abs(ref), 1e-300)).max())


def finite_rel_err(got, ref):
    return rel_err(got, ref) if np.isfinite(got).all() else float("inf")


def describe(lib, shp, x3):
    out8 = (ctypes.c_int * 8)()
    rc = lib.raw("ds_conv_bf16_plan_describe")(ctypes.byref(shp), int(x3), out8)
    return rc, list(out8)


def check_tile(cfg, out8):
    """the plan is the forced configuration's: M tile, N tile and threads per workgroup (1 and 3 share a tile)"""
    if cfg >= 0:
        assert (out8[0], out8[1], out8[6]) == CFG_TILES[cfg], (cfg, out8)
        return cfg
    return f"planner {out8[0]}x{out8[1]}/{out8[6]}"


# ---------------------------------------------------------------------------------------------------------------------
# a. forward convolution, every tile configuration
# ---------------------------------------------------------------------------------------------------------------------
# (B, Cin, Cout, H, W, KS, stride); 256 output channels: every N tile divides them
FWD_CFG_CASES = [
    (5, 16, 256, 10, 4, 3, 1),      # multi-image tiles, ragged last tile
    (2, 16, 256, 9, 32, 3, 1),      # part-empty last row block
    (3, 16, 256, 7, 8, 5, 2),
    (2, 16, 256, 13, 16, 5, 2),     # odd height
]


@functools.lru_cache(maxsize=None)
def fwd_inputs(case):
    """inputs and float64 references of one forward case; the shift and the residual are wide enough that the reference
    sits on BOTH clip edges for more than 1 % of the outputs"""
    b, ci, co, h, w, k, s = case
    rs = np.random.RandomState(seed_of(*case))
    ho, wo = out_dims(h, w, k, s)
    x = rs.randn(b, ci, h, w).astype(F32)
    wt = (rs.randn(co, ci, k, k) / np.sqrt(ci * k * k)).astype(F32)
    scale = rs.uniform(0.5, 1.5, co).astype(F32)
    shift = (10.0 + rs.randn(co)).astype(F32)
    res = (rs.randn(b, co, ho, wo) * 12.0).astype(F32)
    z = O.conv2d(x.astype(F64), wt.astype(F64), s, k // 2)
    ref = np.clip(z * scale[None, :, None, None] + shift[None, :, None, None] + res, 0.0, 20.0)
    at0, at20 = float((ref == 0).mean()), float((ref == 20).mean())
    assert at0 > 0.01 and at20 > 0.01, (at0, at20)
    return frozen(x=to_nhwc(x), wt=wt, scale=scale, shift=shift, res=to_nhwc(res), z=z, ref=ref,
                  s1=z.sum(axis=(0, 2, 3)), s2=(z * z).sum(axis=(0, 2, 3)), edges=(at0, at20))


def pack_fwd_bank(be, wt, x3):
    co, ci, k, _ = wt.shape
    w_d = be.put(wt)
    hi, lo = be.nan(wt.size, U16), (be.nan(wt.size, U16) if x3 else None)
    be.lib.call("ds_pack_conv_weight_bf16", be.p(w_d), be.p(hi), be.p(lo), co, ci, k, be.stream)
    return hi, lo


def body_conv_fwd(be, case, x3, cfgs):
    """ds_conv_fwd_bf16 under each configuration of `cfgs` (-1: the planner's choice): the fused epilogue and the raw
    launch against float64; the statistics rows of both launches against the column sums of the un-affined convolution"""
    lib, p = be.lib, be.p
    b, ci, co, h, w, k, s = case
    ho, wo = out_dims(h, w, k, s)
    I = fwd_inputs(case)
    shp = ConvShape(b, h, w, ci, co, k, s)
    hi, lo = pack_fwd_bank(be, I["wt"], x3)
    x_d, sc, sh, rs_d = (be.put(I[n]) for n in ("x", "scale", "shift", "res"))
    arith = "bf16x3" if x3 else "bf16"
    y_bar, st_rtol, st_atol = (2e-5, 1e-4, 1e-3) if x3 else (2e-2, 2e-2, 0.5)
    for cfg in cfgs:
        with forced_cfg(lib, cfg):
            rc, out8 = describe(lib, shp, x3)
            assert rc == 0, f"{case} {arith}: configuration {cfg} is not feasible (code {rc})"
            what = check_tile(cfg, out8)
            rows = lib.raw("ds_conv_bf16_stats_rows")(ctypes.byref(shp), int(x3))
            assert rows > 0, rows
            y1, st1 = be.nan((b, ho, wo, co), F32), be.nan((rows, co, 2), F32)
            y2, st2 = be.nan((b, ho, wo, co), F32), be.nan((rows, co, 2), F32)
            lib.call("ds_conv_fwd_bf16", ctypes.byref(shp), p(x_d), p(hi), p(lo), p(sc), p(sh), p(rs_d), p(y1), p(st1),
                     DS_EPI_AFFINE | DS_EPI_RESIDUAL | DS_EPI_CLIP | DS_EPI_STATS, be.stream)
            lib.call("ds_conv_fwd_bf16", ctypes.byref(shp), p(x_d), p(hi), p(lo), None, None, None, p(y2), p(st2),
                     DS_EPI_STATS, be.stream)
        LAUNCHED.add((k, arith, "plain", what))
        e1, e2 = finite_rel_err(to_nchw(be.get(y1)), I["ref"]), finite_rel_err(to_nchw(be.get(y2)), I["z"])
        errs = []
        for st in (st1, st2):
            rows_h = be.get(st).astype(F64)
            assert np.isfinite(rows_h).all(), f"{case} {arith} cfg {cfg}: a statistics row holds a NaN"
            tot = rows_h.sum(axis=0)
            errs += [tol_err(tot[:, 0], I["s1"], st_atol), tol_err(tot[:, 1], I["s2"], st_atol)]
        print(f"conv fwd {case} {arith} cfg {what} ({out8[0]}x{out8[1]}, {out8[4]} workgroups, {rows} rows; clip edges "
              f"{I['edges'][0]:.2f} / {I['edges'][1]:.2f}): fused {e1:.2e} raw {e2:.2e} (bar {y_bar:.0e}), sums "
              f"{max(errs[0], errs[2]):.2e} squares {max(errs[1], errs[3]):.2e} (rtol {st_rtol:.0e} beyond atol {st_atol:g})")
        assert e1 < y_bar and e2 < y_bar, (case, arith, cfg, e1, e2)
        if not x3:
            assert e1 > 1e-4 and e2 > 1e-4, (case, cfg, e1, e2)            # really is the reduced-precision path
        assert max(errs) <= st_rtol, (case, arith, cfg, errs)


def address(pointer):
    """a backend's pointer (an int, a c_void_p or None) as a structure field"""
    return pointer.value if isinstance(pointer, ctypes.c_void_p) else pointer


PACK_BATCH_JOBS = [(64, 16, 3, True), (128, 32, 5, False), (256, 64, 5, True)]     # (Cout, Cin, KS, with a lo plane)


def body_pack_batch(be):
    """ds_pack_conv_weights_bf16_batch over three filters == three ds_pack_conv_weight_bf16 calls, bit for bit; a job
    without a `lo` plane leaves none"""
    lib, p = be.lib, be.p
    rs = np.random.RandomState(5)
    jobs = (PackJob * len(PACK_BATCH_JOBS))()
    keep, pairs = [], []
    for j, (co, ci, k, with_lo) in enumerate(PACK_BATCH_JOBS):
        wt = rs.randn(co, ci, k, k).astype(F32)
        w_d = be.put(wt)
        hi1, lo1 = be.nan(wt.size, U16), (be.nan(wt.size, U16) if with_lo else None)
        hi2, lo2 = be.nan(wt.size, U16), (be.nan(wt.size, U16) if with_lo else None)
        lib.call("ds_pack_conv_weight_bf16", p(w_d), p(hi1), p(lo1), co, ci, k, be.stream)
        jobs[j] = PackJob(address(p(w_d)), address(p(hi2)), address(p(lo2)), co, ci, k, 0)
        keep.append(w_d)
        pairs += [(hi1, hi2, wt, "hi")] + ([(lo1, lo2, wt, "lo")] if with_lo else [])
    lib.call("ds_pack_conv_weights_bf16_batch", jobs, len(PACK_BATCH_JOBS), be.stream)
    for one, batch, wt, plane in pairs:
        assert be.same(one, batch), (wt.shape, plane)
        bits = be.get(one).view(U16).astype(np.uint32) << 16
        vals = bits.view(F32)
        assert np.isfinite(vals).all()                                  # every element written (the prefill is a bf16 NaN)
        if plane == "hi":                                               # the bank holds the filter, rounded to bf16
            co, ci, k, _ = wt.shape
            bank = vals.reshape(ci // 16, k * k, co, 16)
            want = wt.reshape(co, ci // 16, 16, k * k).transpose(1, 3, 0, 2)
            assert np.abs(bank - want).max() <= 2.0 ** -8 * np.abs(want).max()


# ---------------------------------------------------------------------------------------------------------------------
# b. fused data gradient + BatchNorm backward
# ---------------------------------------------------------------------------------------------------------------------
# (forward shape, G, forced configurations); -1 = the planner's own choice
DGRAD_BN_CASES = [
    ((6, 64, 64, 9, 32, 3, 1), 3, (-1, 0, 2, 6)),
    ((6, 128, 128, 20, 8, 3, 1), 3, (-1, 0, 1, 2, 3, 5, 7)),
    ((6, 256, 256, 10, 4, 3, 1), 1, (-1, 0, 1, 3, 4, 7, 8)),
    ((6, 256, 256, 10, 4, 3, 1), 3, (1, 3, 4)),
    ((6, 64, 128, 9, 31, 5, 2), 3, (-1, 0)),        # odd map: parity classes of different sizes
    ((24, 64, 64, 1, 32, 5, 2), 3, (-1, 0)),        # H = 1: the odd-row classes are empty
]
# the planner's own choice straddles members here (three 40-pixel images per tile, two images per member): refused
DGRAD_BN_PLANNER_REFUSES = ((6, 256, 256, 10, 4, 3, 1), 3)
# refused under every configuration; the callers rely on the code to fall back to the two-step sequence
DGRAD_BN_REFUSED = ((6, 64, 256, 13, 7, 5, 2), 1)
MASK_MARGIN = 1e-3


@functools.lru_cache(maxsize=None)
def dgrad_bn_inputs(case, G):
    """inputs and float64 references of one fused case.  3x3: the mask comes from z * msc + msh, and z is nudged until
    every float64 value of that is MASK_MARGIN away from 0 and from 20 (no float32 evaluation can flip it).  5x5: the
    mask comes from `act`, which holds exact 0, exact 20 (masked) and their inward neighbours (passing)."""
    b, ci, co, h, w, k, s = case
    rs = np.random.RandomState(seed_of(*case, G))
    ho, wo = out_dims(h, w, k, s)
    n_pix = (b // G) * h * w
    wt = (rs.randn(co, ci, k, k) * (s / np.sqrt(co * k * k))).astype(F32)
    gz_up = rs.randn(b, co, ho, wo).astype(F32)
    z = (rs.randn(b, h, w, ci) * 2 + 1).astype(F32)
    gamma = rs.uniform(0.5, 1.5, ci).astype(F32)
    gx = to_nhwc(O.conv2d_bwd(np.zeros((b, ci, h, w)), wt.astype(F64), gz_up.astype(F64), s, k // 2)[0])
    gx32 = torch.nn.grad.conv2d_input((b, ci, h, w), torch.from_numpy(wt), torch.from_numpy(gz_up), stride=s, padding=k // 2)
    gx32 = gx32.permute(0, 2, 3, 1).contiguous().numpy()
    g2 = act = msc = msh = None
    if k == 3:
        g2 = rs.randn(b, h, w, ci).astype(F32)
        msc, msh = rs.uniform(2.0, 5.0, (G, ci)).astype(F32), (rs.randn(G, ci) * 3 + 6).astype(F32)
        zm = z.reshape(G, n_pix, ci)
        for _ in range(8):
            pre = zm.astype(F64) * msc[:, None] + msh[:, None]
            close = (np.abs(pre) < MASK_MARGIN) | (np.abs(pre - 20) < MASK_MARGIN)
            if not close.any():
                break
            zm[close] += (F32(3 * MASK_MARGIN) / np.broadcast_to(msc[:, None], zm.shape)[close]).astype(F32)
        assert not close.any()
        pre = pre.reshape(b, h, w, ci)
        mask, low, high = (pre > 0) & (pre < 20), float((pre <= 0).mean()), float((pre >= 20).mean())
        gy = (gx + g2) * mask
        gy32 = (gx32 + g2) * mask
    else:
        act = np.clip(rs.randn(b, h, w, ci) * 8 + 8, 0.0, 20.0).astype(F32)
        flat = act.reshape(-1)
        spots = np.linspace(0, flat.size - 1, 16).astype(np.int64)                  # first and last element among them
        edge = [F32(0), F32(20), np.nextafter(F32(0), F32(1)), np.nextafter(F32(20), F32(0))]
        for i, at in enumerate(spots):
            flat[at] = edge[i % 4]
        mask = (act > 0) & (act < 20)
        assert not mask.reshape(-1)[spots[0::4]].any() and not mask.reshape(-1)[spots[1::4]].any()
        assert mask.reshape(-1)[spots[2::4]].all() and mask.reshape(-1)[spots[3::4]].all()
        low, high = float((act == 0).mean()), float((act == 20).mean())
        gy = gx * mask
        gy32 = gx32 * mask
    assert low > 0.01 and high > 0.01, (low, high)
    zs = z.reshape(G, n_pix, ci).astype(F64)
    mean, invstd = zs.mean(1).astype(F32), (1 / np.sqrt(zs.var(1) + EPS)).astype(F32)
    xhat = (zs - mean[:, None].astype(F64)) * invstd[:, None].astype(F64)
    gym = gy.reshape(G, n_pix, ci)
    sums = np.stack([gym.sum(1), (gym * xhat).sum(1)], axis=-1)                     # [G][Cin][2]
    gz = np.empty((G, n_pix, ci))
    gg, gb = np.zeros(ci), np.zeros(ci)
    for m in range(G):
        gz_m, gg_m, gb_m = O.bn_train_bwd(zs[m].T.reshape(1, ci, n_pix, 1), mean[m].astype(F64), invstd[m].astype(F64),
                                          gamma.astype(F64), gym[m].T.reshape(1, ci, n_pix, 1))
        gz[m] = gz_m[0, :, :, 0].T
        gg, gb = gg + gg_m, gb + gb_m
    xhat32 = (z.reshape(G, n_pix, ci) - mean[:, None]) * invstd[:, None]
    return frozen(wt=wt, gz_up=to_nhwc(gz_up), z=z, g2=g2, act=act, msc=msc, msh=msh, gamma=gamma, mean=mean, invstd=invstd,
                  gy=gy, sums=sums, gz=gz.reshape(b, h, w, ci), gg=gg, gb=gb, gy32=gy32.astype(F32),
                  xhat32=xhat32.astype(F32).reshape(b, h, w, ci), masked=(low, high), n_pix=n_pix)


def restated_sums(I, case, G, mt):
    """the float32 restatement of the partial sums: torch's float32 convolution backward, float32 sums over runs of
    `mt` pixels (the M tile; per parity class for the stride-2 layer, as the launches walk them), folded in float64"""
    b, ci, co, h, w, k, s = case
    out = np.zeros((G, ci, 2))
    classes = [(0, 0)] if s == 1 else [(0, 0), (0, 1), (1, 0), (1, 1)]
    step = 1 if s == 1 else 2
    for ph, pw in classes:
        g = I["gy32"][:, ph::step, pw::step].reshape(G, -1, ci)
        xh = I["xhat32"][:, ph::step, pw::step].reshape(G, -1, ci)
        if g.shape[1] == 0:
            continue
        cuts = np.arange(0, g.shape[1], mt)
        out[..., 0] += np.add.reduceat(g, cuts, axis=1).astype(F64).sum(1)
        out[..., 1] += np.add.reduceat(g * xh, cuts, axis=1).astype(F64).sum(1)
    return out


def dgrad_bn_shapes(case):
    b, ci, co, h, w, k, s = case
    return ConvShape(b, h, w, ci, co, k, s), ("ds_conv_dgrad_bnbwd_bf16" if k == 3 else "ds_conv_dgrad_s2_bnbwd_bf16")


def pack_dgrad_bank(be, wt, k):
    co, ci = wt.shape[:2]
    n = wt.size if k == 3 else 36 * co * ci
    w_d, hi, lo = be.put(wt), be.nan(n, U16), be.nan(n, U16)
    if k == 3:
        be.lib.call("ds_pack_conv_weight_dgrad_bf16", be.p(w_d), be.p(hi), be.p(lo), co, ci, k, be.stream)
    else:
        be.lib.call("ds_pack_conv_weight_dgrad_s2_bf16", be.p(w_d), be.p(hi), be.p(lo), co, ci, be.stream)
    return hi, lo


def launch_dgrad_bn(be, case, G, dev, hi, lo, gy, partial, raw=False):
    """the fused entry point of the case's kernel size on the device copies `dev` of dgrad_bn_inputs"""
    lib, p = be.lib, be.p
    shp, name = dgrad_bn_shapes(case)
    fn = lib.raw(name) if raw else (lambda *a: lib.call(name, *a))
    if case[5] == 3:
        return fn(ctypes.byref(shp), p(dev["gz_up"]), p(hi), p(lo), p(dev["g2"]), p(dev["z"]), p(dev["mean"]), p(dev["invstd"]),
                  p(dev["msc"]), p(dev["msh"]), G, p(gy), p(partial), be.stream)
    return fn(ctypes.byref(shp), p(dev["gz_up"]), p(hi), p(lo), p(dev["act"]), p(dev["z"]), p(dev["mean"]), p(dev["invstd"]),
              G, p(gy), p(partial), be.stream)


def body_dgrad_bn(be, case, G, cfgs):
    """gy, the members' partial sums and -- after ds_bn_bwd_group_finish_f32 -- gz, dgamma, dbeta against float64"""
    lib, p = be.lib, be.p
    b, ci, co, h, w, k, s = case
    I = dgrad_bn_inputs(case, G)
    n_pix = I["n_pix"]
    shp, name = dgrad_bn_shapes(case)
    rows_fn = lib.raw(name + "_rows")
    hi, lo = pack_dgrad_bank(be, I["wt"], k)
    dev = {n: (None if I[n] is None else be.put(I[n])) for n in ("gz_up", "z", "g2", "act", "msc", "msh", "gamma", "mean", "invstd")}
    # the plan of the (first) launch: a 3x3 stride-1 convolution over the dY grid with the channel roles swapped
    plan_shp = ConvShape(b, h, w, co, ci, 3, 1) if s == 1 else ConvShape(b, (h - 1) // 2 + 1, (w - 1) // 2 + 1, co, ci, 3, 1)
    for cfg in cfgs:
        with forced_cfg(lib, cfg):
            rows = rows_fn(ctypes.byref(shp), G)
            assert rows > 0, f"{case} G={G}: configuration {cfg} is refused (code {rows})"
            rc, out8 = describe(lib, plan_shp, True)
            assert rc == 0, (case, cfg, rc)
            what = check_tile(cfg, out8)
            gy = be.nan((b, h, w, ci), F32)
            partial = be.nan((G * rows + 1, ci, 2), F32)                    # one guard row
            launch_dgrad_bn(be, case, G, dev, hi, lo, gy, partial)
        LAUNCHED.add((k, "bf16x3", "fused", what))
        coef, msums = be.nan((G, 3 * ci), F32), be.nan((2, G, ci), F32)
        gg, gb, gz = be.nan(ci, F32), be.nan(ci, F32), be.nan((b, h, w, ci), F32)
        lib.call("ds_bn_bwd_group_finish_f32", p(partial), rows, p(gy), p(dev["z"]), p(dev["mean"]), p(dev["invstd"]),
                 p(dev["gamma"]), p(coef), p(msums), p(gg), p(gb), p(gz), n_pix, ci, G, be.stream)
        part = be.get(partial).astype(F64)
        assert np.isnan(part[G * rows:]).all(), "a partial row past the members' tables was written"
        part = part[:G * rows].reshape(G, rows, ci, 2)
        assert np.isfinite(part).all(), f"{case} G={G} cfg {cfg}: a partial row holds a NaN"
        got_sums = part.sum(axis=1)
        restated = [rel_err(restated_sums(I, case, G, out8[0])[..., j], I["sums"][..., j]) for j in (0, 1)]
        bars = [bar_from_restatement(3e-5, r) for r in restated]
        e_sums = [rel_err(got_sums[..., j], I["sums"][..., j]) for j in (0, 1)]
        e_gy, e_gz = finite_rel_err(be.get(gy), I["gy"]), finite_rel_err(be.get(gz), I["gz"])
        e_gg, e_gb = finite_rel_err(be.get(gg), I["gg"]), finite_rel_err(be.get(gb), I["gb"])
        print(f"dgrad+bn {case} G={G} cfg {what} ({rows} rows per member; masked {I['masked'][0]:.2f} / {I['masked'][1]:.2f}): "
              f"gy {e_gy:.2e} (bar 3e-5), sum gy f32-restated {restated[0]:.2e} bar {bars[0]:.2e} kernel {e_sums[0]:.2e}, "
              f"sum gy*xhat f32-restated {restated[1]:.2e} bar {bars[1]:.2e} kernel {e_sums[1]:.2e}, "
              f"gz {e_gz:.2e} dgamma {e_gg:.2e} dbeta {e_gb:.2e} (bar 1e-4)")
        assert e_gy < 3e-5, (case, G, cfg, e_gy)
        assert e_sums[0] <= bars[0] and e_sums[1] <= bars[1], (case, G, cfg, e_sums, bars)
        assert e_gz < 1e-4 and e_gg < 1e-4 and e_gb < 1e-4, (case, G, cfg, e_gz, e_gg, e_gb)


def body_dgrad_bn_refusals(be):
    """what the callers rely on to fall back to ds_conv_dgrad_bf16 + ds_bn_bwd_group_f32: a negative code from the
    _rows entry point and from the launch, which then writes nothing"""
    lib = be.lib
    for (case, G), cfgs, code in ((DGRAD_BN_PLANNER_REFUSES, (-1,), DS_ERR_UNSUPPORTED), (DGRAD_BN_REFUSED, range(-1, 9), None)):
        b, ci, co, h, w, k, s = case
        I = dgrad_bn_inputs(case, G)
        shp, name = dgrad_bn_shapes(case)
        hi, lo = pack_dgrad_bank(be, I["wt"], k)
        dev = {n: (None if I[n] is None else be.put(I[n])) for n in ("gz_up", "z", "g2", "act", "msc", "msh", "mean", "invstd")}
        for cfg in cfgs:
            gy, partial = be.nan((b, h, w, ci), F32), be.nan((G * 64, ci, 2), F32)
            with forced_cfg(lib, cfg):
                rows = lib.raw(name + "_rows")(ctypes.byref(shp), G)
                rc = launch_dgrad_bn(be, case, G, dev, hi, lo, gy, partial, raw=True)
            print(f"dgrad+bn {case} G={G} cfg {cfg}: rows {rows}, launch {rc}")
            assert rows < 0 and rc < 0, (case, G, cfg, rows, rc)
            if code is not None:
                assert rows == code and rc == code, (rows, rc)
            assert np.isnan(be.get(gy)).all() and np.isnan(be.get(partial)).all()


# ---------------------------------------------------------------------------------------------------------------------
# c. the one-channel first layer
# ---------------------------------------------------------------------------------------------------------------------
C1_CASES = [(2, 160, 64), (1, 13, 64), (3, 7, 20), (7, 37, 30)]         # (B, H, W); the last: a batch of odd maps


def body_conv1(be, shape):
    lib, p = be.lib, be.p
    b, h, w = shape
    rs = np.random.RandomState(h)
    x = rs.randn(b, 1, h, w).astype(F32)
    wt = (rs.randn(64, 1, 5, 5) * 0.3).astype(F32)
    scale, shift = rs.uniform(0.5, 1.5, 64).astype(F32), rs.randn(64).astype(F32)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    rows = lib.raw("ds_conv5x5s2_c1_stats_rows")(b, h)
    assert rows >= b and (b == 1 or rows > 1), rows
    z = O.conv2d(x.astype(F64), wt.astype(F64), 2, 2)
    ref = np.clip(z * scale[None, :, None, None] + shift[None, :, None, None], 0, 20)
    s1, s2 = z.sum(axis=(0, 2, 3)), (z * z).sum(axis=(0, 2, 3))
    w_d, wp = be.put(wt), be.nan(25 * 64, F32)
    lib.call("ds_pack_conv1_weight_f32", p(w_d), p(wp), 64, be.stream)
    x_d, sc, sh = be.put(x), be.put(scale), be.put(shift)
    flags = DS_EPI_AFFINE | DS_EPI_CLIP | DS_EPI_STATS
    for name, abs_bar, rel_bar, rtol, atol in (("ds_conv5x5s2_c1_fwd_f32", 1e-5, None, 1e-4, 1e-4),
                                               ("ds_conv5x5s2_c1_fwd_bf16", 3e-4, 3e-5, 1e-3, 2e-3)):
        y, stats = be.nan((b, ho, wo, 64), F32), be.nan((rows, 64, 2), F32)
        lib.call(name, p(x_d), p(wp), p(sc), p(sh), p(y), p(stats), b, h, w, 64, flags, be.stream)
        got, st = to_nchw(be.get(y)), be.get(stats).astype(F64)
        assert np.isfinite(got).all() and np.isfinite(st).all(), name
        e_abs, e_rel = float(np.abs(got - ref).max()), rel_err(got, ref)
        tot = st.sum(axis=0)
        e1, e2 = tol_err(tot[:, 0], s1, atol), tol_err(tot[:, 1], s2, atol)
        print(f"{name} {shape} ({rows} rows): abs {e_abs:.2e} (bar {abs_bar:.0e}) rel {e_rel:.2e}" +
              (f" (bar {rel_bar:.0e})" if rel_bar else "") + f", sums {e1:.2e} squares {e2:.2e} (rtol {rtol:.0e} beyond atol {atol:g})")
        assert e_abs < abs_bar and (rel_bar is None or e_rel < rel_bar), (name, e_abs, e_rel)
        assert e1 <= rtol and e2 <= rtol, (name, e1, e2)


# ---------------------------------------------------------------------------------------------------------------------
# d. the f32 BatchNorm family
# ---------------------------------------------------------------------------------------------------------------------
BN_FWD_CASES = [(5, 8, 128, 10, 4, 3, 1), (2, 8, 64, 9, 32, 3, 1), (3, 16, 128, 7, 8, 5, 2)]     # rows of conv_cases.CASES


def body_bn_forward(be, case):
    """statistics rows of a real ds_conv_fwd_f32 launch -> ds_bn_stats_finalize_f32 -> ds_bn_apply_f32 -> ds_bn_fold_f32;
    ds_partial_sum_f64 + ds_bn_stats_from_sums_f32 give the same tables bit for bit, ds_bn_stats_from_sums_group_f32 those
    of three single calls; the rows form once more on synthetic rows (1 / 129 / 300 of them, part-full last workgroups)"""
    lib, p = be.lib, be.p
    b, ci, co, h, w, k, s = case
    ho, wo = out_dims(h, w, k, s)
    n = b * ho * wo
    rs = np.random.RandomState(seed_of(*case))
    x = (rs.randn(b, ci, h, w) + 0.5).astype(F32)
    wt = (rs.randn(co, ci, k, k) / np.sqrt(ci * k * k)).astype(F32)
    gamma, beta = rs.uniform(4.0, 8.0, co).astype(F32), (8 + rs.randn(co)).astype(F32)
    rm, rv = (rs.randn(co) * 0.1).astype(F32), rs.uniform(0.5, 1.5, co).astype(F32)
    res = (rs.randn(b, ho, wo, co) * 3).astype(F32)
    shp = ConvShape(b, h, w, ci, co, k, s)
    rows = lib.raw("ds_conv_stats_rows")(ctypes.byref(shp))
    assert rows > 0
    w_d, wp, x_d = be.put(wt), be.nan(wt.size, F32), be.put(to_nhwc(x))
    lib.call("ds_pack_conv_weight_f32", p(w_d), p(wp), co, ci, k, 0, be.stream)
    z_d, stats = be.nan((b, ho, wo, co), F32), be.nan((rows, co, 2), F32)
    lib.call("ds_conv_fwd_f32", ctypes.byref(shp), p(x_d), p(wp), None, None, None, p(z_d), p(stats), DS_EPI_STATS, be.stream)
    g_d, b_d = be.put(gamma), be.put(beta)
    t1 = [be.nan(co, F32) for _ in range(4)]                        # mean, invstd, scale, shift
    rm1, rv1 = be.put(rm), be.put(rv)
    lib.call("ds_bn_stats_finalize_f32", p(stats), rows, n, p(g_d), p(b_d), EPS, MOMENTUM, p(rm1), p(rv1), *(p(t) for t in t1),
             co, be.stream)
    # the data-parallel pair, with the count as an argument and (count = 0) read from sums[2C]
    for count in (n, 0):
        sums = be.put(np.full(2 * co + 1, float(n) if count == 0 else np.nan))
        t2 = [be.nan(co, F32) for _ in range(4)]
        rm2, rv2 = be.put(rm), be.put(rv)
        lib.call("ds_partial_sum_f64", p(stats), rows, p(sums), co, be.stream)
        lib.call("ds_bn_stats_from_sums_f32", p(sums), count, p(g_d), p(b_d), EPS, MOMENTUM, p(rm2), p(rv2), *(p(t) for t in t2),
                 co, be.stream)
        for a, c in zip(t1 + [rm1, rv1], t2 + [rm2, rv2]):
            assert be.same(a, c), f"split form, count {count}"
    # the sums form of G = 3 members in one launch against three single calls (count 0: each row's own count slot),
    # the running statistics chained in call order; once without running statistics
    rs3 = np.random.RandomState(seed_of(*case) + 3)
    sums3 = np.empty((3, 2 * co + 1), F64)
    for m in range(3):
        zs = rs3.randn(37 + 11 * m, co) * (1 + m) + m
        sums3[m, :2 * co] = np.stack([zs.sum(0), (zs * zs).sum(0)], axis=1).ravel()
        sums3[m, 2 * co] = zs.shape[0]
    s3, s1 = be.put(sums3), [be.put(sums3[m:m + 1]) for m in range(3)]
    for with_running in (True, False):
        tg = [be.nan((3, co), F32) for _ in range(4)]
        ts = [[be.nan((1, co), F32) for _ in range(4)] for m in range(3)]
        rg = [be.put(rm), be.put(rv)] if with_running else [None, None]
        rc = [be.put(rm), be.put(rv)] if with_running else [None, None]
        lib.call("ds_bn_stats_from_sums_group_f32", p(s3), p(g_d), p(b_d), EPS, MOMENTUM, p(rg[0]), p(rg[1]), *(p(t) for t in tg),
                 co, 3, be.stream)
        for m in range(3):
            lib.call("ds_bn_stats_from_sums_f32", p(s1[m]), 0, p(g_d), p(b_d), EPS, MOMENTUM, p(rc[0]), p(rc[1]),
                     *(p(t) for t in ts[m]), co, be.stream)
            for a, c in zip(tg, ts[m]):
                assert np.isfinite(be.get(c)).all() and be.same(be.part(a, m, 1), c), f"grouped sums form, member {m}"
        if with_running:
            assert be.same(rg[0], rc[0]) and be.same(rg[1], rc[1]), "grouped sums form, running statistics"
            assert np.isfinite(be.get(rg[0])).all() and np.isfinite(be.get(rg[1])).all()
    mean_k, invstd_k, scale_k, shift_k = (be.get(t) for t in t1)
    # float64 reference and the float32 restatement (torch float32 convolution, float32 sums per statistics row)
    z64 = O.conv2d(x.astype(F64), wt.astype(F64), s, k // 2)
    zf = to_nhwc(z64).reshape(n, co)
    mean, var = zf.mean(0), zf.var(0)
    invstd = 1 / np.sqrt(var + EPS)
    scale = gamma * invstd
    shift = beta - mean * scale
    unb = var * (n / (n - 1.0))
    erm, erv = (1 - MOMENTUM) * rm + MOMENTUM * mean, (1 - MOMENTUM) * rv + MOMENTUM * unb
    z32 = torch.nn.functional.conv2d(torch.from_numpy(x), torch.from_numpy(wt), stride=s, padding=k // 2)
    z32 = z32.permute(0, 2, 3, 1).reshape(n, co).numpy()
    cuts = np.arange(0, n, max(1, -(-n // rows)))
    r1 = np.add.reduceat(z32, cuts, axis=0).astype(F64).sum(0)
    r2 = np.add.reduceat(z32 * z32, cuts, axis=0).astype(F64).sum(0)
    m_r = r1 / n
    v_r = np.maximum(r2 / n - m_r * m_r, 0)
    i_r = 1 / np.sqrt(v_r + EPS)
    restated = {"mean": tol_err(m_r, mean, 1e-6), "invstd": tol_err(i_r, invstd),
                "running_mean": tol_err((1 - MOMENTUM) * rm + MOMENTUM * m_r, erm, 1e-6),
                "running_var": tol_err((1 - MOMENTUM) * rv + MOMENTUM * v_r * (n / (n - 1.0)), erv, 1e-6)}
    bars = {kk: bar_from_restatement(1e-5, v) for kk, v in restated.items()}
    got = {"mean": tol_err(mean_k, mean, 1e-6), "invstd": tol_err(invstd_k, invstd),
           "running_mean": tol_err(be.get(rm1), erm, 1e-6), "running_var": tol_err(be.get(rv1), erv, 1e-6)}
    # scale = gamma * invstd carries invstd's error; shift = beta - mean * scale the sum of both, on the larger term
    got_scale = tol_err(scale_k, scale)
    got_shift = float((np.abs(shift_k - shift) / (np.abs(beta) + np.abs(mean * scale) + 1e-6)).max())
    print(f"bn forward {case} ({rows} rows, {n} pixels): " +
          ", ".join(f"{kk} f32-restated {restated[kk]:.2e} bar {bars[kk]:.2e} kernel {got[kk]:.2e}" for kk in got) +
          f", scale {got_scale:.2e}, shift {got_shift:.2e}")
    for kk in got:
        assert got[kk] <= bars[kk], (kk, got[kk], bars[kk])
    assert got_scale <= bars["invstd"] + 1e-7 and got_shift <= bars["invstd"] + bars["mean"] + 1e-7, (got_scale, got_shift)
    # ds_bn_stats_finalize_f32 on synthetic partial rows: the convolution cases give few rows, and nothing else reaches
    # past the first stride of the fold's 128 row lanes.  1 / 129 / 300 rows; 66 and 65 channels: a last workgroup of
    # the sums form (256 channels each) and of the rows form (2 channels each) that is only part full.  Reference: the
    # same float32 rows added in float64, under the bars derived above; and the split pair, bit for bit.
    for rows_s, cs in [(r, c) for r in (1, 129, 300) for c in (64, 66)] + [(129, 65)]:
        rs2 = np.random.RandomState(seed_of(rows_s, cs))
        zs = (rs2.randn(rows_s, 4, cs) * 2 + 1).astype(F32)                       # four pixels per row
        part = np.stack([zs.sum(1), (zs * zs).sum(1)], axis=2).astype(F32)         # [rows][C][2]
        ns = rows_s * 4
        gam, bet = rs2.uniform(4.0, 8.0, cs).astype(F32), (8 + rs2.randn(cs)).astype(F32)
        rms, rvs = (rs2.randn(cs) * 0.1).astype(F32), rs2.uniform(0.5, 1.5, cs).astype(F32)
        fold = part.astype(F64).sum(0)
        mean_s = fold[:, 0] / ns
        var_s = np.maximum(fold[:, 1] / ns - mean_s * mean_s, 0)
        invstd_s = 1 / np.sqrt(var_s + EPS)
        scale_s = gam * invstd_s
        shift_s = bet - mean_s * scale_s
        erm_s = (1 - MOMENTUM) * rms + MOMENTUM * mean_s
        erv_s = (1 - MOMENTUM) * rvs + MOMENTUM * var_s * (ns / (ns - 1.0))
        part_d, gs_d, bs_d = be.put(part), be.put(gam), be.put(bet)
        ta, tb = [be.nan(cs, F32) for _ in range(4)], [be.nan(cs, F32) for _ in range(4)]
        ra, rb = [be.put(rms), be.put(rvs)], [be.put(rms), be.put(rvs)]
        sums_s = be.nan(2 * cs, F64)
        lib.call("ds_bn_stats_finalize_f32", p(part_d), rows_s, ns, p(gs_d), p(bs_d), EPS, MOMENTUM, p(ra[0]), p(ra[1]),
                 *(p(t) for t in ta), cs, be.stream)
        lib.call("ds_partial_sum_f64", p(part_d), rows_s, p(sums_s), cs, be.stream)
        lib.call("ds_bn_stats_from_sums_f32", p(sums_s), ns, p(gs_d), p(bs_d), EPS, MOMENTUM, p(rb[0]), p(rb[1]),
                 *(p(t) for t in tb), cs, be.stream)
        mk, ik, sk, hk = (be.get(t) for t in ta)
        got_s = {"mean": tol_err(mk, mean_s, 1e-6), "invstd": tol_err(ik, invstd_s),
                 "running_mean": tol_err(be.get(ra[0]), erm_s, 1e-6), "running_var": tol_err(be.get(ra[1]), erv_s, 1e-6)}
        e_scale = tol_err(sk, scale_s)
        e_shift = float((np.abs(hk - shift_s) / (np.abs(bet) + np.abs(mean_s * scale_s) + 1e-6)).max()) if np.isfinite(hk).all() else float("inf")
        e_fold = tol_err(be.get(sums_s).reshape(cs, 2), fold, 1e-9)
        print(f"bn finalize, synthetic {rows_s} rows x {cs} channels: " + ", ".join(f"{kk} {got_s[kk]:.2e} (bar {bars[kk]:.2e})" for kk in got_s) +
              f", scale {e_scale:.2e}, shift {e_shift:.2e}, float64 fold {e_fold:.2e}")
        for kk in got_s:
            assert got_s[kk] <= bars[kk], (rows_s, cs, kk, got_s[kk], bars[kk])
        assert e_scale <= bars["invstd"] + 1e-7 and e_shift <= bars["invstd"] + bars["mean"] + 1e-7, (rows_s, cs, e_scale, e_shift)
        assert e_fold <= 1e-12, (rows_s, cs, e_fold)                # float64 sums of at most 300 rows in another order
        for a, c in zip(ta + ra, tb + rb):
            assert be.same(a, c), f"synthetic rows {rows_s} x {cs}: split form"
    # normalise: the kernel's own tables and its own z, in float64.  A float32 evaluation rounds at most three times
    # (product, sum, residual sum), each by 2^-24 of a value no larger than `top`
    z_h = be.get(z_d).astype(F64).reshape(n, co)
    res_d = be.put(res)
    pre = z_h * scale_k.astype(F64) + shift_k.astype(F64)
    both = pre + res.reshape(n, co)
    assert float((both <= 0).mean()) > 0.01 and float((both >= 20).mean()) > 0.01
    for flags, want in ((0, pre), (DS_EPI_CLIP, np.clip(pre, 0, 20)), (DS_EPI_RESIDUAL | DS_EPI_CLIP, np.clip(both, 0, 20))):
        y = be.nan((n, co), F32)
        lib.call("ds_bn_apply_f32", p(z_d), p(t1[2]), p(t1[3]), p(res_d) if flags & DS_EPI_RESIDUAL else None, p(y), n, co, flags,
                 be.stream)
        top = float((np.abs(z_h * scale_k) + np.abs(shift_k) + (np.abs(res.reshape(n, co)) if flags & DS_EPI_RESIDUAL else 0)).max())
        got_y = be.get(y)
        worst = float(np.abs(got_y - want).max()) if np.isfinite(got_y).all() else float("inf")
        print(f"bn apply {case} flags {flags}: max abs err {worst:.3e} (bar {3 * 2.0 ** -24 * top:.3e}, largest value {top:.3g})")
        assert worst <= 3 * 2.0 ** -24 * top, (flags, worst)
    # eval-mode fold of the updated running statistics: two tables of three float32 roundings each (sum, root, quotient,
    # product ...), so y = x * scale + shift stays within 1e-6 of O.bn_eval relative to its largest value
    sc_f, sh_f = be.nan(co, F32), be.nan(co, F32)
    lib.call("ds_bn_fold_f32", p(g_d), p(b_d), p(rm1), p(rv1), EPS, p(sc_f), p(sh_f), co, be.stream)
    rm_k, rv_k = be.get(rm1), be.get(rv1)
    assert abs(O.BN_EPS - EPS) < 1e-12
    want = O.bn_eval(z64, gamma, beta, rm_k, rv_k)
    got_y = z64 * be.get(sc_f).astype(F64)[None, :, None, None] + be.get(sh_f).astype(F64)[None, :, None, None]
    e_fold = finite_rel_err(got_y, want)
    print(f"bn fold {case}: {e_fold:.2e} (bar 1e-6)")
    assert e_fold < 1e-6, e_fold


# (C, n_pix, with g2, with act): test_bn_bwd's four, the 2048-row cap, three small rows
BN_BWD_CASES = [(64, 700, True, True), (128, 300, False, True), (512, 50, False, False), (256, 1030, True, False),
                (64, 300000, False, True), (512, 40, True, True)]
BN_BWD_ROWS = {(64, 300000): 2048, (512, 40): 3}
BN_BWD_GROUP_MAX_PIX = 2000                 # the grouped form (G = 3) runs where three members stay small


def _same_all(be, got, want, names, what):
    for name in names:
        assert be.same(got[name], want[name]), f"{what}: {name}"


def body_bn_bwd(be, C, n_pix, with_g2, with_act):
    """ds_bn_bwd_f32 against float64; the split form (reduce -> float64 fold -> apply), the grouped entry points with
    G = 1 (what backward._bn_bwd calls for one member: one call, reduce + apply, finish) and the grouped form (G = 3, its
    members' dgamma / dbeta folded by ds_colsum_f32; one call, reduce + apply, finish) agree with it bit for bit.  With
    G = 1 the member_sums scratch is NOT touched (the coefficient kernel writes dgamma / dbeta in place, no member sum);
    ds_partial_sum_f64 leaves the count slot behind its [C][2] alone, the grouped reduce writes it."""
    lib, p = be.lib, be.p
    G = 3 if n_pix <= BN_BWD_GROUP_MAX_PIX else 1
    rows = lib.raw("ds_bn_bwd_partial_rows")(n_pix, C)
    assert rows == BN_BWD_ROWS.get((C, n_pix), rows), rows
    gen = torch.Generator().manual_seed(C + n_pix)
    z = (torch.randn((G * n_pix, C), generator=gen) * 2 + 1).numpy()
    g1 = torch.randn((G * n_pix, C), generator=gen).numpy()
    g2 = torch.randn((G * n_pix, C), generator=gen).numpy() if with_g2 else None
    act = (torch.rand((G * n_pix, C), generator=gen) * 30 - 5).clamp(0, 20).numpy() if with_act else None
    gamma = np.random.RandomState(C).uniform(0.5, 1.5, C).astype(F32)
    zs = z.reshape(G, n_pix, C).astype(F64)
    mean, invstd = zs.mean(1).astype(F32), (1 / np.sqrt(zs.var(1) + EPS)).astype(F32)
    gy_ref = g1.astype(F64) + (g2 if with_g2 else 0)
    if with_act:
        gy_ref = gy_ref * ((act > 0) & (act < 20))
    gy_ref = gy_ref.reshape(G, n_pix, C)
    g1_d, g2_d, act_d, z_d = be.put(g1), (be.put(g2) if with_g2 else None), (be.put(act) if with_act else None), be.put(z)
    mean_d, invstd_d, gm = be.put(mean), be.put(invstd), be.put(gamma)

    def member(h, m):
        return None if h is None else be.part(h, m * n_pix, n_pix)

    one_call = []
    for m in range(G):
        mu, is_ = be.put(mean[m]), be.put(invstd[m])
        args = (p(member(g1_d, m)), p(member(g2_d, m)), p(member(act_d, m)), p(member(z_d, m)), p(mu), p(is_))
        gy, gz = be.nan((n_pix, C), F32), be.nan((n_pix, C), F32)
        partial, coef, gg, gb = be.nan((rows, C, 2), F32), be.nan(3 * C, F32), be.nan(C, F32), be.nan(C, F32)
        lib.call("ds_bn_bwd_f32", *args, p(gm), p(gy), p(partial), p(coef), p(gg), p(gb), p(gz), n_pix, C, be.stream)
        # the split form around the float64 fold
        gy2, gz2 = be.nan((n_pix, C), F32), be.nan((n_pix, C), F32)
        partial2, coef2, gg2, gb2 = be.nan((rows, C, 2), F32), be.nan(3 * C, F32), be.nan(C, F32), be.nan(C, F32)
        sums = be.nan(2 * C + 1, F64)
        lib.call("ds_bn_bwd_reduce_f32", *args, p(gy2), p(partial2), n_pix, C, be.stream)
        lib.call("ds_partial_sum_f64", p(partial2), rows, p(sums), C, be.stream)
        lib.call("ds_bn_bwd_apply_f32", p(sums), n_pix, p(gy2), p(member(z_d, m)), p(mu), p(is_), p(gm), p(coef2), p(gg2), p(gb2),
                 p(gz2), n_pix, C, be.stream)
        for a, c, what in ((gy, gy2, "gy"), (gz, gz2, "gz"), (partial, partial2, "partial"), (coef, coef2, "coef"),
                           (gg, gg2, "dgamma"), (gb, gb2, "dbeta")):
            assert be.same(a, c), f"split form: {what} of member {m}"
        sums_h = be.get(sums)
        assert np.isfinite(sums_h[:2 * C]).all() and np.isnan(sums_h[2 * C]), "ds_partial_sum_f64 writes [C][2], no count"
        # the grouped entry points with G = 1
        want = dict(gy=gy, gz=gz, partial=partial, coef=coef, gg=gg, gb=gb)
        names = ("gy", "gz", "partial", "coef", "gg", "gb")

        def fresh():
            o = dict(gy=be.nan((n_pix, C), F32), gz=be.nan((n_pix, C), F32), partial=be.nan((rows, C, 2), F32),
                     coef=be.nan(3 * C, F32), gg=be.nan(C, F32), gb=be.nan(C, F32), msums=be.nan((2, 1, C), F32))
            tail = (p(member(z_d, m)), p(mu), p(is_), p(gm), p(o["coef"]), p(o["msums"]), p(o["gg"]), p(o["gb"]), p(o["gz"]),
                    n_pix, C, 1, be.stream)
            return o, tail

        o, _ = fresh()
        lib.call("ds_bn_bwd_group_f32", *args, p(gm), p(o["gy"]), p(o["partial"]), p(o["coef"]), p(o["msums"]), p(o["gg"]),
                 p(o["gb"]), p(o["gz"]), n_pix, C, 1, be.stream)
        _same_all(be, o, want, names, f"ds_bn_bwd_group_f32, G = 1, member {m}")
        assert np.isnan(be.get(o["msums"])).all(), "G = 1: member_sums is not touched"
        o, tail = fresh()
        sums1 = be.nan((1, 2 * C + 1), F64)
        lib.call("ds_bn_bwd_group_reduce_f32", *args, p(o["gy"]), p(o["partial"]), p(sums1), n_pix, C, 1, be.stream)
        assert be.get(sums1)[0, 2 * C] == n_pix
        assert np.array_equal(be.get(sums1)[0, :2 * C], sums_h[:2 * C])
        lib.call("ds_bn_bwd_group_apply_f32", p(sums1), p(o["gy"]), *tail)
        _same_all(be, o, want, names, f"group reduce + apply, G = 1, member {m}")
        assert np.isnan(be.get(o["msums"])).all(), "G = 1: member_sums is not touched"
        o, tail = fresh()
        lib.call("ds_bn_bwd_group_finish_f32", p(partial), rows, p(gy), *tail)
        _same_all(be, o, want, ("gz", "coef", "gg", "gb"), f"ds_bn_bwd_group_finish_f32, G = 1, member {m}")
        assert np.isnan(be.get(o["msums"])).all(), "G = 1: member_sums is not touched"
        gz_ref, gg_ref, gb_ref = O.bn_train_bwd(zs[m].T.reshape(1, C, n_pix, 1), mean[m].astype(F64), invstd[m].astype(F64),
                                                gamma.astype(F64), gy_ref[m].T.reshape(1, C, n_pix, 1))
        assert np.isfinite(be.get(partial)).all()
        errs = (finite_rel_err(be.get(gy), gy_ref[m]), finite_rel_err(be.get(gz), gz_ref[0, :, :, 0].T),
                finite_rel_err(be.get(gg), gg_ref), finite_rel_err(be.get(gb), gb_ref))
        print(f"bn_bwd C={C} n_pix={n_pix} rows={rows} g2={with_g2} act={with_act} member {m}: gy {errs[0]:.2e} (bar 1e-6), "
              f"gz {errs[1]:.2e} dgamma {errs[2]:.2e} dbeta {errs[3]:.2e} (bar 1e-4)")
        assert errs[0] < 1e-6 and max(errs[1:]) < 1e-4, errs
        one_call.append((gy, gz, coef, gg, gb))
    if G == 1:
        return
    gy, gz = be.nan((G * n_pix, C), F32), be.nan((G * n_pix, C), F32)
    partial, coef, msums = be.nan((G, rows, C, 2), F32), be.nan((G, 3 * C), F32), be.nan((2, G, C), F32)
    gg, gb = be.nan(C, F32), be.nan(C, F32)
    lib.call("ds_bn_bwd_group_f32", p(g1_d), p(g2_d), p(act_d), p(z_d), p(mean_d), p(invstd_d), p(gm), p(gy), p(partial), p(coef),
             p(msums), p(gg), p(gb), p(gz), n_pix, C, G, be.stream)
    gy_h, gz_h, coef_h = be.get(gy), be.get(gz), be.get(coef)
    for m, (gy1, gz1, coef1, _, _) in enumerate(one_call):
        sl = slice(m * n_pix, (m + 1) * n_pix)
        assert np.array_equal(gy_h[sl], be.get(gy1)) and np.array_equal(gz_h[sl], be.get(gz1)), f"grouped form, member {m}"
        assert np.array_equal(coef_h[m], be.get(coef1))
    # dgamma / dbeta: the members' rows added in member order == the column sum of the one-call results
    for got, idx, what in ((gg, 3, "dgamma"), (gb, 4, "dbeta")):
        stacked = be.put(np.stack([be.get(o[idx]) for o in one_call]))
        folded = be.nan(C, F32)
        lib.call("ds_colsum_f32", p(stacked), p(folded), G, C, be.stream)
        assert be.same(got, folded), what
    # the grouped form split at the all-reduce, and its second half alone from the grouped partial rows
    want = dict(gy=gy, gz=gz, partial=partial, coef=coef, msums=msums, gg=gg, gb=gb)

    def fresh():
        o = dict(gy=be.nan((G * n_pix, C), F32), gz=be.nan((G * n_pix, C), F32), partial=be.nan((G, rows, C, 2), F32),
                 coef=be.nan((G, 3 * C), F32), msums=be.nan((2, G, C), F32), gg=be.nan(C, F32), gb=be.nan(C, F32))
        tail = (p(z_d), p(mean_d), p(invstd_d), p(gm), p(o["coef"]), p(o["msums"]), p(o["gg"]), p(o["gb"]), p(o["gz"]),
                n_pix, C, G, be.stream)
        return o, tail

    o, tail = fresh()
    sums = be.nan((G, 2 * C + 1), F64)
    lib.call("ds_bn_bwd_group_reduce_f32", p(g1_d), p(g2_d), p(act_d), p(z_d), p(mean_d), p(invstd_d), p(o["gy"]),
             p(o["partial"]), p(sums), n_pix, C, G, be.stream)
    assert (be.get(sums)[:, 2 * C] == n_pix).all()
    lib.call("ds_bn_bwd_group_apply_f32", p(sums), p(o["gy"]), *tail)
    _same_all(be, o, want, ("gy", "gz", "partial", "coef", "msums", "gg", "gb"), "group reduce + apply, G = 3")
    o, tail = fresh()
    lib.call("ds_bn_bwd_group_finish_f32", p(partial), rows, p(gy), *tail)
    _same_all(be, o, want, ("gz", "coef", "msums", "gg", "gb"), "ds_bn_bwd_group_finish_f32, G = 3")


# The argument lists of the f32 BatchNorm backward's entry points and the calls they REFUSE: (entry point, argument, bad
# value, return code) with None = a null pointer and "+4" = the pointer moved by 4 bytes; everything else about the call is
# valid (n_pix 16, C 8, G 2, one partial row).  The codes are those of the library before the entry points shared their
# launches (-1 bad shape, -2 alignment, -3 null): each entry point checks what it always checked, and they differ -- only the
# grouped forms look at the alignment of g2, ds_bn_bwd_apply_f32 and the float64 folds at none, and the folds take any C > 0.
# Only refused calls are listed: one that is accepted would launch with the bad argument.
BN_BWD_ARGS = {
    "ds_bn_bwd_f32": "g1 g2 act z mean invstd gamma gy partial coef gg gb gz n_pix C",
    "ds_bn_bwd_reduce_f32": "g1 g2 act z mean invstd gy partial n_pix C",
    "ds_bn_bwd_apply_f32": "sums count gy z mean invstd gamma coef gg gb gz n_pix C",
    "ds_bn_bwd_group_f32": "g1 g2 act z mean invstd gamma gy partial coef msums gg gb gz n_pix C G",
    "ds_bn_bwd_group_reduce_f32": "g1 g2 act z mean invstd gy partial sums n_pix C G",
    "ds_bn_bwd_group_apply_f32": "sums gy z mean invstd gamma coef msums gg gb gz n_pix C G",
    "ds_bn_bwd_group_finish_f32": "partial n_partial gy z mean invstd gamma coef msums gg gb gz n_pix C G",
    "ds_partial_sum_f64": "partial n_partial sums C",
    "ds_partial_sum_f64_group": "partial n_partial sums count C G",
}
BN_BWD_REFUSALS = [
    ("ds_bn_bwd_f32", "z", None, -3), ("ds_bn_bwd_f32", "gb", None, -3), ("ds_bn_bwd_f32", "C", 6, -1),
    ("ds_bn_bwd_f32", "C", 2048, -1), ("ds_bn_bwd_f32", "n_pix", 0, -1), ("ds_bn_bwd_f32", "g1", "+4", -2),
    ("ds_bn_bwd_f32", "coef", "+4", -2),
    ("ds_bn_bwd_reduce_f32", "partial", None, -3), ("ds_bn_bwd_reduce_f32", "C", 6, -1),
    ("ds_bn_bwd_reduce_f32", "n_pix", 0, -1), ("ds_bn_bwd_reduce_f32", "g1", "+4", -2),
    ("ds_bn_bwd_apply_f32", "sums", None, -3), ("ds_bn_bwd_apply_f32", "gamma", None, -3),
    ("ds_bn_bwd_apply_f32", "C", 6, -1), ("ds_bn_bwd_apply_f32", "n_pix", 0, -1), ("ds_bn_bwd_apply_f32", "count", -1, -1),
    ("ds_bn_bwd_group_f32", "z", None, -3), ("ds_bn_bwd_group_f32", "msums", None, -3), ("ds_bn_bwd_group_f32", "C", 6, -1),
    ("ds_bn_bwd_group_f32", "G", 0, -1), ("ds_bn_bwd_group_f32", "G", 65, -1), ("ds_bn_bwd_group_f32", "n_pix", 0, -1),
    ("ds_bn_bwd_group_f32", "g1", "+4", -2), ("ds_bn_bwd_group_f32", "g2", "+4", -2), ("ds_bn_bwd_group_f32", "act", "+4", -2),
    ("ds_bn_bwd_group_reduce_f32", "sums", None, -3), ("ds_bn_bwd_group_reduce_f32", "C", 6, -1),
    ("ds_bn_bwd_group_reduce_f32", "G", 0, -1), ("ds_bn_bwd_group_reduce_f32", "G", 65, -1),
    ("ds_bn_bwd_group_reduce_f32", "n_pix", 0, -1), ("ds_bn_bwd_group_reduce_f32", "g1", "+4", -2),
    ("ds_bn_bwd_group_reduce_f32", "g2", "+4", -2),
    ("ds_bn_bwd_group_apply_f32", "sums", None, -3), ("ds_bn_bwd_group_apply_f32", "msums", None, -3),
    ("ds_bn_bwd_group_apply_f32", "C", 6, -1), ("ds_bn_bwd_group_apply_f32", "G", 0, -1),
    ("ds_bn_bwd_group_apply_f32", "G", 65, -1), ("ds_bn_bwd_group_apply_f32", "n_pix", 0, -1),
    ("ds_bn_bwd_group_apply_f32", "gy", "+4", -2),
    ("ds_bn_bwd_group_finish_f32", "partial", None, -3), ("ds_bn_bwd_group_finish_f32", "C", 6, -1),
    ("ds_bn_bwd_group_finish_f32", "G", 0, -1), ("ds_bn_bwd_group_finish_f32", "G", 65, -1),
    ("ds_bn_bwd_group_finish_f32", "n_pix", 0, -1), ("ds_bn_bwd_group_finish_f32", "n_partial", 0, -1),
    ("ds_bn_bwd_group_finish_f32", "coef", "+4", -2),
    ("ds_partial_sum_f64", "sums", None, -3), ("ds_partial_sum_f64", "C", 0, -1), ("ds_partial_sum_f64", "n_partial", 0, -1),
    ("ds_partial_sum_f64_group", "partial", None, -3), ("ds_partial_sum_f64_group", "C", 0, -1),
    ("ds_partial_sum_f64_group", "G", 0, -1), ("ds_partial_sum_f64_group", "G", 65, -1),
    ("ds_partial_sum_f64_group", "n_partial", 0, -1), ("ds_partial_sum_f64_group", "count", 0, -1),
]


def bn_bwd_refused_calls(be, refusals):
    """[(entry point, argument, bad value, return code of the call)] for `refusals`, then: nothing was written"""
    n_pix, C, G = 16, 8, 2
    shapes = dict(g1=(G * n_pix, C), g2=(G * n_pix, C), act=(G * n_pix, C), z=(G * n_pix, C), gy=(G * n_pix, C),
                  gz=(G * n_pix, C), mean=(G, C), invstd=(G, C), gamma=(C,), partial=(G, 1, C, 2), coef=(G, 3 * C),
                  msums=(2, G, C), gg=(C,), gb=(C,))
    bufs = {name: be.nan(shape, F32) for name, shape in shapes.items()}
    bufs["sums"] = be.nan((G, 2 * C + 1), F64)
    scalars = dict(n_pix=n_pix, C=C, G=G, n_partial=1, count=n_pix)
    assert be.lib.raw("ds_bn_bwd_partial_rows")(n_pix, C) == 1
    got = []
    for entry, arg, bad, _ in refusals:
        names = BN_BWD_ARGS[entry].split()
        assert arg in names, (entry, arg)
        args = []
        for name in names:
            v = scalars[name] if name in scalars else address(be.p(bufs[name]))
            if name == arg:
                v = v + 4 if bad == "+4" else bad
            args.append(v)
        got.append((entry, arg, bad, be.lib.raw(entry)(*args, be.stream)))
    for name, h in bufs.items():
        assert np.isnan(be.get(h)).all(), f"a refused call wrote to {name}"
    return got


def body_bn_bwd_refusals(be):
    """every entry point of the f32 BatchNorm backward refuses what it refused before, with the same code, and launches
    nothing"""
    got = bn_bwd_refused_calls(be, BN_BWD_REFUSALS)
    for row in got:
        print("refused: %s(%s = %r) -> %d" % row)
    assert all(rc != 0 for _, _, _, rc in got)
    assert got == BN_BWD_REFUSALS


COLSUM_CASES = [(1031, 77), (3, 512), (40, 32)]                     # (rows, columns): columns no multiple of the 32 per workgroup


def body_colsum(be, R, C):
    """ds_colsum_f32 against float64; the restatement: eight float32 row lanes, folded in lane order"""
    x = np.random.RandomState(R + C).randn(R, C).astype(F32)
    x_d, out = be.put(x), be.nan(C + 8, F32)
    be.lib.call("ds_colsum_f32", be.p(x_d), be.p(out), R, C, be.stream)
    got = be.get(out)
    assert np.isnan(got[C:]).all(), "written past the last column"
    ref = x.astype(F64).sum(0)
    lanes = np.stack([x[l::8].sum(0, dtype=F32) if l < R else np.zeros(C, F32) for l in range(8)])
    restated = rel_err(np.add.reduce(lanes, axis=0, dtype=F32), ref)
    bar, err = bar_from_restatement(1e-6, restated), finite_rel_err(got[:C], ref)
    print(f"colsum {R}x{C}: f32-restated {restated:.2e} bar {bar:.2e} kernel {err:.2e}")
    assert err <= bar, (err, bar)
