"""The fp16 forward convolutions (conv_mfma_f16_kernel.h, conv_mfma_f16_pkernel.h, conv_block_f16.hip), one kernel at a time
under EVERY tile configuration of kCfgH: case lists, float64 references and the test bodies, written once against the backend
adapter of bf16_train_cases.py and run by test_emul_f16_kernels.py (host emulator, numpy memory) and
test_gpu_f16_kernels.py (MI355X, torch device memory).

    a. ds_conv_fwd_f16 LAUNCHED under configurations 0 .. 6 (ds_conv_f16_set_forced_cfg) and the planner's own choice, in
       every form a launch can take (persistent / one tile per workgroup / single-buffered / 64-wide / 16-channel chunks /
       plane-major input), each with three epilogues: raw f32, affine + residual + clip to fp16, the same to 16-channel planes
    b. persistent workgroups that walk several tiles, every configuration (device only: the batch comes from the CU count)
    c. ds_conv_fwd_f16_splitk: 8, 4 and 2 ways, an uneven split, the one-pass fall-backs
    d. ds_conv_block_f16 / _masked: output flags, the XCD-dealt tile order (device only)
    e. what a forced configuration, a layout flag or a shape must still refuse

Rules (bf16_train_cases.py): every output and workspace starts as NaN; a bar never comes from the kernel's output; every body
prints its errors and bars; the hook goes back to -1 whatever happens.

Operands (test_gpu_f16_plans.py::_operands): x = |randn| * 2 and the residual |randn| * 8 rounded to fp16, filters
randn / sqrt(Cin KS^2) rounded to fp16, scale in [0.5, 1.5], shift randn, seeded from the case.

Bars.  Raw f32 output: 2e-6 on the max-norm relative error (conftest.rel_err) against the float64 convolution of the SAME
fp16-rounded operands -- the bar of test_emul_f16.py: fp16 products are exact in f32, only the summation order differs.
fp16 output of the epilogue: 20 * 2^-11 + 1e-5 absolute -- one fp16 rounding of a value in [0, 20] plus the f32 epilogue, the
TOL of test_gpu_f16_plans.py.  The FIRST output of each epilogue kind is held to its bar; every other configuration and form is
bit for bit the first (a pixel's contraction order -- chunks, taps, k steps -- does not depend on the plan), and
the un-permuted plane-major output is bit for bit the channels-last one."""
import contextlib
import ctypes
import functools

import numpy as np
import torch

from bf16_train_cases import F32, F64, DS_ERR_UNSUPPORTED, finite_rel_err, frozen, out_dims, seed_of
from f16_plan_cases import BAD
from deepspeaker_pytorch_amd._native import (ConvShape, DS_CONV_HINT_CHUNK16, DS_CONV_HINT_NO_PERSIST, DS_CONV_HINT_NO_WIDE,
                                             DS_CONV_HINT_ONE_QUEUE, DS_CONV_HINT_SINGLE_BUFFER, DS_CONV_IN_PLANES16,
                                             DS_EPI_AFFINE, DS_EPI_CLIP, DS_EPI_OUT_F32, DS_EPI_OUT_PLANES16, DS_EPI_RESIDUAL)

F16, I32 = np.float16, np.int32

# kCfgH of conv_mfma_f16_kernel.h, rows 0 .. 6: (M tile, N tile) and threads per workgroup; row 7 (128 x 256 on two waves) is
# what the persistent kernel widens row 4 to for a 3x3 layer with Cout % 256 == 0 and cannot be forced
CFG_TILES = [(160, 128), (160, 256), (320, 128), (320, 64), (128, 128), (128, 256), (640, 64)]
CFG_THREADS = [128, 256, 256, 128, 128, 256, 256]
WIDE_TILE = (128, 256, 128)
CFGS = (-1, 0, 1, 2, 3, 4, 5, 6)
RAW_BAR = 2e-6
F16_BAR = 20 * 2.0 ** -11 + 1e-5
FUSED = DS_EPI_AFFINE | DS_EPI_RESIDUAL | DS_EPI_CLIP

# every launch of body a / b: (KS, M tile, N tile, threads, persistent, double-buffered, 16-channel chunks, NIT)
LAUNCHED = set()
FWD_RAN = set()             # the cases body a ran in every form under every configuration
# the largest errors of this process, by kind (printed by the coverage test)
WORST = {}


@contextlib.contextmanager
def forced_cfg(lib, cfg):
    """plan every fp16 convolution with tile configuration `cfg` (-1: the planner's choice) -- a process-global hook that
    later tests plan through, so it goes back to -1 whatever happens"""
    try:
        lib.raw("ds_conv_f16_set_forced_cfg")(cfg)
        yield
    finally:
        lib.raw("ds_conv_f16_set_forced_cfg")(-1)


def describe(lib, shp, hint=0):
    out8 = (ctypes.c_int * 8)()
    rc = lib.raw("ds_conv_f16_plan_describe_hinted")(ctypes.byref(shp), hint, out8)
    return rc, list(out8)


def plan_row(ks, out8):
    """out8[7] = 10000 persistent + 1000 double-buffered + 100 16-channel chunks + staging items per thread"""
    return (ks, out8[0], out8[1], out8[6], out8[7] >= 10000, out8[7] % 10000 >= 1000, out8[7] % 1000 >= 100, out8[7] % 100)


def check_tile(cfg, ks, hint, out8):
    """the plan is the forced configuration's; the wide tile only where widen_persistent applies"""
    tile = (out8[0], out8[1], out8[6])
    if tile == WIDE_TILE:
        assert cfg in (-1, 4) and ks == 3 and out8[7] >= 10000 and not hint & DS_CONV_HINT_NO_WIDE, (cfg, ks, hint, out8)
    elif cfg >= 0:
        assert tile == CFG_TILES[cfg] + (CFG_THREADS[cfg],), (cfg, out8)
    else:
        assert tile in [t + (n,) for t, n in zip(CFG_TILES, CFG_THREADS)], out8


def note(kind, err):
    WORST[kind] = max(WORST.get(kind, 0.0), err)


def conv64(x_nhwc, wt, k, s):
    """float64 convolution of channels-last fp16 pixels with OIHW filters, channels-last"""
    xt = torch.from_numpy(np.ascontiguousarray(x_nhwc)).double().permute(0, 3, 1, 2)
    z = torch.nn.functional.conv2d(xt, torch.from_numpy(np.ascontiguousarray(wt)).double(), None, s, k // 2)
    return z.permute(0, 2, 3, 1).contiguous().numpy()


@functools.lru_cache(maxsize=None)
def conv_inputs(case, n_ref=None):
    """operands (channels-last) and float64 references of one case; the references cover the first n_ref images"""
    b, ci, co, h, w, k, s = case
    rs = np.random.RandomState(seed_of(*case))
    ho, wo = out_dims(h, w, k, s)
    x = (np.abs(rs.randn(b, h, w, ci)) * 2).astype(F16)
    wt = (rs.randn(co, ci, k, k) / np.sqrt(ci * k * k)).astype(F16).astype(F32)
    scale, shift = rs.uniform(0.5, 1.5, co).astype(F32), rs.randn(co).astype(F32)
    res = (np.abs(rs.randn(b, ho, wo, co).astype(F32)) * 8).astype(F16)
    nb = b if n_ref is None else min(b, n_ref)
    z = conv64(x[:nb], wt, k, s)
    ref = np.clip(z * scale.astype(F64) + shift.astype(F64) + res[:nb].astype(F64), 0.0, 20.0)
    return frozen(x=x, wt=wt, scale=scale, shift=shift, res=res, z=z, ref=ref, nb=nb)


def planes16(a, c):
    """channels-last [..., C] -> plane-major [C/16][pixels][16]"""
    return np.ascontiguousarray(a.reshape(-1, c // 16, 16).transpose(1, 0, 2))


def from_planes16(a, shape):
    """plane-major [C/16][pixels][16] -> channels-last `shape`"""
    c = shape[-1]
    return np.ascontiguousarray(a.reshape(c // 16, -1, 16).transpose(1, 0, 2)).reshape(shape)


def pack_bank(be, wt):
    co, ci, k, _ = wt.shape
    w_d, wp = be.put(wt), be.nan(wt.size, F16)
    be.lib.call("ds_pack_conv_weight_f16", be.p(w_d), be.p(wp), co, ci, k, be.stream)
    return wp


def raw_err(got, ref):
    return finite_rel_err(np.asarray(got, F64), ref)


def f16_err(got, ref):
    got = np.asarray(got, F64)
    return float(np.abs(got - ref).max()) if np.isfinite(got).all() else float("inf")


# ---------------------------------------------------------------------------------------------------------------------
# a. ds_conv_fwd_f16, every tile configuration and every form of a launch
# ---------------------------------------------------------------------------------------------------------------------
# (B, Cin, Cout, H, W, KS, stride); 256 output channels: every N tile of kCfgH divides them
FWD_CASES = [
    (3, 32, 256, 20, 8, 3, 1),      # one image per 160-pixel tile, NI = 1 .. 3 by M tile
    (5, 64, 256, 10, 4, 3, 1),      # several whole images per tile, ragged last tile, two chunks
    (2, 32, 256, 27, 32, 3, 1),     # row blocks of one image, ragged last block, NIT up to 12 with LIN
    (1, 32, 256, 3, 5, 3, 1),       # tiny map: every tile row ragged
    (3, 32, 256, 9, 8, 5, 2),       # 5x5 stride 2, multi-image tiles
    (2, 64, 256, 21, 16, 5, 2),     # 5x5 stride 2, odd height, the 32 -> 16 chunk-width switch
    (1, 64, 256, 21, 64, 5, 2),     # wide stride-2 input: not persistent by default, NIT 11 - 14
]
# the default plan is the persistent kernel's, except here: one tile per workgroup (more than 8 staging items per thread on
# an input row that does not divide a pass of the workgroup: plan_persistent)
NOT_PERSISTENT_BY_DEFAULT = {((1, 64, 256, 21, 64, 5, 2), c) for c in (-1, 0, 3, 4)}
# the host emulator runs every form on these two and the default and one-tile forms on EMUL_TWO_FORMS (its whole file: 68 s
# measured); the device runs every form on all seven
EMUL_ALL_FORMS = [(1, 32, 256, 3, 5, 3, 1), (3, 32, 256, 9, 8, 5, 2)]
EMUL_TWO_FORMS = [(3, 32, 256, 20, 8, 3, 1), (5, 64, 256, 10, 4, 3, 1)]

EPILOGUES = (("raw", DS_EPI_OUT_F32, F32), ("fused", FUSED, F16), ("planes", FUSED | DS_EPI_OUT_PLANES16, F16))
TWO_FORMS = (("default", 0), ("one tile", DS_CONV_HINT_NO_PERSIST))


def forms_of(ks):
    forms = list(TWO_FORMS) + [("single buffer", DS_CONV_HINT_SINGLE_BUFFER)]
    if ks == 3:
        return forms + [("64-wide", DS_CONV_HINT_NO_WIDE)]
    return forms + [("chunk16", DS_CONV_HINT_CHUNK16), ("chunk16 one tile", DS_CONV_HINT_CHUNK16 | DS_CONV_HINT_NO_PERSIST),
                    ("planes in", DS_CONV_IN_PLANES16), ("planes in one tile", DS_CONV_IN_PLANES16 | DS_CONV_HINT_NO_PERSIST)]


class FirstOutputs:
    """the first output of each epilogue kind, held to its bar against float64; every later one bit for bit the first"""

    def __init__(self, be, case, I, what):
        self.be, self.case, self.I, self.what = be, case, I, what
        self.first, self.label, self.fused_host = {}, {}, None

    def check(self, kind, y, label, rows=None):
        """rows: y holds the first `rows` images of the case only"""
        be, I, nb = self.be, self.I, self.I["nb"]
        if kind == "planes":                    # the layout reference: un-permuted here, against the channels-last bits
            got = from_planes16(be.get(y), self.fused_host.shape)
            assert got.tobytes() == self.fused_host.tobytes(), \
                f"{self.case} {label}: the un-permuted planes differ from the channels-last output of {self.label['fused']}"
            return
        if kind in self.first:
            first = self.first[kind] if rows is None else be.part(self.first[kind], 0, rows)
            assert be.same(first, y), f"{self.case} {label}: {kind} output differs from {self.label[kind]}"
            return
        assert rows is None or rows == self.case[0]
        got = be.get(y)
        assert np.isfinite(got.astype(F32)).all(), f"{self.case} {label}: {kind} output left unwritten or not finite"
        if kind == "raw":
            err, bar = raw_err(got[:nb], I["z"]), RAW_BAR
        else:
            err, bar = f16_err(got[:nb], I["ref"]), F16_BAR
            self.fused_host = np.array(got)
        note(f"{self.what} {kind}", err)
        print(f"{self.what} {self.case} {label}: {kind} {err:.2e} (bar {bar:.2e}, float64 on {nb} of {self.case[0]} images)")
        assert err <= bar, (self.case, label, kind, err, bar)
        self.first[kind], self.label[kind] = y, label


def launch_fwd(be, shp, x_d, wp, sc, sh, rs_d, epi, dt, hint):
    b, ci, co, h, w, k, s = shp.B, shp.Cin, shp.Cout, shp.H, shp.W, shp.KS, shp.stride
    ho, wo = out_dims(h, w, k, s)
    p = be.p
    y = be.nan((b, ho, wo, co), dt)
    aff = epi & DS_EPI_AFFINE
    be.lib.call("ds_conv_fwd_f16", ctypes.byref(shp), p(x_d), p(wp), p(sc) if aff else None, p(sh) if aff else None,
                p(rs_d) if epi & DS_EPI_RESIDUAL else None, p(y), epi | hint, be.stream)
    return y


def body_conv_fwd(be, case, forms=None, cfgs=CFGS):
    """ds_conv_fwd_f16 under each configuration of `cfgs` in each form of `forms` (default: all of forms_of) with the three
    epilogues; what the plan of every launch was goes to LAUNCHED"""
    lib = be.lib
    b, ci, co, h, w, k, s = case
    I = conv_inputs(case)
    shp = ConvShape(b, h, w, ci, co, k, s)
    wp = pack_bank(be, I["wt"])
    x_d, sc, sh, rs_d = (be.put(I[n]) for n in ("x", "scale", "shift", "res"))
    xp_d = be.put(planes16(I["x"], ci)) if k == 5 else None
    outs = FirstOutputs(be, case, I, "conv fwd f16")
    for cfg in cfgs:
        plans = []
        for name, hint in (forms or forms_of(k)):
            ys = []
            with forced_cfg(lib, cfg):
                rc, out8 = describe(lib, shp, hint)
                assert rc == 0, f"{case} cfg {cfg} {name}: not feasible (code {rc})"
                check_tile(cfg, k, hint, out8)
                row = plan_row(k, out8)
                if hint == 0:
                    assert row[4] == ((case, cfg) not in NOT_PERSISTENT_BY_DEFAULT), (case, cfg, out8)
                if hint & DS_CONV_HINT_NO_PERSIST:
                    assert not row[4], (case, cfg, name, out8)
                if hint & DS_CONV_HINT_SINGLE_BUFFER:
                    assert not row[4] and not row[5], (case, cfg, name, out8)
                if hint & (DS_CONV_HINT_CHUNK16 | DS_CONV_IN_PLANES16):
                    assert row[6], (case, cfg, name, out8)
                x_in = xp_d if hint & DS_CONV_IN_PLANES16 else x_d
                for kind, epi, dt in EPILOGUES:
                    ys.append((kind, launch_fwd(be, shp, x_in, wp, sc, sh, rs_d, epi, dt, hint)))
            LAUNCHED.add(row)
            plans.append(f"{name}: {out8[0]}x{out8[1]}/{out8[6]} RT {out8[2]} NI {out8[3]} tiles {out8[4]} {out8[7]}")
            for kind, y in ys:
                outs.check(kind, y, f"cfg {cfg} {name}")
        print(f"conv fwd f16 {case} cfg {cfg}: " + "; ".join(plans) + " -- all bit for bit")
    if forms is None and tuple(cfgs) == CFGS:
        FWD_RAN.add(case)


def coverage_wants(nit_rows):
    """what body a must have launched: (description, predicate on a LAUNCHED row)"""
    wants = []
    for c, ((mt, nt), thr) in enumerate(zip(CFG_TILES, CFG_THREADS)):
        tile = (mt, nt, thr)
        for ks in (3, 5):
            for pers in (True, False):
                wants.append((f"KS {ks} cfg {c} {'persistent' if pers else 'one tile per workgroup'}",
                              lambda r, ks=ks, tile=tile, pers=pers: r[0] == ks and r[1:4] == tile and r[4] == pers))
            wants.append((f"k{ks}sb cfg {c}", lambda r, ks=ks, tile=tile: r[0] == ks and r[1:4] == tile and not r[4] and not r[5]))
            if nit_rows:
                for pers in (True, False):
                    if (ks, c, pers) in NIT16_ROWS:
                        wants.append((f"KS {ks} cfg {c} {'persistent (LIN)' if pers else 'one tile'}, more than 8 items per thread",
                                      lambda r, ks=ks, tile=tile, pers=pers: r[0] == ks and r[1:4] == tile and r[4] == pers and
                                      r[5] and r[7] > 8))
        wants.append((f"pk5c16 cfg {c}", lambda r, tile=tile: r[0] == 5 and r[1:4] == tile and r[4] and r[6]))
        wants.append((f"k5c16 cfg {c}", lambda r, tile=tile: r[0] == 5 and r[1:4] == tile and not r[4] and r[6]))
    wants.append(("pk3 wide tile 7", lambda r: r[0] == 3 and r[1:4] == WIDE_TILE and r[4]))
    return wants


# double-buffered launches with more than 8 staging items per thread (the NIT = 16 instantiations: LIN in the persistent
# kernel) that FWD_CASES reach, as (KS, configuration, persistent); read off ds_conv_f16_plan_describe_hinted, which does
# not depend on the device
NIT16_ROWS = {(3, 3, False), (3, 3, True), (3, 6, False), (3, 6, True), (5, 0, False), (5, 0, True), (5, 1, False), (5, 2, False),
              (5, 2, True), (5, 3, False), (5, 3, True), (5, 4, False), (5, 4, True), (5, 5, False), (5, 6, False), (5, 6, True)}


def body_fwd_coverage(nit_rows):
    for row in sorted(LAUNCHED):
        print("launched: KS %d %dx%d/%d %s %s %s NIT %d" % (row[:4] + ("persistent" if row[4] else "one-tile  ",
                                                                       "db" if row[5] else "sb", "ck16" if row[6] else "ck32", row[7])))
    for kind in sorted(WORST):
        print(f"largest error, {kind}: {WORST[kind]:.2e}")
    missing = [what for what, pred in coverage_wants(nit_rows) if not any(pred(r) for r in LAUNCHED)]
    assert not missing, missing


# ---------------------------------------------------------------------------------------------------------------------
# b. persistent workgroups that walk several tiles (device only: the batch comes from the CU count)
# ---------------------------------------------------------------------------------------------------------------------
# The tile search weighs the fill of the chip (conv_plan.h), so the segmentation it picks for a forced configuration changes
# with the batch, and with it whether the persistent kernel takes the plan (plan_persistent: double-buffered, a tile that is
# one row block or a run of whole images).  No single batch of the 20x8 or the 21x16 map gives a persistent plan with more
# tiles than resident workgroups under every configuration at 256 CUs (describe, swept over B = 40 .. 1400), so the batch is
# per configuration: base geometry -> {configuration: images per 64 CUs}.  At 256 CUs: 3x3 on 20x8, B = 416 (rows -1, 0, 1,
# 2), 320 (row 6) and 208 (row 5); rows 3 and 4 get no such plan at any batch on that map (two images, or a ragged pair of
# row blocks, per tile), which is what the 27x32 map is for: B = 96 under every row, row blocks with up to 12 staging items
# (LIN).  5x5 on 21x16: B = 260 (rows 0, 3, 4), 448 (rows -1, 1, 2, 5), 224 (row 6).  Every launch asserts from describe that
# the plan is the persistent kernel's and that its tiles exceed the resident workgroups (2 x CUs on two waves, 1 x CUs on
# four); test_emul_f16_kernels.py checks the table against the planner as a 256-CU device sees it.  The shapes are chosen
# through the planner; no bar is.
# To sweep the table again (after a change to ds_plan_fill_occupancy, the tile preferences of plan_f16 or plan_persistent): with
# DS_EMUL_CUS=256 and the emulator library, for every base geometry and configuration call walk_plan(lib, ConvShape(B, ...),
# cfg, name, hint, 256) under forced_cfg for every form of walk_forms and B = 40 .. 1400, keep the B for which none raises,
# pick per configuration a B inside a run of good ones (the fewest distinct values), and write B * 64 / 256 here.
WALK_BASES = {
    (32, 256, 20, 8, 3, 1): {-1: 104, 0: 104, 1: 104, 2: 104, 5: 52, 6: 80},
    (32, 256, 27, 32, 3, 1): {c: 24 for c in CFGS},
    (64, 256, 21, 16, 5, 2): {-1: 112, 0: 65, 1: 112, 2: 112, 3: 65, 4: 65, 5: 112, 6: 56},
}
WALK_EPILOGUES = (EPILOGUES[0], EPILOGUES[1])
N_REF = 8


def walk_batch(base, cfg, cus):
    return -(-WALK_BASES[base][cfg] * cus // 64)


def walk_forms(ks):
    forms = [("default", 0), ("one queue", DS_CONV_HINT_ONE_QUEUE), ("one tile", DS_CONV_HINT_NO_PERSIST)]
    return forms + ([("planes in", DS_CONV_IN_PLANES16)] if ks == 5 else [])


def walk_plan(lib, shp, cfg, name, hint, cus):
    """the plan of one walk launch (under the hook): the persistent kernel's, more tiles than resident workgroups"""
    what = f"{(shp.Cin, shp.Cout, shp.H, shp.W, shp.KS, shp.stride)} B {shp.B} cfg {cfg} {name}"
    rc, out8 = describe(lib, shp, hint)
    assert rc == 0, f"{what}: not feasible (code {rc})"
    check_tile(cfg, shp.KS, hint, out8)
    row = plan_row(shp.KS, out8)
    tiles = out8[4] // (2 if row[1:4] == WIDE_TILE else 1)          # (out8[4] counts the tiles before the widening)
    # wg_per_cu x CUs of plan_persistent RESTATED (one wave per SIMD: 256 / threads workgroups per CU); describe reports the
    # tiles, not the grid, so this is not a value read back from the planner
    resident = (256 // out8[6]) * cus
    if hint & DS_CONV_HINT_NO_PERSIST:
        assert not row[4], (what, out8)
    else:
        assert row[4], f"{what}: not the persistent kernel's plan {out8}"
        assert tiles > resident, f"{what}: {tiles} tiles, {resident} resident workgroups"
    return out8, row, tiles, resident


def body_walk_plans(lib, base, cus):
    """describe only: every configuration's batch gives the plan body_walk wants on a device of `cus` compute units"""
    ci, co, h, w, k, s = base
    for cfg in WALK_BASES[base]:
        for name, hint in walk_forms(k):
            with forced_cfg(lib, cfg):
                walk_plan(lib, ConvShape(walk_batch(base, cfg, cus), h, w, ci, co, k, s), cfg, name, hint, cus)


def body_walk(be, base, cus):
    """default (XCD queues), one queue and one tile per workgroup -- 5x5: also the plane-major input -- under every
    configuration, raw and fp16 epilogue, bit for bit over the whole tensor (configurations with a smaller batch: over their
    images, a prefix of the same operands); float64 on the first N_REF images"""
    lib = be.lib
    ci, co, h, w, k, s = base
    b_max = max(walk_batch(base, c, cus) for c in WALK_BASES[base])
    case = (b_max,) + base
    I = conv_inputs(case, N_REF)
    wp = pack_bank(be, I["wt"])
    x_d, sc, sh, rs_d = (be.put(I[n]) for n in ("x", "scale", "shift", "res"))
    xp_d = {}
    forms = walk_forms(k)
    outs = FirstOutputs(be, case, I, "conv fwd f16 walk")
    for cfg in sorted(WALK_BASES[base], key=lambda c: -walk_batch(base, c, cus)):       # (the largest batch first)
        b = walk_batch(base, cfg, cus)
        shp = ConvShape(b, h, w, ci, co, k, s)
        if k == 5 and b not in xp_d:
            xp_d[b] = be.put(planes16(I["x"][:b], ci))
        plans = []
        for name, hint in forms:
            with forced_cfg(lib, cfg):
                out8, row, tiles, resident = walk_plan(lib, shp, cfg, name, hint, cus)
                x_in = xp_d[b] if hint & DS_CONV_IN_PLANES16 else x_d
                ys = [(kind, launch_fwd(be, shp, x_in, wp, sc, sh, rs_d, epi, dt, hint)) for kind, epi, dt in WALK_EPILOGUES]
            LAUNCHED.add(row)
            plans.append(f"{name}: {out8[0]}x{out8[1]}/{out8[6]} RT {out8[2]} NI {out8[3]} tiles {tiles} on "
                         f"{min(tiles, resident) if row[4] else tiles} workgroups {out8[7]}")
            for kind, y in ys:
                outs.check(kind, y, f"B {b} cfg {cfg} {name}", rows=b)
            del ys
        print(f"conv fwd f16 walk {base} B {b} cfg {cfg}: " + "; ".join(plans) + " -- all bit for bit")
    conv_inputs.cache_clear()           # (the walk operands are tens of MB each: not kept for the rest of the process)


# ---------------------------------------------------------------------------------------------------------------------
# c. split-K
# ---------------------------------------------------------------------------------------------------------------------
# case -> (ways the workspace is sized for = ws_bytes / (4 n_out), splits that run; 0: one pass, the workspace untouched)
SPLITK_CASES = {
    (1, 256, 64, 5, 8, 3, 1): (8, 8),
    (1, 128, 64, 5, 8, 3, 1): (4, 4),
    (1, 160, 64, 5, 8, 3, 1): (4, 3),       # five chunks, two per split: the last quarter of the workspace stays NaN
    (5, 96, 128, 10, 4, 3, 1): (2, 2),      # three chunks, 2 + 1
    (1, 64, 128, 80, 32, 5, 2): (2, 2),
    (2, 64, 128, 21, 16, 5, 2): (2, 0),     # the launch switches to 16-channel chunks and computes more ways than the
}                                           # workspace holds: one pass (kResolveNoChunkSwitch, conv_mfma_f16.hip)
SPLITK_EPILOGUES = (("raw", DS_EPI_OUT_F32, F32), ("fused", FUSED, F16), ("fused f32", FUSED | DS_EPI_OUT_F32, F32))


def body_splitk(be, case):
    lib, p = be.lib, be.p
    b, ci, co, h, w, k, s = case
    ho, wo = out_dims(h, w, k, s)
    ways, runs = SPLITK_CASES[case]
    I = conv_inputs(case)
    shp = ConvShape(b, h, w, ci, co, k, s)
    n_out = b * ho * wo * co
    ws_bytes = lib.raw("ds_conv_f16_splitk_workspace_bytes")(ctypes.byref(shp))
    assert ws_bytes == ways * n_out * 4, (case, ws_bytes, n_out)
    wp = pack_bank(be, I["wt"])
    x_d, sc, sh, rs_d = (be.put(I[n]) for n in ("x", "scale", "shift", "res"))

    def launch(epi, dt, given_bytes, flat=False):
        ws, y = be.nan((ways, n_out), F32), be.nan(n_out if flat else (b, ho, wo, co), dt)
        aff = epi & DS_EPI_AFFINE
        lib.call("ds_conv_fwd_f16_splitk", ctypes.byref(shp), p(x_d), p(wp), p(sc) if aff else None, p(sh) if aff else None,
                 p(rs_d) if epi & DS_EPI_RESIDUAL else None, p(y), epi, p(ws), given_bytes, be.stream)
        ws_h = be.get(ws)
        return be.get(y), np.isfinite(ws_h).all(axis=1), np.isnan(ws_h).all(axis=1)

    def errs(kind, got):
        if not np.isfinite(got.astype(F32)).all():
            return float("inf"), 0.0
        if kind == "raw":
            return raw_err(got, I["z"]), RAW_BAR
        if kind == "fused":
            return f16_err(got, I["ref"]), F16_BAR
        return raw_err(got, I["ref"]), RAW_BAR           # the f32 store of the epilogue: no fp16 rounding

    one_pass_fused = None
    for given, want_written in ((ws_bytes, runs), (ws_bytes - 1, 0)):
        for kind, epi, dt in SPLITK_EPILOGUES:
            got, written, untouched = launch(epi, dt, given)
            # split i writes plane i whole; of the planes past the last split, or of all of them in one pass, EVERY element
            # is still the NaN it started as
            assert written.tolist() == [i < want_written for i in range(ways)], (case, kind, given, written.tolist())
            assert untouched.tolist() == [i >= want_written for i in range(ways)], (case, kind, given, untouched.tolist())
            err, bar = errs(kind, got)
            note(f"split-K {kind}", err)
            print(f"split-K {case} workspace {given} of {ws_bytes} bytes ({ways} ways), {want_written or 'no'} splits ran: "
                  f"{kind} {err:.2e} (bar {bar:.2e})")
            assert err <= bar, (case, kind, given, err, bar)
            if kind == "fused" and not want_written:
                one_pass_fused = got
    # plane-major output is the one-pass kernel's: a workspace does not split it
    got, written, untouched = launch(FUSED | DS_EPI_OUT_PLANES16, F16, ws_bytes, flat=True)
    assert not written.any() and untouched.all(), (case, written.tolist(), untouched.tolist())
    got = from_planes16(got, (b, ho, wo, co))
    err = f16_err(got, I["ref"])
    print(f"split-K {case} with OUT_PLANES16: one pass, {err:.2e} (bar {F16_BAR:.2e})")
    assert err <= F16_BAR and got.tobytes() == one_pass_fused.tobytes(), (case, err)


# ---------------------------------------------------------------------------------------------------------------------
# d. the BasicBlock kernel (device; the emulator has the flag matrix in test_emul_f16.py)
# ---------------------------------------------------------------------------------------------------------------------
BLOCK_FLAG_GEOMS = [(3, 11, 32, 64), (3, 11, 16, 128), (1, 3, 16, 128)]          # (B, H, W, C)
BLOCK_FLAGS = {"f16": 0, "f32": DS_EPI_OUT_F32, "planes": DS_EPI_OUT_PLANES16}
BLOCK_XCD_WIDTHS = [(32, 64), (16, 128)]
BLOCK_ROWS = 8                                                                  # BK_R of conv_block_f16.hip


def block_xcd_geom(cus, w, c):
    """more 8-row tiles than the 2 x CUs resident workgroups, a batch of >= 8 that is no multiple of 8: (67, 59, ..) at 256 CUs"""
    h = 59
    b = 2 * cus // -(-h // BLOCK_ROWS) + 3
    if b % 8 == 0:
        b += 1
    return (b, h, w, c)


def body_block(be, geom, oflag=0, masked=False):
    """ds_conv_block_f16 (masked: ds_conv_block_f16_masked) bit for bit against two ds_conv_fwd_f16 calls"""
    lib, p, st = be.lib, be.p, be.stream
    b, h, w, c = geom
    assert lib.raw("ds_conv_block_f16_supported")(b, h, w, c) == 1
    rs = np.random.RandomState(seed_of(*geom, oflag, masked))
    x_d = be.put((np.abs(rs.randn(b, h, w, c).astype(F32)) * 2).astype(F16))
    packs = [pack_bank(be, (rs.randn(c, c, 3, 3) / np.sqrt(c * 9)).astype(F32)) for _ in range(2)]
    folds = [(be.put(rs.uniform(0.5, 1.5, c).astype(F32)), be.put((rs.randn(c) * 0.5).astype(F32))) for _ in range(2)]
    lens = lens_d = None
    if masked:
        lens = rs.randint(0, h + 1, b).astype(I32)
        lens[:3] = (0, h, h - 6)                    # nothing, everything, an extent inside an 8-row tile
        assert b >= 3 and (h - 6) % BLOCK_ROWS != 0
        lens_d = be.put(lens)
        lib.call("ds_mask_rows", p(x_d), p(lens_d), b, h, w * c * 2, st)        # as the variable-length forward hands it over
    shp = ConvShape(b, h, w, c, c, 3, 1)
    dt = F32 if oflag & DS_EPI_OUT_F32 else F16
    shape = (b * h * w * c,) if oflag & DS_EPI_OUT_PLANES16 else (b, h, w, c)
    mid, ref, got = be.nan((b, h, w, c), F16), be.nan(shape, dt), be.nan(shape, dt)
    lib.call("ds_conv_fwd_f16", ctypes.byref(shp), p(x_d), p(packs[0]), p(folds[0][0]), p(folds[0][1]), None, p(mid),
             DS_EPI_AFFINE | DS_EPI_CLIP, st)
    if masked:
        lib.call("ds_mask_rows", p(mid), p(lens_d), b, h, w * c * 2, st)
    lib.call("ds_conv_fwd_f16", ctypes.byref(shp), p(mid), p(packs[1]), p(folds[1][0]), p(folds[1][1]), p(x_d), p(ref),
             FUSED | oflag, st)
    args = (p(x_d), p(packs[0]), p(packs[1]), p(folds[0][0]), p(folds[0][1]), p(folds[1][0]), p(folds[1][1]), p(got))
    if masked:
        assert oflag == 0
        lib.call("ds_mask_rows", p(ref), p(lens_d), b, h, w * c * 2, st)
        lib.call("ds_conv_block_f16_masked", *args, p(lens_d), b, h, w, c, oflag, st)
    else:
        lib.call("ds_conv_block_f16", *args, b, h, w, c, oflag, st)
    got_h = be.get(got)
    assert np.isfinite(got_h.astype(F32)).all() and float(np.abs(got_h.astype(F32)).max()) > 0, geom
    assert be.same(got, ref), f"block kernel {geom} flags {oflag} masked {masked}: differs from two convolution calls"
    if oflag & DS_EPI_OUT_PLANES16:         # ... and the planes are the channels-last output's (its own layout reference)
        cl = be.nan((b, h, w, c), F16)
        lib.call("ds_conv_block_f16", *args[:-1], p(cl), b, h, w, c, 0, st)
        assert from_planes16(got_h, (b, h, w, c)).tobytes() == be.get(cl).tobytes(), geom
    if masked:
        for i, n in enumerate(lens):
            assert not got_h[i, n:].any(), f"image {i}: rows past its extent {n} are not zero"
        assert got_h[1].any() and got_h[2, :h - 6].any()
    print(f"block kernel {geom} flags {oflag} masked {masked}: {b * -(-h // BLOCK_ROWS)} tiles, bit for bit two convolution calls")


# ---------------------------------------------------------------------------------------------------------------------
# e. refusals
# ---------------------------------------------------------------------------------------------------------------------
NARROW = (2, 32, 64, 9, 8, 3, 1)            # 64 output channels: the N tiles of rows 0, 1, 2, 4 and 5 do not divide them
NARROW_REFUSED = (0, 1, 2, 4, 5)


def body_refusals(be):
    lib, p = be.lib, be.p
    fwd = lib.raw("ds_conv_fwd_f16")
    # shapes no configuration takes: refused by the describe entry point and, only then, by the launch (whose buffers
    # here are small: nothing may be written)
    x_d, w_d = be.put(np.zeros(4096, F16)), be.put(np.zeros(4096, F16))
    for case in BAD:
        b, ci, co, h, w, k, s = case
        shp = ConvShape(b, h, w, ci, co, k, s)
        for cfg in CFGS:
            y = be.nan(4096, F16)
            with forced_cfg(lib, cfg):
                rc_d, _ = describe(lib, shp)
                assert rc_d < 0, (case, cfg, rc_d)
                rc = fwd(ctypes.byref(shp), p(x_d), p(w_d), None, None, None, p(y), 0, be.stream)
            assert rc == rc_d, (case, cfg, rc, rc_d)
            assert np.isnan(be.get(y).astype(F32)).all()
        print(f"conv fwd f16 {case}: refused under every configuration (code {rc_d})")
    # a forced configuration whose N tile does not divide Cout
    b, ci, co, h, w, k, s = NARROW
    I = conv_inputs(NARROW)
    shp = ConvShape(b, h, w, ci, co, k, s)
    x_d, wp = be.put(I["x"]), pack_bank(be, I["wt"])
    for cfg in CFGS:
        y = be.nan((b, h, w, co), F32)
        with forced_cfg(lib, cfg):
            rc_d, out8 = describe(lib, shp)
            rc = fwd(ctypes.byref(shp), p(x_d), p(wp), None, None, None, p(y), DS_EPI_OUT_F32, be.stream)
        print(f"conv fwd f16 {NARROW} cfg {cfg}: describe {rc_d}, launch {rc}")
        if cfg in NARROW_REFUSED:
            assert rc_d == rc == DS_ERR_UNSUPPORTED, (cfg, rc_d, rc)
            assert np.isnan(be.get(y)).all()
        else:
            assert rc_d == rc == 0 and raw_err(be.get(y), I["z"]) <= RAW_BAR, (cfg, rc_d, rc)
    # layouts
    y = be.nan((b, h, w, co), F32)
    assert fwd(ctypes.byref(shp), p(x_d), p(wp), None, None, None, p(y), DS_CONV_IN_PLANES16 | DS_EPI_OUT_F32,
               be.stream) == DS_ERR_UNSUPPORTED                                 # plane-major input: 5x5 only
    assert fwd(ctypes.byref(shp), p(x_d), p(wp), None, None, None, p(y), DS_EPI_OUT_PLANES16 | DS_EPI_OUT_F32,
               be.stream) == DS_ERR_UNSUPPORTED                                 # planes are fp16
    assert np.isnan(be.get(y)).all()
    # the hook is back at -1 also after a body that raised, and values outside [0, 7) mean the planner's choice
    try:
        with forced_cfg(lib, 1):
            raise RuntimeError("a failing test body")
    except RuntimeError:
        pass
    rc, out8 = describe(lib, shp)
    assert rc == 0, rc
    for bad in (7, 8, 99, -7):
        with forced_cfg(lib, bad):
            assert describe(lib, shp) == (rc, out8), bad


def body_hook_is_back(lib):
    """after everything above the planner chooses again: the recorded plans of tests/golden/f16_conv_plans.json (planner's
    choice, no padding) WITHOUT touching the hook -- resolve_rows of f16_plan_cases.py sets it for every row, so it cannot see
    a value left behind"""
    from f16_plan_cases import load_fixture
    rows = [r for r in load_fixture() if r["cfg"] == -1 and r["pad"] == 0 and r["rc"] == 0]
    tiles = set()
    for r in rows:
        b, ci, co, h, w, k, s = r["s"]
        assert describe(lib, ConvShape(b, h, w, ci, co, k, s), r["f"]) == (0, r["o8"]), r
        tiles.add((r["o8"][0], r["o8"][1]))
    assert len(rows) > 300 and len(tiles) >= 5, (len(rows), tiles)         # (no one forced configuration gives them all)
