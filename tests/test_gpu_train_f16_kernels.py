"""The kernels of the opt-in fp16 training step, one at a time, on the device (through the C ABI on device tensors) against
float64 references of the same operation on the same fp16-rounded operands (tests/train_f16_cases.py): BatchNorm
statistics / normalise / backward, their data-parallel split forms, the fp16 filter gradients, the data-gradient banks run
through ds_conv_fwd_f16, the casts and the overflow detector -- at the shapes the emulator cannot reach: partial-row folds
over hundreds of rows (128-row steps, the 768-row cap, empty trailing rows), grid-stride element-wise launches, pixel
splits up to 256-way, the mask re-derived from the pre-activation by whatever fma the device compiler emitted.

Bars.  Where the shape class is the emulator suite's, its bar: statistics rtol 1e-5, gz rel-L2 1e-3 (fp16 storage),
dgamma / dbeta 1e-5, filter gradients 2e-6 (conv1: 1e-5), data gradients 1e-3 (fp16 storage), gy and the casts bit for bit.
For the reductions every test computes, on the CPU, the error of a plain float32 restatement of the same operation
against the float64 reference (float32 partial sums in the kernel's documented partition; torch float32 convolution
backward) and holds the kernel to max(emulator bar, 4 x that error).

Every test prints its rows / S values, the float32 restatement's error, the bar and the kernel's error (`-s`).

Figures of the same test bodies run against the host emulator (small cases only; restatement error -> bar -> kernel):
  statistics C=64 n_pix=32845 rows=129, mean 8 / std 0.5: invstd 6.1e-06 -> 2.4e-05 (every other case stays at 1e-5)
  backward, rows <= 3: dgamma 1.8e-07 -> 1e-05 -> 1.8e-07, dbeta 3.9e-08 -> 1e-05 -> 5.2e-08, gz 2.1e-04 (bar 1e-3)
  filter gradient 64->64 25x16 b=5, S=9: 7.8e-07 -> 3.1e-06 -> 8.8e-08; 128->256 5x5 b=24, S=32: 1.0e-06 -> 4.1e-06 -> 1.1e-07
  conv1 filter gradient 21x16: 1.6e-07 -> 1e-05 -> 8.1e-08; data gradients 2.1e-04 (bar 1e-3)
Split counts the filter-gradient table expects on a 256-CU device, as the host emulator plans them when told 256 CUs
(asserted exactly on such a device): 256, 10, 9, 64, 1, 5, 16, 1, 4, 4, 25, 128, 3, 32, 1, 3, 8.  Partial rows the statistics
table expects (asserted): 1, 301, 768 (8 empty), 768 (23 empty), 129, 768.  The device's own figures for the large
reductions (bench-size statistics, the offset case, the 81920-pixel filter gradient) are printed by every run.
"""
import ctypes

import numpy as np
import pytest
import torch

import train_f16_cases as TC
from train_f16_cases import r16, rel_l2

pytestmark = pytest.mark.gpu

EPS, MOMENTUM = 1e-5, 0.1
NAN = float("nan")


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    from deepspeaker_pytorch_amd.model import get_engine
    return get_engine()


def dev(a, dtype=None):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def full(shape, dtype, fill=NAN):
    return torch.full(shape, fill, dtype=dtype, device="cuda")


def host(t):
    return t.cpu().numpy()


def rand16(gen, shape, scale=1.0, shift=0.0, absolute=False):
    """fp16 host tensor of scale * randn + shift (|.| with absolute)"""
    t = torch.randn(shape, generator=gen) * scale + shift
    return (t.abs() if absolute else t).half()


def partial_rows(eng, n_pix, c):
    return eng.lib.raw("ds_bn_f16_partial_rows")(n_pix, c)


# ---------------------------------------------------------------------------------------------------------------------
# a. statistics + normalise
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,n_pix,rows_cls,dist", TC.STATS_CASES_GPU)
def test_bn_stats_and_apply(eng, c, n_pix, rows_cls, dist):
    from deepspeaker_pytorch_amd._native import DS_EPI_CLIP, DS_EPI_OUT_F32, DS_EPI_RESIDUAL
    G = 3
    rows = partial_rows(eng, n_pix, c)
    TC.check_rows_class(rows, n_pix, c, rows_cls)
    gen = torch.Generator().manual_seed(c * 7 + n_pix % 1000)
    z = rand16(gen, (G * n_pix, c), 0.5, 8.0) if dist == "offset" else rand16(gen, (G * n_pix, c), 3.0, 1.0)
    res = rand16(gen, (G * n_pix, c), absolute=True)
    rs = np.random.RandomState(c + rows)
    gamma, beta = rs.uniform(0.5, 1.5, c).astype(np.float32), (rs.randn(c) * 0.1).astype(np.float32)
    rm, rv = (rs.randn(c) * 0.1).astype(np.float32), rs.uniform(0.5, 1.5, c).astype(np.float32)
    z_d, res_d, g_d, b_d = dev(z), dev(res), dev(gamma), dev(beta)
    st = eng._stream(z_d)
    p = eng._p
    # the fused call
    partial, tables = full((G, rows, c, 2), torch.float32), full((4, G, c), torch.float32)
    rm_d, rv_d = dev(rm), dev(rv)
    eng.lib.call("ds_bn_stats_group_f16", p(z_d), p(partial), n_pix, p(g_d), p(b_d), EPS, MOMENTUM, p(rm_d), p(rv_d),
                 p(tables[0]), p(tables[1]), p(tables[2]), p(tables[3]), c, G, st)
    # the data-parallel pair: partial sums -> float64 fold -> tables
    partial2, tables2, sums = full((G, rows, c, 2), torch.float32), full((4, G, c), torch.float32), full((G, 2 * c + 1), torch.float64)
    rm2_d, rv2_d = dev(rm), dev(rv)
    eng.lib.call("ds_bn_stats_partial_f16", p(z_d), p(partial2), n_pix, c, G, st)
    eng.lib.call("ds_partial_sum_f64_group", p(partial2), rows, p(sums), n_pix, c, G, st)
    eng.lib.call("ds_bn_stats_from_sums_group_f32", p(sums), p(g_d), p(b_d), EPS, MOMENTUM, p(rm2_d), p(rv2_d), p(tables2[0]),
                 p(tables2[1]), p(tables2[2]), p(tables2[3]), c, G, st)
    # three G = 1 calls on the member slices, the running statistics chained in call order
    tables1 = full((4, G, c), torch.float32)
    rm1_d, rv1_d = dev(rm), dev(rv)
    for m in range(G):
        partial1 = full((rows, c, 2), torch.float32)
        eng.lib.call("ds_bn_stats_group_f16", p(z_d[m * n_pix:(m + 1) * n_pix]), p(partial1), n_pix, p(g_d), p(b_d), EPS, MOMENTUM,
                     p(rm1_d), p(rv1_d), p(tables1[0][m]), p(tables1[1][m]), p(tables1[2][m]), p(tables1[3][m]), c, 1, st)
    # normalise: all four flag combinations
    combos = ((DS_EPI_CLIP, torch.float16), (DS_EPI_CLIP | DS_EPI_RESIDUAL, torch.float16),
              (DS_EPI_CLIP | DS_EPI_RESIDUAL | DS_EPI_OUT_F32, torch.float32), (0, torch.float16))
    ys = []
    for flags, dt in combos:
        y = full((G * n_pix, c), dt)
        eng.lib.call("ds_bn_apply_group_f16", p(z_d), p(tables[2]), p(tables[3]), p(res_d), p(y), n_pix, c, G, flags, st)
        ys.append(y)
    torch.cuda.synchronize()

    zh = z.numpy()
    mean, var = TC.bn_member_stats(zh, G)
    invstd, scale, shift = TC.bn_tables_ref(mean, var, gamma, beta, EPS)
    erm, erv = TC.bn_running_ref(mean, var, n_pix, rm, rv, MOMENTUM)
    # the float32 restatement's own error -> the bars
    m_r, v_r, i_r = TC.bn_stats_f32_restatement(zh, G, EPS)
    rm_r, rv_r = TC.bn_running_ref(m_r, v_r, n_pix, rm, rv, MOMENTUM)
    restated = {"mean": TC.tol_err(m_r, mean, 1e-6), "invstd": TC.tol_err(i_r, invstd),
                "running_mean": TC.tol_err(rm_r, erm, 1e-6), "running_var": TC.tol_err(rv_r, erv, 1e-6)}
    bars = {k: TC.bar_from_restatement(1e-5, v) for k, v in restated.items()}
    for name, tb, r_m, r_v in (("fused", host(tables), host(rm_d), host(rv_d)), ("split", host(tables2), host(rm2_d), host(rv2_d))):
        got = {"mean": TC.tol_err(tb[0], mean, 1e-6), "invstd": TC.tol_err(tb[1], invstd),
               "running_mean": TC.tol_err(r_m, erm, 1e-6), "running_var": TC.tol_err(r_v, erv, 1e-6)}
        # scale = gamma * invstd carries invstd's error; shift = beta - mean * scale the sum of both, on the larger term
        got_scale = TC.tol_err(tb[2], scale)
        got_shift = float((np.abs(tb[3] - shift) / (np.abs(beta)[None] + np.abs(mean * scale) + 1e-6)).max())
        print(f"stats C={c} n_pix={n_pix} rows={rows} ({rows_cls}, {dist}) {name}: " +
              ", ".join(f"{k} f32-restated {restated[k]:.2e} bar {bars[k]:.2e} kernel {got[k]:.2e}" for k in got) +
              f", scale {got_scale:.2e}, shift {got_shift:.2e}")
        for k in got:
            assert got[k] <= bars[k], (name, k, got[k], bars[k])
        assert got_scale <= bars["invstd"] + 1e-7 and got_shift <= bars["invstd"] + bars["mean"] + 1e-7, (name, got_scale, got_shift)
    # one formula, one fold: the fused call, the split pair and the member-by-member calls agree bit for bit
    for name, other in (("split pair", (tables2, rm2_d, rv2_d)), ("three G = 1 calls", (tables1, rm1_d, rv1_d))):
        for what, a, b in zip(("tables", "running mean", "running var"), (tables, rm_d, rv_d), other):
            assert not torch.isnan(b).any() and torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, what)
    tb = host(tables)
    for (flags, dt), y in zip(combos, ys):
        worst, top = TC.bn_apply_errors(host(y), zh, tb[2], tb[3], res.numpy() if flags & DS_EPI_RESIDUAL else None, G,
                                        bool(flags & DS_EPI_CLIP))
        print(f"apply C={c} n_pix={n_pix} flags={flags}: max abs err {worst:.3e} (largest value {top:.3g})")
        assert worst <= TC.bn_apply_bar(top, dt == torch.float32), (flags, worst)


# ---------------------------------------------------------------------------------------------------------------------
# b. BatchNorm + clipped-ReLU backward
# ---------------------------------------------------------------------------------------------------------------------
def _bwd_cases():
    small = [(3, 2, 25, 15, 64), (2, 1, 5, 7, 128)]                 # rows 3 (G = 3) and 1; odd maps for the parity layout
    cases, i = [], 0
    for mode in ("act16", "act32", "none", "z"):                    # every valid instantiation of the reduction
        for parity in (False, True):
            for g2 in (False, True):
                cases.append(small[i % 2] + (mode, parity, g2, None))
                i += 1
    cases += [(1, 12, 25, 15, 512, "z", True, True, "mid"),         # 141 rows
              (3, 12, 25, 15, 512, "act16", False, False, "mid"),   # G = 3, 141 rows
              (1, 66, 25, 15, 512, "act16", True, True, "cap+0"),   # 768 rows, 18 of them empty
              (1, 66, 25, 15, 512, "z", False, False, "cap+0"),
              (1, 104, 80, 32, 64, "none", True, False, "bench")]   # 266240 pixels of 64 channels: grid-stride second half
    return cases


@pytest.mark.parametrize("G,bm,h,w,c,mode,parity,with_g2,rows_cls", _bwd_cases())
def test_bn_bwd_group(eng, G, bm, h, w, c, mode, parity, with_g2, rows_cls):
    from deepspeaker_pytorch_amd._native import DS_EPI_CLIP
    B, n_pix, S = G * bm, bm * h * w, 256.0
    rows = partial_rows(eng, n_pix, c)
    if rows_cls:
        TC.check_rows_class(rows, n_pix, c, rows_cls)
    gen = torch.Generator().manual_seed(G * 1000 + c + h + 17 * len(mode) + 2 * parity + with_g2)
    z = rand16(gen, (B * h * w, c), 4.0, 1.0)
    g1 = rand16(gen, (B * h * w, c), 1e-3 * S)
    g2 = rand16(gen, (B * h * w, c), 1e-3 * S) if with_g2 else None
    rs = np.random.RandomState(c + h)
    gamma = rs.uniform(0.5, 1.5, c).astype(np.float32)
    mean, var = TC.bn_member_stats(z.numpy(), G)
    mean_t, invstd_t = mean.astype(np.float32), (1 / np.sqrt(var + EPS)).astype(np.float32)
    sc_t, sh_t = rs.uniform(2.0, 6.0, (G, c)).astype(np.float32), (rs.randn(G, c) * 3 + 6).astype(np.float32)
    p = eng._p
    z_d, g2_d, mt, it, gm = dev(z), (dev(g2) if with_g2 else None), dev(mean_t), dev(invstd_t), dev(gamma)
    st = eng._stream(z_d)
    g1_host = g1.numpy().reshape(B, h, w, c)
    g1_d = dev(TC.parity_scatter(g1_host, h, w, fill=np.nan)) if parity else dev(g1)     # unread cells hold NaN
    act_d = msc = msh = None
    if mode == "act16":
        act = rand16(gen, (B * h * w, c), 8.0, 8.0).clamp(0, 20)
        act_d = dev(act)
    elif mode == "act32":
        act = rand16(gen, (B * h * w, c), 8.0, 8.0).clamp(0, 20)
        act_d = dev(act, torch.float32)
    elif mode == "z":                       # the activation the forward stored from z and these tables
        msc, msh = dev(sc_t), dev(sh_t)
        act_d = full((B * h * w, c), torch.float16)
        eng.lib.call("ds_bn_apply_group_f16", p(z_d), p(msc), p(msh), None, p(act_d), n_pix, c, G, DS_EPI_CLIP, st)
    outs = []
    for split in (False, True):
        gy, gz = full((B * h * w, c), torch.float16), full((B * h * w, c), torch.float16)
        partial, coef = full((G, rows, c, 2), torch.float32), full((G, 3 * c), torch.float32)
        gg, gb = full((c,), torch.float32), full((c,), torch.float32)
        a_p = p(act_d) if mode in ("act16", "act32") else None
        if not split:
            eng.lib.call("ds_bn_bwd_group_f16", p(g1_d), int(parity), p(g2_d), a_p, int(mode == "act32"), p(msc), p(msh), p(z_d),
                         p(mt), p(it), p(gm), p(gy), p(partial), p(coef), p(gg), p(gb), p(gz), n_pix, h, w, c, G, 1.0 / S, st)
        else:                               # the data-parallel pair around the float64 fold
            sums = full((G, 2 * c + 1), torch.float64)
            eng.lib.call("ds_bn_bwd_group_reduce_f16", p(g1_d), int(parity), p(g2_d), a_p, int(mode == "act32"), p(msc), p(msh),
                         p(z_d), p(mt), p(it), p(gy), p(partial), n_pix, h, w, c, G, st)
            eng.lib.call("ds_partial_sum_f64_group", p(partial), rows, p(sums), n_pix, c, G, st)
            eng.lib.call("ds_bn_bwd_group_apply_f16", p(sums), p(gy), 0, p(msc), p(msh), p(z_d), p(mt), p(it), p(gm), p(coef),
                         p(gg), p(gb), p(gz), n_pix, c, G, 1.0 / S, st)
        outs.append((gy, gz, gg, gb))
    torch.cuda.synchronize()

    act_h = None if mode == "none" else host(act_d)
    if mode == "z":                         # the reference's mask comes from the host's own fma, not from the device's
        act_host = TC.act_from_z(z.numpy(), sc_t, sh_t, G)
        assert np.array_equal(act_h.view(np.uint16), act_host.view(np.uint16))     # what ds_bn_apply_group_f16 stored
        act_h = act_host
        frac = float(((act_h > 0) & (act_h < 20)).mean())
        assert 0.2 < frac < 0.9, frac
    gy_ref, gz_ref, gg_ref, gb_ref = TC.bn_bwd_ref(z.numpy(), g1.numpy(), g2.numpy() if with_g2 else None, act_h, mean_t, invstd_t,
                                                   gamma, G)
    gg_r, gb_r = TC.bn_bwd_sums_f32_restatement(z.numpy(), gy_ref, mean_t, invstd_t, G)
    restated = (rel_l2(gg_r, gg_ref), rel_l2(gb_r, gb_ref))
    bars = tuple(TC.bar_from_restatement(1e-5, v) for v in restated)
    assert torch.equal(outs[0][0], outs[1][0])                                  # gy of the split form: bit for bit
    for name, (gy, gz, gg, gb) in zip(("fused", "split"), outs):
        assert np.array_equal(host(gy).astype(np.float32), gy_ref), name        # bit for bit (NaN anywhere fails)
        e_gz, e_gg, e_gb = rel_l2(host(gz), gz_ref), rel_l2(host(gg), gg_ref / S), rel_l2(host(gb), gb_ref / S)
        print(f"bn_bwd G={G} n_pix={n_pix} C={c} rows={rows} {mode} parity={parity} g2={with_g2} {name}: gz {e_gz:.2e} (bar 1e-3), "
              f"dgamma f32-restated {restated[0]:.2e} bar {bars[0]:.2e} kernel {e_gg:.2e}, "
              f"dbeta f32-restated {restated[1]:.2e} bar {bars[1]:.2e} kernel {e_gb:.2e}")
        assert np.isfinite(host(gz).astype(np.float32)).all() and e_gz < 1e-3, (name, e_gz)
        assert e_gg <= bars[0] and e_gb <= bars[1], (name, e_gg, e_gb, bars)


@pytest.mark.parametrize("G,bm,h,w,c,with_g2,store_gy", [(3, 2, 6, 4, 64, True, True), (2, 2, 5, 3, 128, False, False),
                                                         (1, 1, 4, 4, 512, False, True), (3, 12, 25, 15, 512, False, False),
                                                         (1, 104, 80, 32, 64, False, False)])
def test_bn_bwd_mask_from_preactivation(eng, G, bm, h, w, c, with_g2, store_gy):
    """The clip mask re-derived from z and the forward's scale / shift tables must be the mask of the activation
    ds_bn_apply_group_f16 stored -- both kernels' ds_bn_affine compiled to the same fma, the same fp16 rounding -- so every
    result equals the act-masked call's bit for bit, also when the masked gradient is never stored (gy NULL: the second
    launch recomputes it; the last case does so in its grid-stride loop).  The tables put a good share of the values on
    both clip boundaries and many exactly on fp16 rounding ties (fp16 z times a scale with few mantissa bits)."""
    from deepspeaker_pytorch_amd._native import DS_EPI_CLIP
    B, n_pix, S = G * bm, bm * h * w, 256.0
    rows = partial_rows(eng, n_pix, c)
    gen = torch.Generator().manual_seed(11 * G + c + h)
    z = rand16(gen, (B * h * w, c), 4.0, 1.0)
    g1 = rand16(gen, (B * h * w, c), 1e-3 * S)
    g2 = rand16(gen, (B * h * w, c), 1e-3 * S) if with_g2 else None
    rs = np.random.RandomState(11 * G + c)
    gamma = rs.uniform(0.5, 1.5, c).astype(np.float32)
    mean, var = TC.bn_member_stats(z.numpy(), G)
    # half the channels: an integer scale and a shift that is a multiple of 1/8 -- z * scale + shift is then exact and lands
    # on fp16 rounding ties for a large share of the values; the other half arbitrary f32 tables (the fma's single rounding
    # decides)
    sc_t, sh_t = rs.uniform(2.0, 6.0, (G, c)).astype(np.float32), (rs.randn(G, c) * 3 + 6).astype(np.float32)
    sc_t[:, ::2], sh_t[:, ::2] = np.round(sc_t[:, ::2]), np.round(sh_t[:, ::2] * 8) / 8
    p = eng._p
    z_d, g1_d, g2_d = dev(z), dev(g1), (dev(g2) if with_g2 else None)
    mt, it, gm = dev(mean.astype(np.float32)), dev((1 / np.sqrt(var + EPS)).astype(np.float32)), dev(gamma)
    msc, msh = dev(sc_t), dev(sh_t)
    st = eng._stream(z_d)
    act = full((B * h * w, c), torch.float16)                       # what the forward stored
    eng.lib.call("ds_bn_apply_group_f16", p(z_d), p(msc), p(msh), None, p(act), n_pix, c, G, DS_EPI_CLIP, st)
    outs = []
    for maskz in (False, True):
        gy = full((B * h * w, c), torch.float16) if (store_gy or not maskz) else None
        gz = full((B * h * w, c), torch.float16)
        partial, coef = full((G, rows, c, 2), torch.float32), full((G, 3 * c), torch.float32)
        gg, gb = full((c,), torch.float32), full((c,), torch.float32)
        eng.lib.call("ds_bn_bwd_group_f16", p(g1_d), 0, p(g2_d), None if maskz else p(act), 0, p(msc) if maskz else None,
                     p(msh) if maskz else None, p(z_d), p(mt), p(it), p(gm), p(gy), p(partial), p(coef), p(gg), p(gb), p(gz),
                     n_pix, h, w, c, G, 1.0 / S, st)
        outs.append((gy, gz, gg, gb))
    # the data-parallel form with the z-derived mask (and, gy not stored, the regenerating second half)
    gy3 = full((B * h * w, c), torch.float16) if store_gy else None
    gz3, partial, coef = full((B * h * w, c), torch.float16), full((G, rows, c, 2), torch.float32), full((G, 3 * c), torch.float32)
    gg3, gb3, sums = full((c,), torch.float32), full((c,), torch.float32), full((G, 2 * c + 1), torch.float64)
    rcs = []
    if not with_g2:
        eng.lib.call("ds_bn_bwd_group_reduce_f16", p(g1_d), 0, None, None, 0, p(msc), p(msh), p(z_d), p(mt), p(it), p(gy3),
                     p(partial), n_pix, h, w, c, G, st)
        eng.lib.call("ds_partial_sum_f64_group", p(partial), rows, p(sums), n_pix, c, G, st)
        eng.lib.call("ds_bn_bwd_group_apply_f16", p(sums), p(gy3 if store_gy else g1_d), int(not store_gy), p(msc), p(msh), p(z_d),
                     p(mt), p(it), p(gm), p(coef), p(gg3), p(gb3), p(gz3), n_pix, c, G, 1.0 / S, st)
    # combinations the ABI refuses: no stored gradient with g2 / a parity layout / an act mask; act and tables together
    raw = eng.lib.raw("ds_bn_bwd_group_f16")
    scratch = (p(full((G, rows, c, 2), torch.float32)), p(coef), p(gg3), p(gb3), p(full((B * h * w, c), torch.float16)))
    tail = (n_pix, h, w, c, G, 1.0 / S, st)
    rcs.append(raw(p(g1_d), 0, p(g1_d), None, 0, p(msc), p(msh), p(z_d), p(mt), p(it), p(gm), None, *scratch, *tail))
    rcs.append(raw(p(g1_d), 1, None, None, 0, p(msc), p(msh), p(z_d), p(mt), p(it), p(gm), None, *scratch, *tail))
    rcs.append(raw(p(g1_d), 0, None, p(act), 0, None, None, p(z_d), p(mt), p(it), p(gm), None, *scratch, *tail))
    rcs.append(raw(p(g1_d), 0, None, p(act), 0, p(msc), p(msh), p(z_d), p(mt), p(it), p(gm), p(act), *scratch, *tail))
    rcs.append(raw(p(g1_d), 0, None, None, 0, p(msc), None, p(z_d), p(mt), p(it), p(gm), p(act), *scratch, *tail))
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in rcs), rcs
    a = host(act).astype(np.float32)
    frac = float(((a > 0) & (a < 20)).mean())
    zz = z.numpy().astype(np.float64).reshape(G, n_pix, c)
    exact = zz * sc_t.astype(np.float64)[:, None] + sh_t.astype(np.float64)[:, None]
    inside = (exact > 0) & (exact < 20)
    near = exact.astype(np.float16)                                 # a tie: the fp16 neighbour on the other side is as far away
    other = np.nextafter(near, np.where(exact > near.astype(np.float64), np.inf, -np.inf).astype(np.float16)).astype(np.float64)
    dist = np.abs(exact - near.astype(np.float64))
    ties = float(((dist > 0) & (np.abs(exact - other) == dist))[inside].mean())
    print(f"mask-from-z C={c} n_pix={n_pix} rows={rows}: {frac:.2f} strictly inside the clip, {ties:.3f} of those on an fp16 tie")
    assert 0.2 < frac < 0.9, frac
    assert ties > 0.01, ties
    (gy0, gz0, gg0, gb0), (gy1, gz1, gg1, gb1) = outs
    assert bool(torch.isfinite(gz0.float()).all()) and bool(torch.isfinite(gg0).all()) and bool(torch.isfinite(gb0).all())
    if gy1 is not None:
        assert torch.equal(gy0, gy1)
    assert torch.equal(gz0, gz1) and torch.equal(gg0, gg1) and torch.equal(gb0, gb1)
    if not with_g2:
        if gy3 is not None:
            assert torch.equal(gy0, gy3)
        # the float64 fold of the same partial rows: gz may differ in the last fp16 bit of a few values, no more
        assert rel_l2(host(gz3), host(gz0).astype(np.float64)) < 1e-3
        assert rel_l2(host(gg3), host(gg0)) < 1e-5 and rel_l2(host(gb3), host(gb0)) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# c. filter gradients
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,ci,co,h,w,ks,st,loss_scale,split_cls,s256", TC.WGRAD_CASES_GPU)
def test_conv_wgrad_f16(eng, b, ci, co, h, w, ks, st, loss_scale, split_cls, s256):
    import deepspeaker_oracle as O
    from deepspeaker_pytorch_amd._native import ConvShape
    shp = ConvShape(b, h, w, ci, co, ks, st)
    n_ws = eng.lib.raw("ds_conv_wgrad_f16_workspace_floats")(ctypes.byref(shp))
    assert n_ws > 0 and n_ws % (ks * ks * co * ci) == 0
    n_split = n_ws // (ks * ks * co * ci)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    TC.check_split_class(n_split, cus, ci, co, split_cls, s256)
    ho, wo = O.conv_out_size(h, ks, st, ks // 2), O.conv_out_size(w, ks, st, ks // 2)
    gen = torch.Generator().manual_seed(b + ci + co + h + ks)
    x = rand16(gen, (b, h, w, ci), absolute=True)
    gy = rand16(gen, (b, ho, wo, co), 1e-3 * loss_scale)
    x_d, g_d = dev(x), dev(gy)
    p = eng._p
    gws = []
    for _ in range(2):
        ws, gw = full((n_ws,), torch.float32), full((co, ci, ks, ks), torch.float32)
        eng.lib.call("ds_conv_wgrad_f16", ctypes.byref(shp), p(x_d), p(g_d), p(ws), p(gw), 1.0 / loss_scale, eng._stream(x_d))
        gws.append(gw)
    torch.cuda.synchronize()
    xn, gn = x.permute(0, 3, 1, 2).numpy(), gy.permute(0, 3, 1, 2).numpy()
    ref = TC.wgrad_ref(xn, gn, ks, st) / loss_scale
    restated = rel_l2(TC.wgrad_ref(xn, gn, ks, st, dtype=torch.float32) / np.float32(loss_scale), ref)
    bar = TC.bar_from_restatement(2e-6, restated)
    got = host(gws[0])
    err = rel_l2(got, ref) if np.isfinite(got).all() else float("inf")
    print(f"wgrad b={b} {ci}->{co} {h}x{w} k{ks}s{st} loss scale {loss_scale:g}: S={n_split} ({split_cls}, {cus} CUs), "
          f"{b * ho * wo} pixels, f32-restated {restated:.2e} bar {bar:.2e} kernel {err:.2e}")
    assert torch.equal(gws[0], gws[1])                      # fixed-order fold
    assert err <= bar, (err, bar)


@pytest.mark.parametrize("b,h,w", [(4, 160, 64), (3, 21, 16), (5, 37, 64)])
def test_conv_wgrad_c1_f16(eng, b, h, w):
    from deepspeaker_pytorch_amd._native import ConvShape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    loss_scale = 1024.0
    gen = torch.Generator().manual_seed(b + h)
    x = torch.randn((b, h, w), generator=gen)
    gy = rand16(gen, (b, ho, wo, 64), 1e-3 * loss_scale)
    shp = ConvShape(b, h, w, 1, 64, 5, 2)
    n_ws = eng.lib.raw("ds_conv_wgrad_workspace_floats")(ctypes.byref(shp))
    assert n_ws > 0
    x_d, g_d = dev(x), dev(gy)
    p = eng._p
    gws = []
    for _ in range(2):
        ws, gw = full((n_ws,), torch.float32), full((64, 1, 5, 5), torch.float32)
        eng.lib.call("ds_conv_wgrad_c1_f16", ctypes.byref(shp), p(x_d), p(g_d), p(ws), p(gw), 1.0 / loss_scale, eng._stream(x_d))
        gws.append(gw)
    torch.cuda.synchronize()
    xn, gn = x.numpy()[:, None], gy.permute(0, 3, 1, 2).numpy()
    ref = TC.wgrad_ref(xn, gn, 5, 2) / loss_scale
    restated = rel_l2(TC.wgrad_ref(xn, gn, 5, 2, dtype=torch.float32) / np.float32(loss_scale), ref)
    bar = TC.bar_from_restatement(1e-5, restated)
    got = host(gws[0])
    err = rel_l2(got, ref) if np.isfinite(got).all() else float("inf")
    print(f"wgrad conv1 b={b} {h}x{w}: f32-restated {restated:.2e} bar {bar:.2e} kernel {err:.2e}")
    assert torch.equal(gws[0], gws[1])
    assert err <= bar, (err, bar)


# ---------------------------------------------------------------------------------------------------------------------
# d. data-gradient banks through the fp16 convolution
# ---------------------------------------------------------------------------------------------------------------------
def _conv16(eng, g_d, bank, shp, out_shape):
    y = full(out_shape, torch.float16)
    eng.lib.call("ds_conv_fwd_f16", ctypes.byref(shp), eng._p(g_d), eng._p(bank), None, None, None, eng._p(y), 0, eng._stream(g_d))
    return y


@pytest.mark.parametrize("b,ci,co,h,w", TC.DGRAD3_CASES_GPU)
def test_dgrad_3x3_through_the_fp16_convolution(eng, b, ci, co, h, w):
    from deepspeaker_pytorch_amd._native import ConvShape
    gen = torch.Generator().manual_seed(ci + h + w)
    wt = (torch.randn((co, ci, 3, 3), generator=gen) / (ci * 9) ** 0.5).half().float()
    gy = rand16(gen, (b, h, w, co))
    w_d, g_d = dev(wt), dev(gy)
    bank = full((wt.numel(),), torch.float16)
    eng.lib.call("ds_pack_conv_weight_dgrad_f16", eng._p(w_d), eng._p(bank), co, ci, 3, 1, eng._stream(w_d))
    y = _conv16(eng, g_d, bank, ConvShape(b, h, w, co, ci, 3, 1), (b, h, w, ci))
    torch.cuda.synchronize()
    ref = TC.dgrad_ref(wt.numpy(), gy.permute(0, 3, 1, 2).numpy(), 1, (h, w))
    got = host(y).astype(np.float32).transpose(0, 3, 1, 2)
    err = rel_l2(got, ref) if np.isfinite(got).all() else float("inf")
    print(f"dgrad 3x3 b={b} {ci}->{co} {h}x{w}: {err:.2e} (bar 1e-3)")
    assert err < 1e-3


@pytest.mark.parametrize("b,ci,co,h,w", TC.DGRAD5_CASES_GPU)
def test_dgrad_5x5_stride2_parity_classes(eng, b, ci, co, h, w):
    """dX of a 5x5 stride-2 pad-2 layer with input [h, w]: the 36 * Cout * Cin bank through ds_conv_fwd_f16 gives
    [B][ho][wo][2][2][ci]; the only cells not compared are the classes past an odd edge (garbage by contract)"""
    from deepspeaker_pytorch_amd._native import ConvShape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    gen = torch.Generator().manual_seed(ci + co + h)
    wt = (torch.randn((co, ci, 5, 5), generator=gen) / (ci * 25) ** 0.5).half().float()
    gy = rand16(gen, (b, ho, wo, co))
    w_d, g_d = dev(wt), dev(gy)
    bank = full((36 * co * ci,), torch.float16)
    eng.lib.call("ds_pack_conv_weight_dgrad_f16", eng._p(w_d), eng._p(bank), co, ci, 5, 2, eng._stream(w_d))
    y = _conv16(eng, g_d, bank, ConvShape(b, ho, wo, co, 4 * ci, 3, 1), (b, ho, wo, 4 * ci))
    torch.cuda.synchronize()
    ref = TC.dgrad_ref(wt.numpy(), gy.permute(0, 3, 1, 2).numpy(), 2, (h, w))
    got = TC.parity_gather(host(y).astype(np.float32).reshape(b, ho, wo, 2, 2, ci), h, w).transpose(0, 3, 1, 2)
    err = rel_l2(got, ref) if np.isfinite(got).all() else float("inf")
    print(f"dgrad 5x5 s2 b={b} {ci}->{co} input {h}x{w}: {err:.2e} (bar 1e-3)")
    assert err < 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# e. casts and the overflow detector
# ---------------------------------------------------------------------------------------------------------------------
def _finite_f16_bits():
    bits = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    return bits[(bits & 0x7C00) != 0x7C00]


def _special_f32():
    """f32 values around everything fp16 rounding can get wrong: every midpoint between neighbouring fp16 values (ties to
    even, subnormals included, the last one rounds to inf), values just off those midpoints, overflow, signed zeros"""
    pos = _finite_f16_bits()
    pos = np.sort(pos[pos < 0x7C00].view(np.float16).astype(np.float64))
    mid = np.concatenate([(pos[:-1] + pos[1:]) / 2, [65520.0]])                 # exact in f32
    mid32 = mid.astype(np.float32)
    v = np.concatenate([mid32, np.nextafter(mid32, np.float32(np.inf)), np.nextafter(mid32, np.float32(0)),
                        np.array([0.0, 65504.0, 65519.996, 65536.0, 1e5, 3e38, 2.0 ** -25, 2.0 ** -26, 1e-30], np.float32)])
    v = np.concatenate([v, -v]).astype(np.float32)
    assert np.signbit(v).sum() == v.size // 2                                   # -0.0 is among them
    return v


def test_scale_cast_f32_to_f16(eng):
    scale = 1024.0
    n = TC.TF_GRID_CAP * 256 * 8 + 8 * 40000 + 8                                # past the grid cap: grid-stride loop
    x = (np.random.RandomState(1).randn(n) * 1e-4).astype(np.float32)
    special = _special_f32() / np.float32(scale)                                # (a power of two: the product is the value)
    assert special.size < 8 * 40000
    x[:special.size] = special
    x[-special.size:] = special[::-1]                                           # and in the strided tail
    mid = TC.TF_GRID_CAP * 256 * 4
    x[mid:mid + special.size] = special
    with np.errstate(over="ignore"):
        want = (x * np.float32(scale)).astype(np.float16)
    assert np.isinf(want).sum() >= 12 and (want == np.float16(65504)).sum() >= 6
    x_d = dev(x)
    y = full((n + 8,), torch.float16, 7.0)
    eng.lib.call("ds_scale_cast_f32_to_f16", eng._p(x_d), eng._p(y), n, scale, eng._stream(x_d))
    rc = eng.lib.raw("ds_scale_cast_f32_to_f16")(eng._p(x_d), eng._p(y), 12, scale, eng._stream(x_d))
    torch.cuda.synchronize()
    assert rc != 0                                                              # n not a multiple of 8
    got = host(y)
    assert np.array_equal(got[:n].view(np.uint16), want.view(np.uint16))        # bits: signed zeros, inf (not 65504)
    assert (got[n:] == 7.0).all()


def test_cast_f32_f16_round_trip_and_rounding(eng):
    p = eng._p
    bits = _finite_f16_bits()
    assert bits.size == 63488
    h_d = dev(bits.view(np.float16))
    st = eng._stream(h_d)
    f_d, back = full((bits.size + 4,), torch.float32, 7.0), full((bits.size + 4,), torch.float16, 7.0)
    eng.lib.call("ds_cast_f16_to_f32", p(h_d), p(f_d), bits.size, st)
    eng.lib.call("ds_cast_f32_to_f16", p(f_d), p(back), bits.size, st)
    # rounding: the special values, in a tensor past the 8192-workgroup cap with a tail, and n = 1 (n > 0 is the only rule)
    special = _special_f32()
    special = np.concatenate([special, np.array([np.inf, -np.inf, np.nan], np.float32)])
    n = 8192 * 256 + 77
    x = (np.random.RandomState(2).randn(n) * 100).astype(np.float32)
    x[:special.size] = special
    x[-special.size:] = special[::-1]
    x_d = dev(x)
    y, y32 = full((n + 4,), torch.float16, 7.0), full((n + 4,), torch.float32, 7.0)
    eng.lib.call("ds_cast_f32_to_f16", p(x_d), p(y), n, st)
    eng.lib.call("ds_cast_f16_to_f32", p(y), p(y32), n, st)
    one16, one32 = full((4,), torch.float16, 7.0), full((4,), torch.float32, 7.0)
    eng.lib.call("ds_cast_f32_to_f16", p(x_d[5:]), p(one16), 1, st)
    eng.lib.call("ds_cast_f16_to_f32", p(h_d[1234:]), p(one32), 1, st)
    rcs = [eng.lib.raw("ds_cast_f32_to_f16")(p(x_d), p(y), 0, st), eng.lib.raw("ds_cast_f16_to_f32")(p(y), p(y32), 0, st)]
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in rcs)
    f = host(f_d)
    assert np.array_equal(f[:bits.size].view(np.uint32), bits.view(np.float16).astype(np.float32).view(np.uint32))
    assert np.array_equal(host(back)[:bits.size].view(np.uint16), bits)         # exact round trip, subnormals and -0 included
    assert (f[bits.size:] == 7.0).all() and (host(back)[bits.size:] == 7.0).all()
    with np.errstate(over="ignore"):
        want = x.astype(np.float16)
    got = host(y)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got[:n]), nan) and nan.sum() == 2
    assert np.array_equal(got[:n].view(np.uint16)[~nan], want.view(np.uint16)[~nan])
    assert np.array_equal(host(y32)[:n].view(np.uint32)[~nan], want.astype(np.float32).view(np.uint32)[~nan])
    assert (got[n:] == 7.0).all() and (host(y32)[n:] == 7.0).all()
    assert np.array_equal(host(one16).view(np.uint16), np.array([x[5]], np.float16).view(np.uint16).tolist() + [0x4700] * 3)
    assert host(one32).tolist() == [float(bits.view(np.float16)[1234])] + [7.0] * 3


def test_nonfinite_flag(eng):
    p = eng._p
    # the launch takes ceil(n / 4096) workgroups, at most 1024; a workgroup covers 256 * 4 elements per sweep, so the cap
    # holds above 1024 * 4096 elements and one sweep of the capped grid then covers 1024 * 1024 of them
    sweep = 1024 * 1024
    n_capped = 5 * sweep + 4099
    assert -(-n_capped // 4096) > 1024
    flags, expect = [], []
    for n in (1, 4099, n_capped):
        x = torch.randn(n, device="cuda")
        st = eng._stream(x)

        def run(start=0):
            f = torch.full((1,), start, dtype=torch.int32, device="cuda")
            eng.lib.call("ds_nonfinite_flag_f32", p(x), n, p(f), st)
            flags.append(f)

        run()
        expect.append(0)                                    # a clean tensor leaves 0
        run(1)
        expect.append(1)                                    # ... and a raised flag stays raised
        # first, middle, last; in the capped case also the second sweep, the last full sweep and the ragged tail
        for pos in sorted({0, n // 2, n - 1, min(n - 1, sweep + 5), min(n - 1, 4 * sweep + 1023), max(0, n - 3)}):
            for val in (NAN, float("inf"), float("-inf")):
                keep = x[pos].clone()
                x[pos] = val
                run()
                expect.append(1)
                x[pos] = keep
        run()
        expect.append(0)                                    # restored: clean again
    torch.cuda.synchronize()
    got = [int(f) for f in flags]
    assert got == expect, [i for i, (a, b) in enumerate(zip(got, expect)) if a != b]
