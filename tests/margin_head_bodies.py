"""The test bodies of the angular-margin head's suites, written once against the backend adapter of loss_side_bodies.py
(be.full / put / get / p / call / rc / plain) plus, for the autograd bodies, be.eng (an Engine on the backend's library) and
be.tensor(host array) -> a torch tensor in the backend's memory.  Run by test_emul_margin_head.py (host emulator) and
test_gpu_margin_head.py (MI355X).

The kernel bodies drive the C ABI in the order model._MarginHeadFn does: normalise x and W, pack W^ twice, cosine GEMM +
margin + cross entropy, gc / r / q, the two gradient GEMMs of the plain head, the two tangent projections.  Outputs start
as NaN with a NaN guard tail that must survive (loss_side_bodies.Buf).  Bars: margin_head_cases -- max(floor, 4 x the
float32 restatement's error against float64), printed with the kernel's error; no case is exempt."""
import ctypes

import numpy as np
import torch

import margin_head_cases as MC
from deepspeaker_pytorch_amd._native import ConvShape
from loss_side_bodies import bits, hold, inp, out, same_bits, say
from margin_head_cases import F32, F64, FLOOR_CE, FLOOR_COS, KINDS, max_rel, pad128, rel_l2


def normalize(be, a, rows_out):
    R, K = a.shape
    src, hat, inv = inp(be, a), out(be, (rows_out, K)), out(be, rows_out)
    be.call("ds_row_normalize_f32", src.p(), hat.p(), inv.p(), R, rows_out, K)
    return hat, inv


def pack_weight(be, w):
    """W -> (W^ [Np, K], 1 / norm [Np], forward packing, data-gradient packing); rows n_cls .. Np-1 are zero"""
    n, K = w.shape
    Np = pad128(n)
    what, inv_w = normalize(be, w, Np)
    wp, wd = out(be, Np * K), out(be, Np * K)
    be.call("ds_pack_fc_weight_f32", what.p(), wp.p(), Np, K, 1)
    be.call("ds_pack_fc_weight_dgrad_f32", what.p(), wd.p(), Np, K, 1)
    wh = what.get("what")
    assert (bits(wh[n:]) == 0).all() and (bits(inv_w.get("inv_w")[n:]) == 0).all(), "the pad rows are +0"
    return what, inv_w, wp, wd


def run_chain(be, x, w, labels, s, m, kind, gloss, pack=None):
    """the whole head, forward and backward, through the C ABI; host arrays of everything it wrote"""
    M, K = x.shape
    n = w.shape[0]
    Np = pad128(n)
    what, inv_w, wp, wd = pack or pack_weight(be, w)
    xhat, inv_x = normalize(be, x, M)
    blab = inp(be, labels)
    ws_n = int(be.plain("ds_fc_margin_workspace_floats", M, K, Np))
    assert ws_n == MC.EXPECTED_S[K] * M * Np, (ws_n, K)
    ws, c, row, lse, loss = out(be, ws_n), out(be, (M, Np)), out(be, M), out(be, M), out(be, 1)
    be.call("ds_fc_margin_ce_fwd_f32", xhat.p(), wp.p(), ws.p(), c.p(), blab.p(), row.p(), lse.p(), loss.p(), M, K, Np, n,
            s, m, KINDS[kind])
    ws.get("workspace")
    bgl, gc, r, q = inp(be, np.array([gloss], F32)), out(be, (M, Np)), out(be, M), out(be, Np)
    be.call("ds_margin_ce_bwd_f32", c.p(), blab.p(), lse.p(), bgl.p(), gc.p(), r.p(), q.p(), M, Np, n, s, m, KINDS[kind])
    ws2, a, gx = out(be, int(be.plain("ds_fc_workspace_floats", M, Np, K))), out(be, (M, K)), out(be, (M, K))
    be.call("ds_fc_l2norm_fwd_f32", gc.p(), wd.p(), None, ws2.p(), a.p(), None, M, Np, K, 1.0, 0.0)
    be.call("ds_margin_grad_fixup_f32", a.p(), xhat.p(), r.p(), inv_x.p(), gx.p(), M, K)
    shp = ConvShape(1, M, 1, K, Np, 1, 1)
    ws3 = out(be, int(be.plain("ds_conv_wgrad_workspace_floats", ctypes.byref(shp))))
    bm, gw = out(be, (Np, K)), out(be, (n, K))
    be.call("ds_conv_wgrad_f32", ctypes.byref(shp), xhat.p(), gc.p(), ws3.p(), bm.p(), 0)
    be.call("ds_margin_grad_fixup_f32", bm.p(), what.p(), q.p(), inv_w.p(), gw.p(), n, K)
    got = {k: v.get(k) for k, v in dict(xh=xhat, inv_x=inv_x, c=c, row_loss=row, lse=lse, loss=loss, gc=gc, r=r, q=q, gx=gx,
                                        gw=gw).items()}
    got["wh"], got["inv_w"] = what.get("what"), inv_w.get("inv_w")
    return got


def body_margin(be, M, n, K, kind, m, s, plant):
    tag = f"margin M={M} n_cls={n} K={K} {kind} m={m:g} s={s:g} {plant}".rstrip()
    Np = pad128(n)
    x, w, labels = MC.margin_inputs(M, n, K, plant, 1000 * M + 7 * n + K)
    gloss = 0.8
    r64, r32 = MC.margin_ref(x, w, labels, s, m, kind, gloss), MC.margin_ref(x, w, labels, s, m, kind, gloss, F32)
    lc = float(np.abs(r64["label_cos"]).max())
    print(f"{tag}: label cosines {r64['label_cos'].min():+.3f} .. {r64['label_cos'].max():+.3f}, padded to {Np} columns")
    saturated = plant == "saturated"
    assert saturated == (lc > MC.LABEL_COS_LIMIT), "input condition: |label cosine| <= 0.99 except on the saturated plant"
    if plant == "fallback":
        assert r64["label_cos"][0] < -0.96 and (M < 2 or r64["label_cos"][1] > 0.88)
        assert (r64["label_cos"][0] <= -np.cos(m)) == (m == 0.5), "m = 0.5 puts row 0 on the fallback branch, m = 0.2 does not"
    if plant in ("padwin", "padwin_deep"):
        assert r64["c"].max() < -0.3, "input condition: every real cosine is negative"
    if plant == "padwin_deep":
        assert s * r64["c"].max() < -104, "input condition: expf(s c - 0) is 0 in float32 for every real column"

    pack = pack_weight(be, w)
    got = run_chain(be, x, w, labels, s, m, kind, gloss, pack)
    again = run_chain(be, x, w, labels, s, m, kind, gloss, pack)
    for k in got:
        assert same_bits(got[k], again[k]), (tag, k, "two calls give identical bits")

    hold(tag, "x^", got["xh"], r64["xh"], r32["xh"], FLOOR_COS, max_rel)
    hold(tag, "w^", got["wh"][:n], r64["wh"], r32["wh"], FLOOR_COS, max_rel)
    ch = got["c"]
    assert (bits(ch[:, n:]) == 0).all() and (bits(got["gc"][:, n:]) == 0).all(), "pad columns: c = 0 and gc = 0 exactly"
    assert np.abs(ch).max() <= 1.0, "c is clamped"
    hold(tag, "c", ch[:, :n], r64["c"], r32["c"], FLOOR_COS, max_rel)
    top = max(1.0, float(np.abs(r64["lse"]).max()))
    absmax = lambda a, b: float(np.abs(np.asarray(a, F64) - np.asarray(b, F64)).max() / top)      # noqa: E731
    hold(tag, "lse", got["lse"], r64["lse"], r32["lse"], FLOOR_CE, rel_l2)
    hold(tag, "row_loss", got["row_loss"], r64["row_loss"], r32["row_loss"], FLOOR_CE, absmax)
    hold(tag, "loss", got["loss"], [r64["loss"]], [r32["loss"]], FLOOR_CE, absmax)
    for k in ("gc", "r", "q", "gx", "gw"):
        g = got[k][:, :n] if k == "gc" else got[k][:n] if k == "q" else got[k]
        assert np.isfinite(g).all(), (tag, k, "finite")
        if saturated:                       # dphi/dc sits on the floor's 1 / 1e-3 there: finite is what is promised
            continue
        hold(tag, k, g, r64[k], r32[k], FLOOR_COS, max_rel)
    if saturated:
        assert abs(float(ch[0, labels[0]]) - 1.0) <= 1e-6
    if plant == "zero":
        z = 1 % n
        assert (ch[M - 1] == 0).all() and (ch[:, z] == 0).all(), "a zero row has cosine 0 to everything"
        assert (got["gx"][M - 1] == 0).all() and (got["gw"][z] == 0).all(), "and receives no gradient"
        assert got["inv_x"][M - 1] == 0 and got["inv_w"][z] == 0

    # batch invariance: the first rows alone, with the incoming gradient scaled to the same gloss / M
    Ms = 1 if M < 3 else 2                  # (a power of two: gloss / M * Ms / Ms is exact in f32)
    if Ms < M:
        gsub = float(F32(gloss) / F32(M) * F32(Ms))
        assert F32(gsub) / F32(Ms) == F32(gloss) / F32(M), "input condition: the same gloss / M in f32"
        sub = run_chain(be, x[:Ms], w, labels[:Ms], s, m, kind, gsub, pack)
        for k in ("c", "lse", "row_loss", "gc", "r", "gx"):
            assert same_bits(sub[k], got[k][:Ms]), (tag, k, "a row does not depend on the other rows of the batch")


def body_forward_only(be, M, n, K, kind, m, s):
    """both forward entry points at a K the backward does not take (1 and 2 K-slices): c, lse, row loss and loss against
    float64 under the bars of body_margin, pad columns, two calls bit for bit"""
    tag = f"forward M={M} n_cls={n} K={K} {kind} m={m:g} s={s:g}"
    Np = pad128(n)
    x, w, labels = MC.margin_inputs(M, n, K, "", 500 * M + 3 * n + K)
    r64, r32 = MC.margin_ref(x, w, labels, s, m, kind), MC.margin_ref(x, w, labels, s, m, kind, dtype=F32)
    assert float(np.abs(r64["label_cos"]).max()) <= MC.LABEL_COS_LIMIT
    what, inv_w, wp, _ = pack_weight(be, w)
    xhat, _ = normalize(be, x, M)
    blab = inp(be, labels)
    ws_n = int(be.plain("ds_fc_margin_workspace_floats", M, K, Np))
    print(f"{tag}: {MC.EXPECTED_S[K]} K-slice(s), workspace {ws_n} floats")
    assert ws_n == MC.EXPECTED_S[K] * M * Np
    runs = []
    for _ in range(2):
        ws, c, row, lse, loss = out(be, ws_n), out(be, (M, Np)), out(be, M), out(be, M), out(be, 1)
        be.call("ds_fc_margin_ce_fwd_f32", xhat.p(), wp.p(), ws.p(), c.p(), blab.p(), row.p(), lse.p(), loss.p(), M, K, Np, n,
                s, m, KINDS[kind])
        assert np.isfinite(ws.get("workspace")).all(), "S * M * Np partials, all written, none past them"
        ws2, c2, cos = out(be, ws_n), out(be, (M, Np)), out(be, (M, n))
        be.call("ds_fc_cosine_fwd_f32", xhat.p(), wp.p(), ws2.p(), c2.p(), cos.p(), M, K, Np, n, s)
        ws2.get("workspace")
        runs.append(dict(c=c.get("c"), row_loss=row.get("row_loss"), lse=lse.get("lse"), loss=loss.get("loss"), c2=c2.get("c"),
                         cos=cos.get("cos_out")))
    for k in runs[0]:
        assert same_bits(runs[0][k], runs[1][k]), (tag, k, "two calls give identical bits")
    got = runs[0]
    assert (bits(got["c"][:, n:]) == 0).all() and np.abs(got["c"]).max() <= 1.0, "pad columns: c = 0 exactly; c is clamped"
    assert same_bits(got["c2"], got["c"]) and same_bits(got["cos"], F32(s) * got["c"][:, :n]), "the cosine head: the same c, times the scale"
    hold(tag, "c", got["c"][:, :n], r64["c"], r32["c"], FLOOR_COS, max_rel)
    top = max(1.0, float(np.abs(r64["lse"]).max()))
    absmax = lambda a, b: float(np.abs(np.asarray(a, F64) - np.asarray(b, F64)).max() / top)      # noqa: E731
    hold(tag, "lse", got["lse"], r64["lse"], r32["lse"], FLOOR_CE, rel_l2)
    hold(tag, "row_loss", got["row_loss"], r64["row_loss"], r32["row_loss"], FLOOR_CE, absmax)
    hold(tag, "loss", got["loss"], [r64["loss"]], [r32["loss"]], FLOOR_CE, absmax)


def body_margin_zero_equals_cosine_ce(be, M, n, K, s):
    """aam with m = 0 is am with m = 0 bit for bit (phi = c exactly in both), and both are classify_cosine's logits under
    the plain cross entropy"""
    tag = f"m=0 M={M} n_cls={n} K={K} s={s:g}"
    x, w, labels = MC.margin_inputs(M, n, K, "fallback", 31 * M + n)         # (row 0 near c = -1: aam's fallback branch at m = 0)
    pack = pack_weight(be, w)
    a, b = run_chain(be, x, w, labels, s, 0.0, "aam", 1.0, pack), run_chain(be, x, w, labels, s, 0.0, "am", 1.0, pack)
    for k in a:
        assert same_bits(a[k], b[k]), (tag, k)
    Np = pad128(n)
    xhat, _ = normalize(be, x, M)
    ws, c, cos = out(be, int(be.plain("ds_fc_margin_workspace_floats", M, K, Np))), out(be, (M, Np)), out(be, (M, n))
    be.call("ds_fc_cosine_fwd_f32", xhat.p(), pack[2].p(), ws.p(), c.p(), cos.p(), M, K, Np, n, s)
    cosh = cos.get("cos_out")
    assert same_bits(c.get("c"), a["c"]) and same_bits(cosh, F32(s) * a["c"][:, :n]), "the same cosines, times the scale"
    blab, row, lse, loss = inp(be, labels), out(be, M), out(be, M), out(be, 1)
    be.call("ds_cross_entropy_fwd_f32", cos.p(), blab.p(), row.p(), lse.p(), loss.p(), M, n, n)
    top = max(1.0, float(np.abs(a["lse"]).max()))
    for name, mine, plain in (("lse", a["lse"], lse.get()), ("row_loss", a["row_loss"], row.get()), ("loss", a["loss"], loss.get())):
        d = float(np.abs(mine.astype(F64) - plain.astype(F64)).max() / top)
        print(f"{tag}: {name} against ds_cross_entropy_fwd_f32 on classify_cosine's logits {d:.2e} (floor {FLOOR_CE:g})")
        assert d <= FLOOR_CE


def body_cosine_bwd(be, M, n, K, s):
    """the cosine head's backward (dphi/dc = 1 everywhere) against float64"""
    tag = f"cosine bwd M={M} n_cls={n} K={K} s={s:g}"
    x, w, _ = MC.margin_inputs(M, n, K, "", M + n + K)
    rs = np.random.RandomState(M * n)
    gout = rs.randn(M, n).astype(F32)
    Np = pad128(n)
    what, inv_w, wp, wd = pack_weight(be, w)
    xhat, inv_x = normalize(be, x, M)
    ws, c, cos = out(be, int(be.plain("ds_fc_margin_workspace_floats", M, K, Np))), out(be, (M, Np)), out(be, (M, n))
    be.call("ds_fc_cosine_fwd_f32", xhat.p(), wp.p(), ws.p(), c.p(), cos.p(), M, K, Np, n, s)
    bg, gc, r, q = inp(be, gout), out(be, (M, Np)), out(be, M), out(be, Np)
    be.call("ds_cosine_bwd_f32", c.p(), bg.p(), gc.p(), r.p(), q.p(), M, Np, n, s)
    gch = gc.get("gc")
    assert (bits(gch[:, n:]) == 0).all() and same_bits(gch[:, :n], F32(s) * gout)
    ws2, a, gx = out(be, int(be.plain("ds_fc_workspace_floats", M, Np, K))), out(be, (M, K)), out(be, (M, K))
    be.call("ds_fc_l2norm_fwd_f32", gc.p(), wd.p(), None, ws2.p(), a.p(), None, M, Np, K, 1.0, 0.0)
    be.call("ds_margin_grad_fixup_f32", a.p(), xhat.p(), r.p(), inv_x.p(), gx.p(), M, K)
    shp = ConvShape(1, M, 1, K, Np, 1, 1)
    ws3 = out(be, int(be.plain("ds_conv_wgrad_workspace_floats", ctypes.byref(shp))))
    bm, gw = out(be, (Np, K)), out(be, (n, K))
    be.call("ds_conv_wgrad_f32", ctypes.byref(shp), xhat.p(), gc.p(), ws3.p(), bm.p(), 0)
    be.call("ds_margin_grad_fixup_f32", bm.p(), what.p(), q.p(), inv_w.p(), gw.p(), n, K)
    g64, g32 = MC.cosine_bwd_ref(x, w, gout, s), MC.cosine_bwd_ref(x, w, gout, s, F32)
    hold(tag, "gx", gx.get("gx"), g64[0], g32[0], FLOOR_COS, max_rel)
    hold(tag, "gw", gw.get("gw"), g64[1], g32[1], FLOOR_COS, max_rel)


def body_abi_errors(be):
    """refusals before any launch, with the plain head's codes: null -3, shape -1, alignment -2; a rule outside its range -1,
    an unknown kind -4"""
    M, K, n, Np = 3, 512, 21, 128
    f = lambda *shape: out(be, shape)                                                                # noqa: E731
    xh, wp, ws, c, row, lse, loss = f(M, K), f(Np * K), f(8 * M * Np), f(M, Np), f(M), f(M), f(1)
    lab = inp(be, np.zeros(M, np.int64))
    gl, gc, r, q, inv = inp(be, np.ones(1, F32)), f(M, Np), f(M), f(Np), f(Np)

    def fwd(xh_=xh.p(), wp_=wp.p(), ws_=ws.p(), c_=c.p(), lab_=lab.p(), row_=row.p(), lse_=lse.p(), loss_=loss.p(), M_=M, K_=K,
            N_=Np, n_=n, s_=30.0, m_=0.2, kind_=0):
        return be.rc("ds_fc_margin_ce_fwd_f32", xh_, wp_, ws_, c_, lab_, row_, lse_, loss_, M_, K_, N_, n_, s_, m_, kind_)

    for k in ("xh_", "wp_", "ws_", "c_", "lab_", "row_", "lse_", "loss_"):
        assert fwd(**{k: None}) == MC.DS_ERR_NULL, k
    for kw in (dict(M_=0), dict(M_=-1), dict(n_=Np + 1), dict(n_=0), dict(N_=Np + 64), dict(N_=0), dict(K_=0), dict(K_=100),
               dict(K_=520), dict(s_=0.0), dict(s_=-1.0), dict(s_=float("inf")), dict(m_=-0.1), dict(m_=1.5708), dict(m_=float("nan"))):
        assert fwd(**kw) == MC.DS_ERR_BAD_SHAPE, kw
    assert fwd(kind_=2) == MC.DS_ERR_UNSUPPORTED and fwd(kind_=-1) == MC.DS_ERR_UNSUPPORTED
    for k, b in (("xh_", xh), ("wp_", wp), ("ws_", ws), ("c_", c)):
        assert fwd(**{k: b.p(1)}) == MC.DS_ERR_ALIGNMENT, k
    assert int(be.plain("ds_fc_margin_workspace_floats", 0, K, Np)) == MC.DS_ERR_BAD_SHAPE
    assert int(be.plain("ds_fc_margin_workspace_floats", M, 100, Np)) == MC.DS_ERR_BAD_SHAPE
    assert int(be.plain("ds_fc_margin_workspace_floats", M, K, 100)) == MC.DS_ERR_BAD_SHAPE
    cos = f(M, n)
    assert be.rc("ds_fc_cosine_fwd_f32", xh.p(), wp.p(), ws.p(), c.p(), None, M, K, Np, n, 1.0) == MC.DS_ERR_NULL
    assert be.rc("ds_fc_cosine_fwd_f32", xh.p(), wp.p(), ws.p(), c.p(), cos.p(), M, K, Np, Np + 1, 1.0) == MC.DS_ERR_BAD_SHAPE
    assert be.rc("ds_fc_cosine_fwd_f32", xh.p(), wp.p(), ws.p(), c.p(), cos.p(), M, K, Np, n, 0.0) == MC.DS_ERR_BAD_SHAPE
    assert be.rc("ds_fc_cosine_fwd_f32", xh.p(1), wp.p(), ws.p(), c.p(), cos.p(), M, K, Np, n, 1.0) == MC.DS_ERR_ALIGNMENT

    def bwd(c_=c.p(), lab_=lab.p(), lse_=lse.p(), gl_=gl.p(), gc_=gc.p(), r_=r.p(), q_=q.p(), M_=M, N_=Np, n_=n, s_=30.0, m_=0.2,
            kind_=1):
        return be.rc("ds_margin_ce_bwd_f32", c_, lab_, lse_, gl_, gc_, r_, q_, M_, N_, n_, s_, m_, kind_)

    for k in ("c_", "lab_", "lse_", "gl_", "gc_", "r_", "q_"):
        assert bwd(**{k: None}) == MC.DS_ERR_NULL, k
    for kw in (dict(M_=0), dict(n_=Np + 1), dict(N_=Np + 64), dict(s_=0.0), dict(m_=1.6)):
        assert bwd(**kw) == MC.DS_ERR_BAD_SHAPE, kw
    assert bwd(kind_=7) == MC.DS_ERR_UNSUPPORTED
    assert bwd(c_=c.p(1)) == MC.DS_ERR_ALIGNMENT and bwd(gc_=gc.p(2)) == MC.DS_ERR_ALIGNMENT
    g = f(M, n)
    assert be.rc("ds_cosine_bwd_f32", c.p(), None, gc.p(), r.p(), q.p(), M, Np, n, 1.0) == MC.DS_ERR_NULL
    assert be.rc("ds_cosine_bwd_f32", c.p(), g.p(), gc.p(), r.p(), q.p(), M, Np + 1, n, 1.0) == MC.DS_ERR_BAD_SHAPE
    assert be.rc("ds_cosine_bwd_f32", c.p(3), g.p(), gc.p(), r.p(), q.p(), M, Np, n, 1.0) == MC.DS_ERR_ALIGNMENT

    assert be.rc("ds_row_normalize_f32", None, xh.p(), inv.p(), M, M, K) == MC.DS_ERR_NULL
    assert be.rc("ds_row_normalize_f32", xh.p(), c.p(), None, M, M, K) == MC.DS_ERR_NULL
    assert be.rc("ds_row_normalize_f32", xh.p(), c.p(), inv.p(), 0, M, K) == MC.DS_ERR_BAD_SHAPE
    assert be.rc("ds_row_normalize_f32", xh.p(), c.p(), inv.p(), M, M - 1, K) == MC.DS_ERR_BAD_SHAPE
    assert be.rc("ds_row_normalize_f32", xh.p(), c.p(), inv.p(), M, M, 6) == MC.DS_ERR_BAD_SHAPE
    assert be.rc("ds_row_normalize_f32", xh.p(1), c.p(), inv.p(), M, M, K) == MC.DS_ERR_ALIGNMENT
    assert be.rc("ds_margin_grad_fixup_f32", xh.p(), xh.p(), None, inv.p(), c.p(), M, K) == MC.DS_ERR_NULL
    assert be.rc("ds_margin_grad_fixup_f32", xh.p(), xh.p(), r.p(), inv.p(), c.p(), M, 6) == MC.DS_ERR_BAD_SHAPE
    assert be.rc("ds_margin_grad_fixup_f32", xh.p(), xh.p(1), r.p(), inv.p(), c.p(), M, K) == MC.DS_ERR_ALIGNMENT
    for b in (xh, wp, ws, c, row, lse, loss, gc, r, q, inv, cos, g):
        assert np.isnan(b.get()).all(), "a refused call launches nothing"


# ---------------------------------------------------------------------------------------------------------------------
# autograd and plumbing (DeepSpeakerModel on the backend's engine)
# ---------------------------------------------------------------------------------------------------------------------
def make_model(be, n_cls, seed=3):
    from deepspeaker_pytorch_amd.model import DeepSpeakerModel
    torch.manual_seed(seed)
    model = DeepSpeakerModel(512, n_cls)
    with torch.no_grad():
        model.model.classifier.weight.copy_(torch.from_numpy((0.05 * np.random.RandomState(seed).randn(n_cls, 512)).astype(F32)))
    return model.to(be.device)


def body_autograd(be, kind):
    """margin_loss(...).backward(): weight and embedding gradients against float64, bias.grad None, the pack cached per
    weight version, an incoming gradient != 1 (loss scaling)"""
    M, n = 6, 21
    model = make_model(be, n)
    assert len(model.state_dict()) == 76, "the state_dict keeps the reference's 76 keys"
    cls = model.model.classifier
    x, _, labels = MC.margin_inputs(M, n, 512, "", 77)
    w = cls.weight.detach().cpu().numpy().copy()
    pack = model._margin_head()
    assert model._margin_head() is pack, "the pack is re-used while the weight is unchanged"
    with torch.no_grad():
        cls.bias.add_(1.0)
    assert model._margin_head() is pack, "the pack is keyed on the weight only"
    for gscale in (1.0, 1024.0):
        emb = be.tensor(x).requires_grad_(True)
        cls.weight.grad = cls.bias.grad = None
        loss = model.margin_loss(emb, be.tensor(labels), margin=0.2, scale=30.0, kind=kind)
        assert loss.shape == () and loss.dtype == torch.float32
        (loss * gscale).backward()
        ref, r32 = MC.margin_ref(x, w, labels, 30.0, 0.2, kind, gscale), MC.margin_ref(x, w, labels, 30.0, 0.2, kind, gscale, F32)
        tag = f"autograd {kind} gloss={gscale:g}"
        hold(tag, "loss", [loss.item()], [ref["loss"]], [r32["loss"]], FLOOR_CE, lambda a, b: abs(float(a[0]) - float(b[0])) / max(1.0, abs(float(b[0]))))
        hold(tag, "embeddings.grad", emb.grad.cpu().numpy(), ref["gx"], r32["gx"], FLOOR_COS, max_rel)
        hold(tag, "classifier.weight.grad", cls.weight.grad.cpu().numpy(), ref["gw"], r32["gw"], FLOOR_COS, max_rel)
        assert cls.bias.grad is None, "the bias receives no gradient"
    # an embedding that needs no gradient, and a weight that needs none
    loss = model.margin_loss(be.tensor(x), be.tensor(labels), kind=kind)
    cls.weight.grad = None
    loss.backward()
    assert cls.weight.grad is not None
    # an in-place weight update (what the fused optimizers do through raw pointers + increment_version) rebuilds the pack
    with torch.no_grad():
        cls.weight.mul_(-1.0)
    pack2 = model._margin_head()
    assert pack2 is not pack and model._margin_head() is pack2
    flipped = model.margin_loss(be.tensor(x), be.tensor(labels), margin=0.2, scale=30.0, kind=kind)
    want = MC.margin_ref(x, -w, labels, 30.0, 0.2, kind)["loss"]
    assert abs(flipped.item() - want) <= 1e-5 * max(1.0, abs(want)), "the rebuilt pack holds the new weight"


def body_cosine_autograd(be):
    """classify_cosine: scale * cosines, differentiable through the margin head's backward with dphi/dc = 1; under the plain
    CrossEntropyLoss it is margin_loss at margin 0"""
    from deepspeaker_pytorch_amd.model import CrossEntropyLoss
    M, n = 5, 21
    model = make_model(be, n)
    cls = model.model.classifier
    x, _, labels = MC.margin_inputs(M, n, 512, "", 78)
    w = cls.weight.detach().cpu().numpy().copy()
    emb = be.tensor(x).requires_grad_(True)
    logits = model.classify_cosine(emb, scale=30.0)
    assert tuple(logits.shape) == (M, n) and logits.is_contiguous()
    ref, r32 = MC.margin_ref(x, w, labels, 30.0, 0.0, "am"), MC.margin_ref(x, w, labels, 30.0, 0.0, "am", dtype=F32)
    hold("classify_cosine", "logits", logits.detach().cpu().numpy(), 30.0 * ref["c"], F32(30.0) * r32["c"], FLOOR_COS, max_rel)
    loss = CrossEntropyLoss()(logits, be.tensor(labels))
    loss.backward()
    via_margin = model.margin_loss(be.tensor(x), be.tensor(labels), margin=0.0, scale=30.0, kind="aam")
    d = abs(loss.item() - via_margin.item()) / max(1.0, float(np.abs(ref["lse"]).max()))
    print(f"classify_cosine + CrossEntropyLoss against margin_loss(margin=0): {d:.2e} (floor {FLOOR_CE:g})")
    assert d <= FLOOR_CE
    hold("classify_cosine", "embeddings.grad", emb.grad.cpu().numpy(), ref["gx"], r32["gx"], FLOOR_COS, max_rel)
    hold("classify_cosine", "classifier.weight.grad", cls.weight.grad.cpu().numpy(), ref["gw"], r32["gw"], FLOOR_COS, max_rel)
    assert cls.bias.grad is None
    assert model.classify_cosine(be.tensor(x)).detach().abs().max().item() <= 1.0, "scale defaults to 1: plain cosines"


def body_python_errors(be):
    import pytest
    model = make_model(be, 21)
    x, _, labels = MC.margin_inputs(4, 21, 512, "", 5)
    emb, lab = be.tensor(x), be.tensor(labels)
    with pytest.raises(ValueError, match="kind"):
        model.margin_loss(emb, lab, kind="arc")
    with pytest.raises(ValueError, match="kind"):
        model.margin_loss(emb, lab, kind=0)
    assert model.margin_loss(emb, lab, margin=1.5707963, kind="am").isfinite().item(), "the largest float32 below pi/2 is in range"
    for bad in (-0.1, 1.5708, float("nan"), 1.57079632):                   # (the last rounds to the float32 above pi/2)
        with pytest.raises(ValueError, match="margin"):
            model.margin_loss(emb, lab, margin=bad)
    for bad in (0.0, -30.0, float("inf"), 1e39, 1e-50, 10 ** 400):          # (inf and 0 as the float32 the kernels take)
        with pytest.raises(ValueError, match="scale"):
            model.margin_loss(emb, lab, scale=bad)
        with pytest.raises(ValueError, match="scale"):
            model.classify_cosine(emb, scale=bad)
    with pytest.raises(TypeError, match="margin"):
        model.margin_loss(emb, lab, margin="0.2")
    with pytest.raises(TypeError, match="scale"):
        model.margin_loss(emb, lab, scale=be.tensor(np.array([30.0], F32)))
    with pytest.raises(TypeError, match="integer"):
        model.margin_loss(emb, lab.float())
    with pytest.raises(ValueError, match="shape"):
        model.margin_loss(emb, lab[:3])
    with pytest.raises(ValueError, match="shape"):
        model.margin_loss(emb, lab.reshape(4, 1))
    with pytest.raises(ValueError, match="embeddings"):
        model.margin_loss(emb[:, :256], lab)
    assert model.margin_loss(emb, lab.to(torch.int32)).item() == model.margin_loss(emb, lab).item(), "any integer dtype"
