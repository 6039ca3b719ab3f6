"""The test bodies of the loss-side / head / scoring kernel suites, written once against a small backend adapter and run by
test_emul_loss_side.py (host emulator, numpy memory) and test_gpu_loss_side_kernels.py (MI355X, torch device memory).

The adapter (`be`):
    be.name, be.is_device, be.cus                   "emul" / "gpu"; the compute-unit count the library plans with
    be.full(n, dtype, fill) -> handle               1-D buffer of n elements, 16-byte aligned
    be.put(handle, host_array)                      copy a host array to the start of the buffer
    be.get(handle) -> host array                    waits for the queued work first
    be.p(handle, offset=0)                          pointer `offset` elements in
    be.call(name, *args)                            entry point on the backend's stream; raises unless it returns DS_OK
    be.rc(name, *args) -> int                       the same, returning the code
    be.plain(name, *args)                           entry points without a stream argument

Rules every body follows: outputs start as NaN (floats) or a sentinel (integers) and carry a guard tail of GUARD elements
that must keep it; inputs carry a NaN (or, for index lists, out-of-list) guard tail, and whatever the contract says is not
read is poisoned the same way; the bar never comes from the kernel's output (loss_side_cases: max(floor, 4 x the float32
restatement's error against float64)); restatement error, bar and kernel error are printed."""
import numpy as np

import deepspeaker_oracle as O
import loss_side_cases as LC
from loss_side_cases import F32, F64, bar_from_restatement, max_rel, rel_l2

GUARD = 64
SENTINEL = -7777


def _fill_of(dtype):
    return np.nan if np.dtype(dtype).kind == "f" else SENTINEL


class Buf:
    """a buffer of prod(shape) elements plus GUARD more; `data`: initial contents (inputs), else all fill (outputs)"""

    def __init__(self, be, shape, dtype=F32, data=None, fill=None):
        self.be, self.shape, self.dtype = be, tuple(np.atleast_1d(shape)), np.dtype(dtype)
        self.n = int(np.prod(self.shape))
        self.fill = _fill_of(dtype) if fill is None else fill
        self.h = be.full(self.n + GUARD, dtype, self.fill)
        if data is not None:
            be.put(self.h, np.ascontiguousarray(data, dtype).reshape(-1))

    def p(self, off=0):
        return self.be.p(self.h, off)

    def get(self, what="buffer"):
        a = self.be.get(self.h)
        tail = a[self.n:]
        intact = np.isnan(tail).all() if isinstance(self.fill, float) and np.isnan(self.fill) else (tail == self.fill).all()
        assert intact, f"{what}: guard tail overwritten"
        return a[:self.n].reshape(self.shape).copy()


def inp(be, a, dtype=None):
    a = np.asarray(a)
    return Buf(be, a.shape, dtype or a.dtype, data=a)


def out(be, shape, dtype=F32, fill=None):
    return Buf(be, shape, dtype, fill=fill)


def say(tag, what, restated, bar, err):
    print(f"{tag}: {what} f32-restated {restated:.2e} bar {bar:.2e} kernel {err:.2e}")


def hold(tag, what, got, ref64, ref32, floor, metric=rel_l2):
    """kernel against float64 with the bar from the float32 restatement"""
    restated = metric(ref32, ref64)
    bar = bar_from_restatement(floor, restated)
    err = metric(got, ref64)
    say(tag, what, restated, bar, err)
    assert err <= bar, (tag, what, err, bar)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


# ---------------------------------------------------------------------------------------------------------------------
# row kernels
# ---------------------------------------------------------------------------------------------------------------------
def body_rows(be, rows, D):
    tag = f"rows={rows} D={D}"
    x1, x2 = LC.row_inputs(rows, D, 100 * rows + D)
    rs = np.random.RandomState(rows + 7 * D)
    x3 = (rs.randn(rows, D) / np.sqrt(2 * D)).astype(F32)
    ge, gd = rs.randn(rows, D).astype(F32), rs.randn(rows).astype(F32)
    alpha, eps = 10.0, 1e-10
    b1, b2, b3, bge, bgd = (inp(be, v) for v in (x1, x2, x3, ge, gd))

    # L2 normalisation and its gradient (model.py:172-183); row 0 is all zero: norm = sqrt(eps), e = 0
    e, gf = out(be, (rows, D)), out(be, (rows, D))
    be.call("ds_l2norm_scale_f32", b1.p(), e.p(), rows, D, alpha, eps)
    be.call("ds_l2norm_scale_bwd_f32", b1.p(), bge.p(), gf.p(), rows, D, alpha, eps)
    eh, gfh = e.get("e"), gf.get("gf")
    hold(tag, "l2norm", eh, LC.l2norm(x1, alpha, eps), LC.l2norm(x1, alpha, eps, F32), LC.FLOOR)
    hold(tag, "l2norm bwd", gfh, LC.l2norm_bwd(x1, ge, alpha, eps), LC.l2norm_bwd(x1, ge, alpha, eps, F32), LC.FLOOR)
    assert (eh[0] == 0).all(), "all-zero row: e = 0"
    zero_row = ge[0].astype(F64) * alpha / np.sqrt(eps)
    assert rel_l2(gfh[0], zero_row) <= 1e-6, "all-zero row: gf = alpha ge / sqrt(eps)"

    # pairwise distance, p = 2 kernel and the any-norm kernel
    d = out(be, rows)
    be.call("ds_pairwise_distance_f32", b1.p(), b2.p(), d.p(), rows, D)
    dh = d.get("d")
    hold(tag, "distance", dh, LC.pdist(x1, x2), LC.pdist(x1, x2, 2, F32), LC.FLOOR_DIST)
    assert abs(float(dh[rows - 1]) / np.sqrt(1e-4 / D) - 1) <= 1e-6, "bit-identical rows: d = sqrt(eps)"
    g1, g2 = out(be, (rows, D)), out(be, (rows, D))
    bd = inp(be, dh)
    be.call("ds_pairwise_distance_bwd_f32", b1.p(), b2.p(), bd.p(), bgd.p(), g1.p(), g2.p(), rows, D)
    g1h, g2h = g1.get("g1"), g2.get("g2")
    hold(tag, "distance bwd", g1h, LC.pdist_bwd(x1, x2, dh, gd), LC.pdist_bwd(x1, x2, dh, gd, 2, F32), LC.FLOOR)
    assert same_bits(g2h, -g1h), "g2 == -g1 bit for bit"
    assert (g1h[rows - 1] == 0).all(), "bit-identical rows: gradient exactly 0"
    for p in LC.PNORMS:
        dp_ = out(be, rows)
        be.call("ds_pairwise_distance_p_f32", b1.p(), b2.p(), dp_.p(), rows, D, p)
        dph = dp_.get("d_p-norm")
        hold(tag, f"distance p={p}", dph, LC.pdist(x1, x2, p), LC.pdist(x1, x2, p, F32), LC.FLOOR_PNORM)
        want = (1e-4 / D) ** (1.0 / p)
        assert abs(float(dph[rows - 1]) / want - 1) <= 1e-5, "bit-identical rows: d = eps^(1/p)"
        g1, g2, bd = out(be, (rows, D)), out(be, (rows, D)), inp(be, dph)
        be.call("ds_pairwise_distance_p_bwd_f32", b1.p(), b2.p(), bd.p(), bgd.p(), g1.p(), g2.p(), rows, D, p)
        g1h, g2h = g1.get("g1"), g2.get("g2")
        hold(tag, f"distance bwd p={p}", g1h, LC.pdist_bwd(x1, x2, dph, gd, p), LC.pdist_bwd(x1, x2, dph, gd, p, F32), LC.FLOOR_PNORM_BWD)
        assert same_bits(g2h, -g1h) and (g1h[rows - 1] == 0).all(), "g2 == -g1 bit for bit; identical rows: exactly 0"

    # TripletMarginLoss forward (model.py:27-33) and backward
    margin = 0.25
    d_p, d_n, loss = out(be, rows), out(be, rows), out(be, 1)
    be.call("ds_triplet_margin_fwd_f32", b1.p(), b2.p(), b3.p(), margin, d_p.p(), d_n.p(), loss.p(), rows, D)
    r64, r32 = LC.triplet_fwd(x1, x2, x3, margin), LC.triplet_fwd(x1, x2, x3, margin, F32)
    hold(tag, "triplet d_p", d_p.get(), r64[0], r32[0], LC.FLOOR_DIST)
    hold(tag, "triplet d_n", d_n.get(), r64[1], r32[1], LC.FLOOR_DIST)
    absdiff = lambda a, b: float(np.abs(np.asarray(a, F64) - np.asarray(b, F64)).max())        # noqa: E731
    hold(tag, "triplet loss (absolute, distances near 1)", loss.get(), [r64[2]], [r32[2]], LC.FLOOR_DIST, absdiff)
    # backward on handed-in distances: row 1 holds a hinge argument of exactly 0 (the gradient passes), row 2 one ulp below
    dpb, dnb = r64[0].astype(F32), r64[1].astype(F32)
    if rows >= 3:
        dpb[1], dnb[1] = 1.0, 1.25
        dpb[2], dnb[2] = 1.0, np.nextafter(F32(1.25), F32(2))
    arg32, arg64 = (F32(margin) + dpb) - dnb, (margin + dpb.astype(F64)) - dnb.astype(F64)
    assert ((arg32 >= 0) == (arg64 >= 0)).all(), "input condition: no hinge decision depends on the f32 rounding"
    gl = np.array([1.7], F32)
    ga, gp, gn = out(be, (rows, D)), out(be, (rows, D)), out(be, (rows, D))
    bdp, bdn, bgl = inp(be, dpb), inp(be, dnb), inp(be, gl)
    be.call("ds_triplet_margin_bwd_f32", b1.p(), b2.p(), b3.p(), bdp.p(), bdn.p(), margin, bgl.p(), ga.p(), gp.p(), gn.p(), rows, D)
    got = (ga.get("ga"), gp.get("gp"), gn.get("gn"))
    w64, w32 = LC.triplet_bwd(x1, x2, x3, dpb, dnb, margin, gl[0]), LC.triplet_bwd(x1, x2, x3, dpb, dnb, margin, gl[0], F32)
    for k, name in enumerate(("ga", "gp", "gn")):
        if np.abs(w64[k]).max() > 0:
            hold(tag, "triplet bwd " + name, got[k], w64[k], w32[k], LC.FLOOR)
        else:
            assert (got[k] == 0).all()
    if rows >= 3:
        assert np.abs(got[1][1]).max() > 0, "hinge argument exactly 0: the gradient passes (clamp(min=0) subgradient 1)"
        assert all((g[2] == 0).all() for g in got), "hinge argument below 0: no gradient"


# ---------------------------------------------------------------------------------------------------------------------
# scan family
# ---------------------------------------------------------------------------------------------------------------------
def _check_scan(tag, ref, N, idx, count, loss, mean_diff, d_p, d_n, margin):
    assert ref["flips"] == 0, "input condition: no decision depends on the rounding of the f32 subtraction"
    c = int(count.get("count")[0])
    ih = idx.get("idx")
    assert c == len(ref["idx"]) and (ih[:c] == ref["idx"]).all(), (tag, "the filter list is the ascending reference list")
    assert (ih[c:] == SENTINEL).all(), (tag, "idx[count:] is untouched")
    l32, m32 = LC.scan_f32(d_p, d_n, margin)
    absdiff = lambda a, b: float(np.abs(np.asarray(a, F64) - np.asarray(b, F64)).max())        # noqa: E731
    if loss is not None:
        hold(tag, "loss", loss.get("loss"), [ref["loss"]], [l32], LC.FLOOR_DIST, absdiff)
    hold(tag, "mean_diff", mean_diff.get("mean_diff"), [ref["mean_diff"]], [m32], LC.FLOOR_DIST, absdiff)


def body_scan(be, N, filt, cap_s, probe_s, near):
    tag = f"scan N={N} {filt} cap={cap_s} probe={probe_s} near={near}"
    cap = {"0": 0, "1": 1, "5": 5, "64": 64, "N+7": N + 7}[cap_s]
    probe = {"none": -1, "0": 0, "last": N - 1}[probe_s]
    # (A) the scan and the filter alone, on planted distances: d_n - d_p exactly at margin is NOT selected
    d_p, d_n, margin, band = LC.scan_inputs(N, filt, near, 31 * N + cap)
    ref = LC.scan_ref(d_p, d_n, margin, None)
    if filt == "mix" and N >= 3:
        assert N - 1 not in ref["idx"] and N - 2 in ref["idx"], "the plants: exactly at margin / one ulp below"
    assert {"nothing": len(ref["idx"]) == 0, "everything": len(ref["idx"]) == N}.get(filt, True)
    bp, bn = inp(be, d_p), inp(be, d_n)
    idx, count, loss, md = out(be, N, np.int64), out(be, 1, np.int32), out(be, 1), out(be, 1)
    be.call("ds_triplet_scan_f32", bp.p(), bn.p(), margin, loss.p(), idx.p(), count.p(), md.p(), N)
    _check_scan(tag + " [scan]", ref, N, idx, count, loss, md, d_p, d_n, margin)
    idx, count, md = out(be, N, np.int64), out(be, 1, np.int32), out(be, 1)
    be.call("ds_triplet_filter_f32", bp.p(), bn.p(), margin, idx.p(), count.p(), md.p(), N)
    _check_scan(tag + " [filter]", ref, N, idx, count, None, md, d_p, d_n, margin)

    # (B) distances + scan in one call, with the near-tie list.  Decisions are taken in float64 on the DEVICE'S OWN d_p / d_n.
    D = 512 if N == 768 else 16
    rs = np.random.RandomState(17 * N + cap + 3)
    a = rs.randn(N, D).astype(F32)
    u, v = rs.randn(N, D), rs.randn(N, D)
    r_p, r_n = d_p.astype(F64), d_n.astype(F64)
    if near == "none":
        r_n[-2:] += 0.3                     # (the margin plants of (A) would be near ties here)
    p = (a + u / np.linalg.norm(u, axis=1, keepdims=True) * r_p[:, None]).astype(F32)
    n = (a + v / np.linalg.norm(v, axis=1, keepdims=True) * r_n[:, None]).astype(F32)
    ba, bpp, bnn = inp(be, a), inp(be, p), inp(be, n)

    def run(margin, band):
        o = {"d_p": out(be, N), "d_n": out(be, N), "loss": out(be, 1), "idx": out(be, N, np.int64), "count": out(be, 1, np.int32),
             "md": out(be, 1), "amb": out(be, cap, np.int64), "ac": out(be, 1, np.int32)}
        args = (ba.p(), bpp.p(), bnn.p(), margin, band, o["d_p"].p(), o["d_n"].p(), o["loss"].p(), o["idx"].p(), o["count"].p(),
                o["md"].p(), o["amb"].p(), o["ac"].p(), cap)
        if probe >= 0:
            be.call("ds_triplet_tail_probe_f32", *args, probe, N, D)
        else:
            be.call("ds_triplet_tail_f32", *args, N, D)
        return o

    o = run(margin, band)
    dp1, dn1 = o["d_p"].get("d_p"), o["d_n"].get("d_n")
    replant = filt == "mix" and near != "none"      # ("none" keeps amb_count = 0: a row at margin is itself a near tie)
    if replant:                             # re-plant on the device's own numbers: one row exactly at margin, one exactly at band
        diff = dn1 - dp1                    # (operands in [1, 4), results near 0.25: the f32 subtraction is exact)
        k = int(np.argmin(np.abs(diff - F32(0.25))))
        margin = float(diff[k])
        off = np.abs(diff - F32(margin))
        inside = np.where((off < F32(band)) & (off > 0))[0]
        if len(inside):
            band = float(off[inside[np.argmax(off[inside])]])
        o = run(margin, band)
        dp1, dn1 = o["d_p"].get("d_p"), o["d_n"].get("d_n")
        assert float(dn1[k]) - float(dp1[k]) == margin, "the kernels are deterministic: the plant holds on the second run"
    hold(tag, "d_p", dp1, LC.pdist(a, p), LC.pdist(a, p, 2, F32), LC.FLOOR_DIST)
    hold(tag, "d_n", dn1, LC.pdist(a, n), LC.pdist(a, n, 2, F32), LC.FLOOR_DIST)
    ref = LC.scan_ref(dp1, dn1, margin, band)
    if replant:
        assert k not in ref["idx"] and k in ref["amb"], "exactly at margin: not selected (strict), and a near tie"
        if len(inside):
            assert inside[np.argmax(off[inside])] not in ref["amb"], "exactly at band: not a near tie (strict)"
    _check_scan(tag + " [tail]", ref, N, o["idx"], o["count"], o["loss"], o["md"], dp1, dn1, margin)
    amb = o["amb"].get("amb_idx")
    if cap > 0:
        na = len(ref["amb"])
        print(f"{tag}: near ties {na}, cap {cap}")
        assert {"none": na == 0, "overflow": na > cap or cap > N or filt != "mix", "few": True}[near], (na, cap)
        assert int(o["ac"].get("amb_count")[0]) == na, "amb_count is the TRUE count, also past the cap"
        assert (amb == LC.amb_slots(ref["amb"], cap, probe, N)).all(), "first amb_cap near ties in order, then 0 / the probes"


# ---------------------------------------------------------------------------------------------------------------------
# refinement
# ---------------------------------------------------------------------------------------------------------------------
def body_refine(be, cap, cls, N, D, dup):
    tag = f"refine cap={cap} count={cls} N={N} D={D} dup={dup}"
    rs = np.random.RandomState(cap * 1000 + N + D)
    count = LC.refine_count(cls, cap)
    e_ref = rs.randn(3 * cap, D).astype(F32)
    slots = rs.choice(N, cap, replace=False).astype(np.int64)
    if dup and cap >= 2:
        slots[cap - 1] = slots[0]           # a later slot (a probe when count < cap) names the first near tie's triplet again
    d_p0, d_n0 = (1 + rs.rand(N)).astype(F32), (1 + rs.rand(N)).astype(F32)
    emb = [rs.randn(N, D).astype(F32) for _ in range(3)]
    for t in range(3):                      # the path's own embeddings of the sampled triplets: e_ref plus a small error
        emb[t][slots] = e_ref[t * cap:(t + 1) * cap] + (rs.randn(cap, D) * 1e-3).astype(F32)
    if dup and cap >= 2:
        for t in range(3):
            emb[t][slots[0]] = e_ref[t * cap] + F32(1e-3)
    new64, new32 = LC.refine_ref(e_ref, slots, cap), LC.refine_ref(e_ref, slots, cap, F32)
    be_ref, bcount = inp(be, e_ref), inp(be, np.array([count], np.int32))
    b0p, b0n = inp(be, d_p0), inp(be, d_n0)
    bemb = [inp(be, m) for m in emb]

    def check_patch(name, dph, dnh, live):
        named = {}
        for s in range(live):
            named.setdefault(int(slots[s]), []).append(s)
        rest = np.setdiff1d(np.arange(N), list(named))
        assert same_bits(dph[rest], d_p0[rest]) and same_bits(dnh[rest], d_n0[rest]), (tag, name, "rows no slot names: bit-identical")
        worst = 0.0
        for i, ss in named.items():         # a triplet named twice may hold either slot's distances (whichever wave wrote last)
            ep = min(abs(float(dph[i]) - new64[0][s]) / new64[0][s] for s in ss)
            en = min(abs(float(dnh[i]) - new64[1][s]) / new64[1][s] for s in ss)
            worst = max(worst, ep, en)
        restated = max(max_rel(new32[0], new64[0]), max_rel(new32[1], new64[1]))
        bar = bar_from_restatement(LC.FLOOR_DIST, restated)
        say(tag + " " + name, "patched distances", restated, bar, worst)
        assert worst <= bar

    # plain form: the first min(count, cap) slots are patched in place; the slots past them are not read -- they name row N,
    # the first element of the guard tail, which would then lose its NaN
    live = min(count, cap)
    sl = slots.copy()
    sl[live:] = N
    bsl = inp(be, sl)
    dp, dn = inp(be, d_p0), inp(be, d_n0)
    be.call("ds_refine_distances_f32", be_ref.p(), bsl.p(), bcount.p(), cap, dp.p(), dn.p(), D)
    check_patch("plain", dp.get("d_p"), dn.get("d_n"), live)

    # probe and fused forms: every slot is live; err[0] comes from the untouched "before" distances
    bsl = inp(be, slots)
    delta = np.array([(new64[1][s] - new64[0][s]) - (float(d_n0[slots[s]]) - float(d_p0[slots[s]])) for s in range(cap)])
    delta32 = np.array([(new32[1][s] - new32[0][s]) - (d_n0[slots[s]] - d_p0[slots[s]]) for s in range(cap)], F32)
    for with_emb in (True, False):
        ediff = max(float(np.abs(e_ref[t * cap:(t + 1) * cap] - emb[t][slots]).max()) for t in range(3)) if with_emb else 0.0
        emax = float(np.abs(e_ref).max()) if with_emb else 0.0
        ep = [b.p() for b in bemb] if with_emb else [None] * 3
        for fused in (False, True):
            name = ("fused" if fused else "probe") + ("+emb" if with_emb else "")
            err = out(be, 5 if fused else 4)
            if fused:
                dp, dn = out(be, N), out(be, N)
                be.call("ds_refine_distances_fused_f32", be_ref.p(), bsl.p(), bcount.p(), cap, dp.p(), dn.p(), b0p.p(), b0n.p(), *ep, N, D, err.p())
            else:
                dp, dn = inp(be, d_p0), inp(be, d_n0)
                be.call("ds_refine_distances_probe_f32", be_ref.p(), bsl.p(), bcount.p(), cap, dp.p(), dn.p(), b0p.p(), b0n.p(), *ep, D, err.p())
            check_patch(name, dp.get("d_p"), dn.get("d_n"), cap)
            eh = err.get("err")
            absdiff = lambda a, b: abs(float(a) - float(b))                                      # noqa: E731
            hold(tag + " " + name, "err[0]", eh[0], np.abs(delta).max(), np.abs(delta32).max(), 1e-5 * max(1.0, np.abs(delta).max()), absdiff)
            assert eh[1] == cap and float(eh[2]) == F32(ediff) and float(eh[3]) == F32(emax), (name, eh, ediff, emax)
            if fused:
                assert eh[4] == count, "err[4] = the near-tie count"
            assert same_bits(b0p.get(), d_p0) and same_bits(b0n.get(), d_n0), "the before distances are inputs"
    # refusals, before any launch: before == after, and only some of the three embedding tables
    dp, dn, err = inp(be, d_p0), inp(be, d_n0), out(be, 5)
    e3 = [b.p() for b in bemb]
    assert be.rc("ds_refine_distances_probe_f32", be_ref.p(), bsl.p(), bcount.p(), cap, dp.p(), dn.p(), dp.p(), b0n.p(), *e3, D, err.p()) == LC.DS_ERR_UNSUPPORTED
    assert be.rc("ds_refine_distances_fused_f32", be_ref.p(), bsl.p(), bcount.p(), cap, dp.p(), dn.p(), b0p.p(), dn.p(), *e3, N, D, err.p()) == LC.DS_ERR_UNSUPPORTED
    assert be.rc("ds_refine_distances_probe_f32", be_ref.p(), bsl.p(), bcount.p(), cap, dp.p(), dn.p(), b0p.p(), b0n.p(), e3[0], None, e3[2], D, err.p()) == LC.DS_ERR_NULL
    assert be.rc("ds_refine_distances_fused_f32", be_ref.p(), bsl.p(), bcount.p(), cap, dp.p(), dn.p(), b0p.p(), b0n.p(), None, e3[1], None, N, D, err.p()) == LC.DS_ERR_NULL
    assert same_bits(dp.get(), d_p0) and same_bits(dn.get(), d_n0) and np.isnan(err.get()).all(), "a refused call launches nothing"


# ---------------------------------------------------------------------------------------------------------------------
# semi-hard search
# ---------------------------------------------------------------------------------------------------------------------
def _mine(be, anchor, d_p, alab, cand, clab, want_rc=0):
    N, D, M = anchor.shape[0], anchor.shape[1], cand.shape[0]
    ws_n = int(be.plain("ds_mine_workspace_floats", N, M))
    assert ws_n == -(-M // 256) * N * 4
    bufs = [inp(be, v) for v in (anchor, d_p, alab, cand, clab)]
    ws, oi, od = out(be, ws_n), out(be, N, np.int64), out(be, N)
    rc = be.rc("ds_mine_semihard_f32", bufs[0].p(), bufs[1].p(), bufs[2].p(), bufs[3].p(), bufs[4].p(), ws.p(), oi.p(), od.p(), N, M, D)
    assert rc == want_rc, (rc, want_rc)
    ws.get("workspace")
    return oi.get("out_index"), od.get("out_dist")


def body_mine(be, N, M, D, cls):
    A = LC.mine_anchors_per_group(N, M, D, be.cus)
    a256 = LC.mine_anchors_per_group(N, M, D, 256)
    want = {"lds4": 4, "lds2": 2}.get(cls, cls)
    print(f"mine N={N} M={M} D={D}: anchors per workgroup {A} with {be.cus} compute units (256 units: {a256}, class {cls})")
    assert a256 == want, "the table's class holds on a 256-unit device"
    if be.cus == 256:
        assert A == want
    if cls in ("lds4", "lds2"):
        assert LC.mine_anchors_per_group(N, M, 64, 256) == 8, "the LDS budget, not the grid, reduces the anchors"
    anchor, cand, alab, clab, d_p, d64 = LC.mine_inputs(N, M, D, N + 3 * M + D)
    d32 = LC.mine_dist(anchor, cand, F32)
    restated = float((np.abs(d32 - d64) / d64).max())
    gap = bar_from_restatement(LC.FLOOR_MINE_DIST, restated)
    win, wd, accept = LC.mine_ref(d64, d_p, alab, clab, gap)
    escapes = sum(a is not None for a in accept)
    print(f"mine N={N} M={M} D={D}: f32-restated distance error {restated:.2e}, gap {gap:.2e}, anchors on the escape {escapes} of {N}")
    assert escapes <= LC.MINE_ESCAPE_CAP * N or escapes <= 1 and N < 50, "input condition (float64 only): at most 2 % ambiguous anchors"
    oi, od = _mine(be, anchor, d_p, alab, cand, clab)
    oi2, od2 = _mine(be, anchor, d_p, alab, cand, clab)
    assert (oi == oi2).all() and same_bits(od, od2), "two runs are bit-identical"
    worst = 0.0
    for i in range(N):
        if accept[i] is None:
            assert oi[i] == win[i], (i, oi[i], win[i])
        else:
            assert int(oi[i]) in accept[i], (i, oi[i], accept[i])
        ref_d = d64[i, oi[i]] if oi[i] >= 0 else 0.0
        worst = max(worst, abs(float(od[i]) - ref_d) / max(ref_d, 1e-30) if oi[i] >= 0 else abs(float(od[i])))
    say(f"mine N={N} M={M} D={D}", "out_dist", restated, gap, worst)
    assert worst <= gap


def body_mine_planted(be, plant):
    """small-integer coordinates: every squared distance is an exact f32 integer below 2^24, distinct sums are at least 1
    apart (their roots many ulps), so the oracle's f32 search IS the definition and the index must match exactly"""
    rs = np.random.RandomState(len(plant) * 13)
    N, D = 9, 64
    M = 600 if plant in ("dup_across_tiles", "no_semihard") else 200
    anchor = rs.randint(-2, 3, (N, D)).astype(F32)
    cand = rs.randint(-2, 3, (M, D)).astype(F32)
    alab, clab = rs.randint(0, 4, N).astype(np.int64), rs.randint(0, 4, M).astype(np.int64)
    sq = ((anchor[:, None, :].astype(F64) - cand[None].astype(F64)) ** 2).sum(2)
    d_p = np.sqrt(np.floor(np.median(sq, axis=1)) + 0.5).astype(F32)    # between two integers: no distance equals d_p
    if plant == "same_label":
        alab[:] = 2
        clab[:] = 2
    elif plant == "no_semihard":
        d_p[:] = 1e3
    elif plant in ("dup_in_tile", "dup_across_tiles"):
        for i in range(N):                                             # the winner's row again, later in the list
            ok = clab != alab[i]
            semi = ok & (sq[i] + 1e-4 / D > float(d_p[i]) ** 2)
            j = int(np.argmin(np.where(semi, sq[i], np.inf)))
            j2 = j + 256 if plant == "dup_across_tiles" else (j + 3 + i) % 200
            if j2 < M and clab[j2] != alab[i] and j2 > j:
                cand[j2] = cand[j]
        sq = ((anchor[:, None, :].astype(F64) - cand[None].astype(F64)) ** 2).sum(2)
    elif plant == "equals_positive":
        pass
    want = O.mine_semihard(anchor, d_p, alab, cand, clab)
    if plant == "equals_positive":
        # candidate 5 is the positive itself, d_p comes from ds_pairwise_distance_f32: a lane-strided sum, where the search
        # adds the dimensions in sequence.  The header promises no equality of the two roundings (on these integers both are
        # exact, elsewhere they need not be), so only this is asserted: the answer is the search's with candidate 5 taken as
        # semi-hard or as not semi-hard.
        pos = np.repeat(cand[5][None], N, 0)
        bufs = inp(be, anchor), inp(be, pos)
        dd = out(be, N)
        be.call("ds_pairwise_distance_f32", bufs[0].p(), bufs[1].p(), dd.p(), N, D)
        d_p = dd.get()
        lo, hi = O.mine_semihard(anchor, np.nextafter(d_p, F32(0)), alab, cand, clab), O.mine_semihard(anchor, np.nextafter(d_p, F32(1e9)), alab, cand, clab)
        oi, od = _mine(be, anchor, d_p, alab, cand, clab)
        assert all(oi[i] in (lo[i], hi[i]) for i in range(N)), (oi, lo, hi)
        return
    oi, od = _mine(be, anchor, d_p, alab, cand, clab)
    print(f"mine planted {plant}: indices {oi.tolist()}")
    assert (oi == want).all(), (plant, oi, want)
    if plant == "same_label":
        assert (oi == -1).all() and (od == 0).all(), "every candidate shares the label: index -1, distance 0"
    else:
        refd = np.sqrt(sq[np.arange(N), want] + 1e-4 / D)
        assert max_rel(od, refd) <= LC.FLOOR_MINE_DIST
    if plant.startswith("dup"):
        dups = sum(int((sq[i] == sq[i, want[i]]).sum() > 1) for i in range(N))
        assert dups >= N // 2, "the plant: most winners have a bit-identical later twin"


def body_mine_refused(be):
    """a row the LDS budget cannot hold is refused by return code, before any launch: the outputs keep their fill"""
    for D in (LC.MINE_MAX_D + 4, 4096, 8192):
        N, M = 2, 3
        anchor, cand = np.zeros((N, D), F32), np.zeros((M, D), F32)
        oi, od = _mine(be, anchor, np.ones(N, F32), np.zeros(N, np.int64), cand, np.ones(M, np.int64), LC.DS_ERR_BAD_SHAPE)
        assert (oi == SENTINEL).all() and np.isnan(od).all()


# ---------------------------------------------------------------------------------------------------------------------
# row movers
# ---------------------------------------------------------------------------------------------------------------------
def body_movers(be, N, M, D):
    rs = np.random.RandomState(N + M + D)
    src = [rs.randn(M, D).astype(F32) for _ in range(3)]
    idx = rs.randint(0, M, N).astype(np.int64)
    idx[0] = -1                             # a negative index gathers zeros
    if N > 2:
        idx[2] = idx[1]                     # a repeated row
    want = [np.where(idx[:, None] >= 0, s[np.maximum(idx, 0)], F32(0)) for s in src]
    bs, bi = [inp(be, s) for s in src], inp(be, idx)
    dst = out(be, (N, D))
    be.call("ds_gather_rows_f32", bs[0].p(), bi.p(), dst.p(), N, D)
    assert same_bits(dst.get("gather"), want[0])
    dst3 = out(be, (3, N, D))
    be.call("ds_gather_rows3_f32", bs[0].p(), bs[1].p(), bs[2].p(), bi.p(), dst3.p(), N, D)
    assert same_bits(dst3.get("gather3"), np.stack(want))
    # the adjoint: destination rows hit twice, once and never; rows past M and negative indices contribute nothing
    g = rs.randn(N, D).astype(F32)
    sidx = rs.randint(0, M, N).astype(np.int64)
    sidx[N - 1] = sidx[0]
    if N > 3:
        sidx[1] = -1
    absent = np.setdiff1d(np.arange(M), sidx)
    assert len(absent) > 0 or M <= N
    bg, bsi = inp(be, g), inp(be, sidx)
    dst0 = rs.randn(M, D).astype(F32)
    for accumulate in (0, 1):
        dst = Buf(be, (M, D), F32, data=dst0) if accumulate else out(be, (M, D))
        be.call("ds_scatter_add_rows_f32", bg.p(), bsi.p(), dst.p(), N, M, D, accumulate)
        got = dst.get("scatter")
        assert same_bits(got, LC.scatter_add_ref(g, sidx, dst0, M, accumulate)), "the sequential f32 sum over ascending i, bit for bit"
        if not accumulate and len(absent):
            assert (got[absent] == 0).all()
    print(f"movers N={N} M={M} D={D}: bit-exact (parts = {8 if D >= 4096 else 1})")


# ---------------------------------------------------------------------------------------------------------------------
# pools
# ---------------------------------------------------------------------------------------------------------------------
def body_pools(be, B, Hr, Wc, C):
    tag = f"pool B={B} Hr={Hr} Wc={Wc} C={C}"
    K = Wc * C
    print(f"{tag}: {B * K // 4} output vectors ({2048 * 256} = the forward grid cap), {B * Hr * K // 4} backward ({4096 * 256})")
    rs = np.random.RandomState(B + Hr + K)
    x = (rs.rand(B, Hr, K) * 25 - 2).astype(F32)
    bx, pooled = inp(be, x), out(be, (B, K))
    be.call("ds_avgpool_time_f32", bx.p(), pooled.p(), B, Hr, Wc, C)
    hold(tag, "mean over time", pooled.get("pooled"), LC.pool_ref(x), LC.pool_ref(x, None, F32), LC.FLOOR)
    # masked: rows at or past lens are NaN -- never read by the pool, zeroed by the mask
    lens = np.array([{"Hr": Hr, "Hr+5": Hr + 5}.get(v, v) for v in LC.POOL_LENS] * (B // len(LC.POOL_LENS) + 1), np.int32)[:B]
    rs.shuffle(lens)
    keep = np.clip(lens, 0, Hr)
    xm = x.copy()
    for b in range(B):
        xm[b, keep[b]:] = np.nan
    bxm, bl, pooled = inp(be, xm), inp(be, lens), out(be, (B, K))
    be.call("ds_avgpool_time_masked_f32", bxm.p(), bl.p(), pooled.p(), B, Hr, Wc, C)
    hold(tag, "masked mean", pooled.get("pooled"), LC.pool_ref(xm, lens), LC.pool_ref(xm, lens, F32), LC.FLOOR)
    be.call("ds_mask_rows", bxm.p(), bl.p(), B, Hr, K * 4)
    got = bxm.get("masked")
    for b in range(B):
        assert same_bits(got[b, :keep[b]], x[b, :keep[b]]) and (bits(got[b, keep[b]:]) == 0).all(), (tag, b, "kept rows bit-identical, the rest +0")
    # backward of clip -> mean: activations exactly 0 and exactly 20 pass nothing
    act = np.clip(x, 0, LC.CLIP_MAX)
    act.reshape(-1)[::7] = 0.0
    act.reshape(-1)[3::11] = LC.CLIP_MAX
    gp = rs.randn(B, K).astype(F32)
    ba, bg, gx = inp(be, act), inp(be, gp), out(be, (B, Hr, K))
    be.call("ds_avgpool_time_bwd_f32", bg.p(), ba.p(), gx.p(), B, Hr, Wc, C)
    gh = gx.get("gx")
    hold(tag, "pool bwd", gh, LC.pool_bwd_ref(gp, act), LC.pool_bwd_ref(gp, act, F32), LC.FLOOR)
    assert (gh[(act == 0) | (act == LC.CLIP_MAX)] == 0).all()


def body_mask_rows(be, row_bytes):
    B, H = 7, 6
    lens = np.array([-3, 0, 1, H, H + 5, 3, 5], np.int32)
    keep = np.clip(lens, 0, H)
    rs = np.random.RandomState(row_bytes)
    x = rs.randn(B, H, row_bytes // 4).astype(F32)
    xm = x.copy()
    for b in range(B):
        xm[b, keep[b]:] = np.nan
    bx, bl = inp(be, xm), inp(be, lens)
    be.call("ds_mask_rows", bx.p(), bl.p(), B, H, row_bytes)
    got = bx.get("masked")
    for b in range(B):
        assert same_bits(got[b, :keep[b]], x[b, :keep[b]]) and (bits(got[b, keep[b]:]) == 0).all(), (row_bytes, b)


def body_max_abs_diff(be, n):
    rs = np.random.RandomState(n % 9973)
    a, b = rs.randn(n).astype(F32), rs.randn(n).astype(F32)
    a[n - 1], b[n // 2] = 9.5, -7.25         # the maxima sit on the last element and in the middle
    ba, bb, o = inp(be, a), inp(be, b), out(be, 2)
    be.call("ds_max_abs_diff_f32", ba.p(), bb.p(), n, o.p())
    got = o.get("out2")
    assert got[0] == np.abs(a - b).max() and got[1] == np.abs(b).max(), "the maxima are exact"
    for which, val, pos in (("a", np.nan, n - 1), ("b", np.nan, 0), ("a", np.inf, n // 3), ("b", -np.inf, n - 1)):
        a2, b2 = a.copy(), b.copy()
        (a2 if which == "a" else b2)[pos] = val
        ba, bb, o = inp(be, a2), inp(be, b2), out(be, 2)
        be.call("ds_max_abs_diff_f32", ba.p(), bb.p(), n, o.p())
        assert o.get("out2")[0] == np.inf, (n, which, val, "a non-finite operand makes out[0] +inf")


# ---------------------------------------------------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------------------------------------------------
def body_ce(be, M, n_cls, pad, spread):
    tag = f"ce M={M} n_cls={n_cls} pad={pad} spread={spread:g}"
    ld = -(-n_cls // 128) * 128 if pad else n_cls
    ld_out = ld + 4 if pad else n_cls + 3
    logits, labels = LC.ce_inputs(M, n_cls, spread, M + n_cls)
    assert labels[0] in (0, n_cls - 1) and labels[M - 1] == n_cls - 1
    lp = np.full((M, ld), np.nan, F32)          # the pad columns are not read
    lp[:, :n_cls] = logits
    bl, blab = inp(be, lp), inp(be, labels)
    row, lse, loss = out(be, M), out(be, M), out(be, 1)
    be.call("ds_cross_entropy_fwd_f32", bl.p(), blab.p(), row.p(), lse.p(), loss.p(), M, n_cls, ld)
    r64, r32 = LC.ce_ref(logits, labels), LC.ce_ref(logits, labels, F32)
    lseh = lse.get("lse")
    hold(tag, "lse", lseh, r64[0], r32[0], LC.FLOOR_CE)
    absmax = lambda a, b: float(np.abs(np.asarray(a, F64) - np.asarray(b, F64)).max() / max(1.0, np.abs(r64[0]).max()))   # noqa: E731
    hold(tag, "row_loss", row.get("row_loss"), r64[1], r32[1], LC.FLOOR_CE, absmax)      # lse - logit: an error of the size of lse
    hold(tag, "loss", loss.get("loss"), [r64[2]], [r32[2]], LC.FLOOR_CE, absmax)
    gl = np.array([0.8], F32)
    bgl, blse, dl = inp(be, gl), inp(be, lseh), out(be, (M, ld_out))
    be.call("ds_cross_entropy_bwd_f32", bl.p(), blab.p(), blse.p(), bgl.p(), dl.p(), M, n_cls, ld, ld_out)
    dh = dl.get("dlogits")
    assert (bits(dh[:, n_cls:]) == 0).all(), "the pad columns of dlogits are exactly 0"
    g64, g32 = LC.ce_bwd_ref(logits, labels, lseh, gl[0]), LC.ce_bwd_ref(logits, labels, lseh, gl[0], F32)
    scale = float(gl[0]) / M
    absg = lambda a, b: float(np.abs(np.asarray(a, F64) - np.asarray(b, F64)).max() / scale)      # noqa: E731
    # exp(x - lse) carries the rounding of the difference: |x - lse| ulps of f32, the restatement's own error
    restated = absg(g32, g64)
    bar = bar_from_restatement(LC.FLOOR_CE, restated)
    err = absg(dh[:, :n_cls], g64)
    say(tag, "dlogits / (gloss / M)", restated, bar, err)
    assert err <= bar
    rowsum = float(np.abs(dh[:, :n_cls].astype(F64).sum(1)).max() / scale)
    rowsum_ref = float(np.abs(g32.astype(F64).sum(1) - g64.sum(1)).max() / scale)
    bar_s = bar_from_restatement(LC.FLOOR_CE * n_cls ** 0.5, rowsum_ref + abs(float(np.abs(g64.sum(1)).max() / scale)))
    say(tag, "rows of dlogits sum to 0", rowsum_ref, bar_s, rowsum)
    assert rowsum <= bar_s


# ---------------------------------------------------------------------------------------------------------------------
# head
# ---------------------------------------------------------------------------------------------------------------------
def _pack_fc(be, w, C):
    N, K = w.shape
    bw, wp = inp(be, w), out(be, N * K)
    be.call("ds_pack_fc_weight_f32", bw.p(), wp.p(), N, C, K // C)
    got = wp.get("w_packed")
    want = w[:, LC.fc_feature_order(K, C)].reshape(N, K // 8, 8).transpose(1, 0, 2).reshape(-1)     # [K/8][N][8]
    assert same_bits(got, want), "the packing is an exact permutation"
    return wp


def body_fc(be, B, K, N, with_bias, with_e):
    tag = f"fc B={B} K={K} N={N} bias={with_bias} e={with_e}"
    S = LC.fc_splits(K)
    assert S == LC.FC_EXPECTED_S[K]
    ws_n = int(be.plain("ds_fc_workspace_floats", B, K, N))
    print(f"{tag}: S={S}, workspace {ws_n} floats")
    assert ws_n == S * B * N
    rs = np.random.RandomState(B + K + N)
    C = 8 if K % 16 == 0 else 4
    x, w = rs.randn(B, K).astype(F32), (rs.randn(N, K) / np.sqrt(K)).astype(F32)
    bias = (rs.randn(N) * 0.1).astype(F32) if with_bias else None
    alpha, eps = 10.0, 1e-10
    wp, bx, bb = _pack_fc(be, w, C), inp(be, x), (inp(be, bias) if with_bias else None)
    runs = []
    for _ in range(2):
        ws, f, e = out(be, ws_n), out(be, (B, N)), out(be, (B, N))
        be.call("ds_fc_l2norm_fwd_f32", bx.p(), wp.p(), bb.p() if bb else None, ws.p(), f.p(), e.p() if with_e else None, B, K, N, alpha, eps)
        wsh = ws.get("workspace")
        assert np.isfinite(wsh).all(), "S * B * N partials, all written"
        runs.append((f.get("f"), e.get("e")))
    assert same_bits(runs[0][0], runs[1][0]) and (not with_e or same_bits(runs[0][1], runs[1][1])), "two runs are bit-identical"
    f64, f32 = LC.fc_ref(x, w, bias, C), LC.fc_ref(x, w, bias, C, F32)
    hold(tag, "f", runs[0][0], f64, f32, LC.FLOOR_FC, max_rel)
    if with_e:
        hold(tag, "e", runs[0][1], LC.l2norm(f64, alpha, eps), LC.l2norm(f32, alpha, eps, F32), LC.FLOOR_FC, max_rel)
    else:
        assert np.isnan(runs[0][1]).all(), "e == NULL: nothing but f is written"


def body_fc_ce(be, M, K, N, n_cls, shift):
    tag = f"fc_ce M={M} K={K} N={N} n_cls={n_cls} shift={shift:g}"
    rs = np.random.RandomState(M + K + n_cls)
    C = 8
    x = rs.randn(M, K).astype(F32)
    w = np.zeros((N, K), F32)               # the pad classes carry zero filter rows
    w[:n_cls] = (rs.randn(n_cls, K) * (3.0 / np.sqrt(K))).astype(F32)
    bias = np.zeros(N, F32)
    bias[:n_cls] = (rs.randn(n_cls) * 0.1 + shift).astype(F32)
    labels = rs.randint(0, n_cls, M).astype(np.int64)
    labels[0], labels[M - 1] = 0, n_cls - 1
    wp, bx, bb, blab = _pack_fc(be, w, C), inp(be, x), inp(be, bias), inp(be, labels)
    ws = out(be, int(be.plain("ds_fc_workspace_floats", M, K, N)))
    logits, row, lse, loss = out(be, (M, N)), out(be, M), out(be, M), out(be, 1)
    be.call("ds_fc_ce_fwd_f32", bx.p(), wp.p(), bb.p(), ws.p(), logits.p(), blab.p(), row.p(), lse.p(), loss.p(), M, K, N, n_cls)
    lh = logits.get("logits")
    hold(tag, "logits", lh, LC.fc_ref(x, w, bias, C), LC.fc_ref(x, w, bias, C, F32), LC.FLOOR_FC, max_rel)
    # the epilogue against the stand-alone kernel and against float64, both ON THE SAME (returned) logits
    row2, lse2, loss2 = out(be, M), out(be, M), out(be, 1)
    be.call("ds_cross_entropy_fwd_f32", logits.p(), blab.p(), row2.p(), lse2.p(), loss2.p(), M, n_cls, N)
    r64, r32 = LC.ce_ref(lh[:, :n_cls], labels), LC.ce_ref(lh[:, :n_cls], labels, F32)
    top = max(1.0, float(np.abs(r64[0]).max()))
    absmax = lambda a, b: float(np.abs(np.asarray(a, F64) - np.asarray(b, F64)).max() / top)      # noqa: E731
    for name, got, other, k in (("lse", lse, lse2, 0), ("row_loss", row, row2, 1), ("loss", loss, loss2, 2)):
        g, o2 = got.get(name), other.get(name)
        hold(tag, name, g, np.atleast_1d(r64[k]), np.atleast_1d(r32[k]), LC.FLOOR_CE, absmax)
        both = absmax(g, o2)
        print(f"{tag}: {name} fused against ds_cross_entropy_fwd_f32 {both:.2e} ({'bit-identical' if same_bits(g, o2) else 'not bit-identical'})")
        assert both <= 2 * bar_from_restatement(LC.FLOOR_CE, absmax(np.atleast_1d(r32[k]), np.atleast_1d(r64[k])))


def body_tail_small(be, B, Hr, K, N):
    tag = f"tail_small B={B} Hr={Hr} K={K} N={N}"
    rs = np.random.RandomState(B + Hr + K + N)
    C = 4
    a, w = (rs.rand(B, Hr, K) * 3).astype(F32), (rs.randn(N, K) / np.sqrt(K)).astype(F32)
    bias = (rs.randn(N) * 0.1).astype(F32)
    alpha, eps = 10.0, 1e-10
    bw, wr = inp(be, w), out(be, (N, K))
    be.call("ds_pack_fc_weight_rows_f32", bw.p(), wr.p(), N, C, K // C)
    assert same_bits(wr.get("w_rows"), w[:, LC.fc_feature_order(K, C)]), "the packing is an exact permutation"
    ba, bb = inp(be, a), inp(be, bias)
    for with_bias in (True, False):
        f, e = out(be, (B, N)), out(be, (B, N))
        be.call("ds_tail_small_f32", ba.p(), wr.p(), bb.p() if with_bias else None, f.p(), e.p(), B, Hr, K, N, alpha, eps)
        bv = bias if with_bias else None
        f64, f32 = LC.fc_ref(LC.pool_ref(a), w, bv, C), LC.fc_ref(LC.pool_ref(a, None, F32), w, bv, C, F32)
        hold(tag, f"f (bias={with_bias})", f.get("f"), f64, f32, LC.FLOOR_FC, max_rel)
        hold(tag, f"e (bias={with_bias})", e.get("e"), LC.l2norm(f64, alpha, eps), LC.l2norm(f32, alpha, eps, F32), LC.FLOOR_FC, max_rel)


def body_tail_small_refused(be):
    """more than DS_TAIL_SMALL_MAX_B utterances, and a pooled vector that does not fit 64 KiB of LDS: refused before any launch"""
    K, N = 100, 8
    ba, bw, f, e = inp(be, np.zeros((5, 1, K), F32)), inp(be, np.zeros((N, K), F32)), out(be, (5, N)), out(be, (5, N))
    assert be.rc("ds_tail_small_f32", ba.p(), bw.p(), None, f.p(), e.p(), 5, 1, K, N, 10.0, 1e-10) == LC.DS_ERR_BAD_SHAPE
    assert be.rc("ds_tail_small_f32", ba.p(), bw.p(), None, f.p(), e.p(), 1, 1, 16388, N, 10.0, 1e-10) == LC.DS_ERR_BAD_SHAPE
    assert be.rc("ds_tail_small_f32", ba.p(), bw.p(), None, f.p(), e.p(), 4, 1, K, N, 10.0, 1e-10) == 0
    fh = f.get("f")
    assert (fh[:4] == 0).all() and np.isnan(fh[4:]).all() and np.isnan(e.get("e")[4:]).all()


# ---------------------------------------------------------------------------------------------------------------------
# scoring
# ---------------------------------------------------------------------------------------------------------------------
def body_group_mean(be, n_groups, G):
    tag = f"group_mean n={n_groups} G={G}"
    rs = np.random.RandomState(n_groups + G)
    x = (rs.rand(n_groups, G) * 3).astype(F32)
    bx, o = inp(be, x), out(be, n_groups)
    be.call("ds_group_mean_f32", bx.p(), o.p(), n_groups, G)
    hold(tag, "group mean", o.get("out"), x.astype(F64).mean(1), x.sum(1, dtype=F32) / F32(G), LC.FLOOR, max_rel)
    # segments of different sizes over the same numbers; some are empty (mean 0), one holds everything past the middle
    flat = x.reshape(-1)
    cuts = np.sort(rs.randint(0, flat.size + 1, n_groups - 1)) if n_groups > 1 else np.zeros(0, np.int64)
    off = np.concatenate([[0], cuts, [flat.size]]).astype(np.int64)
    if n_groups > 4:
        off[2] = off[1]                     # an empty segment
    want64 = np.array([flat[a:b].astype(F64).mean() if b > a else 0.0 for a, b in zip(off[:-1], off[1:])])
    want32 = np.array([flat[a:b].sum(dtype=F32) / F32(b - a) if b > a else 0.0 for a, b in zip(off[:-1], off[1:])], F32)
    bf, bo, o = inp(be, flat), inp(be, off), out(be, n_groups)
    be.call("ds_segment_mean_f32", bf.p(), bo.p(), o.p(), n_groups)
    got = o.get("out")
    hold(tag, "segment mean", got, want64, want32, LC.FLOOR, max_rel)
    assert (got[np.diff(off) == 0] == 0).all(), "an empty segment gives 0"


def body_assemble_crops(be):
    rs = np.random.RandomState(5)
    F, T, rows = 64, 20, 300
    feat = rs.randn(rows, F).astype(F32)
    # crops inside an utterance, running past its end (zero padded), starting AT its end (all zero), ending at the corpus end
    start = np.array([0, 50, 95, 100, 290, 300, 7], np.int64)
    end = np.array([100, 100, 100, 100, 300, 300, 8], np.int64)
    B = len(start)
    want = np.zeros((B, T, F), F32)
    for b in range(B):
        n = int(np.clip(end[b] - start[b], 0, T))
        want[b, :n] = feat[start[b]:start[b] + n]
    bf, bs, be_, o = inp(be, feat), inp(be, start), inp(be, end), out(be, (B, T, F))
    be.call("ds_assemble_crops_f32", bf.p(), bs.p(), be_.p(), o.p(), B, T, F)
    assert same_bits(o.get("crops"), want), "crops are moves: bit-exact, zero (+0) past the utterance end"


def body_roc(be, N, n_thr, grid, labels):
    tag = f"roc N={N} n_thr={n_thr} {grid} {labels}"
    thr0, dthr, thr = LC.roc_thresholds(grid, n_thr)
    dist, same = LC.roc_inputs(N, n_thr, grid, labels, N + n_thr)
    if grid == "ref":
        clear = LC.roc_clearance_ulps(dist, grid, n_thr)
        print(f"{tag}: distances keep {clear:.1f} f32 ulps from every threshold")
        assert clear >= LC.ROC_ULPS, "input condition"
    else:
        assert (thr.astype(F32).astype(F64) == thr).all() and (np.isin(dist, thr.astype(F32)).any() or N < 3)
    n_same, n_diff = int(same.sum()), int(N - same.sum())
    assert {"same": n_diff == 0, "diff": n_same == 0}.get(labels, True)
    bd, bs = inp(be, dist), inp(be, same)
    tp, fp, summ = out(be, n_thr, np.int32), out(be, n_thr, np.int32), out(be, 6)
    be.call("ds_roc_sweep_f32", bd.p(), bs.p(), N, thr0, dthr, n_thr, n_same, n_diff, tp.p(), fp.p(), summ.p())
    tph, fph, sh = tp.get("tp"), fp.get("fp"), summ.get("summary6")
    d64 = dist.astype(F64)                                  # the float64 sweep: dist < threshold, strict (eval_metrics.py:41)
    order = np.sort(d64[same != 0]), np.sort(d64[same == 0])
    want_tp, want_fp = np.searchsorted(order[0], thr, "left"), np.searchsorted(order[1], thr, "left")
    assert (tph == want_tp).all() and (fph == want_fp).all(), (tag, "tp / fp equal the float64 sweep exactly")
    if N <= 1100 and n_thr <= 300:                           # the oracle's own sweep agrees (it walks every pair: small cases)
        otp, ofp = O.roc_sweep(dist, same, thr)[:2]
        assert (otp == want_tp).all() and (ofp == want_fp).all()
    ref = LC.roc_summary_ref(tph, fph, n_same, n_diff, N, thr0, dthr)
    err = float(np.abs(sh.astype(F64)[1:] - ref[1:]).max())
    print(f"{tag}: summary6 {sh.tolist()} against float64 from the returned counts: {err:.2e} (bar 1e-6 + 1e-6 |.|)")
    # equal accuracies give the first index; the kernel compares f32 quotients, float64 ties are f32 ties
    acc32 = ((tph + (n_diff - fph)).astype(F32) / F32(N))
    assert int(sh[0]) == int(np.argmax(acc32)) and acc32[int(sh[0])] == acc32.max()
    if int(sh[0]) != int(ref[0]):
        assert abs(acc32[int(ref[0])] - acc32.max()) <= 1e-6
        ref[1:3] = [tph[int(sh[0])] / n_same if n_same else 0.0, fph[int(sh[0])] / n_diff if n_diff else 0.0]
    assert np.all(np.abs(sh.astype(F64)[1:] - ref[1:]) <= 1e-6 + 1e-6 * np.abs(ref[1:])), (sh, ref)
