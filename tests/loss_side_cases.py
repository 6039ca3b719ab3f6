"""Float64 references, float32 restatements and case tables of the kernels around the convolution stack: the loss side
(tail_loss.hip), the projection head (fc_mfma_f32.hip) and verification scoring (scoring.hip).  Shared by the emulator
suite (test_emul_loss_side.py) and the device suite (test_gpu_loss_side_kernels.py) through loss_side_bodies.py.
A plain helper module: host arrays in, host arrays out; no GPU, no emulator, no fixtures.

Every reference is written from the operation's definition in include/deepspeaker_hip.h (and the reference lines cited
there), takes `dtype`: np.float64 is the reference, np.float32 the plain restatement whose distance from the reference
sizes the bar (train_f16_cases.bar_from_restatement: max(floor, 4 x that distance), never the kernel's own output).
The floors are the emulator suite's bars for the same kernel (test_emul_kernels.py / test_emul_engine.py), 1e-6 where it
has none.

Case tables: a trailing "gpu" marks a case only the device runs (too long for the host emulator, or dependent on the
compute-unit count); the emulator suite runs every other one."""
import numpy as np

import deepspeaker_oracle as O
from train_f16_cases import bar_from_restatement, rel_l2  # noqa: F401  (re-exported: one definition for both suites)

F32, F64 = np.float32, np.float64
FLOOR = 1e-6                    # where the emulator suite has no bar of its own
FLOOR_DIST = 1e-6               # test_emul_engine.test_loss_side: distances, loss, mean difference
FLOOR_PNORM, FLOOR_PNORM_BWD = 2e-6, 5e-6      # test_emul_kernels.test_pairwise_distance_any_norm
FLOOR_MINE_DIST = 2e-6          # test_emul_kernels.test_mine_semihard_shapes_and_ties
FLOOR_FC = 2e-6                 # test_emul_engine.test_small_batch_tail_equals_the_three_launch_tail
FLOOR_CE = 1e-6                 # test_emul_engine.test_classifier_head_and_cross_entropy
DS_ERR_BAD_SHAPE, DS_ERR_NULL, DS_ERR_UNSUPPORTED = -1, -3, -4
MINE_MAX_D = 3584               # DS_MINE_MAX_D: 2 anchors x D floats next to the 36 KiB candidate tile in 64 KiB of LDS


def emul_cases(table):
    return [c for c in table if c[-1] != "gpu"]


def max_rel(got, ref):
    """largest |got - ref| / max |ref| (the emulator suite's rel_err); inf if got holds a non-finite value ref does not"""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    if got.shape != ref.shape or not np.isfinite(got[np.isfinite(ref)]).all():
        return float("inf")
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)) if got.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# row kernels
# ---------------------------------------------------------------------------------------------------------------------
def l2norm(f, alpha, eps, dtype=F64):
    f = f.astype(dtype)
    return dtype(alpha) * f / np.sqrt((f * f).sum(1, dtype=dtype) + dtype(eps))[:, None]


def l2norm_bwd(f, ge, alpha, eps, dtype=F64):
    f, ge = f.astype(dtype), ge.astype(dtype)
    nrm = np.sqrt((f * f).sum(1, dtype=dtype) + dtype(eps))[:, None]
    dot = (f * ge).sum(1, dtype=dtype)[:, None]
    return dtype(alpha) * (ge / nrm - f * dot / (nrm * nrm * nrm))


def pdist(x1, x2, p=2, dtype=F64):
    """PairwiseDistance.forward (model.py:13-18): the oracle's, in `dtype`"""
    return O.pairwise_distance(x1.astype(dtype), x2.astype(dtype), p)


def pdist_bwd(x1, x2, d, gd, p=2, dtype=F64):
    """gradient of pdist with respect to x1 for the distances `d` the kernel is handed: gd d^(1-p) |x1-x2|^(p-1) sign(x1-x2),
    exactly 0 where x1 == x2 (torch.abs' gradient); g2 = -g1"""
    x1, x2, d, gd = (v.astype(dtype) for v in (x1, x2, d, gd))
    if p == 2:
        return O.pairwise_distance_bwd(x1, x2, d, gd)[0]
    df = x1 - x2
    with np.errstate(divide="ignore", invalid="ignore"):
        g = (gd * np.power(d, dtype(1.0 - p)))[:, None] * np.power(np.abs(df), dtype(p - 1.0)) * np.sign(df)
    return np.where(df == 0, dtype(0), g)


def triplet_fwd(a, p, n, margin, dtype=F64):
    """TripletMarginLoss.forward (model.py:27-33) -> (d_p, d_n, loss)"""
    loss, d_p, d_n = O.triplet_margin_loss(a.astype(dtype), p.astype(dtype), n.astype(dtype), margin)
    return d_p, d_n, dtype(np.maximum(dtype(margin) + d_p - d_n, 0).mean(dtype=F64))


def triplet_bwd(a, p, n, d_p, d_n, margin, gloss, dtype=F64):
    """gradient of mean(clamp(margin + d_p - d_n, min=0)) for the distances handed in; the clamp passes gradient at
    exactly 0 (torch.clamp(min=0); oracle triplet_margin_loss_bwd)"""
    a, p, n, d_p, d_n = (v.astype(dtype) for v in (a, p, n, d_p, d_n))
    act = ((dtype(margin) + d_p - d_n) >= 0).astype(dtype) * dtype(gloss) / dtype(a.shape[0])
    ga1, gp = O.pairwise_distance_bwd(a, p, d_p, act)
    ga2, gn = O.pairwise_distance_bwd(a, n, d_n, -act)
    return ga1 + ga2, gp, gn


# (rows, D): every D of {1, 63, 64, 65, 512, 1000} and every row count of {1, 3, 4, 5, 257}, then the model's own shape
ROW_CASES = [(1, 1, ""), (3, 63, ""), (4, 64, ""), (5, 65, ""), (257, 512, ""), (5, 1000, ""), (257, 1, ""), (1, 1000, ""),
             (3, 512, ""), (4, 65, ""), (768, 512, "")]
PNORMS = (0.5, 1.0, 2.0, 3.0)


def row_inputs(rows, D, seed):
    """x1, x2 [rows, D] f32.  Row 0 of x1 is all zero (norm = sqrt(eps)); the LAST row of x2 is bit-identical to x1's
    (d = sqrt(eps), gradient exactly 0).  With one row the two plants fall on the same row: both zero."""
    rs = np.random.RandomState(seed)
    x1, x2 = (rs.randn(rows, D) / np.sqrt(2 * D)).astype(F32), (rs.randn(rows, D) / np.sqrt(2 * D)).astype(F32)     # distances near 1
    x1[0] = 0
    x2[rows - 1] = x1[rows - 1]
    return x1, x2


# ---------------------------------------------------------------------------------------------------------------------
# scan family
# ---------------------------------------------------------------------------------------------------------------------
def scan_ref(d_p, d_n, margin, band):
    """The scan's decisions in float64 ON THE GIVEN f32 numbers (the kernel's own distances): filter d_n - d_p < margin
    (train_triplet.py:253, strict), near ties |d_n - d_p - margin| < band (strict), loss = mean hinge (model.py:30-31),
    mean(d_n - d_p).  Also `flips`: how many decisions the f32 subtraction (one IEEE operation, what the reference's own
    f32 tensors do) takes differently from float64 -- a condition on the inputs the bodies assert to be 0."""
    dp, dn, m = d_p.astype(F64), d_n.astype(F64), float(F32(margin))
    diff = dn - dp
    sel = diff < m
    amb = np.abs(diff - m) < float(F32(band)) if band is not None else np.zeros(len(dp), bool)
    diff32 = d_n.astype(F32) - d_p.astype(F32)
    sel32 = diff32 < F32(margin)
    amb32 = np.abs(diff32 - F32(margin)) < F32(band) if band is not None else amb
    return {"idx": np.where(sel)[0].astype(np.int64), "amb": np.where(amb)[0].astype(np.int64),
            "loss": float(np.maximum(m + dp - dn, 0).mean()), "mean_diff": float(diff.mean()),
            "flips": int((sel != sel32).sum() + (amb != amb32).sum())}


def scan_f32(d_p, d_n, margin):
    """plain f32 restatement of the two means"""
    dp, dn, m = d_p.astype(F32), d_n.astype(F32), F32(margin)
    return float(np.maximum(m + dp - dn, F32(0)).sum(dtype=F32) / F32(len(dp))), float((dn - dp).sum(dtype=F32) / F32(len(dp)))


def amb_slots(amb, cap, probe_base, N):
    """the near-tie list the header promises: the first `cap` near ties in order, then 0 (no probes) or the probe triplets
    (probe_base + k) % N, k = 0, 1, ... in the slots the near ties leave unused"""
    out = np.zeros(cap, np.int64)
    n = min(len(amb), cap)
    out[:n] = amb[:n]
    if probe_base >= 0 and cap > n:
        out[n:] = (probe_base + np.arange(cap - n)) % N
    return out


SCAN_N = (1, 63, 64, 255, 256, 257, 768, 1000)
# (N, filter, amb_cap as a function of N, probe_base: "none" / 0 / "last", near ties: "none" / "few" / "overflow")
SCAN_CASES = []
for _i, _n in enumerate(SCAN_N):
    SCAN_CASES += [(_n, "mix", ("0", "1", "5", "N+7")[_i % 4], ("none", "0", "last")[_i % 3], ("few", "overflow", "none")[_i % 3], ""),
                   (_n, ("nothing", "everything")[_i % 2], ("N+7", "5", "1", "0")[_i % 4], ("last", "none", "0")[_i % 3],
                    ("overflow", "none", "few")[_i % 3], "")]
SCAN_CASES += [(768, "mix", "64", "last", "few", ""), (1000, "mix", "5", "0", "overflow", ""), (257, "mix", "N+7", "last", "overflow", "")]


def scan_inputs(N, filt, near, seed):
    """d_p, d_n f32 [N], margin, band with plants: rows 0.. hold, when N allows, d_n - d_p EXACTLY at margin (not selected:
    strict), one ulp below (selected), |diff - margin| EXACTLY at band (not a near tie), one ulp inside (a near tie)"""
    rs = np.random.RandomState(seed)
    margin = {"mix": 0.25, "nothing": -100.0, "everything": 100.0}[filt]
    band = 2.0 ** -10
    d_p = (1.0 + rs.rand(N) * 0.5).astype(F32)
    gap = rs.rand(N) * 0.5 + 0.01                       # diff - margin, away from the band
    if near == "few":
        k = rs.choice(N, max(1, N // 50), replace=False)
        gap[k] = rs.rand(len(k)) * band * 0.9
    elif near == "overflow":
        k = rs.choice(N, max(1, (N * 2) // 3), replace=False)
        gap[k] = rs.rand(len(k)) * band * 0.9
    sign = np.where(rs.rand(N) < 0.5, -1.0, 1.0)
    d_n = (d_p.astype(F64) + 0.25 + sign * gap).astype(F32)        # the near ties sit around 0.25, the "mix" margin
    plants = [(1.0, 1.25), (1.0, np.nextafter(F32(1.25), F32(0))), (1.0, 1.25 + band), (1.0, np.nextafter(F32(1.25 + band), F32(0))),
              (1.0, 1.25 - band), (1.0, np.nextafter(F32(1.25 - band), F32(2)))]
    if near != "none":
        for i, (a, b) in enumerate(plants[:max(0, min(len(plants), N - 1))]):
            d_p[N - 1 - i], d_n[N - 1 - i] = a, b
    else:
        for i, (a, b) in enumerate(plants[:2][:max(0, N - 1)]):
            d_p[N - 1 - i], d_n[N - 1 - i] = a, b
    return d_p, d_n, margin, band


# ---------------------------------------------------------------------------------------------------------------------
# refinement
# ---------------------------------------------------------------------------------------------------------------------
# (cap, amb_count class, N, D, duplicate a slot, tag)
REFINE_CASES = [(1, "0", 9, 16, False, ""), (3, "lt", 40, 65, True, ""), (4, "eq", 40, 64, False, ""), (6, "gt", 300, 100, True, ""),
                (64, "lt", 768, 512, True, ""), (64, "gt", 256, 512, False, ""), (6, "0", 40, 512, False, ""), (3, "eq", 5, 4, True, "")]


def refine_count(cls, cap):
    return {"0": 0, "lt": max(cap - 2, 1) if cap > 1 else 0, "eq": cap, "gt": cap + 5}[cls]


def refine_ref(e_ref, slots, cap, dtype=F64):
    """distances of the re-embedded slots: (d_p, d_n) [cap] from e_ref rows (s, cap + s, 2 cap + s)"""
    a, p, n = e_ref[:cap], e_ref[cap:2 * cap], e_ref[2 * cap:3 * cap]
    return pdist(a, p, 2, dtype), pdist(a, n, 2, dtype)


# ---------------------------------------------------------------------------------------------------------------------
# semi-hard search
# ---------------------------------------------------------------------------------------------------------------------
def mine_anchors_per_group(N, M, D, cus):
    """the launcher's rule (ds_mine_semihard_f32): 8 anchors per workgroup, halved while the grid would hold fewer workgroups
    than a quarter of the compute units, halved again while the anchor rows do not fit next to the candidate tile"""
    ct = -(-M // 256)
    A = 8
    while A > 2 and -(-N // A) * ct < cus // 4:
        A //= 2
    while A > 2 and (A * D + max(256 * 36, 4 * A * 256)) * 4 > 64 * 1024:
        A //= 2
    return A


def mine_dist(anchor, cand, dtype=F64):
    """[N, M] distances, eps = 1e-4 / D inside the root (model.py:13-18 applied to every pair).  The float32 restatement adds
    the dimensions one after the other, the order the search documents for itself (numpy's pairwise sum would understate
    what any sequential f32 sum of a long row carries)"""
    a, c = anchor.astype(dtype), cand.astype(dtype)
    out = np.empty((a.shape[0], c.shape[0]), dtype)
    eps = dtype(1e-4 / a.shape[1])
    for i in range(a.shape[0]):
        df = a[i][None] - c
        ss = (df * df).sum(1, dtype=dtype) if dtype == F64 else np.cumsum(df * df, axis=1, dtype=dtype)[:, -1]
        out[i] = np.sqrt(ss + eps)
    return out


def mine_ref(d, d_p, alab, clab, gap):
    """float64 winner per anchor of the documented rule (closest other-label candidate farther than d_p, else the closest
    other-label one, lowest index on ties, -1 without any), and per anchor the set of indices a correct f32 search may
    return instead: empty unless the winner is closer than the relative `gap` to the runner-up or an other-label candidate
    lies within `gap` of the d_p boundary ("escape" anchors).  The accepted set then holds every candidate within `gap` of
    the winner of the search with the boundary at d_p (1 - gap), at d_p (1 + gap) or (a semi-hard set that may be empty)
    absent."""
    N, M = d.shape
    win, dist, accept = np.full(N, -1, np.int64), np.zeros(N), [None] * N
    for i in range(N):
        ok = clab != alab[i]
        if not ok.any():
            continue
        di, dp = d[i], float(d_p[i])

        def best(pool):
            dd = np.where(pool, di, np.inf)
            return int(np.argmin(dd)), dd

        semi = ok & (di > dp)
        j, dd = best(semi if semi.any() else ok)
        win[i], dist[i] = j, di[j]
        others = np.delete(dd, j)
        close = others.size and others.min() <= di[j] * (1 + gap)
        edge = bool((ok & (np.abs(di - dp) <= gap * dp)).any())
        if close or edge:
            acc = set()
            pools = [ok & (di > dp * (1 - gap)), ok & (di > dp * (1 + gap))]
            pools = [q for q in pools if q.any()] + ([ok] if not all(q.any() for q in pools) else [])
            for q in pools:
                jq, dq = best(q)
                acc |= set(np.where(dq <= di[jq] * (1 + gap))[0].tolist())
            accept[i] = acc | {j}
    return win, dist, accept


# (N, M, D, anchors-per-workgroup class on a 256-CU device, tag).  Every D of {4, 36, 64, 100, 512, 1024, 2048}, M of {1, 255,
# 256, 257, 1500}, N of {1, 2, 5, 9, 64, 300}; "lds4" / "lds2": the LDS budget, not the grid, reduces the anchors (D = 1024 does
# not fit 8, D = 2048 not 4); 100 and 36 leave a slab tail (D % 32 != 0)
MINE_CASES = [(300, 512, 64, 8, ""), (300, 512, 1024, "lds4", ""), (300, 512, 2048, "lds2", ""), (1, 1, 4, 2, ""), (2, 255, 36, 2, ""), (5, 256, 64, 2, ""), (9, 257, 100, 2, ""), (64, 257, 512, 2, ""),
              (300, 256, 64, 4, ""), (300, 1500, 36, 8, "gpu"), (300, 1500, 512, 8, "gpu"), (768, 768, 512, 8, "gpu"),
              (300, 1500, 1024, "lds4", "gpu"), (300, 1500, 2048, "lds2", "gpu"), (9, 257, 1024, 2, ""), (5, 255, 2048, 2, ""),
              (64, 600, MINE_MAX_D, 2, "gpu")]
MINE_ESCAPE_CAP = 0.02


def mine_inputs(N, M, D, seed):
    """random anchors / candidates / labels (5 speakers) and positive distances d_p.  Random rows of a high dimension
    concentrate their distances, so a d_p taken blindly falls within f32 rounding of some candidate for a tenth of the
    anchors; the search's ORDER is what is under test, so d_p is put where float64 leaves no doubt: in the middle of a wide
    gap of the anchor's sorted other-label distances around their 30 % quantile, with the next two candidates apart as well.
    15 % of the anchors get a d_p past every candidate: nothing is semi-hard, the closest other-label one wins."""
    rs = np.random.RandomState(seed)
    anchor, cand = rs.randn(N, D).astype(F32), rs.randn(M, D).astype(F32)
    alab, clab = rs.randint(0, 5, N).astype(np.int64), rs.randint(0, 5, M).astype(np.int64)
    d = mine_dist(anchor, cand)
    d_p = np.empty(N, F32)
    for i in range(N):
        s = np.sort(d[i][clab != alab[i]])
        if rs.rand() < 0.15 or len(s) < 8:
            d_p[i] = d[i].max() * 2 if len(s) < 8 or rs.rand() < 0.5 else d[i].min() / 2
            continue
        lo, hi = int(0.25 * len(s)), max(int(0.35 * len(s)), int(0.25 * len(s)) + 1)
        k = lo + int(np.argmax([min(s[k + 1] - s[k], s[min(k + 2, len(s) - 1)] - s[k + 1] if k + 2 < len(s) else np.inf)
                                for k in range(lo, min(hi, len(s) - 1))]))
        d_p[i] = 0.5 * (s[k] + s[k + 1])
    return anchor, cand, alab, clab, d_p, d


# ---------------------------------------------------------------------------------------------------------------------
# row movers
# ---------------------------------------------------------------------------------------------------------------------
# (N rows gathered / scattered, M source / destination rows, D, tag): D on both sides of the parts = 8 switch (4096), rows not
# divisible by 2048 (the 8 x 256 stride of the long-row path)
MOVER_CASES = [(5, 7, 4, ""), (9, 6, 100, ""), (3, 4, 4096, ""), (3, 4, 4100, ""), (4, 5, 10240, ""), (64, 768, 10240, "gpu")]


def scatter_add_ref(g, idx, dst0, M, accumulate):
    """dst[j] (+)= sum over ascending i with idx[i] == j of g[i], sequentially in f32 (the documented order: bit for bit)"""
    out = dst0.astype(F32).copy() if accumulate else np.zeros_like(dst0, F32)
    for i in range(len(idx)):
        if 0 <= idx[i] < M:
            out[idx[i]] = out[idx[i]] + g[i]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# pools
# ---------------------------------------------------------------------------------------------------------------------
# (B, Hr, Wc, C, tag).  "cap2048": more than 2048 x 256 output vectors (the forward pools' grid-stride loop); "cap4096": more
# than 4096 x 256 vectors in the backward
POOL_CASES = [(1, 1, 1, 4, ""), (3, 10, 4, 512, ""), (5, 50, 3, 20, ""), (2, 10, 1, 2052, ""), (1025, 1, 4, 512, "cap2048"),
              (1030, 2, 4, 512, "gpu")]
POOL_LENS = (-3, 0, 1, "Hr", "Hr+5")
MASK_ROW_BYTES = (16, 4096, 8208)
CLIP_MAX = 20.0


def pool_ref(x, lens=None, dtype=F64):
    """x [B, Hr, K] -> [B, K]: mean over time (model.py:207), over the first lens[b] rows (clamped to Hr) when lens is given;
    an utterance without rows (lens <= 0) pools to 0, as its rows zeroed by ds_mask_rows do"""
    x = x.astype(dtype)
    if lens is None:
        return x.sum(1, dtype=dtype) / dtype(x.shape[1])
    out = np.zeros((x.shape[0], x.shape[2]), dtype)
    for b in range(x.shape[0]):
        n = min(int(lens[b]), x.shape[1])
        if n > 0:
            out[b] = x[b, :n].sum(0, dtype=dtype) / dtype(n)
    return out


def pool_bwd_ref(gpooled, out, dtype=F64):
    """gx[b, h] = gpooled[b] / Hr where 0 < out < 20 (strict: the clipped ReLU passes nothing at 0 and at 20), else 0"""
    g = gpooled.astype(dtype)[:, None, :] / dtype(out.shape[1])
    return np.where((out > 0) & (out < CLIP_MAX), g, dtype(0))


# ---------------------------------------------------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------------------------------------------------
# (M, n_cls, pad ld to 128, spread, tag)
CE_CASES = [(1, 1, False, 1.0, ""), (3, 2, True, 1.0, ""), (4, 63, False, 1e4, ""), (5, 64, True, 1.0, ""), (770, 65, True, 1e4, ""),
            (5, 1000, False, 1e4, ""), (3, 5994, True, 1.0, ""), (770, 5994, True, 1e4, "gpu"), (4, 64, False, 1e4, ""), (1, 65, True, 1e4, "")]


def ce_ref(logits, labels, dtype=F64):
    """nn.CrossEntropyLoss pieces (train_triplet.py:281-287): lse [M], row_loss [M], loss"""
    z = logits.astype(dtype)
    mx = z.max(1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(z - mx).sum(1, dtype=dtype))
    row = lse - z[np.arange(len(labels)), labels]
    return lse, row, dtype(row.mean(dtype=F64))


def ce_bwd_ref(logits, labels, lse, gloss, dtype=F64):
    """dlogits = gloss / M * (softmax - onehot) from the lse handed in"""
    z = logits.astype(dtype)
    g = np.exp(z - lse.astype(dtype)[:, None])
    g[np.arange(len(labels)), labels] -= 1
    return g * (dtype(gloss) / dtype(len(labels)))


def ce_inputs(M, n_cls, spread, seed):
    rs = np.random.RandomState(seed)
    logits = (rs.rand(M, n_cls) - 0.5).astype(F32) * F32(spread)
    labels = rs.randint(0, n_cls, M).astype(np.int64)
    labels[0] = 0
    labels[M - 1] = n_cls - 1 if M > 1 or n_cls == 1 else labels[M - 1]
    if M == 1:
        labels[0] = n_cls - 1
    return logits, labels


# ---------------------------------------------------------------------------------------------------------------------
# head
# ---------------------------------------------------------------------------------------------------------------------
def fc_splits(K):
    """the launcher's split of the contraction: the largest S in {8, 4, 2} with (K / 8) % (4 S) == 0, else 1"""
    for s in (8, 4, 2):
        if (K // 8) % (4 * s) == 0:
            return s
    return 1


# (B, K, N, bias, e, tag): K of {32, 64, 96, 128, 192, 2048} -> S = 1, 2, 1, 4, 2, 8; N on each reduce instantiation (<= 128,
# <= 256, <= 512, wide); B with and without an M tail
FC_CASES = [(1, 32, 128, True, True, ""), (31, 64, 256, True, True, ""), (32, 96, 512, False, True, ""), (33, 128, 640, True, False, ""),
            (100, 192, 1024, True, True, ""), (33, 2048, 128, True, True, ""), (100, 128, 256, False, False, ""),
            (768, 2048, 512, True, True, "gpu"), (768, 192, 640, True, True, "gpu"), (4, 2048, 512, True, True, "")]
FC_EXPECTED_S = {32: 1, 64: 2, 96: 1, 128: 4, 192: 2, 2048: 8}
# (M, K, N, n_cls, shift, tag).  shift: added to the bias of the REAL classes; at -300 the pad columns (logit 0) tower over them,
# so an epilogue that let a pad column into its row maximum would take expf of -300: log(0)
FC_CE_CASES = [(5, 64, 128, 100, 0.0, ""), (33, 128, 256, 129, -300.0, ""), (3, 32, 128, 1, -300.0, ""), (4, 96, 128, 128, 0.0, ""),
               (100, 2048, 640, 600, -300.0, "gpu"), (770, 512, 6016, 5994, 0.0, "gpu")]
# (B, Hr, K, N, tag)
TAIL_SMALL_CASES = [(1, 1, 100, 8, ""), (2, 10, 100, 128, ""), (3, 50, 2048, 16, ""), (4, 10, 2048, 512, "gpu"), (1, 50, 2048, 512, "gpu")]


def fc_feature_order(K, C):
    """k' = f * C + c of the pooled channels-last vector -> the reference's column c * F + f (model.py:164,208)"""
    F = K // C
    kp = np.arange(K)
    return (kp % C) * F + kp // C


def fc_ref(x, w, bias, C, dtype=F64):
    """f = x . W'^T + b with W'[n, k'] = w[n, c * F + f] (model.py:209 on the pooled vector's order)"""
    wk = w[:, fc_feature_order(w.shape[1], C)].astype(dtype)
    f = x.astype(dtype) @ wk.T
    return f + bias.astype(dtype)[None] if bias is not None else f


# ---------------------------------------------------------------------------------------------------------------------
# scoring
# ---------------------------------------------------------------------------------------------------------------------
# (n_groups, G)
GROUP_CASES = [(1, 1, ""), (255, 8, ""), (256, 1, ""), (257, 10, ""), (1000, 3, "")]
# ROC: (N, n_thr, grid: "pow2" thresholds i * 2^-6 (exact in f32 however contracted) / "ref" the reference's 0.01 grid, labels, tag)
ROC_CASES = [(1, 1, "pow2", "mixed", ""), (1023, 255, "pow2", "mixed", ""), (1024, 256, "ref", "mixed", ""), (1025, 257, "pow2", "same", ""),
             (5000, 3000, "ref", "mixed", ""), (1025, 257, "ref", "diff", ""), (5000, 3000, "pow2", "mixed", ""), (1024, 1, "ref", "mixed", ""),
             (1, 3000, "ref", "same", ""), (1023, 256, "pow2", "diff", "")]
ROC_ULPS = 4                    # distances of the "ref" grid keep this many f32 ulps from every threshold


def roc_thresholds(grid, n_thr):
    """(thr0, dthr, float64 thresholds as the reference forms them: np.arange(0, ., step))"""
    dt = 2.0 ** -6 if grid == "pow2" else 0.01
    return 0.0, dt, np.arange(n_thr, dtype=F64) * dt


def roc_inputs(N, n_thr, grid, labels, seed):
    rs = np.random.RandomState(seed)
    _, dt, thr = roc_thresholds(grid, n_thr)
    top = float(thr[-1]) + 2 * dt
    dist = (rs.rand(N) * top).astype(F32)
    if grid == "pow2":              # a third of the distances exactly on a threshold, one ulp below or one ulp above it
        k = rs.rand(N) < 0.34
        on = thr[rs.randint(0, n_thr, N)].astype(F32)
        side = rs.randint(-1, 2, N)
        on = np.where(side < 0, np.nextafter(on, F32(-1)), np.where(side > 0, np.nextafter(on, F32(1e9)), on)).astype(F32)
        dist = np.where(k, on, dist).astype(F32)
    else:                           # keep ROC_ULPS ulps from every threshold the sweep could form (the f32 product, the fused one)
        t32 = np.unique(np.concatenate([(F32(dt) * np.arange(n_thr + 3, dtype=F32)).astype(F32), (np.arange(n_thr + 3) * float(F32(dt))).astype(F32),
                                        (np.arange(n_thr + 3) * dt).astype(F32)]))
        for _ in range(4):
            j = np.clip(np.searchsorted(t32, dist), 1, len(t32) - 1)
            near = np.minimum(np.abs(dist - t32[j - 1]), np.abs(dist - t32[j])) <= ROC_ULPS * np.spacing(np.maximum(dist, F32(1e-30)))
            dist = np.where(near, dist + F32(0.3 * dt), dist).astype(F32)
    same = {"same": np.ones(N, bool), "diff": np.zeros(N, bool), "mixed": rs.rand(N) < 0.4}[labels]
    dist = np.where(same, dist * F32(0.6), dist).astype(F32) if grid == "pow2" else dist
    return np.abs(dist).astype(F32), same.astype(np.int32)


def roc_clearance_ulps(dist, grid, n_thr):
    """smallest distance, in f32 ulps of the distance, between a distance and any f32 threshold of the grid"""
    _, dt, thr = roc_thresholds(grid, n_thr)
    t32 = np.unique(np.concatenate([(F32(dt) * np.arange(n_thr, dtype=F32)).astype(F32), thr.astype(F32)]))
    j = np.clip(np.searchsorted(t32, dist), 1, max(len(t32) - 1, 1))
    lo, hi = t32[np.minimum(j - 1, len(t32) - 1)], t32[np.minimum(j, len(t32) - 1)]
    return float((np.minimum(np.abs(dist - lo), np.abs(dist - hi)) / np.spacing(np.maximum(dist, F32(1e-30)))).min())


def roc_summary_ref(tp, fp, n_same, n_diff, N, thr0, dthr):
    """summary6 from the returned counts in float64: first argmax of accuracy (eval_metrics.py:33,49), tpr / fpr / accuracy
    there (:47-48), EER (oracle equal_error_rate) and its threshold"""
    tp, fp = tp.astype(F64), fp.astype(F64)
    acc = (tp + (n_diff - fp)) / float(N)
    best = int(np.argmax(acc))
    fpr = fp / n_diff if n_diff else np.zeros_like(fp)
    fnr = 1.0 - tp / n_same if n_same else np.zeros_like(tp)
    cross = fpr >= fnr
    if cross.any():
        i = int(np.argmax(cross))
        if i == 0:
            eer, eer_thr = 0.5 * (fpr[0] + fnr[0]), thr0
        else:
            d0, d1 = fnr[i - 1] - fpr[i - 1], fpr[i] - fnr[i]
            w = d0 / (d0 + d1) if d0 + d1 > 0 else 0.0
            eer, eer_thr = fpr[i - 1] + w * (fpr[i] - fpr[i - 1]), thr0 + dthr * (i - 1 + w)
        if n_same and n_diff:
            assert abs(eer - O.equal_error_rate(tp, fp, n_same, n_diff)) < 1e-12
    else:
        eer, eer_thr = 1.0, thr0
    return np.array([best, tp[best] / n_same if n_same else 0.0, fp[best] / n_diff if n_diff else 0.0, acc[best], eer, eer_thr])
