"""TEST INFRASTRUCTURE: float64 restatement of the score-normalisation contract (scoring.cohort_stats /
normalise_scores / min_dcf, csrc/score_norm.hip), written from the contract and not from the kernels:

  * an embedding's cohort selection is the min(K, eligible) cohort rows with the smallest squared Euclidean distance,
    ties to the lowest cohort index; with a label filter only the eligible rows take part;
  * its statistics are the mean and the population standard deviation (ddof 0) of the PairwiseDistance(2) of the
    selected pairs, sqrt(sum (q - g)^2 + eps) with eps = 1e-4 / D; nothing selected: count 0, mean +inf, std 0;
  * a normalised score is the mean over the sides that apply of (raw - mean) / max(std, min_std);
  * minDCF is the minimum over the threshold grid of
    (c_miss P_miss p + c_fa P_fa (1 - p)) / min(c_miss p, c_fa (1 - p)), P_miss = 1 - tp / n_same, P_fa = fp / n_diff
    (0 where the class is empty), predictions being dist < threshold.
"""
import numpy as np


def squared_distances(emb, cohort):
    """Exact d^2 [N, M] in float64 by direct differences (no cancellation)."""
    q = np.asarray(emb, np.float64)
    g = np.asarray(cohort, np.float64)
    out = np.empty((q.shape[0], g.shape[0]), np.float64)
    for i in range(q.shape[0]):
        diff = g - q[i]
        out[i] = np.einsum("md,md->m", diff, diff)
    return out


def select(d2, top_k, labels=None, cohort_labels=None, exclude=None):
    """-> bool [N, M]: per row the top_k eligible cohort rows in stable ascending order of d2 (all, if fewer)."""
    n, m = d2.shape
    sel = np.zeros((n, m), bool)
    cl = None if cohort_labels is None else np.asarray(cohort_labels)
    for i in range(n):
        if exclude is None:
            rows = np.arange(m)
        elif exclude == "same":
            rows = np.nonzero(cl != labels[i])[0]
        elif exclude == "other":
            rows = np.nonzero(cl == labels[i])[0]
        else:
            raise ValueError(exclude)
        sel[i, rows[np.argsort(d2[i, rows], kind="stable")][:top_k]] = True
    return sel


def stats_of(d2, sel, dim):
    """(mean, std, count) in float64 of sqrt(d2 + 1e-4 / dim) over each row's selected set."""
    n = d2.shape[0]
    mean = np.full(n, np.inf)
    std = np.zeros(n)
    count = sel.sum(axis=1).astype(np.int64)
    for i in range(n):
        if count[i]:
            d = np.sqrt(d2[i, sel[i]] + 1e-4 / dim)
            mean[i] = d.mean()
            std[i] = np.sqrt(((d - mean[i]) ** 2).mean())
    return mean, std, count


def cohort_stats(emb, cohort, top_k, labels=None, cohort_labels=None, exclude=None):
    """-> (d2, sel, mean, std, count)"""
    d2 = squared_distances(emb, cohort)
    sel = select(d2, top_k, labels, cohort_labels, exclude)
    return (d2, sel) + stats_of(d2, sel, np.asarray(emb).shape[1])


def unpack_mask(mask_words, m):
    """int32 [N, ceil(M / 32)] (bit j % 32 of word j // 32) -> bool [N, M]"""
    w = np.ascontiguousarray(mask_words).view(np.uint32)
    bits = (w[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1
    return bits.reshape(w.shape[0], -1)[:, :m].astype(bool)


def apply(raw, mean_a, std_a, index_a=None, mean_b=None, std_b=None, index_b=None, min_std=1e-6):
    raw = np.asarray(raw, np.float64)
    t = np.arange(len(raw))

    def side(mean, std, index):
        i = t if index is None else np.asarray(index)
        return (raw - np.asarray(mean, np.float64)[i]) / np.maximum(np.asarray(std, np.float64)[i], float(min_std))

    za = side(mean_a, std_a, index_a)
    if mean_b is None:
        return za
    return 0.5 * (za + side(mean_b, std_b, index_b))


def thresholds_f32(thr_start, thr_stop, thr_step):
    """The sweep's thresholds: thr_start + thr_step * i in float32, once with a rounded product and once fused (the
    two ways a device may evaluate it); test scores keep clear of both."""
    n = len(np.arange(thr_start, thr_stop, thr_step))
    i = np.arange(n, dtype=np.float32)
    t0, dt = np.float32(thr_start), np.float32(thr_step)
    plain = (t0 + (dt * i).astype(np.float32)).astype(np.float32)
    fused = (np.float64(t0) + np.float64(dt) * i.astype(np.float64)).astype(np.float32)
    return plain, fused


def roc_counts(dist, labels, thr):
    """tp / fp per threshold: predictions dist < thr"""
    dist = np.asarray(dist, np.float32)
    same = np.asarray(labels) != 0
    order = np.sort(dist[same]), np.sort(dist[~same])
    tp = np.searchsorted(order[0], thr, side="left")
    fp = np.searchsorted(order[1], thr, side="left")
    return tp.astype(np.int64), fp.astype(np.int64)


def equal_error_rate(tp, fp, n_same, n_diff):
    """First crossing of FPR and FNR on the grid, linearly interpolated (0.5 (fpr + fnr) if they cross at once;
    1.0 if never)."""
    fpr = fp / n_diff if n_diff else np.zeros(len(fp))
    fnr = 1.0 - tp / n_same if n_same else np.zeros(len(tp))
    cross = fpr >= fnr
    if not cross.any():
        return 1.0
    i = int(np.argmax(cross))
    if i == 0:
        return 0.5 * (fpr[0] + fnr[0])
    d0, d1 = fnr[i - 1] - fpr[i - 1], fpr[i] - fnr[i]
    w = d0 / (d0 + d1) if d0 + d1 > 0 else 0.0
    return fpr[i - 1] + w * (fpr[i] - fpr[i - 1])


def min_dcf(tp, fp, n_same, n_diff, p_target=0.01, c_miss=1.0, c_fa=1.0):
    """-> (value, index of the first threshold that attains it)"""
    tp, fp = np.asarray(tp, np.float64), np.asarray(fp, np.float64)
    p_miss = 1.0 - tp / n_same if n_same else np.zeros_like(tp)
    p_fa = fp / n_diff if n_diff else np.zeros_like(fp)
    cost = (c_miss * p_target * p_miss + c_fa * (1.0 - p_target) * p_fa) / min(c_miss * p_target, c_fa * (1.0 - p_target))
    i = int(np.argmin(cost))
    return float(cost[i]), i
