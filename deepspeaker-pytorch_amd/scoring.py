"""Verification scoring on the device.

`trial_scores` = the reference's test-time score (train_triplet.py:337-350): both utterances of a trial
are embedded as `crops` fixed-length crops, the distance is taken crop-by-crop and averaged.
`evaluate` = the threshold sweep of eval_metrics.py:5-50 (tpr / fpr / accuracy at the best-accuracy
threshold) plus the equal error rate the reference never computes.
`speaker_models` / `nearest` / `identify` = identification, which the reference does not have: enrolled speaker models,
the k nearest gallery rows of every query (csrc/identify.hip) and rank-1 ... rank-k accuracy.
`cohort_stats` / `normalise_scores` = score normalisation (Z / T / S / AS-norm, csrc/score_norm.hip) between the raw trial
score and `evaluate`; `min_dcf` = the minimum detection cost on `evaluate`'s counts.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .model import _require_cuda, get_engine

_engine_override = None        # tests may bind the host emulator


def _eng():
    return _engine_override if _engine_override is not None else get_engine()


def trial_scores(emb_a: torch.Tensor, emb_p: torch.Tensor, crops: int) -> torch.Tensor:
    """[n_trials*crops, D] x 2 (rows ordered trial-major, crop-minor as train_triplet.py:339-340 builds them)
    -> [n_trials] mean crop-pair distance."""
    eng = _eng()
    d = eng.pairwise_distance(emb_a.contiguous(), emb_p.contiguous())
    n = d.numel() // crops
    out = torch.empty(n, dtype=torch.float32, device=d.device)
    eng.lib.call("ds_group_mean_f32", eng._p(d), eng._p(out), n, crops, eng._stream(d))
    return out


def enrolment_scores(test_emb: torch.Tensor, enrol_emb: torch.Tensor, enrol_sizes) -> torch.Tensor:
    """Score of each trial against its claimed speaker's enrolment set -- sets of different sizes, utterances of
    different lengths (BASELINE configs[4]).  Trial i compares test_emb[i] with the `enrol_sizes[i]` consecutive rows of
    `enrol_emb` that make up its speaker's set and takes the MEAN of the distances, the reference's length
    normalisation (train_triplet.py:348-350 averages a trial's crop-pair distances).  Returns [n_trials]."""
    eng = _eng()
    sizes = np.asarray(enrol_sizes, np.int64)
    if sizes.ndim != 1 or len(sizes) != test_emb.shape[0] or (sizes < 1).any() or int(sizes.sum()) != enrol_emb.shape[0]:
        raise ValueError("enrol_sizes must give one set size >= 1 per trial, summing to the rows of enrol_emb")
    dev = test_emb.device
    def to_dev(a):         # through pinned memory, without blocking the host (a pageable copy waits for the stream's queue)
        t = torch.from_numpy(a)
        return t.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else t.to(dev)
    offsets = to_dev(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
    owner = to_dev(np.repeat(np.arange(len(sizes)), sizes).astype(np.int64))
    n, d = enrol_emb.shape
    expanded = torch.empty((n, d), dtype=torch.float32, device=dev)
    eng.lib.call("ds_gather_rows_f32", eng._p(test_emb.contiguous()), eng._p(owner), eng._p(expanded), n, d,
                 eng._stream(expanded))
    dist = eng.pairwise_distance(expanded, enrol_emb.contiguous())
    out = torch.empty(len(sizes), dtype=torch.float32, device=dev)
    eng.lib.call("ds_segment_mean_f32", eng._p(dist), eng._p(offsets), eng._p(out), len(sizes), eng._stream(dist))
    return out


@dataclass
class Verification:
    tpr: float
    fpr: float
    accuracy: float
    threshold: float
    eer: float
    eer_threshold: float
    tp: torch.Tensor        # per-threshold counts, on the device
    fp: torch.Tensor


def evaluate(distances: torch.Tensor, labels: torch.Tensor, thr_start: float = 0.0, thr_stop: float = 30.0,
             thr_step: float = 0.01) -> Verification:
    """eval_metrics.evaluate (thresholds np.arange(0, 30, 0.01), eval_metrics.py:7) on the device + EER."""
    eng = _eng()
    d = distances.contiguous().float()
    lab = (labels != 0).to(torch.int32).contiguous()
    n = d.numel()
    n_thr = len(np.arange(thr_start, thr_stop, thr_step))
    n_same = int(lab.sum().item())
    tp = torch.empty(n_thr, dtype=torch.int32, device=d.device)
    fp = torch.empty_like(tp)
    summary = torch.empty(6, dtype=torch.float32, device=d.device)
    eng.lib.call("ds_roc_sweep_f32", eng._p(d), eng._p(lab), n, float(thr_start), float(thr_step), n_thr, n_same,
                 n - n_same, eng._p(tp), eng._p(fp), eng._p(summary), eng._stream(d))
    s = summary.cpu().numpy()
    return Verification(float(s[1]), float(s[2]), float(s[3]), thr_start + thr_step * float(s[0]), float(s[4]),
                        float(s[5]), tp, fp)


# ---- identification: enrolled speaker models and the k nearest of them (csrc/identify.hip) ---------------------------
MODEL_ALPHA = 10.0             # the embedding sphere's radius (model.py:181)
NEAREST_MAX_K = 64             # DS_NEAREST_MAX_K
NEAREST_MAX_D = 2048           # DS_NEAREST_MAX_D
_EXCLUDE_MODES = {None: 0, "same": 1, "other": 2}


def _host_to_dev(a: np.ndarray, dev):
    """Host-side tables go through pinned memory, without blocking the host (as `enrolment_scores`)."""
    t = torch.from_numpy(a)
    return t.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else t.to(dev)


def _rows(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dim() != 2 or t.dtype != torch.float32 or t.shape[0] < 1:
        raise ValueError(f"{name}: expected a [rows, D] float32 tensor, got {tuple(t.shape)} {t.dtype}")
    return t.contiguous()


def _labels(t, n: int, name: str, dev) -> torch.Tensor:
    t = torch.as_tensor(t)
    if t.dim() != 1 or t.shape[0] != n or t.dtype.is_floating_point:
        raise ValueError(f"{name}: expected {n} integer labels, got {tuple(t.shape)} {t.dtype}")
    return t.to(device=dev, dtype=torch.int64).contiguous()


def speaker_models(enrol_emb: torch.Tensor, enrol_sizes, renormalise: bool = True) -> torch.Tensor:
    """One model per enrolled speaker: the mean of the speaker's `enrol_sizes[s]` consecutive rows of `enrol_emb`,
    with `renormalise` put back on the embeddings' sphere (L2 norm `MODEL_ALPHA`, the arithmetic of the model's own
    normalisation).  Returns [S, D]."""
    from .engine import L2_EPS
    eng = _eng()
    emb = _rows(enrol_emb, "enrol_emb")
    sizes = np.asarray(enrol_sizes, np.int64)
    if sizes.ndim != 1 or len(sizes) < 1 or (sizes < 1).any() or int(sizes.sum()) != emb.shape[0]:
        raise ValueError("enrol_sizes must give one set size >= 1 per speaker, summing to the rows of enrol_emb")
    offsets = _host_to_dev(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), emb.device)
    out = torch.empty((len(sizes), emb.shape[1]), dtype=torch.float32, device=emb.device)
    eng.lib.call("ds_segment_mean_rows_f32", eng._p(emb), eng._p(offsets), eng._p(out), len(sizes), emb.shape[1],
                 1 if renormalise else 0, MODEL_ALPHA, L2_EPS, eng._stream(emb))
    return out


def nearest(queries: torch.Tensor, gallery: torch.Tensor, k: int, query_labels=None, gallery_labels=None, exclude=None,
            splits: int = 0):
    """The `k` nearest rows of `gallery[M, D]` for every row of `queries[N, D]`: (distances [N, k] float32, indices
    [N, k] int64), ascending, ties to the lowest index.  The candidates come from a fused f32-MFMA search that never
    holds the N x M matrix; the reported distances are `PairwiseDistance(2)` of the pairs, bit for bit.
    `exclude="same"` skips gallery rows that carry the query's label (its hardest negatives), `"other"` keeps only those;
    both need the two label vectors.  Ranks that cannot be filled are index -1, distance +inf.  `splits`: gallery
    ranges searched separately (0: chosen for the device).  Nothing is read back."""
    eng = _eng()
    if exclude not in _EXCLUDE_MODES:
        raise ValueError("exclude must be None, 'same' or 'other'")
    q, g = _rows(queries, "queries"), _rows(gallery, "gallery")
    (n, d), m = q.shape, g.shape[0]
    if g.shape[1] != d or g.device != q.device:
        raise ValueError(f"queries {tuple(q.shape)} and gallery {tuple(g.shape)} must share D and the device")
    if d % 4 != 0 or d > NEAREST_MAX_D:
        raise ValueError(f"D = {d}: the search takes multiples of 4 up to {NEAREST_MAX_D}")
    if not isinstance(k, int) or not 1 <= k <= NEAREST_MAX_K:
        raise ValueError(f"k = {k!r}: expected an integer in 1..{NEAREST_MAX_K}")
    if not isinstance(splits, int) or splits < 0:
        raise ValueError(f"splits = {splits!r}: expected an integer >= 0")
    mode = _EXCLUDE_MODES[exclude]
    ql = gl = None
    if mode:
        if query_labels is None or gallery_labels is None:
            raise ValueError("exclude needs query_labels and gallery_labels")
        ql, gl = _labels(query_labels, n, "query_labels", q.device), _labels(gallery_labels, m, "gallery_labels", q.device)
    nbytes = int(eng.lib.raw("ds_nearest_workspace_bytes")(n, m, d, k, splits))
    if nbytes < 0:
        raise ValueError(f"nearest: unsupported shape N={n} M={m} D={d} k={k}")
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=q.device)
    scr_d = torch.empty((n, k), dtype=torch.float32, device=q.device)
    scr_i = torch.empty((n, k), dtype=torch.int64, device=q.device)
    eng.lib.call("ds_nearest_topk_f32", eng._p(q), eng._p(g), eng._p(ql), eng._p(gl), mode, eng._p(ws), eng._p(scr_d),
                 eng._p(scr_i), n, m, d, k, splits, eng._stream(q))
    dist = torch.empty_like(scr_d)
    idx = torch.empty_like(scr_i)
    eng.lib.call("ds_nearest_rescore_f32", eng._p(q), eng._p(g), eng._p(scr_i), eng._p(dist), eng._p(idx), n, m, d, k,
                 eng._stream(q))
    return dist, idx


@dataclass
class Identification:
    labels: torch.Tensor                 # [N, k] label of the r-th nearest model (-1 where there is none)
    distances: torch.Tensor              # [N, k]
    indices: torch.Tensor                # [N, k] rows of `models`
    hits: Optional[torch.Tensor] = None  # [k] int32 on the device: queries whose own label is among the first r + 1
    rank1: Optional[float] = None
    rank_k: Optional[float] = None


def identify(test_emb: torch.Tensor, models: torch.Tensor, model_labels, test_labels=None, k: int = 5) -> Identification:
    """Closed-set identification: the `k` nearest speaker models of every test embedding and, with `test_labels`, the
    cumulative match counts `hits[r]` (rank-1 ... rank-k accuracy = hits / N; the k counts are the only read-back)."""
    eng = _eng()
    dist, idx = nearest(test_emb, models, k)
    n, dev = idx.shape[0], idx.device
    ml = _labels(model_labels, models.shape[0], "model_labels", dev)
    labels = torch.where(idx >= 0, ml[idx.clamp_min(0)], torch.full_like(idx, -1))
    if test_labels is None:
        return Identification(labels, dist, idx)
    tl = _labels(test_labels, n, "test_labels", dev)
    hits = torch.empty(k, dtype=torch.int32, device=dev)
    eng.lib.call("ds_rank_hits_i32", eng._p(idx), eng._p(ml), eng._p(tl), eng._p(hits), n, k, eng._stream(idx))
    h = hits.cpu().numpy()
    return Identification(labels, dist, idx, hits, float(h[0]) / n, float(h[k - 1]) / n)


# ---- score normalisation: cohort statistics and Z / T / S / AS-norm (csrc/score_norm.hip) -----------------------------
COHORT_MAX_M = 32768           # DS_COHORT_MAX_M
_NORM_KINDS = ("z", "t", "s", "as")


@dataclass
class CohortStats:
    mean: torch.Tensor                   # [N] float32: mean distance to the selected cohort rows (+inf where count is 0)
    std: torch.Tensor                    # [N] float32: their population standard deviation (ddof 0)
    count: torch.Tensor                  # [N] int32: min(top_k, eligible cohort rows)
    mask: Optional[torch.Tensor] = None  # [N, ceil(M / 32)] int32: bit j % 32 of word j // 32 = cohort row j was selected


def cohort_stats(emb: torch.Tensor, cohort: torch.Tensor, top_k: Optional[int] = None, labels=None, cohort_labels=None,
                 exclude=None, row_block: int = 0, return_mask: bool = False) -> CohortStats:
    """Mean and standard deviation of every `emb[N, D]` row's distances to its `top_k` closest rows of `cohort[M, D]`
    (`top_k=None`: to all M -- Z / T / S-norm; a few hundred: the adaptive AS-norm).  The rows are chosen by the
    screening value of `nearest` (the same bits), exactly and with ties to the lowest index, by a radix select that
    never holds the N x M matrix; the statistics are over `PairwiseDistance(2)` of the chosen pairs.
    `exclude="same"` leaves out cohort rows that carry the row's own label (a cohort that contains the speaker),
    `"other"` keeps only those; both need `labels` and `cohort_labels`.  `row_block`: rows screened at once (0: chosen
    for the device); the result does not depend on it.  Nothing is read back."""
    eng = _eng()
    if exclude not in _EXCLUDE_MODES:
        raise ValueError("exclude must be None, 'same' or 'other'")
    q, g = _rows(emb, "emb"), _rows(cohort, "cohort")
    (n, d), m = q.shape, g.shape[0]
    if g.shape[1] != d or g.device != q.device:
        raise ValueError(f"emb {tuple(q.shape)} and cohort {tuple(g.shape)} must share D and the device")
    if d % 4 != 0 or d > NEAREST_MAX_D:
        raise ValueError(f"D = {d}: the search takes multiples of 4 up to {NEAREST_MAX_D}")
    if m > COHORT_MAX_M:
        raise ValueError(f"M = {m}: a cohort has at most {COHORT_MAX_M} rows")
    k = m if top_k is None else top_k
    if not isinstance(k, int) or not 1 <= k <= m:
        raise ValueError(f"top_k = {top_k!r}: expected None or an integer in 1..M = {m}")
    if not isinstance(row_block, int) or row_block < 0:
        raise ValueError(f"row_block = {row_block!r}: expected an integer >= 0")
    mode = _EXCLUDE_MODES[exclude]
    ql = gl = None
    if mode:
        if labels is None or cohort_labels is None:
            raise ValueError("exclude needs labels and cohort_labels")
        ql, gl = _labels(labels, n, "labels", q.device), _labels(cohort_labels, m, "cohort_labels", q.device)
    nbytes = int(eng.lib.raw("ds_cohort_workspace_bytes")(n, m, d, k, row_block))
    if nbytes < 0:
        raise ValueError(f"cohort_stats: unsupported shape N={n} M={m} D={d} K={k}")
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=q.device)
    mean = torch.empty(n, dtype=torch.float32, device=q.device)
    std = torch.empty_like(mean)
    count = torch.empty(n, dtype=torch.int32, device=q.device)
    mask = torch.empty((n, (m + 31) // 32), dtype=torch.int32, device=q.device) if return_mask else None
    eng.lib.call("ds_cohort_stats_f32", eng._p(q), eng._p(g), eng._p(ql), eng._p(gl), mode, eng._p(ws), eng._p(mean),
                 eng._p(std), eng._p(count), eng._p(mask), n, m, d, k, row_block, eng._stream(q))
    return CohortStats(mean, std, count, mask)


def normalise_scores(raw: torch.Tensor, kind: str, enrol_stats: Optional[CohortStats] = None,
                     test_stats: Optional[CohortStats] = None, enrol_index=None, test_index=None,
                     min_std: float = 1e-6) -> torch.Tensor:
    """Normalised trial scores [T] from raw distances `raw[T]` and the two sides' cohort statistics.
    `kind` "z": (raw - mean_e) / std_e with the enrolment side's statistics; "t": the same with the test side's; "s" and
    "as": the mean of the two.  "s" and "as" are ONE arithmetic: whether the result is S-norm or the adaptive AS-norm is
    decided by the `top_k` the statistics were taken with (`cohort_stats(..., top_k=None)` or a few hundred); both
    spellings are accepted so that a recipe can say what it means.
    `enrol_index` / `test_index`: int64 [T], the row of the side's statistics each trial uses (many trials share an
    utterance, so statistics are taken once per distinct embedding); None: trial t uses row t.  A standard deviation
    below `min_std` is replaced by it.  Distances stay distances: lower still means the same speaker, and `evaluate`
    applies unchanged (with a signed threshold grid, e.g. thr_start=-10, thr_stop=10)."""
    eng = _eng()
    if kind not in _NORM_KINDS:
        raise ValueError(f"kind = {kind!r}: expected one of {_NORM_KINDS}")
    need_e, need_t = kind != "t", kind != "z"
    if need_e and enrol_stats is None:
        raise ValueError(f"kind {kind!r} needs enrol_stats")
    if need_t and test_stats is None:
        raise ValueError(f"kind {kind!r} needs test_stats")
    if raw.dim() != 1 or raw.dtype != torch.float32 or raw.numel() < 1:
        raise ValueError(f"raw: expected a [T] float32 tensor, got {tuple(raw.shape)} {raw.dtype}")
    x = raw.contiguous()
    t, dev = x.numel(), x.device
    sides = []
    for use, stats, index, name in ((need_e, enrol_stats, enrol_index, "enrol"), (need_t, test_stats, test_index, "test")):
        if not use:
            continue
        mu, sd = stats.mean.contiguous(), stats.std.contiguous()
        if mu.device != dev or sd.device != dev or mu.dtype != torch.float32 or sd.dtype != torch.float32 or \
                mu.dim() != 1 or mu.shape != sd.shape:
            raise ValueError(f"{name}_stats: mean and std must be float32 vectors of one length on the scores' device")
        if index is None:
            if mu.numel() != t:
                raise ValueError(f"{name}_stats has {mu.numel()} rows for {t} trials: pass {name}_index")
            idx = None
        else:
            idx = _labels(index, t, f"{name}_index", dev)
        sides.append((idx, mu, sd))
    (ia, mu_a, sd_a), (ib, mu_b, sd_b) = sides[0], sides[1] if len(sides) == 2 else (None, None, None)
    out = torch.empty_like(x)
    eng.lib.call("ds_score_norm_apply_f32", eng._p(x), eng._p(ia), eng._p(ib), eng._p(mu_a), eng._p(sd_a), eng._p(mu_b),
                 eng._p(sd_b), float(min_std), eng._p(out), t, eng._stream(x))
    return out


def min_dcf(distances: torch.Tensor, labels: torch.Tensor, p_target: float = 0.01, c_miss: float = 1.0, c_fa: float = 1.0,
            thr_start: float = 0.0, thr_stop: float = 30.0, thr_step: float = 0.01):
    """Minimum normalised detection cost over `evaluate`'s threshold grid: (value, threshold).  At a threshold,
    P_miss = 1 - tp / n_same, P_fa = fp / n_diff and the cost is
    (c_miss P_miss p_target + c_fa P_fa (1 - p_target)) / min(c_miss p_target, c_fa (1 - p_target)); the first minimum
    is returned.  A set without same-speaker trials has P_miss = 0 everywhere, one without different-speaker trials
    P_fa = 0.  Computed on the device from the tp / fp counts `evaluate` leaves there; two scalars are read back."""
    res = evaluate(distances, labels, thr_start, thr_stop, thr_step)
    n = distances.numel()
    n_same = (labels != 0).sum().to(torch.float64)
    n_diff = n - n_same
    tp, fp = res.tp.to(torch.float64), res.fp.to(torch.float64)
    p_miss = torch.where(n_same > 0, 1.0 - tp / n_same.clamp_min(1.0), torch.zeros_like(tp))
    p_fa = torch.where(n_diff > 0, fp / n_diff.clamp_min(1.0), torch.zeros_like(fp))
    cost = (c_miss * p_target * p_miss + c_fa * (1.0 - p_target) * p_fa) / min(c_miss * p_target, c_fa * (1.0 - p_target))
    value = cost.min()
    grid = torch.arange(cost.numel(), device=cost.device)
    where = torch.where(cost == value, grid, torch.full_like(grid, cost.numel())).min()
    both = torch.stack([value, where.to(torch.float64)]).cpu().numpy()
    return float(both[0]), thr_start + thr_step * float(both[1])
