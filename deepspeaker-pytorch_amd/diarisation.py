"""Speaker diarisation on the device: "who spoke when" in recordings with several speakers.

`sliding_windows` cuts every recording of a `FeatureStore` into overlapping windows, the model embeds them, and the
windows of each recording are clustered by agglomerative hierarchical clustering (AHC, csrc/ahc.hip) on the distance
the project already owns: `PairwiseDistance(2)` bits, in the units of `scoring.evaluate`'s thresholds.
`pairwise_distances` -> `linkage` -> `cut` are the three device steps (`cluster` chains them); a batch of recordings
is one ragged packed batch with host offsets, one workgroup per recording in the linkage, and a recording's result
does not depend on what else is in the batch.  `diarise` is the whole chain down to speaker turns.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .features import _plan
from .model import get_engine

_engine_override = None        # tests may bind the host emulator

AHC_MAX_N = 4096               # DS_AHC_MAX_N: windows of one recording
MAX_D = 2048                   # DS_NEAREST_MAX_D
_METHODS = {"average": 0, "complete": 1, "single": 2}       # DS_AHC_AVERAGE / _COMPLETE / _SINGLE


def _eng():
    return _engine_override if _engine_override is not None else get_engine()


def _on_device(eng, t: torch.Tensor, name: str):
    """The kernels take device pointers: a host tensor is refused (the host emulator of the tests takes host memory)."""
    if t.is_cuda == bool(eng.lib.host_memory):
        raise ValueError(f"{name}: expected a tensor on {'the host' if eng.lib.host_memory else 'a ROCm device'}, got {t.device}")


# ---- host arithmetic: windows and turns ------------------------------------------------------------------------------
def sliding_windows(lengths: Sequence[int], window: int = 160, hop: int = 80) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The windows of recordings of `lengths` frames, for `FeatureStore.crops`: (rec_idx [W], starts [W], win_offsets
    [n_rec + 1]), all host int64.  Starts are 0, hop, 2 hop, ... while the window fits, plus one last window flush with
    the end when the hop grid leaves a tail.  A recording shorter than `window` has one window at 0 (`crops` pads it
    with zeros), one of length 0 has none."""
    lens = np.asarray(lengths)
    if lens.ndim != 1 or (lens.size and (lens.dtype.kind not in "iu" or (lens < 0).any())):
        raise ValueError("lengths must be a vector of frame counts >= 0")
    if not isinstance(window, (int, np.integer)) or not isinstance(hop, (int, np.integer)) or window < 1 or hop < 1:
        raise ValueError(f"window = {window!r}, hop = {hop!r}: expected integers >= 1")
    rec, starts, counts = [], [], []
    for r, t in enumerate(lens.tolist()):
        if t == 0:
            s = np.zeros(0, np.int64)
        elif t <= window:
            s = np.zeros(1, np.int64)
        else:
            s = np.arange(0, t - window + 1, hop, dtype=np.int64)
            if s[-1] + window < t:
                s = np.append(s, t - window)
        rec.append(np.full(len(s), r, np.int64))
        starts.append(s)
        counts.append(len(s))
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int64)
    return cat(rec), cat(starts), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def frame_labels(starts: np.ndarray, labels: np.ndarray, window: int, n_frames: int) -> np.ndarray:
    """The label of every frame of one recording: that of the window whose centre (start + (window - 1) / 2) is
    nearest to the frame, ties to the earlier window.  `starts` ascending."""
    starts = np.asarray(starts, np.int64)
    if len(starts) == 0 or n_frames == 0:
        return np.zeros(0, np.int64)
    c2 = 2 * starts + (window - 1)                             # doubled centres
    owner = np.searchsorted(c2[:-1] + c2[1:], 4 * np.arange(n_frames, dtype=np.int64), side="left")
    return np.asarray(labels, np.int64)[owner]


def turns_of(frame_label: np.ndarray, original: Optional[np.ndarray] = None) -> List[Tuple[int, int, int]]:
    """Speaker turns (start_row, end_row, speaker), end exclusive: adjacent frames with equal labels joined.
    `original`: the original index of every (kept) frame, ascending; turns are then reported in those indices and a turn
    is also broken wherever removed frames lie between two kept ones."""
    lab = np.asarray(frame_label, np.int64)
    n = len(lab)
    if n == 0:
        return []
    pos = np.arange(n, dtype=np.int64) if original is None else np.asarray(original, np.int64)
    cut = np.nonzero((lab[1:] != lab[:-1]) | (pos[1:] != pos[:-1] + 1))[0] + 1
    first = np.concatenate([[0], cut])
    last = np.concatenate([cut, [n]]) - 1
    return [(int(pos[a]), int(pos[b]) + 1, int(lab[a])) for a, b in zip(first, last)]


# ---- the device steps ------------------------------------------------------------------------------------------------
def _offsets(win_offsets, n_rows: Optional[int] = None) -> np.ndarray:
    off = np.asarray(win_offsets)
    if off.ndim != 1 or len(off) < 2 or off.dtype.kind not in "iu":
        raise ValueError("win_offsets must be a vector of n_rec + 1 integer row offsets")
    off = off.astype(np.int64)
    if off[0] != 0 or (np.diff(off) < 0).any() or (n_rows is not None and off[-1] != n_rows):
        raise ValueError("win_offsets must rise from 0 to the number of rows")
    if int(np.diff(off).max()) > AHC_MAX_N:
        raise ValueError(f"a recording has {int(np.diff(off).max())} windows: at most {AHC_MAX_N}")
    return off


@dataclass
class _AhcPlan:
    table: torch.Tensor          # the int64 table of ds_ahc_plan on the device
    n_rec: int
    n_tiles: int
    tile_rows: int
    n_max: int
    dim: int


_PLAN_CACHE = {}               # the last few plans: a call repeated with the same offsets (a warm-up, then a stream capture)
_PLAN_CACHE_SIZE = 8           # finds its table on the device and uploads nothing


def _ahc_plan(eng, off: np.ndarray, dim: int, dev: torch.device) -> _AhcPlan:
    n_rec = len(off) - 1
    key = (id(eng), off.tobytes(), int(dim), str(dev))
    plan = _PLAN_CACHE.pop(key, None)
    if plan is None:
        _, counts, table_dev, _ = _plan(eng, dev, "ds_ahc_plan", off, n_rec, (int(dim),), 3, n_counts=6)
        plan = _AhcPlan(table_dev, n_rec, int(counts[1]), int(counts[2]), int(counts[5]), int(dim))
        while len(_PLAN_CACHE) >= _PLAN_CACHE_SIZE:
            _PLAN_CACHE.pop(next(iter(_PLAN_CACHE)))
    _PLAN_CACHE[key] = plan
    return plan


@dataclass
class RaggedMatrices:
    """Square float32 matrices of different sizes packed one after another: recording r, of n_r = offsets[r + 1] -
    offsets[r] rows, owns entries mat_offsets[r] .. mat_offsets[r + 1] of `data` (row-major n_r x n_r)."""
    data: torch.Tensor
    offsets: np.ndarray
    _plan: Optional[_AhcPlan] = None

    def __post_init__(self):
        self.offsets = _offsets(self.offsets)
        n = np.diff(self.offsets)
        self.mat_offsets = np.concatenate([[0], np.cumsum(n * n)]).astype(np.int64)
        if not isinstance(self.data, torch.Tensor) or self.data.dim() != 1 or self.data.dtype != torch.float32 or \
                self.data.numel() != self.mat_offsets[-1]:
            raise ValueError(f"data: expected a flat float32 tensor of {int(self.mat_offsets[-1])} entries")

    @classmethod
    def from_matrices(cls, matrices: Sequence, device) -> "RaggedMatrices":
        mats = [np.ascontiguousarray(m, np.float32) for m in matrices]
        if not mats or any(m.ndim != 2 or m.shape[0] != m.shape[1] for m in mats):
            raise ValueError("expected a sequence of square matrices")
        off = np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])]).astype(np.int64)
        flat = np.concatenate([m.reshape(-1) for m in mats]) if off[-1] else np.zeros(0, np.float32)
        return cls(torch.from_numpy(flat).to(device), off)

    def __len__(self):
        return len(self.offsets) - 1

    def matrix(self, r: int) -> torch.Tensor:
        n = int(self.offsets[r + 1] - self.offsets[r])
        return self.data[int(self.mat_offsets[r]):int(self.mat_offsets[r + 1])].view(n, n)


def pairwise_distances(emb: torch.Tensor, win_offsets) -> RaggedMatrices:
    """The distance matrix of every recording's rows of `emb[N, D]` (recording r: rows win_offsets[r] ..
    win_offsets[r + 1]): entry (i, j) is `PairwiseDistance(2)` of the two rows bit for bit -- direct differences, not
    the screening form, which cancels for the near-duplicate rows of overlapping windows --, symmetric bit for bit, +inf
    on the diagonal.  Nothing is read back."""
    eng = _eng()
    if not isinstance(emb, torch.Tensor) or emb.dim() != 2 or emb.dtype != torch.float32:
        raise ValueError("emb: expected a [rows, D] float32 tensor")
    _on_device(eng, emb, "emb")
    x = emb.contiguous()
    n, d = x.shape
    if not 1 <= d <= MAX_D:
        raise ValueError(f"D = {d}: expected 1..{MAX_D}")
    off = _offsets(win_offsets, n)
    nbytes = int(eng.lib.raw("ds_ahc_workspace_bytes")(off.ctypes.data, len(off) - 1))
    if nbytes < 0:
        raise ValueError("pairwise_distances: unsupported offsets")
    plan = _ahc_plan(eng, off, d, x.device)
    n2 = np.diff(off)
    data = torch.empty(int((n2 * n2).sum()), dtype=torch.float32, device=x.device)
    eng.lib.call("ds_ahc_distances_f32", eng._p(x), eng._p(plan.table), plan.n_rec, plan.n_tiles, plan.tile_rows, d,
                 eng._p(data), eng._stream(x))
    return RaggedMatrices(data, off, plan)


@dataclass
class Dendrogram:
    """The merges of every recording (device tensors, host offsets).  Step s of recording r is row step_offsets[r] + s:
    `pair` (a, b) the two slots, a < b, the merged cluster living on in slot a (its lowest member); `height` the merged
    distance; `size` its members.  `into[i]` / `step[i]` (rows offsets[r] + i): the slot that absorbed slot i and at
    which step, -1 for the survivor."""
    pair: torch.Tensor
    height: torch.Tensor
    size: torch.Tensor
    into: torch.Tensor
    step: torch.Tensor
    offsets: np.ndarray
    step_offsets: np.ndarray
    method: str
    _plan: _AhcPlan

    def __len__(self):
        return len(self.offsets) - 1

    def to_scipy(self, r: int) -> np.ndarray:
        """Recording r as SciPy's linkage matrix Z [n - 1, 4] float64: the steps sorted by height (stably), the cluster
        of the row at sorted position p named n + p.  (One read-back.  Where float32 average linkage inverts two heights
        by an ulp the sorted order may name a cluster before the row that forms it.)"""
        n = int(self.offsets[r + 1] - self.offsets[r])
        s0, s1 = int(self.step_offsets[r]), int(self.step_offsets[r + 1])
        pair = self.pair[s0:s1].cpu().numpy()
        height = self.height[s0:s1].cpu().numpy().astype(np.float64)
        size = self.size[s0:s1].cpu().numpy()
        order = np.argsort(height, kind="stable")
        name_of_step = np.empty(max(n - 1, 0), np.int64)
        name_of_step[order] = n + np.arange(len(order))
        name = np.arange(n, dtype=np.int64)                     # the cluster living in every slot
        z = np.zeros((max(n - 1, 0), 4), np.float64)
        for s in range(n - 1):
            a, b = int(pair[s, 0]), int(pair[s, 1])
            p = int(name_of_step[s]) - n
            z[p] = (min(name[a], name[b]), max(name[a], name[b]), height[s], size[s])
            name[a] = name_of_step[s]
        return z


def linkage(dist: RaggedMatrices, method: str = "average", overwrite: bool = False) -> Dendrogram:
    """Agglomerative clustering of every recording's matrix (symmetric, free of NaN), all merges in one launch, one
    workgroup per recording.  At every step the active pair with the smallest distance is merged, ties to the smallest
    first slot, then the smallest second; distances to the merged cluster follow `method` ("average", "complete" or
    "single"), in float32 with every operation rounded on its own.  The matrices are consumed: a clone unless
    `overwrite`.  Nothing is read back."""
    eng = _eng()
    if method not in _METHODS:
        raise ValueError(f"method = {method!r}: expected one of {tuple(_METHODS)}")
    if not isinstance(dist, RaggedMatrices):
        raise ValueError("dist: expected the RaggedMatrices of pairwise_distances")
    _on_device(eng, dist.data, "dist")
    data = dist.data.contiguous()
    dev = data.device
    off = dist.offsets
    plan = dist._plan if dist._plan is not None and dist._plan.table.device == dev else _ahc_plan(eng, off, 4, dev)
    work = data if overwrite and data is dist.data else data.clone()
    n = np.diff(off)
    step_off = np.concatenate([[0], np.cumsum(np.maximum(n - 1, 0))]).astype(np.int64)
    steps, rows = int(step_off[-1]), int(off[-1])
    pair = torch.empty((steps, 2), dtype=torch.int32, device=dev)
    height = torch.empty(steps, dtype=torch.float32, device=dev)
    size = torch.empty(steps, dtype=torch.int32, device=dev)
    into = torch.empty(rows, dtype=torch.int32, device=dev)
    step = torch.empty(rows, dtype=torch.int32, device=dev)
    eng.lib.call("ds_ahc_linkage_f32", eng._p(work), eng._p(plan.table), plan.n_rec, plan.n_max, _METHODS[method],
                 eng._p(pair), eng._p(height), eng._p(size), eng._p(into), eng._p(step), eng._stream(work))
    return Dendrogram(pair, height, size, into, step, off, step_off, method, plan)


def _per_recording(value, n_rec: int, dtype, name: str, dev):
    """A scalar, or one value per recording as a device vector: (mode, vector, scalar)."""
    if value is None:
        return 0, None, 0
    if isinstance(value, torch.Tensor) or np.ndim(value) > 0:
        t = torch.as_tensor(value)
        if t.dim() != 1 or t.shape[0] != n_rec or t.dtype == torch.bool or \
                (t.dtype.is_floating_point and not dtype.is_floating_point):
            raise ValueError(f"{name}: expected a scalar or {n_rec} values, one per recording")
        if t.device.type == "cpu" and ((torch.isnan(t).any() if dtype.is_floating_point else (t < 1).any())):
            raise ValueError(f"{name}: invalid value")
        return 2, t.to(device=dev, dtype=dtype).contiguous(), 0
    return 1, None, value


def cut(dendrogram: Dendrogram, threshold=None, n_clusters=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Labels from a dendrogram: (labels [rows] int32, n_found [n_rec] int32), both on the device.  `threshold`: the
    leading merges with height <= threshold are kept -- it stops at the first step above, which keeps the cut defined
    where float32 average linkage inverts two heights by an ulp; `n_clusters`: merges stop when that many clusters are
    left.  Both may be given (the cut that merges less wins), either as a scalar or as one value per recording; one is
    required.  Labels are 0, 1, ... in order of first appearance in the recording."""
    eng = _eng()
    if not isinstance(dendrogram, Dendrogram):
        raise ValueError("dendrogram: expected the result of linkage")
    if threshold is None and n_clusters is None:
        raise ValueError("cut needs a threshold, n_clusters or both")
    dev = dendrogram.into.device
    for name in ("pair", "height", "size", "into", "step"):
        t = getattr(dendrogram, name)
        _on_device(eng, t, "dendrogram." + name)
        if t.device != dev or not t.is_contiguous() or t.dtype != (torch.float32 if name == "height" else torch.int32):
            raise ValueError(f"dendrogram.{name}: expected a contiguous {'float32' if name == 'height' else 'int32'} tensor on {dev}")
    n_rec = len(dendrogram)
    t_mode, t_vec, t_val = _per_recording(threshold, n_rec, torch.float32, "threshold", dev)
    c_mode, c_vec, c_val = _per_recording(n_clusters, n_rec, torch.int32, "n_clusters", dev)
    if t_mode == 1:
        if isinstance(t_val, bool) or not isinstance(t_val, (int, float, np.integer, np.floating)) or t_val != t_val:
            raise ValueError(f"threshold = {threshold!r}: expected a number")
        t_val = float(t_val)
    if c_mode == 1:
        if isinstance(c_val, bool) or not isinstance(c_val, (int, np.integer)) or c_val < 1:
            raise ValueError(f"n_clusters = {n_clusters!r}: expected an integer >= 1")
        c_val = int(c_val)
    plan = dendrogram._plan
    labels = torch.empty(int(dendrogram.offsets[-1]), dtype=torch.int32, device=dev)
    n_found = torch.empty(n_rec, dtype=torch.int32, device=dev)
    eng.lib.call("ds_ahc_cut", eng._p(plan.table), plan.n_rec, plan.n_max, eng._p(dendrogram.height),
                 eng._p(dendrogram.into), eng._p(dendrogram.step), eng._p(t_vec), float(t_val), t_mode, eng._p(c_vec),
                 int(c_val), c_mode, eng._p(labels), eng._p(n_found), eng._stream(labels))
    return labels, n_found


def cluster(emb: torch.Tensor, win_offsets, threshold=None, n_clusters=None,
            method: str = "average") -> Tuple[torch.Tensor, torch.Tensor]:
    """`pairwise_distances` -> `linkage` -> `cut`: (labels [N] int32, n_found [n_rec] int32) on the device."""
    if threshold is None and n_clusters is None:
        raise ValueError("cluster needs a threshold, n_clusters or both")
    if method not in _METHODS:
        raise ValueError(f"method = {method!r}: expected one of {tuple(_METHODS)}")
    return cut(linkage(pairwise_distances(emb, win_offsets), method, overwrite=True), threshold, n_clusters)


def diarise(model, store, *, window: int = 160, hop: int = 80, threshold=None, n_clusters=None, method: str = "average",
            batch: int = 768, voiced=None) -> List[List[Tuple[int, int, int]]]:
    """Who spoke when in every recording of `store` (a `data.FeatureStore`): per recording a list of turns (start_row,
    end_row, speaker), end exclusive, speakers 0, 1, ... in order of first appearance.  Windows of `window` frames every
    `hop` are embedded by `model` (eval mode, no gradients, `batch` windows at a time) and clustered per recording
    (`cluster`); a frame takes the label of the window whose centre is nearest (ties to the earlier window).  The labels
    are read back once.  `voiced=(mask, frame_offsets)` of `features.voiced_frames` for a store that was built with
    `vad=`: turns are then in the original frame indices, and a turn is broken wherever removed frames lie between two
    kept rows."""
    if threshold is None and n_clusters is None:
        raise ValueError("diarise needs a threshold, n_clusters or both")
    if method not in _METHODS:
        raise ValueError(f"method = {method!r}: expected one of {tuple(_METHODS)}")
    if not isinstance(batch, (int, np.integer)) or batch < 1:
        raise ValueError(f"batch = {batch!r}: expected an integer >= 1")
    lengths = np.diff(np.asarray(store.offsets, np.int64))
    n_rec = len(lengths)
    rec_idx, starts, win_off = sliding_windows(lengths, window, hop)
    original = [None] * n_rec
    if voiced is not None:
        mask, frame_off = voiced
        frame_off = np.asarray(frame_off, np.int64)
        if not isinstance(mask, torch.Tensor) or mask.dim() != 1 or len(frame_off) != n_rec + 1 or \
                mask.numel() != frame_off[-1]:
            raise ValueError("voiced: expected the (mask, frame_offsets) of features.voiced_frames for this store")
        kept = mask.cpu().numpy() != 0
        original = [np.nonzero(kept[frame_off[r]:frame_off[r + 1]])[0] for r in range(n_rec)]
        if any(len(o) != t for o, t in zip(original, lengths)):
            raise ValueError("voiced: the mask keeps other frame counts than the store holds")
    if len(rec_idx) == 0:
        return [[] for _ in range(n_rec)]
    if int(np.diff(win_off).max()) > AHC_MAX_N:
        raise ValueError(f"a recording has {int(np.diff(win_off).max())} windows: at most {AHC_MAX_N} (a longer hop?)")
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            emb = torch.cat([model(store.crops(rec_idx[s:s + batch], starts[s:s + batch], window))
                             for s in range(0, len(rec_idx), batch)])
    finally:
        model.train(was_training)
    labels, _ = cluster(emb, win_off, threshold, n_clusters, method)
    lab = labels.cpu().numpy()
    out = []
    for r in range(n_rec):
        w0, w1 = int(win_off[r]), int(win_off[r + 1])
        out.append(turns_of(frame_labels(starts[w0:w1], lab[w0:w1], window, int(lengths[r])), original[r]))
    return out
