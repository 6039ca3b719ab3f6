"""TEST INFRASTRUCTURE: float64 restatement of the identification contract (scoring.nearest / speaker_models /
identify, csrc/identify.hip), written from the contract and not from the kernels:

  * the k nearest gallery rows of a query are the k smallest by squared Euclidean distance, ties to the lowest gallery
    index; with a label filter only the eligible rows take part; ranks that cannot be filled are index -1, distance +inf;
  * the reported distance of a pair is PairwiseDistance(2): sqrt(sum (q - g)^2 + eps), eps = 1e-4 / D;
  * a speaker model is the mean of the speaker's enrolment rows, optionally rescaled to L2 norm alpha
    (m / sqrt(sum m^2 + eps) * alpha, eps = 1e-10);
  * hits[r] counts the queries whose own label is among the labels of their first r + 1 results.
"""
import numpy as np

ALPHA = 10.0
L2_EPS = 1e-10


def squared_distances(queries, gallery):
    """Exact d^2 [N, M] in float64 by direct differences (no cancellation)."""
    q = np.asarray(queries, np.float64)
    g = np.asarray(gallery, np.float64)
    out = np.empty((q.shape[0], g.shape[0]), np.float64)
    for i in range(q.shape[0]):
        diff = g - q[i]
        out[i] = np.einsum("md,md->m", diff, diff)
    return out


def nearest(queries, gallery, k, query_labels=None, gallery_labels=None, exclude=None):
    """-> (d2 [N, M] float64, order [N, k] int64, dist [N, k] float64).

    d2: the exact squared distances of every pair (eligible or not); order: per query the eligible gallery rows in
    stable ascending order of d2 (lowest index first among equals), cut to k and padded with -1; dist: the distances
    of those rows with the reference's eps inside the root, +inf where order is -1."""
    d2 = squared_distances(queries, gallery)
    n, m = d2.shape
    dim = np.asarray(queries).shape[1]
    order = np.full((n, k), -1, np.int64)
    dist = np.full((n, k), np.inf, np.float64)
    gl = None if gallery_labels is None else np.asarray(gallery_labels)
    for i in range(n):
        if exclude is None:
            rows = np.arange(m)
        elif exclude == "same":
            rows = np.nonzero(gl != query_labels[i])[0]
        elif exclude == "other":
            rows = np.nonzero(gl == query_labels[i])[0]
        else:
            raise ValueError(exclude)
        best = rows[np.argsort(d2[i, rows], kind="stable")][:k]
        order[i, :len(best)] = best
        dist[i, :len(best)] = np.sqrt(d2[i, best] + 1e-4 / dim)
    return d2, order, dist


def speaker_models(enrol_emb, enrol_sizes, renormalise=True):
    e = np.asarray(enrol_emb, np.float64)
    off = np.concatenate([[0], np.cumsum(enrol_sizes)])
    out = np.stack([e[off[s]:off[s + 1]].mean(axis=0) for s in range(len(enrol_sizes))])
    if renormalise:
        out = out / np.sqrt((out * out).sum(axis=1, keepdims=True) + L2_EPS) * ALPHA
    return out


def rank_hits(indices, gallery_labels, query_labels):
    """hits[r] = number of queries whose label equals the label of one of their results 0..r (-1 never matches)."""
    idx = np.asarray(indices)
    gl = np.asarray(gallery_labels)
    ql = np.asarray(query_labels)
    match = (idx >= 0) & (gl[np.maximum(idx, 0)] == ql[:, None])
    return np.cumsum(match, axis=1).astype(bool).sum(axis=0).astype(np.int64)
