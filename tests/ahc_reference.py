"""TEST INFRASTRUCTURE: restatements of the agglomerative clustering contract of csrc/ahc.hip in NumPy.

`linkage_f32` is the contract's exact arithmetic (every operation rounded to float32 on its own), `linkage_f64` the same
procedure in float64 (validated against SciPy in test_ahc_reference.py).  Both search the WHOLE upper triangle at every
step -- the plain O(n^3) procedure, nothing of the kernel's neighbour bookkeeping: np.argmin returns the first minimum
in row-major order, which is the tie rule (smallest a, then smallest b)."""
import numpy as np


def _linkage(matrix, method, dt, want_gap=False):
    n = len(matrix)
    W = np.array(matrix, dt)
    U = np.full((n, n), np.inf, dt)                  # the active pairs a < b
    iu = np.triu_indices(n, 1)
    U[iu] = W[iu]
    size = np.ones(n, np.int64)
    active = np.ones(n, bool)
    pair = np.zeros((max(n - 1, 0), 2), np.int32)
    height = np.zeros(max(n - 1, 0), dt)
    size_out = np.zeros(max(n - 1, 0), np.int32)
    into = np.full(n, -1, np.int32)
    step = np.full(n, -1, np.int32)
    min_gap = np.inf
    for s in range(n - 1):
        a, b = divmod(int(np.argmin(U)), n)
        h = U[a, b]
        if want_gap and n - s > 2:
            two = np.partition(U.ravel(), 1)[:2]
            min_gap = min(min_gap, float((two[1] - two[0]) / two[0]))
        na, nb = int(size[a]), int(size[b])
        others = active.copy()
        others[[a, b]] = False
        k = np.nonzero(others)[0]
        x, y = W[a, k], W[b, k]
        if method == "single":
            new = np.minimum(x, y)
        elif method == "complete":
            new = np.maximum(x, y)
        elif method == "average":
            pa = (dt(na) * x).astype(dt)
            pb = (dt(nb) * y).astype(dt)
            new = ((pa + pb).astype(dt) / dt(na + nb)).astype(dt)
        else:
            raise ValueError(method)
        W[a, k] = new
        W[k, a] = new
        U[k[k < a], a] = new[k < a]
        U[a, k[k > a]] = new[k > a]
        U[b, :] = np.inf
        U[:, b] = np.inf
        active[b] = False
        size[a] = na + nb
        pair[s] = (a, b)
        height[s] = h
        size_out[s] = na + nb
        into[b] = a
        step[b] = s
    out = dict(pair=pair, height=height, size=size_out, into=into, step=step)
    if want_gap:
        out["min_gap"] = min_gap
    return out


def linkage_f32(matrix, method):
    return _linkage(matrix, method, np.float32)


def linkage_f64(matrix, method, want_gap=False):
    return _linkage(matrix, method, np.float64, want_gap)


def cut(link, n, threshold=None, n_clusters=None):
    """(labels, n_found) of one recording: the prefix rule of the contract on float32 heights."""
    if n == 0:
        return np.zeros(0, np.int32), 0
    m = n - 1
    if threshold is not None:
        above = np.nonzero(~(link["height"].astype(np.float32) <= np.float32(threshold)))[0]
        if len(above):
            m = int(above[0])
    if n_clusters is not None:
        m = min(m, max(n - int(n_clusters), 0))
    root = np.zeros(n, np.int64)
    for i in range(n):
        q = i
        while 0 <= link["step"][q] < m:
            q = link["into"][q]
        root[i] = q
    roots = np.unique(root)
    return np.searchsorted(roots, root).astype(np.int32), len(roots)


def merged_sets(pair, n):
    """the members of the cluster every step forms, in step order"""
    members = [frozenset([i]) for i in range(n)]
    out = []
    for a, b in np.asarray(pair).tolist():
        members[a] = members[a] | members[b]
        out.append(members[a])
    return out


def merged_sets_scipy(Z, n):
    members = [frozenset([i]) for i in range(n)]
    for a, b in Z[:, :2].astype(np.int64).tolist():
        members.append(members[a] | members[b])
    return members[n:]


def distances_f64(x):
    """PairwiseDistance(2) of every pair of rows in float64 (eps = 1e-4 / D inside the root), +inf on the diagonal"""
    x = np.asarray(x, np.float64)
    g = ((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)
    d = np.sqrt(g + 1e-4 / x.shape[1])
    np.fill_diagonal(d, np.inf)
    return d


def first_appearance(labels):
    """labels renamed 0, 1, ... in order of first appearance"""
    _, first, inv = np.unique(labels, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inv]
