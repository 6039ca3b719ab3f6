"""TEST INFRASTRUCTURE: the diarisation cases (deepspeaker_pytorch_amd.diarisation, csrc/ahc.hip) shared by the
host-emulator file and the GPU file, against the restatements in ahc_reference.py.  A case takes `env`: the diarisation
module bound to an engine, that engine and the device."""
from dataclasses import dataclass

import numpy as np
import pytest
import torch

import ahc_reference as R

METHODS = ("average", "complete", "single")
METHOD_CODE = {"average": 0, "complete": 1, "single": 2}
AHC_MAX_N = 4096
LINK_NS = (0, 1, 2, 3, 63, 64, 65, 257, 700)     # empty, no merge, around one wave, several waves, several slots per thread
GUARD = 64                                        # entries behind every buffer that must stay as they were
INT_FILL = -123456789


@dataclass
class Env:
    dia: object
    eng: object
    device: torch.device

    def dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def random_symmetric(rs, n):
    """a symmetric float32 matrix of distinct-looking values in (0.5, 2), not a metric; +inf on the diagonal"""
    m = (0.5 + 1.5 * rs.rand(n, n)).astype(np.float32)
    m = np.triu(m, 1)
    m = m + m.T
    np.fill_diagonal(m, np.inf)
    return m


# ---- 1. the linkage, bit for bit ---------------------------------------------------------------------------------------
_link_cache = {}


def link_data():
    if "m" not in _link_cache:
        rs = np.random.RandomState(101)
        _link_cache["m"] = [random_symmetric(rs, n) for n in LINK_NS]
    return _link_cache["m"]


def link_reference(method):
    key = ("ref", method)
    if key not in _link_cache:
        _link_cache[key] = [R.linkage_f32(m, method) for m in link_data()]
    return _link_cache[key]


def guarded(env, n, dtype):
    """a device buffer of n entries and GUARD more, NaN / INT_FILL everywhere"""
    if dtype == torch.float32:
        return torch.full((n + GUARD,), float("nan"), dtype=dtype, device=env.device)
    return torch.full((n + GUARD,), INT_FILL, dtype=dtype, device=env.device)


def assert_guard(t, n):
    tail = host(t)[n:]
    assert np.isnan(tail).all() if tail.dtype == np.float32 else (tail == INT_FILL).all()


def run_linkage_abi(env, mats, method):
    """ds_ahc_linkage_f32 through the C ABI on buffers of the test's own, filled with NaN and guarded"""
    eng, dia = env.eng, env.dia
    off = np.concatenate([[0], np.cumsum([len(m) for m in mats])]).astype(np.int64)
    plan = dia._ahc_plan(eng, off, 4, env.device)
    n = np.diff(off)
    entries, steps, rows = int((n * n).sum()), int(np.maximum(n - 1, 0).sum()), int(off[-1])
    work = guarded(env, entries, torch.float32)
    work[:entries] = env.dev(np.concatenate([m.reshape(-1) for m in mats]))
    pair, height, size = guarded(env, 2 * steps, torch.int32), guarded(env, steps, torch.float32), guarded(env, steps, torch.int32)
    into, step = guarded(env, rows, torch.int32), guarded(env, rows, torch.int32)
    p = eng._p
    eng.lib.call("ds_ahc_linkage_f32", p(work), p(plan.table), plan.n_rec, plan.n_max, METHOD_CODE[method], p(pair),
                 p(height), p(size), p(into), p(step), eng._stream(work))
    for t, k in ((work, entries), (pair, 2 * steps), (height, steps), (size, steps), (into, rows), (step, rows)):
        assert_guard(t, k)
    s_off = np.concatenate([[0], np.cumsum(np.maximum(n - 1, 0))])
    out = []
    for r in range(len(mats)):
        s0, s1, r0, r1 = int(s_off[r]), int(s_off[r + 1]), int(off[r]), int(off[r + 1])
        out.append(dict(pair=host(pair)[2 * s0:2 * s1].reshape(-1, 2), height=host(height)[s0:s1], size=host(size)[s0:s1],
                        into=host(into)[r0:r1], step=host(step)[r0:r1]))
    return out


def assert_same_linkage(got, want, what=""):
    for key in ("pair", "size", "into", "step"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{what} {key}")
    np.testing.assert_array_equal(bits(got["height"]), bits(want["height"]), err_msg=f"{what} height")


def case_linkage_bit_exact(env, method):
    got = run_linkage_abi(env, link_data(), method)
    for n, g, w in zip(LINK_NS, got, link_reference(method)):
        assert len(g["height"]) == max(n - 1, 0) and len(g["into"]) == n
        assert_same_linkage(g, w, f"{method} n={n}")
        if n:
            assert (g["into"] == -1).sum() == 1 and g["into"][0] == -1       # slot 0 survives: the lowest member


def dendrogram_of(env, r, d):
    """recording r of a Dendrogram as host arrays"""
    s0, s1, r0, r1 = int(d.step_offsets[r]), int(d.step_offsets[r + 1]), int(d.offsets[r]), int(d.offsets[r + 1])
    return dict(pair=host(d.pair)[s0:s1], height=host(d.height)[s0:s1], size=host(d.size)[s0:s1], into=host(d.into)[r0:r1],
                step=host(d.step)[r0:r1])


# ---- 2. ties ---------------------------------------------------------------------------------------------------------
def case_ties(env, method):
    rs = np.random.RandomState(103)
    few = np.triu(rs.randint(1, 4, (130, 130)).astype(np.float32), 1)
    few = few + few.T
    np.fill_diagonal(few, np.inf)
    equal = np.full((65, 65), 2.0, np.float32)
    np.fill_diagonal(equal, np.inf)
    dist = env.dia.RaggedMatrices.from_matrices([few, equal], env.device)
    before = host(dist.data).copy()
    d = env.dia.linkage(dist, method)
    np.testing.assert_array_equal(bits(host(dist.data)), bits(before))         # a clone was consumed
    for r, m in enumerate((few, equal)):
        assert_same_linkage(dendrogram_of(env, r, d), R.linkage_f32(m, method), f"ties {method} rec {r}")
    # all equal: (0, 1), (0, 2), ... at the one height
    np.testing.assert_array_equal(dendrogram_of(env, 1, d)["pair"], np.stack([np.zeros(64), np.arange(1, 65)], 1))
    assert (dendrogram_of(env, 1, d)["height"] == 2.0).all()


# ---- 3. a recording's result does not depend on the batch ----------------------------------------------------------------
def case_independence(env):
    rs = np.random.RandomState(107)
    x = (rs.randn(100, 40)).astype(np.float32)
    others = [rs.randn(n, 40).astype(np.float32) for n in (40, 1, 130)]
    alone = env.dia.pairwise_distances(env.dev(x), [0, 100])
    ref_d = bits(host(alone.matrix(0)))
    ref_l = {m: dendrogram_of(env, 0, env.dia.linkage(alone, m)) for m in METHODS}
    for place in (0, 1, 3):                                        # first, in the middle, last
        parts = list(others)
        parts.insert(place, x)
        off = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
        dist = env.dia.pairwise_distances(env.dev(np.concatenate(parts)), off)
        np.testing.assert_array_equal(bits(host(dist.matrix(place))), ref_d)
        for m in METHODS:
            assert_same_linkage(dendrogram_of(env, place, env.dia.linkage(dist, m)), ref_l[m], f"place {place} {m}")


# ---- 4. distances ----------------------------------------------------------------------------------------------------
DIST_NS = (1, 63, 64, 65, 129)


def case_distances(env, dim):
    rs = np.random.RandomState(109 + dim)
    recs = []
    for n in DIST_NS:
        x = rs.randn(n, dim)
        x = (10.0 * x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
        if n >= 63:
            x[5] = x[2]                                            # a duplicated row
            x[40] = x[7]
            x[40, 3] = np.nextafter(x[40, 3], np.float32(np.inf))  # one coordinate, one ulp
            x[n - 1] = x[0]                                        # across tiles
        recs.append(x)
    off = np.concatenate([[0], np.cumsum(DIST_NS)]).astype(np.int64)
    dist = env.dia.pairwise_distances(env.dev(np.concatenate(recs)), off)
    assert dist.data.dtype == torch.float32 and dist.data.numel() == sum(n * n for n in DIST_NS)
    worst = 0.0
    for r, (n, x) in enumerate(zip(DIST_NS, recs)):
        got = host(dist.matrix(r))
        assert np.isposinf(np.diag(got)).all()
        np.testing.assert_array_equal(bits(got), bits(got.T.copy()))
        if n == 1:
            continue
        i, j = np.nonzero(~np.eye(n, dtype=bool))
        want = host(env.eng.pairwise_distance(env.dev(x[i]), env.dev(x[j])))       # PairwiseDistance's own bits
        np.testing.assert_array_equal(bits(got[i, j]), bits(want), err_msg=f"D={dim} n={n}")
        d64 = R.distances_f64(x)
        worst = max(worst, float((np.abs(got[i, j] - d64[i, j]) / d64[i, j]).max()))
        eps = np.sqrt(np.float32(1e-4 / dim))
        if n >= 63:
            assert bits(got[2, 5]) == bits(eps) and bits(got[0, n - 1]) == bits(eps)
            assert got[7, 40] >= eps
    print(f"distances D={dim}: worst error relative to float64 {worst:.3g}")
    assert worst <= 1e-6


# ---- 5. the cut ------------------------------------------------------------------------------------------------------
def handmade_dendrogram(env, links, ns):
    """a Dendrogram from host arrays (one dict per recording)"""
    dia = env.dia
    off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    s_off = np.concatenate([[0], np.cumsum(np.maximum(np.asarray(ns) - 1, 0))]).astype(np.int64)
    cat = lambda key, dt: env.dev(np.concatenate([np.asarray(l[key], dt).reshape(-1) for l in links]))
    return dia.Dendrogram(cat("pair", np.int32).view(-1, 2), cat("height", np.float32), cat("size", np.int32),
                          cat("into", np.int32), cat("step", np.int32), off, s_off, "average",
                          dia._ahc_plan(env.eng, off, 4, env.device))


def assert_cut(env, d, links, ns, threshold=None, n_clusters=None, what=""):
    labels, n_found = env.dia.cut(d, threshold=threshold, n_clusters=n_clusters)
    assert labels.dtype == torch.int32 and n_found.dtype == torch.int32
    lab, found = host(labels), host(n_found)
    off = np.concatenate([[0], np.cumsum(ns)])
    threshold = host(threshold) if isinstance(threshold, torch.Tensor) else threshold
    for r, (link, n) in enumerate(zip(links, ns)):
        t = None if threshold is None else (threshold if np.ndim(threshold) == 0 else float(np.asarray(threshold)[r]))
        c = None if n_clusters is None else (n_clusters if np.ndim(n_clusters) == 0 else int(np.asarray(n_clusters)[r]))
        want, want_found = R.cut(link, n, t, c)
        np.testing.assert_array_equal(lab[off[r]:off[r + 1]], want, err_msg=f"{what} rec {r}")
        assert found[r] == want_found, (what, r)
        if n:
            assert R.first_appearance(want).tolist() == want.tolist()      # 0, 1, ... in order of first appearance


def case_cut(env):
    ns = [0, 1, 2, 65, 257, 700]
    mats = [link_data()[LINK_NS.index(n)] for n in ns]
    links = [link_reference("average")[LINK_NS.index(n)] for n in ns]
    d = env.dia.linkage(env.dia.RaggedMatrices.from_matrices(mats, env.device), "average")
    h = links[4]["height"]                                         # the 257-row recording's heights (random: not sorted)
    hs = np.sort(h.astype(np.float64))
    for what, t in (("below the first", float(hs[0]) / 2), ("between", float(hs[100] + hs[101]) / 2),
                    ("above the last", float(hs[-1]) * 2), ("on a height", float(h[40])), ("on the first", float(h[0]))):
        assert_cut(env, d, links, ns, threshold=t, what=what)
    for c in (1, 2, 65, 257, 1000):
        assert_cut(env, d, links, ns, n_clusters=c, what=f"n_clusters={c}")
    assert_cut(env, d, links, ns, threshold=float(hs[200]), n_clusters=30, what="both, n_clusters binds")
    assert_cut(env, d, links, ns, threshold=float(hs[20]), n_clusters=3, what="both, the threshold binds")
    thr = np.array([1.0, 1.0, 0.1, float(hs[30]), float(hs[150]), float(hs[250])], np.float32)
    assert_cut(env, d, links, ns, threshold=thr, what="threshold per recording")
    assert_cut(env, d, links, ns, threshold=env.dev(thr), n_clusters=np.array([1, 1, 1, 5, 9, 2], np.int32),
               what="both per recording")
    # the prefix rule: heights 1, 2 (1 - ulp), 3 ... -- step 2 is BELOW step 1's height and still behind the cut
    inv = dict(pair=[(0, 1), (2, 3), (0, 2), (0, 4)], height=np.array([1.0, 2.0, np.nextafter(np.float32(2), np.float32(0)),
                                                                        3.0], np.float32),
               size=[2, 2, 4, 5], into=[-1, 0, 0, 2, 0], step=[-1, 0, 2, 1, 3])
    dh = handmade_dendrogram(env, [inv], [5])
    for t, want in ((0.5, [0, 1, 2, 3, 4]), (1.0, [0, 0, 1, 2, 3]), (1.5, [0, 0, 1, 2, 3]),
                    (float(inv["height"][2]), [0, 0, 1, 2, 3]), (2.0, [0, 0, 0, 0, 1]), (3.0, [0, 0, 0, 0, 0])):
        labels, n_found = env.dia.cut(dh, threshold=t)
        assert host(labels).tolist() == want and host(n_found)[0] == len(set(want)), t
        assert R.cut(inv, 5, t)[0].tolist() == want


# ---- 6. against SciPy end to end -------------------------------------------------------------------------------------
SCIPY_CASES = ((2, 40, 0), (3, 100, 2), (4, 200, 44), (5, 300, 184))       # centres, rows, seed (chosen for the gap condition)
SCIPY_DIM = 8
MIN_GAP = 1e-4


def scipy_points(k, n, seed):
    rs = np.random.RandomState(1000 + seed)
    c = rs.randn(k, SCIPY_DIM)
    c = 10.0 * c / np.linalg.norm(c, axis=1, keepdims=True)
    return (c[rs.randint(0, k, n)] + 0.7 * rs.randn(n, SCIPY_DIM)).astype(np.float32), k


def case_against_scipy(env, k, n, seed):
    from scipy.cluster.hierarchy import fcluster, linkage
    x, k = scipy_points(k, n, seed)
    d64 = R.distances_f64(x)
    ref = R.linkage_f64(d64, "average", want_gap=True)
    assert ref["min_gap"] > MIN_GAP, f"inputs: the float64 gap {ref['min_gap']:.3g} does not exceed {MIN_GAP} (another seed)"
    Z = linkage(d64[np.triu_indices(n, 1)], "average")
    dist = env.dia.pairwise_distances(env.dev(x), [0, n])
    dend = env.dia.linkage(dist, "average")
    got = dendrogram_of(env, 0, dend)
    assert R.merged_sets(got["pair"], n) == R.merged_sets_scipy(Z, n)           # the merge order
    z_got = dend.to_scipy(0)                                       # SciPy's own naming of the clusters
    np.testing.assert_array_equal(z_got[:, [0, 1, 3]], Z[:, [0, 1, 3]])
    np.testing.assert_array_equal(z_got[:, 2], got["height"].astype(np.float64))
    rel = np.abs(got["height"].astype(np.float64) - Z[:, 2]) / Z[:, 2]
    bound = (3 * (n - 1) + 4) * 2.0 ** -24
    print(f"against SciPy k={k} n={n}: worst height error / bound {rel.max() / bound:.3g} (bound {bound:.3g})")
    assert rel.max() <= bound
    t = float(Z[n - k - 1, 2] + Z[n - k, 2]) / 2                   # between the last merge inside and the first across
    labels, n_found = env.dia.cluster(env.dev(x), [0, n], threshold=t)
    want = R.first_appearance(fcluster(Z, t, criterion="distance"))
    assert host(labels).tolist() == want.tolist() and host(n_found)[0] == k
    return rel.max() / bound


# ---- 7. errors -------------------------------------------------------------------------------------------------------
def case_errors(env):
    dia, eng = env.dia, env.eng
    z = lambda n, d=8: torch.zeros((n, d), dtype=torch.float32, device=env.device)
    with pytest.raises(ValueError):
        dia.pairwise_distances(z(AHC_MAX_N + 1), [0, AHC_MAX_N + 1])           # above the cap
    with pytest.raises(ValueError):
        dia.pairwise_distances(z(4), [0, 5])                       # offsets beyond the rows
    with pytest.raises(ValueError):
        dia.pairwise_distances(z(4), [1, 4])                       # not from 0
    with pytest.raises(ValueError):
        dia.pairwise_distances(z(4), [0, 3, 2, 4])                 # decreasing
    with pytest.raises(ValueError):
        dia.pairwise_distances(z(4), [0.0, 4.0])                   # not integers
    with pytest.raises(ValueError):
        dia.pairwise_distances(z(4).double(), [0, 4])              # dtype
    with pytest.raises(ValueError):
        dia.pairwise_distances(z(4, 2052), [0, 4])                 # D
    with pytest.raises(ValueError):
        dia.RaggedMatrices(torch.zeros(5, dtype=torch.float32, device=env.device), [0, 2])
    with pytest.raises(ValueError):
        dia.RaggedMatrices(torch.zeros(4, dtype=torch.float64, device=env.device), [0, 2])
    dist = dia.pairwise_distances(z(4), [0, 4])
    with pytest.raises(ValueError):
        dia.linkage(dist, "ward")                                  # an unknown method
    with pytest.raises(ValueError):
        dia.linkage(dist.data)
    d = dia.linkage(dist)
    with pytest.raises(ValueError):
        dia.cut(d)                                                 # neither
    with pytest.raises(ValueError):
        dia.cut(d, n_clusters=0)
    with pytest.raises(ValueError):
        dia.cut(d, n_clusters=1.5)
    with pytest.raises(ValueError):
        dia.cut(d, threshold=float("nan"))
    with pytest.raises(ValueError):
        dia.cut(d, threshold=[1.0, 2.0])                           # two values, one recording
    with pytest.raises(ValueError):
        dia.cluster(z(4), [0, 4])
    with pytest.raises(ValueError):
        dia.cluster(z(4), [0, 4], threshold=1.0, method="centroid")
    with pytest.raises(ValueError):
        dia.diarise(None, None)
    if env.device.type == "cuda":                                  # host tensors are refused, not handed to a kernel
        with pytest.raises(ValueError):
            dia.pairwise_distances(z(4).cpu(), [0, 4])
        with pytest.raises(ValueError):
            dia.linkage(dia.RaggedMatrices(torch.zeros(4), [0, 2]))
    # the C ABI says no before it launches anything
    r = eng.lib.raw
    off = lambda *v: np.array(v, np.int64)
    counts = np.zeros(6, np.int64)
    plan = lambda o, n_rec, dim: r("ds_ahc_plan")(o.ctypes.data, n_rec, dim, None, counts.ctypes.data)
    assert plan(off(0, AHC_MAX_N), 1, 8) == 0 and counts[5] == AHC_MAX_N
    assert plan(off(0, AHC_MAX_N + 1), 1, 8) == -1
    assert plan(off(0, 3, 2), 2, 8) == -1 and plan(off(1, 3), 1, 8) == -1 and plan(off(0, 3), 1, 0) == -1
    assert plan(off(0, 3), 1, 2052) == -1 and plan(off(0, 3), 0, 8) == -1
    assert r("ds_ahc_plan")(None, 1, 8, None, counts.ctypes.data) == -3
    ws = lambda o, n_rec: r("ds_ahc_workspace_bytes")(o.ctypes.data, n_rec)
    assert ws(off(0, 3, 3, 5), 3) == 64 and ws(off(0, AHC_MAX_N), 1) == 4 * AHC_MAX_N ** 2
    assert ws(off(0, AHC_MAX_N + 1), 1) == -1 and ws(off(0, 3, 2), 2) == -1 and ws(off(1, 3), 1) == -1
    p = eng._p
    tab = dist._plan.table
    f, i = torch.zeros(64, dtype=torch.float32, device=env.device), torch.zeros(64, dtype=torch.int32, device=env.device)
    assert r("ds_ahc_distances_f32")(p(f), None, 1, 1, 32, 8, p(f), None) == -3
    assert r("ds_ahc_distances_f32")(p(f), p(tab), 1, 1, 16, 8, p(f), None) == -1       # not the plan's tile
    assert r("ds_ahc_distances_f32")(p(f), p(tab), 1, 1, 8, 2052, p(f), None) == -1
    assert r("ds_ahc_linkage_f32")(p(f), p(tab), 1, AHC_MAX_N + 1, 0, p(i), p(f), p(i), p(i), p(i), None) == -1
    assert r("ds_ahc_linkage_f32")(p(f), p(tab), 1, 4, 3, p(i), p(f), p(i), p(i), p(i), None) == -4
    assert r("ds_ahc_linkage_f32")(None, p(tab), 1, 4, 0, p(i), p(f), p(i), p(i), p(i), None) == -3
    assert r("ds_ahc_cut")(p(tab), 1, AHC_MAX_N + 1, p(f), p(i), p(i), None, 1.0, 1, None, 0, 0, p(i), p(i), None) == -1
    assert r("ds_ahc_cut")(p(tab), 1, 4, p(f), p(i), p(i), None, 1.0, 0, None, 0, 0, p(i), p(i), None) == -4
    assert r("ds_ahc_cut")(p(tab), 1, 4, p(f), p(i), p(i), None, 1.0, 2, None, 0, 0, p(i), p(i), None) == -3
    assert r("ds_ahc_cut")(p(tab), 1, 4, p(f), p(i), p(i), None, 1.0, 1, None, 0, 1, p(i), p(i), None) == -1


# ---- 8. host arithmetic: windows and turns ---------------------------------------------------------------------------
def case_sliding_windows(dia):
    rec, starts, off = dia.sliding_windows([100, 160, 161, 400, 0, 420, 320], window=160, hop=80)
    assert off.tolist() == [0, 1, 2, 4, 8, 8, 13, 16]
    by = lambda r: starts[off[r]:off[r + 1]].tolist()
    assert by(0) == [0]                                            # T < window: one window, zero padded by crops
    assert by(1) == [0]                                            # T = window
    assert by(2) == [0, 1]                                         # T = window + 1: the flush window
    assert by(3) == [0, 80, 160, 240]                              # the grid ends flush: no extra window
    assert by(4) == []
    assert by(5) == [0, 80, 160, 240, 260]                         # a tail of 20 frames
    assert by(6) == [0, 80, 160]
    assert rec.tolist() == np.repeat(np.arange(7), np.diff(off)).tolist()
    assert all(a.dtype == np.int64 for a in (rec, starts, off))
    rec, starts, off = dia.sliding_windows([], 160, 80)
    assert len(rec) == 0 and off.tolist() == [0]
    for bad in (dict(lengths=[-1]), dict(lengths=[1.5]), dict(lengths=[5], window=0), dict(lengths=[5], hop=0)):
        with pytest.raises(ValueError):
            dia.sliding_windows(**bad)


def case_turns(dia):
    # windows of 4 frames at 0, 2, 4: centres 1.5, 3.5, 5.5; frame 2 is nearest to 1.5 (0.5 against 1.5), frame 3
    # to 3.5; with window 5 (centres 2, 4, 6) frame 3 is a tie and goes to the earlier window
    lab = dia.frame_labels(np.array([0, 2, 4]), np.array([7, 8, 9]), 4, 8)
    assert lab.tolist() == [7, 7, 7, 8, 8, 9, 9, 9]
    lab = dia.frame_labels(np.array([0, 2, 4]), np.array([7, 8, 9]), 5, 9)
    assert lab.tolist() == [7, 7, 7, 7, 8, 8, 9, 9, 9]             # frames 3 and 5: the ties
    assert dia.frame_labels(np.array([0]), np.array([3]), 160, 100).tolist() == [3] * 100
    assert dia.frame_labels(np.zeros(0, np.int64), np.zeros(0, np.int64), 160, 0).tolist() == []
    brute = lambda starts, w, t: [int(np.argmin(np.abs(2 * f - (2 * np.asarray(starts) + w - 1)))) for f in range(t)]
    _, starts, _ = dia.sliding_windows([1000], 160, 80)
    assert dia.frame_labels(starts, np.arange(len(starts)), 160, 1000).tolist() == brute(starts, 160, 1000)
    _, starts, _ = dia.sliding_windows([333], 7, 3)
    assert dia.frame_labels(starts, np.arange(len(starts)), 7, 333).tolist() == brute(starts, 7, 333)
    assert dia.turns_of(np.array([0, 0, 1, 1, 1, 0])) == [(0, 2, 0), (2, 5, 1), (5, 6, 0)]
    assert dia.turns_of(np.zeros(0, np.int64)) == []
    # kept frames 2 3 4 | 8 9 | 10: the gap 5..7 breaks the turn of speaker 0, 9 -> 10 is adjacent
    orig = np.array([2, 3, 4, 8, 9, 10])
    assert dia.turns_of(np.array([0, 0, 0, 0, 1, 1]), orig) == [(2, 5, 0), (8, 9, 0), (9, 11, 1)]
