"""TEST INFRASTRUCTURE: the score-normalisation cases (scoring.cohort_stats / normalise_scores / min_dcf,
csrc/score_norm.hip) shared by the host-emulator file and the GPU file, each against the float64 restatement in
score_norm_reference.py.  A case takes `env`: the scoring module bound to an engine, that engine and the device."""
from dataclasses import dataclass

import numpy as np
import pytest
import torch

import score_norm_reference as R

INT_NS = (1, 33, 130)                           # one wave-row, a ragged block, three query blocks
INT_MS = (1, 5, 127, 128, 129, 700, 2500)       # below / at / above the 128-row tile and the 64-row chunk; 20 tiles
INT_KS = (1, 5, 64, 65, 300, None)              # None: K = M; every K is clipped to M
INT_DS = (4, 512)
ROW_BLOCKS = (0, 64, 100)                       # the library's choice, one query block, a ragged one
COHORT_MAX_M = 32768
STAT_TOL = 2e-6                                 # x d_max: the project's 1e-6 bar on PairwiseDistance plus the reduction


@dataclass
class Env:
    scoring: object
    eng: object
    device: torch.device

    def dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return host(t).view(np.int32)


def mask_of(stats, m):
    return R.unpack_mask(host(stats.mask), m)


def assert_stats_of_returned_set(d2, sel, stats, dim, what=""):
    """mean / std against float64 on the SAME set, within STAT_TOL x the row's largest selected distance (absolute for
    std too: the deviations d - mean inherit the absolute error of d).  -> the two worst errors relative to d_max."""
    mean64, std64, count = R.stats_of(d2, sel, dim)
    live = count > 0
    d_max = np.sqrt(np.where(sel, d2, 0.0).max(axis=1) + 1e-4 / dim)
    e_mean = np.abs(host(stats.mean).astype(np.float64)[live] - mean64[live]) / d_max[live]
    e_std = np.abs(host(stats.std).astype(np.float64)[live] - std64[live]) / d_max[live]
    worst = (e_mean.max(initial=0.0), e_std.max(initial=0.0))
    print(f"{what} mean / std error relative to d_max: {worst[0]:.3g} / {worst[1]:.3g}")
    assert worst[0] <= STAT_TOL and worst[1] <= STAT_TOL, (what, worst)
    np.testing.assert_array_equal(host(stats.count), count)
    return worst


# ---- 1. integer data: the screening is exact, so the selection is the restatement's ----------------------------------
_int_cache = {}


def int_data(D):
    """Entries in {-1, 0, 1}: every norm, dot product and d^2 is an integer below 2^24.  Cohort rows 127, 128 and 650
    are one row (a tie across a tile boundary), and row 0 of emb is that row.  At D = 4 there are only 81 distinct
    rows: every K cuts through a run of equal values."""
    if D not in _int_cache:
        rs = np.random.RandomState(200 + D)
        q = rs.randint(-1, 2, (max(INT_NS), D)).astype(np.float32)
        g = rs.randint(-1, 2, (max(INT_MS), D)).astype(np.float32)
        g[128] = g[127]
        g[650] = g[127]
        q[0] = g[127]
        _int_cache[D] = (q, g, R.squared_distances(q, g), {})
    return _int_cache[D]


def int_selection(D, m, k):
    _, _, d2, sels = int_data(D)
    if (m, k) not in sels:
        sels[(m, k)] = R.select(d2[:, :m], k)
    return sels[(m, k)]


def case_integer_selection(env, D, K, row_block):
    q, g, d2, _ = int_data(D)
    for m in INT_MS:
        k = m if K is None else min(K, m)
        gd = env.dev(g[:m])
        want = int_selection(D, m, k)
        for n in INT_NS:
            st = env.scoring.cohort_stats(env.dev(q[:n]), gd, k, row_block=row_block, return_mask=True)
            assert st.mean.dtype == torch.float32 and st.count.dtype == torch.int32 and st.mask.dtype == torch.int32
            assert tuple(st.mask.shape) == (n, (m + 31) // 32) and tuple(st.mean.shape) == (n,)
            got = mask_of(st, m)
            np.testing.assert_array_equal(got, want[:n], err_msg=f"N={n} M={m} K={k}")
            assert (host(st.count) == k).all()
            pad = R.unpack_mask(host(st.mask), 32 * st.mask.shape[1])[:, m:]
            assert not pad.any()                               # no bit beyond the cohort
        assert_stats_of_returned_set(d2[:n, :m], got, st, D, f"int D={D} M={m} K={k}")
        if D == 512 and m >= 700 and k <= 3:                   # the planted tie, cut in index order
            assert np.nonzero(got[0])[0].tolist() == [127, 128, 650][:k]


def case_tie_cut(env):
    """K inside the run of three equal rows: the lowest indices are taken."""
    q, g, _, _ = int_data(512)
    for k, want in ((1, [127]), (2, [127, 128]), (3, [127, 128, 650])):
        st = env.scoring.cohort_stats(env.dev(q[:2]), env.dev(g[:700]), k, return_mask=True)
        assert np.nonzero(mask_of(st, 700)[0])[0].tolist() == want
        eps = np.float32(1e-4 / 512)
        if k == 1:
            assert bits(st.mean)[0] == np.sqrt(eps).view(np.int32) and host(st.std)[0] == 0.0
        assert abs(float(host(st.mean)[0]) - float(np.sqrt(eps))) <= 1e-9 and host(st.std)[0] <= 1e-9


def case_capacity_edge(env):
    """M = DS_COHORT_MAX_M: the keys of the row fill the LDS beside the histogram; one more row is refused."""
    rs = np.random.RandomState(77)
    m, k = COHORT_MAX_M, 300
    q = rs.randint(-1, 2, (2, 4)).astype(np.float32)
    g = rs.randint(-1, 2, (m + 1, 4)).astype(np.float32)
    st = env.scoring.cohort_stats(env.dev(q), env.dev(g[:m]), k, return_mask=True)
    d2 = R.squared_distances(q, g[:m])
    got = mask_of(st, m)
    np.testing.assert_array_equal(got, R.select(d2, k))
    assert_stats_of_returned_set(d2, got, st, 4, "capacity edge")
    with pytest.raises(ValueError):
        env.scoring.cohort_stats(env.dev(q), env.dev(g), k)
    raw = env.eng.lib.raw
    assert raw("ds_cohort_workspace_bytes")(2, m, 4, k, 0) > 0
    assert raw("ds_cohort_workspace_bytes")(2, m + 1, 4, k, 0) == -1


# ---- 2. real-valued rows on the radius-10 sphere ---------------------------------------------------------------------
REAL_N, REAL_M, REAL_D, REAL_K = 130, 2500, 512, 300
_real_cache = {}


def sphere(rs, n, d=REAL_D):
    x = rs.randn(n, d)
    return (10.0 * x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def real_data():
    if not _real_cache:
        rs = np.random.RandomState(17)
        q, g = sphere(rs, REAL_N), sphere(rs, REAL_M)
        d2 = R.squared_distances(q, g)
        _real_cache["v"] = (q, g, d2)
    return _real_cache["v"]


def real_stats(env, **kw):
    """cohort_stats of the real-valued data with K = REAL_K, once per environment and argument set"""
    key = (env.device.type, tuple(sorted(kw.items())))
    if _real_cache.get("stats_key") != key:
        q, g, _ = real_data()
        _real_cache["stats"] = env.scoring.cohort_stats(env.dev(q), env.dev(g), REAL_K, return_mask=True, **kw)
        _real_cache["stats_key"] = key
    return _real_cache["stats"]


def assert_membership(d2, sel, q, g, k):
    """The a-priori band of the identify test, (D + 2) 2^-24 (|q| + |g|)^2, around the K-th true value: everything
    strictly inside it below is selected, nothing beyond it above, exactly K bits."""
    qn = np.linalg.norm(q.astype(np.float64), axis=1)
    gn = np.linalg.norm(g.astype(np.float64), axis=1)
    band = (q.shape[1] + 2) * 2.0 ** -24 * (qn[:, None] + gn[None, :]) ** 2
    d_k = np.sort(d2, axis=1)[:, k - 1]
    assert (sel.sum(axis=1) == k).all()
    must = d2 < d_k[:, None] - band
    never = d2 > d_k[:, None] + band
    in_band = (~must & ~never).sum(axis=1)
    print("rows inside the band per query: max", in_band.max(), "band max", band.max())
    assert (sel | ~must).all()
    assert not (sel & never).any()


def case_real_valued(env):
    q, g, d2 = real_data()
    st = real_stats(env)
    sel = mask_of(st, REAL_M)
    assert_stats_of_returned_set(d2, sel, st, REAL_D, "real-valued")           # (a)
    assert_membership(d2, sel, q, g, REAL_K)                                    # (b)


def case_duplicate_row(env):
    """(c) an exact copy of a query in the cohort: its screening value is rounding noise around zero, of either sign --
    the signed-key path.  The copy is selected, and at K = 1 the mean is sqrt(eps), bit for bit."""
    q, g, d2 = real_data()
    g2 = g.copy()
    rows, at = (3, 64, 129), (1700, 5, 2499)
    for r, j in zip(rows, at):
        g2[j] = q[r]
    qd, gd = env.dev(q), env.dev(g2)
    _, i = env.scoring.nearest(qd, gd, 1)          # (nearest reports the rescored distance; the copy must win there too)
    assert [int(host(i)[r, 0]) for r in rows] == list(at)
    d2b = R.squared_distances(q, g2)
    eps = np.float32(1e-4 / REAL_D)
    for k in (1, 2, 3):
        st = env.scoring.cohort_stats(qd, gd, k, return_mask=True)
        sel = mask_of(st, REAL_M)
        for r, j in zip(rows, at):
            assert sel[r, j], (k, r)
        assert_membership(d2b, sel, q, g2, k)
        assert_stats_of_returned_set(d2b, sel, st, REAL_D, f"duplicate K={k}")
        if k == 1:
            for r in rows:
                assert bits(st.mean)[r] == np.sqrt(eps).view(np.int32) and host(st.std)[r] == 0.0


def case_independence(env):
    q, g, d2 = real_data()
    qd, gd = env.dev(q), env.dev(g)
    st = real_stats(env)
    sel = mask_of(st, REAL_M)

    def same_bits(other, rows=slice(None)):
        np.testing.assert_array_equal(bits(other.mean), bits(st.mean)[rows])
        np.testing.assert_array_equal(bits(other.std), bits(st.std)[rows])
        np.testing.assert_array_equal(host(other.count), host(st.count)[rows])

    st5 = env.scoring.cohort_stats(qd[:5].contiguous(), gd, REAL_K, return_mask=True)
    same_bits(st5, slice(0, 5))
    np.testing.assert_array_equal(host(st5.mask), host(st.mask)[:5])
    for rb in ROW_BLOCKS:
        s = env.scoring.cohort_stats(qd, gd, REAL_K, row_block=rb, return_mask=True)
        same_bits(s)
        np.testing.assert_array_equal(host(s.mask), host(st.mask))
    far = np.random.RandomState(18).randn(300, REAL_D).astype(np.float32) + 40.0
    sf = env.scoring.cohort_stats(qd, env.dev(np.concatenate([g, far])), REAL_K, return_mask=True)
    same_bits(sf)
    self_far = mask_of(sf, REAL_M + 300)
    np.testing.assert_array_equal(self_far[:, :REAL_M], sel)
    assert not self_far[:, REAL_M:].any()
    # the cohort rotated by 37 rows: the same set (rotated); other tiles, lanes and reduction order
    shifted = np.concatenate([g[-37:], g[:-37]])
    sr = env.scoring.cohort_stats(qd, env.dev(shifted), REAL_K, return_mask=True)
    np.testing.assert_array_equal(np.roll(sel, 37, axis=1), mask_of(sr, REAL_M))
    assert_stats_of_returned_set(np.roll(d2, 37, axis=1), mask_of(sr, REAL_M), sr, REAL_D, "rotated")


def case_agrees_with_nearest(env):
    q, g, d2 = real_data()
    qd, gd = env.dev(q), env.dev(g)
    k = 32
    dist, idx = env.scoring.nearest(qd, gd, k)
    st = env.scoring.cohort_stats(qd, gd, k, return_mask=True)
    want = np.zeros((REAL_N, REAL_M), bool)
    np.put_along_axis(want, host(idx), True, axis=1)
    np.testing.assert_array_equal(mask_of(st, REAL_M), want)
    d = host(dist).astype(np.float64)
    err = np.abs(host(st.mean) - d.mean(axis=1)) / d.max(axis=1)
    print("mean against nearest's distances, relative to d_max:", err.max())
    assert err.max() <= STAT_TOL


def _wave_butterfly_f32(v):
    """the xor butterfly of 64 float32 lane values (32, 16, ... 1): what lane 0 ends up with"""
    v = v.astype(np.float32).copy()
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = (v + v[lanes ^ m]).astype(np.float32)
    return v[0]


def _fixed_order_sum_f32(x):
    """The kernel's documented reduction of up to 256 float32 entries: thread t holds entry t, the lanes of a wave fold
    by butterfly, the four waves' sums are added in wave order."""
    part = np.zeros(256, np.float32)
    part[:len(x)] = x
    w = [_wave_butterfly_f32(part[64 * i:64 * i + 64]) for i in range(4)]
    return np.float32(np.float32(np.float32(w[0] + w[1]) + w[2]) + w[3])


def case_statistics_bits(env):
    """The statistics are the documented fixed-order two-pass reduction of PairwiseDistance's own bits: `nearest`
    reports those bits for the same set (K = 32), so the mean and the deviation are reproducible bit for bit."""
    q, g, _ = real_data()
    qd, gd = env.dev(q), env.dev(g)
    for k in (1, 3, 4, 32):                                    # short groups of the four-pair walk, and full ones
        dist, idx = env.scoring.nearest(qd, gd, k)
        st = env.scoring.cohort_stats(qd, gd, k)
        d, i = host(dist), host(idx)
        by_index = np.take_along_axis(d, np.argsort(i, axis=1), axis=1)        # the list is in index order
        want_mean = np.empty(REAL_N, np.float32)
        want_std = np.empty(REAL_N, np.float32)
        for r in range(REAL_N):
            mu = np.float32(_fixed_order_sum_f32(by_index[r]) / np.float32(k))
            dev = (by_index[r] - mu).astype(np.float32)
            ss = _fixed_order_sum_f32((dev * dev).astype(np.float32))
            want_mean[r], want_std[r] = mu, np.sqrt(np.float32(ss / np.float32(k)))
        np.testing.assert_array_equal(bits(st.mean), want_mean.view(np.int32), err_msg=f"K={k}")
        np.testing.assert_array_equal(bits(st.std), want_std.view(np.int32), err_msg=f"K={k}")


# ---- 3. labels -------------------------------------------------------------------------------------------------------
def case_labels(env, exclude):
    q, g, d2, _ = int_data(512)
    n, m, k = 33, 700, 32
    rs = np.random.RandomState(19)
    ql = rs.randint(0, 5, n).astype(np.int64)
    gl = rs.randint(0, 5, m).astype(np.int64)
    ql[1] = 9                                                  # a label the cohort does not have
    ql[2] = 5
    gl[[3, 400, 699]] = 5                                      # ... and one it has three times: fewer than K
    gl[[127, 128, 650]] = (ql[0], (ql[0] + 1) % 5, ql[0])      # the planted tie: partly the row's speaker
    st = env.scoring.cohort_stats(env.dev(q[:n]), env.dev(g[:m]), k, labels=env.dev(ql), cohort_labels=env.dev(gl),
                                  exclude=exclude, return_mask=True)
    want = R.select(d2[:n, :m], k, ql, gl, exclude)
    got = mask_of(st, m)
    np.testing.assert_array_equal(got, want)
    assert_stats_of_returned_set(d2[:n, :m], got, st, 512, f"labels {exclude}")
    cnt, mean, std = host(st.count), host(st.mean), host(st.std)
    if exclude == "other":
        assert cnt[1] == 0 and np.isposinf(mean[1]) and std[1] == 0.0
        assert cnt[2] == 3 and np.nonzero(got[2])[0].tolist() == [3, 400, 699] and np.isfinite(mean[2])
    else:
        assert cnt[1] == k and cnt[2] == k
    elig = (gl[None, :] != ql[:, None]) if exclude == "same" else (gl[None, :] == ql[:, None])
    assert not (got & ~elig).any()
    assert (cnt == np.minimum(k, elig.sum(axis=1))).all()


# ---- 4. apply --------------------------------------------------------------------------------------------------------
def case_apply(env, T):
    rs = np.random.RandomState(23 + T)
    na, nb = 37, 53
    raw = (14.0 + rs.randn(T)).astype(np.float32)
    mean_a, mean_b = (13.0 + rs.rand(na)).astype(np.float32), (13.5 + rs.rand(nb)).astype(np.float32)
    std_a, std_b = (0.2 + rs.rand(na)).astype(np.float32), (0.3 + rs.rand(nb)).astype(np.float32)
    std_a[5] = 0.01                                            # below min_std
    std_b[7] = 0.0
    ia, ib = rs.randint(0, na, T).astype(np.int64), rs.randint(0, nb, T).astype(np.int64)
    ia[0], ib[0] = 5, 7
    min_std = 0.1
    eng = env.eng

    def run(ia_, ib_, ma, sa, mb, sb):
        t = [None if a is None else env.dev(a) for a in (raw, ia_, ib_, ma, sa, mb, sb)]
        out = torch.empty(T, dtype=torch.float32, device=env.device)
        eng.lib.call("ds_score_norm_apply_f32", *[eng._p(x) for x in t], min_std, eng._p(out), T, eng._stream(out))
        want = R.apply(raw, ma, sa, ia_, mb, sb, ib_, np.float32(min_std))
        err = np.abs(host(out) - want).max() / np.abs(want).max()
        print(f"apply T={T}: error relative to max |out| {err:.3g}")
        assert err <= 1e-6

    run(ia, None, mean_a, std_a, None, None)                   # one side
    run(ia, ib, mean_a, std_a, mean_b, std_b)                  # both sides
    full = lambda v: np.resize(v, T).astype(np.float32)        # NULL indices: tables of T rows
    run(None, None, full(mean_a), full(std_a), full(mean_b), full(std_b))
    run(None, ib, full(mean_a), full(std_a), mean_b, std_b)


# ---- 5. end to end ---------------------------------------------------------------------------------------------------
def case_end_to_end(env, kind):
    q, g, d2e = real_data()
    test = sphere(np.random.RandomState(29), 130)
    d2t = R.squared_distances(test, g)
    rs = np.random.RandomState(31)
    T = 400
    ie, it = rs.randint(0, 130, T).astype(np.int64), rs.randint(0, 130, T).astype(np.int64)
    qd, td, gd = env.dev(q), env.dev(test), env.dev(g)
    top_k = REAL_K
    es = env.scoring.cohort_stats(qd, gd, top_k)
    ts = env.scoring.cohort_stats(td, gd, top_k)
    raw = env.eng.pairwise_distance(qd[env.dev(ie)].contiguous(), td[env.dev(it)].contiguous())
    out = host(env.scoring.normalise_scores(raw, kind, enrol_stats=es if kind != "t" else None,
                                            test_stats=ts if kind != "z" else None,
                                            enrol_index=env.dev(ie), test_index=env.dev(it)))
    k = top_k
    raw64 = np.sqrt(((q[ie].astype(np.float64) - test[it].astype(np.float64)) ** 2).sum(axis=1) + 1e-4 / REAL_D)
    want = np.zeros(T)
    bound = np.zeros(T)
    sides = [(d2e, ie)] * (kind != "t") + [(d2t, it)] * (kind != "z")
    for d2, index in sides:
        sel = R.select(d2, k)
        mean, std, _ = R.stats_of(d2, sel, REAL_D)
        z = (raw64 - mean[index]) / std[index]
        d_max = np.maximum(np.sqrt(np.where(sel, d2, 0.0).max(axis=1))[index], raw64)
        want += z / len(sides)
        bound += STAT_TOL * d_max * (2.0 + np.abs(z)) / std[index]
    err = np.abs(out - want)
    print(f"end to end {kind}: worst error / bound {(err / bound).max():.3g}, |z| up to {np.abs(want).max():.3g}")
    assert (err <= bound).all()
    if kind == "as":           # "s" is the same arithmetic: the spelling says which top_k the statistics were taken with
        again = env.scoring.normalise_scores(raw, "s", enrol_stats=es, test_stats=ts, enrol_index=env.dev(ie),
                                             test_index=env.dev(it))
        np.testing.assert_array_equal(host(again), out)


# ---- 6. minDCF and the signed threshold grid -------------------------------------------------------------------------
def clear_of_grid(scores, thr_start, thr_stop, thr_step):
    """Scores moved away from every threshold of the grid (by a third of a step where closer than 1e-4), so that the
    prediction dist < thr does not hang on how the device rounds the threshold."""
    s = scores.astype(np.float32).copy()
    for thr in R.thresholds_f32(thr_start, thr_stop, thr_step):
        j = np.clip(np.searchsorted(thr, s), 1, len(thr) - 1)
        near = np.minimum(np.abs(s - thr[j - 1]), np.abs(s - thr[j])) < 1e-4
        s[near] += np.float32(thr_step / 3)
    return s


def check_dcf(env, scores, labels, grid, **cost):
    tp, fp = R.roc_counts(scores, labels, R.thresholds_f32(*grid)[0])
    n_same = int((labels != 0).sum())
    want, at = R.min_dcf(tp, fp, n_same, len(labels) - n_same, **cost)
    value, thr = env.scoring.min_dcf(env.dev(scores), env.dev(labels), thr_start=grid[0], thr_stop=grid[1],
                                     thr_step=grid[2], **cost)
    assert abs(value - want) <= 1e-12 * max(1.0, want), (value, want)
    assert abs(thr - (grid[0] + grid[2] * at)) <= 1e-9
    return value


def case_min_dcf(env):
    rs = np.random.RandomState(37)
    grid = (0.0, 30.0, 0.01)
    labels = (rs.rand(2000) < 0.3).astype(np.int64)
    scores = clear_of_grid(np.where(labels != 0, 11.0, 14.5) + 1.5 * rs.randn(2000), *grid)
    v = check_dcf(env, scores, labels, grid)
    assert 0.0 < v < 1.0
    v2 = check_dcf(env, scores, labels, grid, p_target=0.05, c_miss=10.0, c_fa=1.0)
    assert v2 != v
    # perfectly separable: exactly 0
    sep = clear_of_grid(np.where(labels != 0, 5.0, 20.0) + rs.rand(2000), *grid)
    assert check_dcf(env, sep, labels, grid) == 0.0
    # one label only: the missing class's error rate is 0 by definition.  A fifth of the same-speaker scores lies beyond
    # the grid, so P_miss never falls below 0.2 and, with c_miss p the smaller cost, that is the value
    ones = np.ones(2000, np.int64)
    beyond = clear_of_grid(np.where(np.arange(2000) % 5 == 0, 35.0, 12.0) + rs.rand(2000), *grid)
    assert abs(check_dcf(env, beyond, ones, grid) - 0.2) <= 1e-12
    assert check_dcf(env, beyond, np.zeros(2000, np.int64), grid) == 0.0


def case_signed_grid(env):
    """evaluate and min_dcf on normalised (signed) scores over thresholds -10 .. 10."""
    rs = np.random.RandomState(41)
    grid = (-10.0, 10.0, 0.01)
    labels = (rs.rand(3000) < 0.4).astype(np.int64)
    scores = clear_of_grid(np.where(labels != 0, -2.0, 1.0) + 1.2 * rs.randn(3000), *grid)
    scores[:4] = (-12.0, -10.5, 10.5, 12.0)                    # beyond both ends
    res = env.scoring.evaluate(env.dev(scores), env.dev(labels), *grid)
    tp, fp = R.roc_counts(scores, labels, R.thresholds_f32(*grid)[0])
    assert len(tp) == 2000 and (scores < 0).sum() > 1000
    np.testing.assert_array_equal(host(res.tp), tp)
    np.testing.assert_array_equal(host(res.fp), fp)
    n_same = int(labels.sum())
    eer = R.equal_error_rate(tp, fp, n_same, len(labels) - n_same)
    print("signed grid: EER", res.eer, "restatement", eer, "at", res.eer_threshold)
    assert 0.02 < eer < 0.3 and abs(res.eer - eer) <= 1e-5
    assert -10.0 < res.eer_threshold < 10.0 and -10.0 < res.threshold < 10.0
    check_dcf(env, scores, labels, grid)


# ---- 7. errors -------------------------------------------------------------------------------------------------------
def case_errors(env):
    z = lambda n, d: torch.zeros((n, d), dtype=torch.float32, device=env.device)
    S = env.scoring
    lab = lambda n: torch.zeros(n, dtype=torch.int64, device=env.device)
    with pytest.raises(ValueError):
        S.cohort_stats(z(2, 6), z(3, 6))                       # D not a multiple of 4
    with pytest.raises(ValueError):
        S.cohort_stats(z(2, 8), z(3, 8), 0)                    # K < 1
    with pytest.raises(ValueError):
        S.cohort_stats(z(2, 8), z(3, 8), 4)                    # K > M
    with pytest.raises(ValueError):
        S.cohort_stats(z(2, 4), z(COHORT_MAX_M + 1, 4))        # M above the cap
    with pytest.raises(ValueError):
        S.cohort_stats(z(2, 8), z(3, 12))                      # mismatched D
    with pytest.raises(ValueError):
        S.cohort_stats(z(2, 2052), z(3, 2052))
    with pytest.raises(ValueError):
        S.cohort_stats(z(2, 8), z(3, 8), exclude="same")       # exclude without labels
    with pytest.raises(ValueError):
        S.cohort_stats(z(2, 8), z(3, 8), labels=lab(2), exclude="other")
    with pytest.raises(ValueError):
        S.cohort_stats(z(2, 8), z(3, 8), exclude="different")
    with pytest.raises(ValueError):
        S.cohort_stats(z(2, 8), z(3, 8), row_block=-1)
    if env.device.type == "cuda":
        with pytest.raises(ValueError):
            S.cohort_stats(z(2, 8), z(3, 8).cpu())             # mismatched devices
    st = S.cohort_stats(z(2, 8), z(3, 8))
    raw = torch.ones(2, dtype=torch.float32, device=env.device)
    with pytest.raises(ValueError):
        S.normalise_scores(raw, "x", enrol_stats=st)           # an unknown kind
    with pytest.raises(ValueError):
        S.normalise_scores(raw, "z", test_stats=st)            # "z" without enrol_stats
    with pytest.raises(ValueError):
        S.normalise_scores(raw, "as", enrol_stats=st)
    with pytest.raises(ValueError):
        S.normalise_scores(torch.ones(5, dtype=torch.float32, device=env.device), "z", enrol_stats=st)  # no index, 2 rows
    assert tuple(S.normalise_scores(raw, "z", enrol_stats=st).shape) == (2,)
    # the C ABI says no before it launches anything
    r = env.eng.lib.raw
    assert r("ds_cohort_workspace_bytes")(2, 3, 6, 1, 0) == -1
    assert r("ds_cohort_workspace_bytes")(2, 3, 8, 0, 0) == -1
    assert r("ds_cohort_workspace_bytes")(2, 3, 8, 4, 0) == -1
    assert r("ds_cohort_workspace_bytes")(2, 3, 2052, 1, 0) == -1
    assert r("ds_cohort_workspace_bytes")(2, 3, 8, 3, 0) > 0
    assert r("ds_cohort_stats_f32")(None, None, None, None, 0, None, None, None, None, None, 2, 3, 8, 1, 0, None) == -3
    assert r("ds_score_norm_apply_f32")(None, None, None, None, None, None, None, 1e-6, None, 1, None) == -3
    p = env.eng._p
    a, b, ws = z(2, 8), z(3, 8), torch.zeros(64, dtype=torch.int32, device=env.device)
    f, i = torch.zeros(2, dtype=torch.float32, device=env.device), torch.zeros(2, dtype=torch.int32, device=env.device)
    assert r("ds_cohort_stats_f32")(p(a), p(b), None, None, 0, p(ws), p(f), p(f), p(i), None, 2, 3, 6, 1, 0, None) == -1
    assert r("ds_cohort_stats_f32")(p(a), p(b), None, None, 0, p(ws), p(f), p(f), p(i), None, 2, 3, 8, 4, 0, None) == -1
    assert r("ds_cohort_stats_f32")(p(a), p(b), None, None, 1, p(ws), p(f), p(f), p(i), None, 2, 3, 8, 1, 0, None) == -3
    assert r("ds_score_norm_apply_f32")(p(f), None, None, p(f), p(f), p(f), None, 1e-6, p(f), 2, None) == -3
    assert r("ds_score_norm_apply_f32")(p(f), None, None, p(f), p(f), None, None, 1e-6, p(f), 0, None) == -1
