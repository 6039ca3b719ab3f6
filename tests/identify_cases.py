"""TEST INFRASTRUCTURE: the identification cases (scoring.nearest / speaker_models / identify, csrc/identify.hip)
shared by the host-emulator file and the GPU file, each against the float64 restatement in identify_reference.py.
A case takes `env`: the scoring module bound to an engine, that engine and the device the tensors live on."""
from dataclasses import dataclass

import numpy as np
import pytest
import torch

import identify_reference as R

INT_NS = (1, 33, 130)                   # one wave-row, a ragged block, three query blocks
INT_MS = (1, 5, 127, 128, 129, 700)     # below / at / above the 128-row tile, six tiles
INT_KS = (1, 5, 32, 64)
INT_SPLITS = (0, 1, 3)
INT_DS = (4, 512)


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


# ---- 1. integer data: the screening is exact, so the indices are the restatement's ----------------------------------
_int_cache = {}


def int_data(D):
    """Entries in {-1, 0, 1}: every norm, dot product and d^2 is an integer below 2^24.  Gallery rows 127, 128 and 650
    are one row (a tie across a tile boundary and across a split boundary), and query 0 is that row."""
    if D not in _int_cache:
        rs = np.random.RandomState(100 + D)
        q = rs.randint(-1, 2, (max(INT_NS), D)).astype(np.float32)
        g = rs.randint(-1, 2, (max(INT_MS), D)).astype(np.float32)
        g[128] = g[127]
        g[650] = g[127]
        q[0] = g[127]
        ref = {}
        for m in INT_MS:
            _, order, dist = R.nearest(q, g[:m], max(INT_KS))
            ref[m] = (order, dist)
        _int_cache[D] = (q, g, ref)
    return _int_cache[D]


def case_integer_identity(env, D, k, splits):
    q, g, ref = int_data(D)
    for m in INT_MS:
        gd = env.dev(g[:m])
        order, dist = ref[m]
        for n in INT_NS:
            d, i = env.scoring.nearest(env.dev(q[:n]), gd, k, splits=splits)
            assert i.dtype == torch.int64 and d.dtype == torch.float32 and tuple(i.shape) == (n, k)
            np.testing.assert_array_equal(host(i), order[:n, :k], err_msg=f"N={n} M={m}")
            got = host(d)
            assert np.isinf(got[order[:n, :k] < 0]).all() and (got[order[:n, :k] < 0] > 0).all()
            fin = order[:n, :k] >= 0
            assert np.abs(got[fin] - dist[:n, :k][fin]).max(initial=0.0) <= 1e-6 * max(1.0, dist[:n, :k][fin].max(initial=0.0))
    if k >= 3 and D == 512:                    # the planted tie is really there, in index order (at D = 4 many rows are equal)
        assert host(i)[0, :3].tolist() == [127, 128, 650]


# ---- 2. / 3. real-valued data ---------------------------------------------------------------------------------------
REAL_N, REAL_M, REAL_D, REAL_K = 130, 700, 512, 32
_real_cache = {}


def real_data():
    if not _real_cache:
        rs = np.random.RandomState(7)
        q = rs.randn(REAL_N, REAL_D)
        g = rs.randn(REAL_M, REAL_D)
        q = (10.0 * q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
        g = (10.0 * g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
        _real_cache["v"] = (q, g, R.nearest(q, g, REAL_K))
    return _real_cache["v"]


def case_real_valued(env):
    q, g, (d2, order, _) = real_data()
    qd, gd = env.dev(q), env.dev(g)
    d, i = env.scoring.nearest(qd, gd, REAL_K)
    idx, dist = host(i), host(d)
    assert (idx >= 0).all() and (idx < REAL_M).all()
    # the reported distances are PairwiseDistance(2) of the pairs, bit for bit
    pd = env.eng.pairwise_distance(qd.repeat_interleave(REAL_K, 0).contiguous(), gd[i.reshape(-1)].contiguous())
    np.testing.assert_array_equal(bits(d).reshape(-1), bits(pd))
    # ... and within 1e-6 relative of float64 (the parity table's bar for PairwiseDistance)
    true_d2 = np.take_along_axis(d2, idx, axis=1)
    want = np.sqrt(true_d2 + 1e-4 / REAL_D)
    rel = np.abs(dist - want).max() / want.max()
    print("distance rel err vs float64:", rel)
    assert rel <= 1e-6
    # membership, with an a-priori f32 bound of the screening value.  The contract's formula, 2 (D + 2) 2^-24 (|q| + |g|)^2,
    # is 2.5e-2 for rows of norm 10 while its text quotes 1.2e-2 for these inputs: the check takes the smaller, i.e. half
    # the formula, (D + 2) 2^-24 (|q| + |g|)^2 = 1.2e-2.  It still bounds the value's error: with u = 2^-24 the D
    # roundings of the dot product cost at most 2 D u |q| |g| <= D u (|q| + |g|)^2 / 2, the two norms (8 sequential terms
    # and 6 butterfly steps per lane) and the two final operations at most 16 u (|q|^2 + |g|^2), and D / 2 + 16 < D + 2.
    qn = np.linalg.norm(q.astype(np.float64), axis=1)
    gn = np.linalg.norm(g.astype(np.float64), axis=1)
    band = (REAL_D + 2) * 2.0 ** -24 * (qn[:, None] + gn[None, :]) ** 2
    d_k = d2[np.arange(REAL_N), order[:, REAL_K - 1]]
    print("band max", band.max(), "d2 spread", d2.max() - d2.min())
    assert (true_d2 <= d_k[:, None] + np.take_along_axis(band, idx, axis=1)).all()
    must = d2 < d_k[:, None] - band
    returned = np.zeros_like(must)
    np.put_along_axis(returned, idx, True, axis=1)
    assert (returned | ~must).all()
    assert (returned.sum(axis=1) == REAL_K).all()              # no row twice
    # ascending; equal distances in index order
    assert (np.diff(dist, axis=1) >= 0).all()
    eq = np.diff(dist, axis=1) == 0
    assert (np.diff(idx, axis=1)[eq] > 0).all()


def case_batch_independence(env):
    q, g, _ = real_data()
    qd, gd = env.dev(q), env.dev(g)
    d, i = env.scoring.nearest(qd, gd, REAL_K)
    d5, i5 = env.scoring.nearest(qd[:5].contiguous(), gd, REAL_K)
    np.testing.assert_array_equal(bits(d5), bits(d)[:5])
    np.testing.assert_array_equal(host(i5), host(i)[:5])
    for splits in (1, 3):
        ds, is_ = env.scoring.nearest(qd, gd, REAL_K, splits=splits)
        np.testing.assert_array_equal(bits(ds), bits(d))
        np.testing.assert_array_equal(host(is_), host(i))
    far = np.random.RandomState(8).randn(300, REAL_D).astype(np.float32) + 40.0
    df, if_ = env.scoring.nearest(qd, env.dev(np.concatenate([g, far])), REAL_K)
    np.testing.assert_array_equal(bits(df), bits(d))
    np.testing.assert_array_equal(host(if_), host(i))


def case_screening_bits_do_not_move(env):
    """The screening value itself (ds_nearest_topk_f32, before rescoring): the bits of a pair do not depend on the
    split count, on the batch or on where the row sits in the gallery (a gallery shifted by 37 rows: other tiles,
    other lanes)."""
    q, g, _ = real_data()
    eng = env.eng

    def screen(qa, ga, k, splits):
        qd, gd = env.dev(qa), env.dev(ga)
        n, m, d = qa.shape[0], ga.shape[0], qa.shape[1]
        nb = int(eng.lib.raw("ds_nearest_workspace_bytes")(n, m, d, k, splits))
        assert nb > 0
        ws = torch.empty(nb // 4, dtype=torch.int32, device=env.device)
        sd = torch.empty((n, k), dtype=torch.float32, device=env.device)
        si = torch.empty((n, k), dtype=torch.int64, device=env.device)
        eng.lib.call("ds_nearest_topk_f32", eng._p(qd), eng._p(gd), None, None, 0, eng._p(ws), eng._p(sd), eng._p(si),
                     n, m, d, k, splits, eng._stream(qd))
        return bits(sd), host(si)

    k = 8
    s0, i0 = screen(q, g, k, 0)
    for splits in (1, 3):
        s, i = screen(q, g, k, splits)
        np.testing.assert_array_equal(s, s0)
        np.testing.assert_array_equal(i, i0)
    s, i = screen(q[40:47], g, k, 1)
    np.testing.assert_array_equal(s, s0[40:47])
    np.testing.assert_array_equal(i, i0[40:47])
    shifted = np.concatenate([g[-37:], g[:-37]])
    s, i = screen(q, shifted, k, 2)
    np.testing.assert_array_equal(s, s0)
    np.testing.assert_array_equal((i - 37) % REAL_M, i0)


# ---- 4. label filter ------------------------------------------------------------------------------------------------
def case_label_filter(env, splits):
    q, g, _ = int_data(512)
    n, m, k = 33, 700, 32
    rs = np.random.RandomState(11)
    ql = rs.randint(0, 6, n).astype(np.int64)
    gl = rs.randint(0, 6, m).astype(np.int64)
    gl[[127, 128, 650]] = (ql[0], ql[0] + 1, ql[0])          # the planted tie: partly the query's speaker
    qd, gd = env.dev(q[:n]), env.dev(g[:m])
    for exclude in ("same", "other"):
        d, i = env.scoring.nearest(qd, gd, k, query_labels=env.dev(ql), gallery_labels=env.dev(gl), exclude=exclude,
                                   splits=splits)
        idx, dist = host(i), host(d)
        for a in range(n):
            keep = np.nonzero((gl != ql[a]) if exclude == "same" else (gl == ql[a]))[0]
            _, order, rdist = R.nearest(q[a:a + 1], g[:m][keep], k)       # the restatement on the filtered gallery ...
            want = np.where(order[0] >= 0, keep[np.maximum(order[0], 0)], -1)      # ... mapped back
            np.testing.assert_array_equal(idx[a], want, err_msg=f"{exclude} query {a}")
            got_l = gl[idx[a][idx[a] >= 0]]
            assert ((got_l != ql[a]) if exclude == "same" else (got_l == ql[a])).all()
            fin = want >= 0
            assert np.isinf(dist[a][~fin]).all()
            assert np.abs(dist[a][fin] - rdist[0][fin]).max(initial=0.0) <= 1e-6 * rdist[0][fin].max(initial=1.0)


def case_label_filter_nothing_eligible(env):
    q, g, _ = int_data(512)
    qd, gd = env.dev(q[:3]), env.dev(g[:129])
    d, i = env.scoring.nearest(qd, gd, 5, query_labels=env.dev(np.array([7, 8, 7], np.int64)),
                               gallery_labels=env.dev(np.full(129, 7, np.int64)), exclude="same")
    idx, dist = host(i), host(d)
    assert (idx[[0, 2]] == -1).all() and np.isposinf(dist[[0, 2]]).all()
    assert (idx[1] >= 0).all() and np.isfinite(dist[1]).all()


# ---- 5. speaker models and rank hits --------------------------------------------------------------------------------
def case_speaker_models(env):
    sizes = [1, 2, 7, 40]
    rs = np.random.RandomState(21)
    e = rs.randn(sum(sizes), 512)
    e = (10.0 * e / np.linalg.norm(e, axis=1, keepdims=True)).astype(np.float32)
    for renorm in (False, True):
        got = host(env.scoring.speaker_models(env.dev(e), sizes, renormalise=renorm)).astype(np.float64)
        ref = R.speaker_models(e, sizes, renormalise=renorm)
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print("speaker_models renormalise =", renorm, "rel err", err)
        assert got.shape == (4, 512) and err <= 1e-6
        if renorm:
            assert np.abs(np.linalg.norm(got, axis=1) - R.ALPHA).max() <= 1e-6 * R.ALPHA
    np.testing.assert_array_equal(host(env.scoring.speaker_models(env.dev(e[:1]), [1], renormalise=False)), e[:1])


def identify_data():
    rs = np.random.RandomState(31)
    S, N, D = 40, 130, 512
    centres = rs.randn(S, D)
    sizes = [(1, 2, 7, 40)[s % 4] for s in range(S)]
    owner = np.repeat(np.arange(S), sizes)
    enrol = centres[owner] + 2.0 * rs.randn(len(owner), D)
    enrol = (10.0 * enrol / np.linalg.norm(enrol, axis=1, keepdims=True)).astype(np.float32)
    spk = rs.randint(0, S, N)
    test = centres[spk] + 6.0 * rs.randn(N, D)                 # noisy enough that rank 1 is not always right
    test = (10.0 * test / np.linalg.norm(test, axis=1, keepdims=True)).astype(np.float32)
    model_labels = (1000 + 3 * np.arange(S)).astype(np.int64)
    return enrol, sizes, test, model_labels, model_labels[spk]


def case_identify(env):
    enrol, sizes, test, model_labels, test_labels = identify_data()
    N, k = test.shape[0], 5
    models = env.scoring.speaker_models(env.dev(enrol), sizes)
    res = env.scoring.identify(env.dev(test), models, env.dev(model_labels), env.dev(test_labels), k=k)
    _, order, _ = R.nearest(test, host(models), k)
    np.testing.assert_array_equal(host(res.indices), order)
    np.testing.assert_array_equal(host(res.labels), model_labels[order])
    want = R.rank_hits(order, model_labels, test_labels)
    assert res.hits.dtype == torch.int32 and host(res.hits).tolist() == want.tolist()
    assert 0 < want[0] < N                                      # the data separates rank 1 from rank k
    assert res.rank1 == want[0] / N and res.rank_k == want[k - 1] / N
    plain = env.scoring.identify(env.dev(test), models, env.dev(model_labels), k=k)
    assert plain.hits is None and plain.rank1 is None
    np.testing.assert_array_equal(host(plain.indices), order)
    # more ranks than models: the labels of the missing ranks are -1
    few = env.scoring.identify(env.dev(test[:3]), models[:2].contiguous(), env.dev(model_labels[:2]), k=4)
    assert (host(few.indices)[:, 2:] == -1).all() and (host(few.labels)[:, 2:] == -1).all()


def case_rank_hits_many_queries(env):
    """ds_rank_hits_i32 alone on more queries than one pass of its workgroup (1024), with -1 entries."""
    rs = np.random.RandomState(41)
    n, k, m = 2500, 7, 50
    idx = rs.randint(-1, m, (n, k)).astype(np.int64)
    gl = rs.randint(0, 9, m).astype(np.int64)
    ql = rs.randint(0, 9, n).astype(np.int64)
    hits = torch.empty(k, dtype=torch.int32, device=env.device)
    eng = env.eng
    i_d, g_d, q_d = env.dev(idx), env.dev(gl), env.dev(ql)
    eng.lib.call("ds_rank_hits_i32", eng._p(i_d), eng._p(g_d), eng._p(q_d), eng._p(hits), n, k, eng._stream(i_d))
    assert host(hits).tolist() == R.rank_hits(idx, gl, ql).tolist()


# ---- 6. errors ------------------------------------------------------------------------------------------------------
def case_errors(env):
    z = lambda n, d: torch.zeros((n, d), dtype=torch.float32, device=env.device)
    nearest = env.scoring.nearest
    with pytest.raises(ValueError):
        nearest(z(2, 6), z(3, 6), 1)
    with pytest.raises(ValueError):
        nearest(z(2, 8), z(3, 8), 0)
    with pytest.raises(ValueError):
        nearest(z(2, 8), z(3, 8), 65)
    with pytest.raises(ValueError):
        nearest(z(2, 8), z(3, 12), 1)
    with pytest.raises(ValueError):
        nearest(z(2, 2052), z(3, 2052), 1)
    with pytest.raises(ValueError):
        nearest(z(2, 8), z(3, 8), 1, exclude="same")
    with pytest.raises(ValueError):
        nearest(z(2, 8), z(3, 8), 1, query_labels=torch.zeros(2, dtype=torch.int64, device=env.device), exclude="other")
    with pytest.raises(ValueError):
        nearest(z(2, 8), z(3, 8), 1, exclude="different")
    with pytest.raises(ValueError):
        nearest(z(2, 8)[0], z(3, 8), 1)
    with pytest.raises(ValueError):
        env.scoring.speaker_models(z(5, 8), [2, 2])
    # the C ABI says no before it launches anything
    raw = env.eng.lib.raw
    assert raw("ds_nearest_workspace_bytes")(2, 3, 6, 1, 0) == -1
    assert raw("ds_nearest_workspace_bytes")(2, 3, 8, 65, 0) == -1
    assert raw("ds_nearest_workspace_bytes")(2, 3, 8, 1, 0) > 0
    assert raw("ds_nearest_topk_f32")(None, None, None, None, 0, None, None, None, 2, 3, 8, 1, 0, None) == -3
