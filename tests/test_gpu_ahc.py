"""GPU: speaker diarisation (csrc/ahc.hip, deepspeaker_pytorch_amd.diarisation) on the device, against the
restatements in tests/ahc_reference.py: the cases of test_emul_ahc.py, plus a recording at the cap, the three steps
replayed from a captured graph and the chain from the model's own embeddings."""
import numpy as np
import pytest
import torch

import ahc_cases as C
import ahc_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture
def env():
    from deepspeaker_pytorch_amd import diarisation
    from deepspeaker_pytorch_amd.model import get_engine
    return C.Env(diarisation, get_engine(), torch.device("cuda", 0))


@pytest.mark.parametrize("method", C.METHODS)
def test_linkage_is_the_float32_restatement_bit_for_bit(env, method):
    C.case_linkage_bit_exact(env, method)


@pytest.mark.parametrize("method", C.METHODS)
def test_ties_go_to_the_lowest_slots(env, method):
    C.case_ties(env, method)


def test_result_does_not_depend_on_the_batch(env):
    C.case_independence(env)


@pytest.mark.parametrize("dim", (512, 40))
def test_distances_are_pairwise_distance_bits(env, dim):
    C.case_distances(env, dim)


def test_cut(env):
    C.case_cut(env)


@pytest.mark.parametrize("k,n,seed", C.SCIPY_CASES)
def test_against_scipy_end_to_end(env, k, n, seed):
    C.case_against_scipy(env, k, n, seed)


def test_errors(env):
    C.case_errors(env)


def test_a_recording_at_the_cap(env):
    """DS_AHC_MAX_N rows: single linkage does no arithmetic, so SciPy's float64 run on the same float32 values has the
    same heights exactly -- sorted, as single linkage is monotone -- and the same seven clusters."""
    from scipy.cluster.hierarchy import fcluster, linkage
    n = C.AHC_MAX_N
    m = C.random_symmetric(np.random.RandomState(113), n)
    dist = env.dia.RaggedMatrices.from_matrices([m], env.device)
    d = env.dia.linkage(dist, "single", overwrite=True)
    Z = linkage(m[np.triu_indices(n, 1)].astype(np.float64), "single")
    got = C.dendrogram_of(env, 0, d)
    np.testing.assert_array_equal(got["height"].astype(np.float64), Z[:, 2])
    assert got["size"][-1] == n and (got["step"] == -1).sum() == 1 and sorted(got["step"].tolist())[1:] == list(range(n - 1))
    labels, n_found = env.dia.cut(d, n_clusters=7)
    assert C.host(n_found)[0] == 7
    assert C.host(labels).tolist() == R.first_appearance(fcluster(Z, 7, criterion="maxclust")).tolist()


def test_three_steps_in_a_captured_graph(env):
    """Nothing in the library allocates, synchronises or reads back: distances, linkage and cut replay from a graph."""
    rs = np.random.RandomState(127)
    off = [0, 90, 90, 91, 300]
    x = env.dev(rs.randn(300, 64).astype(np.float32))

    def run():
        dist = env.dia.pairwise_distances(x, off)
        d = env.dia.linkage(dist, "average")
        labels, n_found = env.dia.cut(d, threshold=10.5, n_clusters=3)
        return dist, d, labels, n_found

    eager = run()                                                  # (also leaves the plan's table on the device)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            dist, d, labels, n_found = run()
    for t in (dist.data, d.height, labels):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(C.bits(C.host(dist.data)), C.bits(C.host(eager[0].data)))
    for key in ("pair", "height", "size", "into", "step"):
        np.testing.assert_array_equal(C.bits(C.host(getattr(d, key))), C.bits(C.host(getattr(eager[1], key))))
    np.testing.assert_array_equal(C.host(labels), C.host(eager[2]))
    np.testing.assert_array_equal(C.host(n_found), C.host(eager[3]))
    assert 1 < C.host(n_found)[3] <= 209 and C.host(n_found)[1] == 0


def test_model_embeddings_to_turns(env):
    """windows -> crops -> a seeded two-stage model -> cluster -> turns: the labels are the restatement's on the model's
    own embeddings, and the turns tile every recording."""
    from deepspeaker_pytorch_amd.data import FeatureStore
    from deepspeaker_pytorch_amd.model import DeepSpeakerModel
    from deepspeaker_pytorch_amd.synthetic import synthetic_state_dict
    sd = synthetic_state_dict(seed=5, num_classes=4, n_stages=2)
    m = DeepSpeakerModel(512, 4, n_stages=2)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    m = m.cuda().eval()
    rs = np.random.RandomState(131)
    voices = 2.0 * rs.randn(3, 64)                                 # three "voices": a mean spectrum each
    plans = ([(0, 400), (1, 330), (0, 250)], [(2, 100)], [(1, 500), (2, 420), (1, 90), (0, 300)])
    recs = [np.concatenate([voices[v] + 0.5 * rs.randn(t, 64) for v, t in plan]).astype(np.float32) for plan in plans]
    store = FeatureStore(recs, device="cuda")
    window, hop = 160, 80
    turns = env.dia.diarise(m, store, window=window, hop=hop, n_clusters=3, batch=16)
    lengths = [len(r) for r in recs]
    rec_idx, starts, win_off = env.dia.sliding_windows(lengths, window, hop)
    with torch.no_grad():
        emb = torch.cat([m(store.crops(rec_idx[s:s + 16], starts[s:s + 16], window)) for s in range(0, len(rec_idx), 16)])
    dist = env.dia.pairwise_distances(emb, win_off)
    for r, t in enumerate(lengths):
        n = int(win_off[r + 1] - win_off[r])
        link = R.linkage_f32(C.host(dist.matrix(r)), "average")
        want, found = R.cut(link, n, n_clusters=3)
        s = starts[win_off[r]:win_off[r + 1]]
        assert turns[r] == env.dia.turns_of(env.dia.frame_labels(s, want, window, t))
        assert turns[r][0][0] == 0 and turns[r][-1][1] == t        # the turns tile the recording
        assert all(a[1] == b[0] and a[2] != b[2] for a, b in zip(turns[r], turns[r][1:]))
        assert all(a < b for a, b, _ in turns[r])
        assert len({sp for _, _, sp in turns[r]}) == found == min(3, n)
    # a store after voice-activity selection: turns in original frame indices, broken at removed frames
    kept = np.ones(sum(lengths), np.uint8)
    kept[200:260] = 0
    off = np.concatenate([[0], np.cumsum(lengths)])
    small = FeatureStore([r[kept[off[i]:off[i + 1]] != 0] for i, r in enumerate(recs)], device="cuda")
    vt = env.dia.diarise(m, small, window=window, hop=hop, n_clusters=3, batch=16,
                         voiced=(torch.from_numpy(kept).cuda(), off))
    assert vt[0][0][0] == 0 and vt[0][-1][1] == lengths[0]
    assert any(a[1] == 200 and b[0] == 260 for a, b in zip(vt[0], vt[0][1:]))
    assert sum(b - a for a, b, _ in vt[0]) == lengths[0] - 60
