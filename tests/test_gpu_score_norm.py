"""GPU: score normalisation (csrc/score_norm.hip, scoring.cohort_stats / normalise_scores / min_dcf) on the device,
against the float64 restatement (tests/score_norm_reference.py): the cases of test_emul_score_norm.py, plus the chain
from the model's own embeddings."""
import numpy as np
import pytest
import torch

import score_norm_cases as C
import score_norm_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture
def env():
    from deepspeaker_pytorch_amd import scoring
    from deepspeaker_pytorch_amd.model import get_engine
    return C.Env(scoring, get_engine(), torch.device("cuda", 0))


@pytest.mark.parametrize("row_block", C.ROW_BLOCKS)
@pytest.mark.parametrize("K", C.INT_KS)
@pytest.mark.parametrize("D", C.INT_DS)
def test_integer_data_selection_is_exact(env, D, K, row_block):
    C.case_integer_selection(env, D, K, row_block)


def test_tie_is_cut_in_index_order(env):
    C.case_tie_cut(env)


def test_lds_capacity_edge(env):
    C.case_capacity_edge(env)


def test_real_valued_statistics_and_membership(env):
    C.case_real_valued(env)


def test_duplicate_row_signed_keys(env):
    C.case_duplicate_row(env)


def test_result_does_not_depend_on_the_batch(env):
    C.case_independence(env)


def test_agrees_with_nearest(env):
    C.case_agrees_with_nearest(env)


def test_statistics_are_the_fixed_order_reduction_of_pairwise_distance_bits(env):
    C.case_statistics_bits(env)


@pytest.mark.parametrize("exclude", ("same", "other"))
def test_label_filter(env, exclude):
    C.case_labels(env, exclude)


@pytest.mark.parametrize("T", (1, 1000, 5000))
def test_apply(env, T):
    C.case_apply(env, T)


@pytest.mark.parametrize("kind", ("z", "t", "as"))
def test_end_to_end(env, kind):
    C.case_end_to_end(env, kind)


def test_min_dcf(env):
    C.case_min_dcf(env)


def test_signed_threshold_grid(env):
    C.case_signed_grid(env)


def test_errors(env):
    C.case_errors(env)


def test_statistics_in_a_captured_graph(env):
    """Nothing in the library allocates, synchronises or reads back: the whole call replays from a graph."""
    q, g, _ = C.real_data()
    qd, gd = env.dev(q), env.dev(g)
    eager = env.scoring.cohort_stats(qd, gd, C.REAL_K, return_mask=True)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            st = env.scoring.cohort_stats(qd, gd, C.REAL_K, return_mask=True)
    st.mean.zero_()
    graph.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(C.bits(st.mean), C.bits(eager.mean))
    np.testing.assert_array_equal(C.bits(st.std), C.bits(eager.std))
    np.testing.assert_array_equal(C.host(st.mask), C.host(eager.mask))


def test_model_embeddings_to_normalised_verification(env):
    """embed -> trial_scores -> cohort_stats -> normalise_scores -> evaluate on a seeded two-stage model: the tensors
    the model produces are accepted as they are, and every stage is the restatement's on the same embeddings."""
    from deepspeaker_pytorch_amd.model import DeepSpeakerModel
    from deepspeaker_pytorch_amd.synthetic import synthetic_state_dict
    sd = synthetic_state_dict(seed=5, num_classes=4, n_stages=2)
    m = DeepSpeakerModel(512, 4, n_stages=2)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    m = m.cuda().eval()
    rs = np.random.RandomState(6)
    voices = rs.randn(6, 1, 160, 64)                           # 6 "speakers": 4 on trial, 2 as the cohort
    spk = np.repeat(np.arange(6), 6)
    x = (voices[spk] + 0.5 * rs.randn(36, 1, 160, 64)).astype(np.float32)
    with torch.no_grad():
        emb = m(torch.from_numpy(x).cuda())
    enrol_rows = np.concatenate([np.nonzero(spk == s)[0][:3] for s in range(4)])
    test_rows = np.concatenate([np.nonzero(spk == s)[0][3:] for s in range(4)])
    cohort = emb[24:]                                          # a view of the model's output
    ie, it = np.repeat(np.arange(12), 12).astype(np.int64), np.tile(np.arange(12), 12).astype(np.int64)
    same = (spk[enrol_rows][ie] == spk[test_rows][it]).astype(np.int64)
    enrol, test = emb[torch.from_numpy(enrol_rows).cuda()], emb[torch.from_numpy(test_rows).cuda()]
    raw = env.scoring.trial_scores(enrol[torch.from_numpy(ie).cuda()], test[torch.from_numpy(it).cuda()], 1)
    es = env.scoring.cohort_stats(enrol, cohort, top_k=8, return_mask=True)
    ts = env.scoring.cohort_stats(test, cohort, top_k=8)
    out = env.scoring.normalise_scores(raw, "as", enrol_stats=es, test_stats=ts, enrol_index=torch.from_numpy(ie).cuda(),
                                       test_index=torch.from_numpy(it).cuda())
    e = emb.cpu().numpy()
    want = np.zeros(len(ie))
    raw64 = np.sqrt(((e[enrol_rows][ie].astype(np.float64) - e[test_rows][it]) ** 2).sum(axis=1) + 1e-4 / 512)
    for rows, index, stats in ((enrol_rows, ie, es), (test_rows, it, ts)):
        d2, sel, mean, std, count = R.cohort_stats(e[rows], e[24:], 8)
        assert (C.host(stats.count) == 8).all() and (count == 8).all()
        if stats.mask is not None:
            C.assert_stats_of_returned_set(d2, C.mask_of(stats, 12), stats, 512, "model chain")
        assert np.abs(C.host(stats.mean) - mean).max() <= 1e-4 * mean.max()    # (the sets may differ inside the band)
        want += 0.5 * (raw64 - mean[index]) / np.maximum(std[index], 1e-6)
    got = C.host(out)
    assert np.isfinite(got).all() and np.abs(got - want).max() <= 1e-3 * max(1.0, np.abs(want).max())
    lo, hi = float(np.floor(got.min())) - 1.0, float(np.ceil(got.max())) + 1.0
    res = env.scoring.evaluate(out, torch.from_numpy(same).cuda(), thr_start=lo, thr_stop=hi, thr_step=0.01)
    tp, fp = R.roc_counts(got, same, R.thresholds_f32(lo, hi, 0.01)[0])
    assert 0.0 <= res.eer <= 1.0 and int(res.tp[-1]) == same.sum() and int(res.fp[-1]) == (1 - same).sum()
    assert np.abs(C.host(res.tp) - tp).sum() <= 2 and np.abs(C.host(res.fp) - fp).sum() <= 2     # scores on a threshold
    value, thr = env.scoring.min_dcf(out, torch.from_numpy(same).cuda(), thr_start=lo, thr_stop=hi, thr_step=0.01)
    assert 0.0 <= value <= 1.0 and lo <= thr <= hi
