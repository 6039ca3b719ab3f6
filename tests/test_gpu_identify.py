"""GPU: speaker identification (csrc/identify.hip, scoring.nearest / speaker_models / identify) on the device, against
the float64 restatement (tests/identify_reference.py): the cases of test_emul_identify.py, plus the chain from the
model's own embeddings."""
import numpy as np
import pytest
import torch

import identify_cases as C
import identify_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture
def env():
    from deepspeaker_pytorch_amd import scoring
    from deepspeaker_pytorch_amd.model import get_engine
    return C.Env(scoring, get_engine(), torch.device("cuda", 0))


@pytest.mark.parametrize("splits", C.INT_SPLITS)
@pytest.mark.parametrize("k", C.INT_KS)
@pytest.mark.parametrize("D", C.INT_DS)
def test_integer_data_indices_are_exact(env, D, k, splits):
    C.case_integer_identity(env, D, k, splits)


def test_real_valued_distances_and_membership(env):
    C.case_real_valued(env)


def test_result_does_not_depend_on_the_batch(env):
    C.case_batch_independence(env)


def test_screening_bits_do_not_move(env):
    C.case_screening_bits_do_not_move(env)


@pytest.mark.parametrize("splits", (0, 3))
def test_label_filter(env, splits):
    C.case_label_filter(env, splits)


def test_label_filter_nothing_eligible(env):
    C.case_label_filter_nothing_eligible(env)


def test_speaker_models(env):
    C.case_speaker_models(env)


def test_identify_and_rank_hits(env):
    C.case_identify(env)


def test_rank_hits_many_queries(env):
    C.case_rank_hits_many_queries(env)


def test_errors(env):
    C.case_errors(env)


def test_model_embeddings_to_identification(env):
    """embed -> speaker_models -> identify on a seeded two-stage model: the tensors the model produces are accepted as
    they are, and the result is the restatement's on the same embeddings."""
    from deepspeaker_pytorch_amd.model import DeepSpeakerModel
    from deepspeaker_pytorch_amd.synthetic import synthetic_state_dict
    sd = synthetic_state_dict(seed=5, num_classes=4, n_stages=2)
    m = DeepSpeakerModel(512, 4, n_stages=2)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    m = m.cuda().eval()
    rs = np.random.RandomState(6)
    voices = rs.randn(4, 1, 160, 64)                           # 4 "speakers": a voice pattern each, 6 noisy utterances of it
    spk = np.repeat(np.arange(4), 6)
    x = (voices[spk] + 0.5 * rs.randn(24, 1, 160, 64)).astype(np.float32)
    with torch.no_grad():
        emb = m(torch.from_numpy(x).cuda())
    enrol_rows = np.concatenate([np.nonzero(spk == s)[0][:4] for s in range(4)])       # 4 enrolment + 2 test each
    test_rows = np.concatenate([np.nonzero(spk == s)[0][4:] for s in range(4)])
    enrol, test = emb[torch.from_numpy(enrol_rows).cuda()], emb[torch.from_numpy(test_rows).cuda()]
    labels = np.array([11, 22, 33, 44], np.int64)
    models = env.scoring.speaker_models(enrol, [4, 4, 4, 4])
    res = env.scoring.identify(test, models, torch.from_numpy(labels).cuda(), torch.from_numpy(labels[spk[test_rows]]).cuda(),
                               k=3)
    e = emb.cpu().numpy()
    ref_models = R.speaker_models(e[enrol_rows], [4, 4, 4, 4])
    assert np.abs(models.cpu().numpy() - ref_models).max() / np.abs(ref_models).max() <= 1e-6
    _, order, dist = R.nearest(e[test_rows], models.cpu().numpy(), 3)
    np.testing.assert_array_equal(res.indices.cpu().numpy(), order)
    np.testing.assert_array_equal(res.labels.cpu().numpy(), labels[order])
    assert np.abs(res.distances.cpu().numpy() - dist).max() / dist.max() <= 1e-6
    want = R.rank_hits(order, labels, labels[spk[test_rows]])
    assert res.hits.cpu().numpy().tolist() == want.tolist() and res.rank1 == want[0] / 8 and res.rank_k == want[2] / 8
