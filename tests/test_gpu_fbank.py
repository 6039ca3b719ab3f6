"""MI355X: the log-mel filterbank front end (csrc/fbank.hip, features.py, FeatureStore.from_waveforms) against the
float64 restatement of the reference's mk_MFB (tests/fbank_reference.py), on seeded synthetic audio.  The cases are
tests/fbank_bodies.py, the same ones tests/test_emul_fbank.py runs through the host emulator; the 8-minute utterance and
waveforms-to-embeddings are the device's alone."""
import numpy as np
import pytest
import torch

import fbank_bodies as B
import fbank_reference as R

pytestmark = pytest.mark.gpu

# max |feature - restatement| in dB (in normalised units for "mean_std"): measured on the MI355X at most 2.1e-4 over
# every signal here, the 8-minute utterance included
TOL_DB = B.TOL_DB
KINDS = ("noise", "quiet_noise", "tone", "quiet_tone", "chirp", "silence", "dc", "ar")
LENGTHS = (1, 399, 400, 401, 560, 561, 16000, 48000)


@pytest.fixture
def ctx():
    from deepspeaker_pytorch_amd import features
    from deepspeaker_pytorch_amd.model import get_engine
    return B.Ctx(features, "cuda", get_engine().lib)


def _signals(sr=16000):
    out = []
    for i, kind in enumerate(KINDS):
        for j, n in enumerate(LENGTHS):
            out.append(R.synthetic_audio(100 * i + j, n, sr, kind))
    return out


@pytest.mark.parametrize("sr", [16000, 8000])
@pytest.mark.parametrize("normalize", [None, "mean", "mean_std"])
def test_features_match_restatement(ctx, sr, normalize):
    xs = _signals(sr)
    B.restatement(ctx, xs + [R.int16_quantised(x) for x in xs[::5]], sr, normalize)


def test_eight_minute_utterance(ctx):
    """48k frames: the per-utterance statistics come from 750 tiles' f64 partials."""
    F = ctx.features
    sr, n = 16000, 16000 * 480
    rs = np.random.RandomState(7)
    t = np.arange(n) / sr
    env = 0.5 + 0.45 * np.sin(2 * np.pi * 0.3 * t)
    x = (env * (0.05 * rs.randn(n) + 0.3 * np.sin(2 * np.pi * (200 + 50 * np.sin(2 * np.pi * 0.05 * t)) * t))).astype(np.float32)
    dev = torch.from_numpy(x).cuda()
    for normalize in ("mean", "mean_std"):
        out, off = F.log_mel_fbank([dev], normalize=normalize)
        assert off.tolist() == [0, R.n_frames(n, 400, 160)]
        err = float(np.abs(out.cpu().numpy() - R.mk_mfb(x, normalize=normalize)).max())
        print(f"fbank 8-minute utterance normalize={normalize}: max abs error {err:.3e}")
        assert err <= TOL_DB, err


def test_preemphasis_bits(ctx):
    B.preemphasis_bits(ctx, 3, 100000)


def test_raw_single_frame_filterbank(ctx):
    B.raw_filterbank(ctx, 5, 400, "ar", rtol=1e-5, atol=1e-12)


def test_raw_filterbank(ctx):
    B.raw_filterbank(ctx, 41, 300, "noise", rtol=2e-5, atol=1e-9)


def test_int16_is_bit_identical_to_scaled_float(ctx):
    B.int16_is_scaled_float(ctx, [R.int16_quantised(x) for x in _signals()[::3]], "mean_std", values=False)


def test_deterministic_and_batch_invariant(ctx):
    B.deterministic(ctx, n_utt=100, n_max=160000, picks=(0, 17, 63, 99))


def test_packed_input_and_feature_store(ctx):
    B.packed_input_and_feature_store(ctx)


def test_end_to_end_waveforms_to_embeddings():
    import deepspeaker_oracle as O
    from deepspeaker_pytorch_amd.data import FeatureStore
    from deepspeaker_pytorch_amd.model import DeepSpeakerModel
    xs = [R.synthetic_audio(200 + i, n, kind=k) for i, (n, k) in
          enumerate(((16000, "ar"), (26000, "noise"), (40000, "chirp"), (20000, "ar"), (33000, "tone")))]
    store = FeatureStore.from_waveforms([torch.from_numpy(x).cuda() for x in xs])
    refs = [R.mk_mfb(x) for x in xs]
    assert len(store) == len(xs) and store.n_feat == 64
    assert [store.length(u) for u in range(len(xs))] == [len(r) for r in refs]
    sd = O.make_state_dict(seed=3, num_classes=8)
    model = DeepSpeakerModel(512, 8)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    model = model.cuda().eval()
    with torch.no_grad():
        emb = model.embed_variable_length(store).cpu().numpy()
    for u, r in enumerate(refs):
        ref = O.forward(sd, r[None, None].astype(np.float32), dtype=np.float64)[0]
        err = np.abs(emb[u] - ref).max() / np.abs(ref).max()
        assert err < 1e-3, (u, err)
    idx, st = [0, 2, 4, 1], [0, 100, 7, 150]
    crops = store.crops(idx, st, 64).cpu().numpy()
    for b, (u, s) in enumerate(zip(idx, st)):
        ref = np.zeros((64, 64))
        seg = refs[u][s:s + 64]
        ref[:len(seg)] = seg
        assert np.abs(crops[b, 0] - ref).max() <= TOL_DB


def test_errors_raise(ctx):
    B.python_errors(ctx)


def test_abi_errors(ctx):
    B.abi_errors(ctx)


def test_plan_table(ctx):
    B.plan_table(ctx)


@pytest.mark.parametrize("sr,nfft,nfilt", [(40000, 1024, 64), (2000, 64, 16), (16000, 512, 128), (8000, 256, 32)])
def test_other_configurations(ctx, sr, nfft, nfilt):
    B.other_configurations(ctx, sr, nfft, nfilt)


@pytest.mark.parametrize("dtype", B.DTYPES)
@pytest.mark.parametrize("name", list(B.CONFS))
def test_configuration(ctx, name, dtype):
    B.configuration(ctx, name, dtype)


@pytest.mark.parametrize("dtype", B.DTYPES)
@pytest.mark.parametrize("name", list(B.CONFS))
def test_loud_successor(ctx, name, dtype):
    B.loud_successor(ctx, name, dtype)


@pytest.mark.parametrize("dtype", B.DTYPES)
@pytest.mark.parametrize("name", [n for n, c in B.CONFS.items() if c.long])
def test_statistics_alone_and_last_of_five(ctx, name, dtype):
    B.statistics_alone_and_last_of_five(ctx, name, dtype)


def test_every_instantiation_was_launched(ctx):
    B.coverage(ctx)
