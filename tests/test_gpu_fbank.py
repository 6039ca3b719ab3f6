"""MI355X: the log-mel filterbank front end (csrc/fbank.hip, features.py, FeatureStore.from_waveforms) against the
float64 restatement of the reference's mk_MFB (tests/fbank_reference.py), on seeded synthetic audio."""
import numpy as np
import pytest
import torch

import fbank_reference as R

pytestmark = pytest.mark.gpu

# max |feature - restatement| in dB (in normalised units for "mean_std"): measured on the MI355X at most 2.1e-4 over
# every signal here, the 8-minute utterance included
TOL_DB = 5e-4
KINDS = ("noise", "quiet_noise", "tone", "quiet_tone", "chirp", "silence", "dc", "ar")
LENGTHS = (1, 399, 400, 401, 560, 561, 16000, 48000)


def _features():
    from deepspeaker_pytorch_amd import features
    return features


def _signals(sr=16000):
    out = []
    for i, kind in enumerate(KINDS):
        for j, n in enumerate(LENGTHS):
            out.append(R.synthetic_audio(100 * i + j, n, sr, kind))
    return out


def _max_err(out, off, refs):
    return max(float(np.abs(out[off[u]:off[u + 1]] - r).max()) for u, r in enumerate(refs))


@pytest.mark.parametrize("sr", [16000, 8000])
@pytest.mark.parametrize("normalize", [None, "mean", "mean_std"])
def test_features_match_restatement(sr, normalize):
    F = _features()
    xs = _signals(sr)
    xs += [R.int16_quantised(x) for x in xs[::5]]
    refs = [R.mk_mfb(x.astype(np.float32) / np.float32(32768) if x.dtype == np.int16 else x, sample_rate=sr,
                     normalize=normalize) for x in xs]
    f32 = [x for x in xs if x.dtype == np.float32]
    i16 = [x for x in xs if x.dtype == np.int16]
    out, off = F.log_mel_fbank([torch.from_numpy(x).cuda() for x in f32], F.FbankConfig(sample_rate=sr), normalize)
    out16, off16 = F.log_mel_fbank([torch.from_numpy(x).cuda() for x in i16], F.FbankConfig(sample_rate=sr), normalize)
    err = max(_max_err(out.cpu().numpy(), off, refs[:len(f32)]), _max_err(out16.cpu().numpy(), off16, refs[len(f32):]))
    print(f"fbank sr={sr} normalize={normalize}: max abs error {err:.3e}")
    assert err <= TOL_DB, err


def test_eight_minute_utterance():
    """48k frames: the per-utterance statistics come from 750 tiles' f64 partials."""
    F = _features()
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


def test_preemphasis_bits():
    from deepspeaker_pytorch_amd.model import get_engine
    eng = get_engine()
    x = R.synthetic_audio(3, 100000, kind="ar")
    for src, ref in ((x, R.preemphasis(x)),
                     (R.int16_quantised(x), R.preemphasis(R.int16_quantised(x).astype(np.float32) / np.float32(32768)))):
        d = torch.from_numpy(src).cuda()
        y = torch.empty(len(src), dtype=torch.float32, device="cuda")
        eng.lib.call("ds_fbank_preemphasis_f32", eng._p(d), 1 if src.dtype == np.int16 else 0, len(src), eng._p(y),
                     eng._stream(y))
        np.testing.assert_array_equal(y.cpu().numpy().view(np.int32), ref.view(np.int32))


def test_raw_single_frame_filterbank():
    F = _features()
    x = R.synthetic_audio(5, 400, kind="ar")
    out, _ = F.log_mel_fbank([torch.from_numpy(x).cuda()], F.FbankConfig(use_logscale=False), normalize=None)
    ref = R.mk_mfb(x, normalize=None, use_logscale=False)
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-5, atol=1e-12)


def test_int16_is_bit_identical_to_scaled_float():
    F = _features()
    q = [R.int16_quantised(x) for x in _signals()[::3]]
    a, _ = F.log_mel_fbank([torch.from_numpy(x).cuda() for x in q], normalize="mean_std")
    b, _ = F.log_mel_fbank([torch.from_numpy(x.astype(np.float32) / np.float32(32768)).cuda() for x in q],
                           normalize="mean_std")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_deterministic_and_batch_invariant():
    F = _features()
    rs = np.random.RandomState(11)
    kinds = ("noise", "ar", "chirp", "tone")
    xs = [torch.from_numpy(R.synthetic_audio(1000 + i, int(rs.randint(1, 160000)), kind=kinds[i % 4])).cuda()
          for i in range(100)]
    for normalize in ("mean", "mean_std", None):
        a, off = F.log_mel_fbank(xs, normalize=normalize)
        b, _ = F.log_mel_fbank(xs, normalize=normalize)
        assert torch.equal(a, b)
        for u in (0, 17, 63, 99):
            alone, _ = F.log_mel_fbank([xs[u]], normalize=normalize)
            assert torch.equal(alone, a[off[u]:off[u + 1]]), (normalize, u)
        packed, off2 = F.log_mel_fbank(torch.cat(xs), lengths=[len(x) for x in xs], normalize=normalize)
        assert torch.equal(packed, a) and off2.tolist() == off.tolist()


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


def test_errors_raise():
    from deepspeaker_pytorch_amd._native import DeepSpeakerHipError
    F = _features()
    x = torch.zeros(1000, device="cuda")
    with pytest.raises(DeepSpeakerHipError, match="bad shape"):
        F.log_mel_fbank([x, torch.zeros(0, device="cuda")])
    with pytest.raises(DeepSpeakerHipError):
        F.log_mel_fbank([x], F.FbankConfig(sample_rate=24000))            # frame_len 600 > nfft 512
    with pytest.raises(DeepSpeakerHipError):
        F.log_mel_fbank([x], F.FbankConfig(nfilt=66))
