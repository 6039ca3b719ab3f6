"""CPU: the filterbank front end (csrc/fbank.hip, features.py) through the host emulator of the kernels, against the
float64 restatement of mk_MFB (tests/fbank_reference.py)."""
import numpy as np
import pytest
import torch

import fbank_reference as R
from emul_util import emul_lib

from deepspeaker_pytorch_amd._native import DeepSpeakerHipError
from deepspeaker_pytorch_amd.engine import Engine

TOL_DB = 5e-4


@pytest.fixture
def features():
    from deepspeaker_pytorch_amd import data, features
    eng = Engine(emul_lib())
    features._engine_override = eng
    data._engine_override = eng
    try:
        yield features
    finally:
        features._engine_override = None
        data._engine_override = None


LENGTHS = (1, 399, 400, 401, 2000)


@pytest.mark.parametrize("sr", [16000, 8000])
@pytest.mark.parametrize("normalize", ["mean", "mean_std", None])
def test_log_mel_fbank_matches_restatement(features, sr, normalize):
    kinds = ("noise", "tone", "ar", "chirp", "quiet_noise")
    xs = [R.synthetic_audio(10 + i, n, sr, kinds[i]) for i, n in enumerate(LENGTHS)]
    cfg = features.FbankConfig(sample_rate=sr)
    out, off = features.log_mel_fbank([torch.from_numpy(x) for x in xs], cfg, normalize=normalize)
    out = out.numpy()
    assert out.dtype == np.float32 and out.shape[1] == 64
    fl, fs = R.frame_params(sr)
    assert off.tolist() == np.concatenate([[0], np.cumsum([R.n_frames(n, fl, fs) for n in LENGTHS])]).tolist()
    for u, x in enumerate(xs):
        ref = R.mk_mfb(x, sample_rate=sr, normalize=normalize)
        err = np.abs(out[off[u]:off[u + 1]] - ref).max()
        assert err <= TOL_DB, (u, err)


def test_int16_input_is_the_scaled_float_input(features):
    xs = [R.int16_quantised(R.synthetic_audio(20 + i, n, kind="ar")) for i, n in enumerate((401, 2000))]
    a, off = features.log_mel_fbank([torch.from_numpy(x) for x in xs])
    b, _ = features.log_mel_fbank([torch.from_numpy(x.astype(np.float32) / 32768.0) for x in xs])
    np.testing.assert_array_equal(a.numpy().view(np.int32), b.numpy().view(np.int32))
    for u, x in enumerate(xs):
        ref = R.mk_mfb(x.astype(np.float32) / np.float32(32768.0))
        assert np.abs(a.numpy()[off[u]:off[u + 1]] - ref).max() <= TOL_DB


def test_packed_input_and_feature_store(features):
    from deepspeaker_pytorch_amd import data
    xs = [R.synthetic_audio(30 + i, n, kind="noise") for i, n in enumerate((900, 2000))]
    packed = torch.from_numpy(np.concatenate(xs))
    a, off = features.log_mel_fbank(packed, lengths=[900, 2000])
    b, _ = features.log_mel_fbank([torch.from_numpy(x) for x in xs])
    assert torch.equal(a, b)
    fs = data.FeatureStore.from_waveforms([torch.from_numpy(x) for x in xs])
    assert len(fs) == 2 and fs.n_feat == 64 and fs.offsets.tolist() == off.tolist()
    assert torch.equal(fs.features, a)
    crop = fs.crops([1], [3], 8).numpy()
    np.testing.assert_array_equal(crop[0, 0], a.numpy()[off[1] + 3:off[1] + 11])


def test_raw_filterbank(features):
    x = R.synthetic_audio(41, 300, kind="noise")
    cfg = features.FbankConfig(use_logscale=False)
    out, _ = features.log_mel_fbank([torch.from_numpy(x)], cfg, normalize=None)
    ref = R.mk_mfb(x, normalize=None, use_logscale=False)
    np.testing.assert_allclose(out.numpy(), ref, rtol=2e-5, atol=1e-9)


def test_abi_errors():
    lib = emul_lib()
    counts = np.zeros(3, np.int64)
    plan = lambda lens, fl, fs, nfft, nfilt: lib.raw("ds_fbank_plan")(lens.ctypes.data, len(lens), fl, fs, nfft, nfilt,
                                                                       None, counts.ctypes.data)
    assert plan(np.array([400, 0], np.int64), 400, 160, 512, 64) == -1          # empty signal
    one = np.array([400], np.int64)
    assert plan(one, 600, 240, 512, 64) == -4                                     # frame_len > nfft
    assert plan(one, 400, 160, 512, 62) == -4                                     # nfilt % 4 != 0
    assert plan(one, 400, 160, 500, 64) == -4                                     # nfft not a power of two
    assert plan(one, 400, 160, 512, 64) == 0 and counts.tolist() == [1, 1, 64]
    assert plan(np.array([160 * 48000 + 1], np.int64), 400, 160, 512, 64) == 0
    assert counts.tolist() == [R.n_frames(160 * 48000 + 1, 400, 160), 750, 64]      # an 8-minute utterance
    assert lib.raw("ds_fbank_logmel_f32")(None, 0, None, 1, 1, None, None, None, 1, 400, 160, 512, 64, 1, None, None,
                                          None) == -3


def test_plan_table():
    """ds_fbank_plan's table entry by entry: utterances of exactly one tile of frames, one frame more, and one frame."""
    lib = emul_lib()
    fl, fs = 400, 160
    counts = np.zeros(3, np.int64)
    plan = lambda lens, table: lib.raw("ds_fbank_plan")(lens.ctypes.data, len(lens), fl, fs, 512, 64,
                                                        None if table is None else table.ctypes.data, counts.ctypes.data)
    assert plan(np.array([1], np.int64), None) == 0
    tm = int(counts[2])
    a, b = fl + (tm - 1) * fs, fl + tm * fs                       # tm and tm + 1 frames (framesig)
    lens = np.array([a, b, 1], np.int64)
    assert plan(lens, None) == 0 and counts.tolist() == [2 * tm + 2, 4, tm]
    table = np.full(3 * 4 + 4, -7, np.int64)
    counts[:] = 0
    assert plan(lens, table) == 0 and counts.tolist() == [2 * tm + 2, 4, tm]
    assert table.tolist() == [0, a, a + b, a + b + 1,  0, tm, 2 * tm + 1, 2 * tm + 2,  0, 1, 3, 4,  0, 1, 1, 2]


def test_python_errors(features):
    with pytest.raises(DeepSpeakerHipError, match="bad shape"):
        features.log_mel_fbank([torch.zeros(400), torch.zeros(0)])
    with pytest.raises(DeepSpeakerHipError):
        features.log_mel_fbank([torch.zeros(400)], features.FbankConfig(sample_rate=24000))   # frame_len 600 > nfft 512
    with pytest.raises(DeepSpeakerHipError):
        features.log_mel_fbank([torch.zeros(400)], features.FbankConfig(nfilt=30))
    with pytest.raises(ValueError):
        features.log_mel_fbank([torch.zeros(400)], normalize="std")
    with pytest.raises(ValueError):
        features.log_mel_fbank([torch.zeros(400, dtype=torch.float64)])


@pytest.mark.parametrize("sr,nfft,nfilt", [(40000, 1024, 64), (2000, 64, 16), (16000, 512, 128), (8000, 256, 32)])
def test_other_configurations(features, sr, nfft, nfilt):
    """Other sample rates, FFT sizes and filter counts; (40000, 1024) takes 32-frame tiles (the 64-frame tile's samples
    and power spectrum do not fit the LDS together)."""
    lib = emul_lib()
    cfg = features.FbankConfig(sample_rate=sr, nfft=nfft, nfilt=nfilt)
    n = (70 * cfg.frame_step + cfg.frame_len)                      # more than one tile of either size
    xs = [R.synthetic_audio(50, n, sr, "ar"), R.synthetic_audio(51, n // 3, sr, "noise")]
    counts = np.zeros(3, np.int64)
    lens = np.array([len(x) for x in xs], np.int64)
    assert lib.raw("ds_fbank_plan")(lens.ctypes.data, 2, cfg.frame_len, cfg.frame_step, nfft, nfilt, None,
                                    counts.ctypes.data) == 0
    assert counts[2] == (32 if nfft == 1024 else 64)
    out, off = features.log_mel_fbank([torch.from_numpy(x) for x in xs], cfg, normalize="mean")
    for u, x in enumerate(xs):
        ref = R.mk_mfb(x, sample_rate=sr, nfilt=nfilt, nfft=nfft, normalize="mean")
        assert np.abs(out.numpy()[off[u]:off[u + 1]] - ref).max() <= TOL_DB


def test_preemphasis_bits():
    lib = emul_lib()
    x = R.synthetic_audio(60, 5000, kind="ar")
    y = np.zeros(len(x), np.float32)
    assert lib.raw("ds_fbank_preemphasis_f32")(x.ctypes.data, 0, len(x), y.ctypes.data, None) == 0
    np.testing.assert_array_equal(y.view(np.int32), R.preemphasis(x).view(np.int32))
    q = R.int16_quantised(x)
    assert lib.raw("ds_fbank_preemphasis_f32")(q.ctypes.data, 1, len(q), y.ctypes.data, None) == 0
    np.testing.assert_array_equal(y.view(np.int32), R.preemphasis(q.astype(np.float32) / np.float32(32768)).view(np.int32))
