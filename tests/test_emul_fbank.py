"""CPU: the filterbank front end (csrc/fbank.hip, features.py) through the host emulator of the kernels, against the
float64 restatement of mk_MFB (tests/fbank_reference.py).  The cases are tests/fbank_bodies.py, shared with
tests/test_gpu_fbank.py; the restatements themselves are checked here."""
import numpy as np
import pytest

import fbank_bodies as B
import fbank_reference as R
from emul_util import emul_lib

from deepspeaker_pytorch_amd.engine import Engine

TOL_DB = B.TOL_DB


@pytest.fixture
def ctx():
    from deepspeaker_pytorch_amd import data, features
    eng = Engine(emul_lib())
    features._engine_override = eng
    data._engine_override = eng
    try:
        yield B.Ctx(features, "cpu", emul_lib())
    finally:
        features._engine_override = None
        data._engine_override = None


# ---- the restatements alone ----
def test_window_keywords_default_to_the_reference():
    """winlen / winstep default to the reference's 0.025 / 0.01; other values reach the framing"""
    x = R.synthetic_audio(1, 3000, kind="ar")
    np.testing.assert_array_equal(R.mk_mfb(x), R.mk_mfb(x, winlen=0.025, winstep=0.01))
    np.testing.assert_array_equal(R.frames(x), R.frames(x, 16000, 0.025, 0.01))
    assert R.frames(x).shape == (R.n_frames(3000, 400, 160), 400)
    fr = R.frames(x, 16000, 401 / 16000, 0.03)
    assert fr.shape == (R.n_frames(3000, 401, 480), 401) == (7, 401)
    y = R.preemphasis(x).astype(np.float64)
    np.testing.assert_array_equal(fr[2], y[960:1361])
    np.testing.assert_array_equal(fr[6], np.concatenate([y[2880:], np.zeros(401 - 120)]))
    assert R.fbank(x, winlen=401 / 16000, winstep=0.03).shape == (7, 64)
    assert R.frame_params(22050) == (551, 221)


def test_float32_restatement_is_the_same_operation():
    """mk_mfb_f32 differs from mk_mfb by float32 rounding and nothing else; a one-sample frame has a flat spectrum"""
    for kw in (dict(), dict(sample_rate=22050, nfft=1024), dict(sample_rate=2000, nfft=64, nfilt=12),
               dict(winlen=401 / 16000, winstep=0.03)):
        x = R.synthetic_audio(2, 5000, kw.get("sample_rate", 16000), "ar")
        for normalize in (None, "mean", "mean_std"):
            a, b = R.mk_mfb_f32(x, normalize=normalize, **kw), R.mk_mfb(x, normalize=normalize, **kw)
            assert a.dtype == np.float32 and a.shape == b.shape
            assert np.abs(a - b).max() <= 1e-4, (kw, normalize)
        a, b = (f(x, normalize=None, use_logscale=False, **kw) for f in (R.mk_mfb_f32, R.mk_mfb))
        assert B.frame_rel(a, b) <= 1e-5, kw
    one = R.mk_mfb_f32(np.array([0.5], np.float32), normalize=None, use_logscale=False)
    want = (0.25 / 512) * R.filterbank().sum(1)
    np.testing.assert_allclose(one[0], np.where(want == 0, np.finfo(float).eps, want), rtol=1e-6)


def test_level_steps_tell_frames_apart():
    """a frame of the stepped signal stored one row off is wrong by orders of magnitude under the per-frame metric"""
    x = R.level_steps(3, 400 + 30 * 160, 160)
    ref = R.mk_mfb(x, normalize=None, use_logscale=False)
    for shift in (1, -1):
        moved = np.roll(ref, shift, axis=0)
        assert B.frame_rel(moved, ref) > 10.0
        per_frame = np.abs(moved - ref).max(1) / np.abs(ref).max(1)
        # most frames are wrong by their own size or more; the two of every six that hold the same loud step whole
        # have nearly the same power spectrum, and even they are a hundred times over bars near 1e-6
        assert (per_frame > 0.5).mean() >= 0.75 and per_frame.min() > 1e-4


# ---- the kernels through the emulator ----
LENGTHS = (1, 399, 400, 401, 2000)


@pytest.mark.parametrize("sr", [16000, 8000])
@pytest.mark.parametrize("normalize", ["mean", "mean_std", None])
def test_log_mel_fbank_matches_restatement(ctx, sr, normalize):
    kinds = ("noise", "tone", "ar", "chirp", "quiet_noise")
    B.restatement(ctx, [R.synthetic_audio(10 + i, n, sr, kinds[i]) for i, n in enumerate(LENGTHS)], sr, normalize)


def test_int16_input_is_the_scaled_float_input(ctx):
    B.int16_is_scaled_float(ctx, [R.int16_quantised(R.synthetic_audio(20 + i, n, kind="ar"))
                                  for i, n in enumerate((401, 2000))], "mean", values=True)


def test_packed_input_and_feature_store(ctx):
    B.packed_input_and_feature_store(ctx)


def test_raw_filterbank(ctx):
    B.raw_filterbank(ctx, 41, 300, "noise", rtol=2e-5, atol=1e-9)


def test_abi_errors(ctx):
    B.abi_errors(ctx)


def test_plan_table(ctx):
    B.plan_table(ctx)


def test_python_errors(ctx):
    B.python_errors(ctx)


@pytest.mark.parametrize("sr,nfft,nfilt", [(40000, 1024, 64), (2000, 64, 16), (16000, 512, 128), (8000, 256, 32)])
def test_other_configurations(ctx, sr, nfft, nfilt):
    B.other_configurations(ctx, sr, nfft, nfilt)


def test_preemphasis_bits(ctx):
    B.preemphasis_bits(ctx, 60, 5000)


def test_deterministic_and_batch_invariant(ctx):
    B.deterministic(ctx, n_utt=12, n_max=6000, picks=(0, 5, 11))


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
