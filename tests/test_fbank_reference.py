"""CPU: pins the float64 restatement of mk_MFB (tests/fbank_reference.py) that the kernels are tested against."""
import numpy as np
import pytest

import fbank_reference as R


def test_frame_parameters_and_counts():
    assert R.frame_params(16000) == (400, 160)
    assert R.frame_params(8000) == (200, 80)
    assert R.n_frames(16000, 400, 160) == 99            # 1 s
    assert R.n_frames(48000, 400, 160) == 299           # 3 s
    assert [R.n_frames(n, 400, 160) for n in (1, 399, 400, 401, 560, 561)] == [1, 1, 1, 2, 2, 3]
    with pytest.raises(ValueError):
        R.frames(np.zeros(0, np.float32))


def test_filterbank_bins_and_sparsity():
    b = R.filter_bins(64, 512, 16000)
    assert b[:12].tolist() == [0, 0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11]
    assert b[-3:].tolist() == [235, 245, 256]
    w = R.filterbank(64, 512, 16000)
    assert w.shape == (64, 257)
    assert np.count_nonzero(w) == 438
    assert np.count_nonzero(w[0]) == 1 and w[0, 0] == 1.0          # filter 0 is the DC bin alone
    assert (np.count_nonzero(w, axis=1) > 0).all()
    assert np.count_nonzero(w, axis=1).max() <= 20


def test_parseval():
    x = R.synthetic_audio(3, 4000, kind="noise")
    fr = R.frames(x)
    p = R.power_spectrum(fr)
    wk = np.full(257, 2.0)
    wk[0] = wk[-1] = 1.0
    np.testing.assert_allclose(p @ wk, (fr ** 2).sum(1), rtol=1e-12, atol=0)


@pytest.mark.parametrize("j", [5, 20, 40, 60])
def test_tone_at_bin_frequency_peaks_in_its_filter(j):
    b = R.filter_bins(64, 512, 16000)
    f = b[j + 1] * 16000 / 512
    t = np.arange(16000) / 16000.0
    x = (0.5 * np.sin(2 * np.pi * f * t)).astype(np.float32)
    fb = R.fbank(x)
    assert (fb[2:-2].argmax(1) == j).all()


def test_silence():
    x = np.zeros(5000, np.float32)
    fb = R.fbank(x)
    assert (fb == -100.0).all()
    for mode in ("mean", "mean_std"):
        assert (R.mk_mfb(x, normalize=mode) == 0.0).all()


def test_preemphasis_is_float32_with_two_roundings():
    x = R.synthetic_audio(7, 20000, kind="ar")
    y = R.preemphasis(x)
    assert y.dtype == np.float32
    prod = (np.float32(0.97) * x[:-1]).astype(np.float32)
    two = np.append(x[0], (x[1:] - prod).astype(np.float32))
    np.testing.assert_array_equal(y.view(np.int32), two.view(np.int32))
    # and it is not the single-rounding (fused) form
    fused = np.append(x[0], (x[1:].astype(np.float64) - np.float64(np.float32(0.97)) * x[:-1]).astype(np.float32))
    assert (fused != y).any()


def test_normalize_frames():
    m = np.random.RandomState(1).randn(50, 64) * 5 - 60
    n = R.normalize_frames(m)
    np.testing.assert_allclose(n.mean(0), 0, atol=1e-12)
    s = R.normalize_frames(m, scale=True)
    np.testing.assert_allclose(s.std(0), 1, atol=1e-9)
