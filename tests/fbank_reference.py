"""TEST INFRASTRUCTURE: float64 NumPy restatement of the reference's feature extraction (`mk_MFB`,
audio_processing.py:9-36 with constants.py: python_speech_features v0.6 `fbank(nfilt=64, winlen=0.025)`, then
20*log10(max(fb, 1e-5)) and `normalize_frames`).  Neither librosa nor python_speech_features is available, so the
arithmetic is restated here from its specification; the spectrum comes from np.fft.rfft, a path independent of the
kernels' DFT-as-GEMM."""
import decimal
import math

import numpy as np


def round_half_up(x):
    return int(decimal.Decimal(x).quantize(decimal.Decimal("1"), rounding=decimal.ROUND_HALF_UP))


def frame_params(sample_rate, winlen=0.025, winstep=0.01):
    return round_half_up(winlen * sample_rate), round_half_up(winstep * sample_rate)


def n_frames(n_samples, frame_len, frame_step):
    if n_samples <= frame_len:
        return 1
    return 1 + int(math.ceil((1.0 * n_samples - frame_len) / frame_step))


def preemphasis(x):
    """float32 in, float32 out: NumPy's own arithmetic (product rounded, then the difference rounded)."""
    x = np.asarray(x, np.float32)
    return np.append(x[0], x[1:] - 0.97 * x[:-1])


def hz2mel(hz):
    return 2595 * np.log10(1 + hz / 700.0)


def mel2hz(mel):
    return 700 * (10 ** (mel / 2595.0) - 1)


def filter_bins(nfilt=64, nfft=512, sample_rate=16000):
    pts = np.linspace(hz2mel(0), hz2mel(sample_rate / 2), nfilt + 2)
    return np.floor((nfft + 1) * mel2hz(pts) / sample_rate)


def filterbank(nfilt=64, nfft=512, sample_rate=16000):
    b = filter_bins(nfilt, nfft, sample_rate)
    w = np.zeros((nfilt, nfft // 2 + 1))
    for j in range(nfilt):
        for i in range(int(b[j]), int(b[j + 1])):
            w[j, i] = (i - b[j]) / (b[j + 1] - b[j])
        for i in range(int(b[j + 1]), int(b[j + 2])):
            w[j, i] = (b[j + 2] - i) / (b[j + 2] - b[j + 1])
    return w


def frames(x, sample_rate=16000):
    """[n_frames, frame_len] float64 frames of the pre-emphasised, zero-padded signal (rectangular window)."""
    fl, fs = frame_params(sample_rate)
    if len(x) == 0:
        raise ValueError("empty signal")
    y = preemphasis(x).astype(np.float64)
    nf = n_frames(len(y), fl, fs)
    pad = np.concatenate([y, np.zeros((nf - 1) * fs + fl - len(y))])
    idx = np.arange(fl)[None, :] + fs * np.arange(nf)[:, None]
    return pad[idx]


def power_spectrum(fr, nfft=512):
    return np.abs(np.fft.rfft(fr, nfft)) ** 2 / nfft


def fbank(x, sample_rate=16000, nfilt=64, nfft=512, use_logscale=True):
    fb = power_spectrum(frames(x, sample_rate), nfft) @ filterbank(nfilt, nfft, sample_rate).T
    fb = np.where(fb == 0, np.finfo(float).eps, fb)
    if use_logscale:
        fb = 20 * np.log10(np.maximum(fb, 1e-5))
    return fb


def normalize_frames(m, scale=False):
    if scale:
        return (m - np.mean(m, axis=0)) / (np.std(m, axis=0) + 2e-12)
    return m - np.mean(m, axis=0)


def mk_mfb(x, sample_rate=16000, nfilt=64, nfft=512, normalize="mean", use_logscale=True):
    """float64 [T, nfilt]; normalize in {"mean", "mean_std", None}"""
    fb = fbank(x, sample_rate, nfilt, nfft, use_logscale)
    if normalize is None:
        return fb
    return normalize_frames(fb, scale=normalize == "mean_std")


def synthetic_audio(seed, n, sample_rate=16000, kind="noise"):
    """Seeded float32 test signals."""
    rs = np.random.RandomState(seed)
    t = np.arange(n) / sample_rate
    if kind == "noise":
        x = 0.1 * rs.randn(n)
    elif kind == "quiet_noise":
        x = 1e-3 * rs.randn(n)
    elif kind == "tone":
        x = 0.9 * np.sin(2 * np.pi * 440.0 * t + 0.3)
    elif kind == "quiet_tone":
        x = 1e-4 * np.sin(2 * np.pi * 1234.5 * t)
    elif kind == "chirp":
        x = 0.5 * np.sin(2 * np.pi * (100.0 * t + 0.5 * 3000.0 * t * t))
    elif kind == "silence":
        x = np.zeros(n)
    elif kind == "dc":
        x = np.full(n, 0.25)
    elif kind == "ar":                   # AR(2)-filtered noise under a slow envelope: speech-like spectrum and level
        e = rs.randn(n) * 0.05
        y = np.zeros(n)
        for i in range(n):
            y[i] = e[i] + (1.6 * y[i - 1] if i >= 1 else 0.0) - (0.8 * y[i - 2] if i >= 2 else 0.0)
        x = y * (0.55 + 0.45 * np.sin(2 * np.pi * 1.7 * t))
        x = x / max(1.0, np.abs(x).max() * 1.1)
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def int16_quantised(x):
    return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
