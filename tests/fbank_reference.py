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


def frames(x, sample_rate=16000, winlen=0.025, winstep=0.01, dtype=np.float64):
    """[n_frames, frame_len] frames (float64 unless `dtype` says otherwise) of the pre-emphasised, zero-padded signal
    (rectangular window)."""
    fl, fs = frame_params(sample_rate, winlen, winstep)
    if len(x) == 0:
        raise ValueError("empty signal")
    y = preemphasis(x).astype(dtype)
    nf = n_frames(len(y), fl, fs)
    pad = np.concatenate([y, np.zeros(max(0, (nf - 1) * fs + fl - len(y)), dtype)])
    idx = np.arange(fl)[None, :] + fs * np.arange(nf)[:, None]
    return pad[idx]


def power_spectrum(fr, nfft=512):
    return np.abs(np.fft.rfft(fr, nfft)) ** 2 / nfft


def fbank(x, sample_rate=16000, nfilt=64, nfft=512, use_logscale=True, winlen=0.025, winstep=0.01):
    fb = power_spectrum(frames(x, sample_rate, winlen, winstep), nfft) @ filterbank(nfilt, nfft, sample_rate).T
    fb = np.where(fb == 0, np.finfo(float).eps, fb)
    if use_logscale:
        fb = 20 * np.log10(np.maximum(fb, 1e-5))
    return fb


def normalize_frames(m, scale=False):
    if scale:
        return (m - np.mean(m, axis=0)) / (np.std(m, axis=0) + 2e-12)
    return m - np.mean(m, axis=0)


def mk_mfb(x, sample_rate=16000, nfilt=64, nfft=512, normalize="mean", use_logscale=True, winlen=0.025, winstep=0.01):
    """float64 [T, nfilt]; normalize in {"mean", "mean_std", None}"""
    fb = fbank(x, sample_rate, nfilt, nfft, use_logscale, winlen, winstep)
    if normalize is None:
        return fb
    return normalize_frames(fb, scale=normalize == "mean_std")


def dft_table_f32(frame_len, nfft):
    """float32 (cos, sin) tables [frame_len, nfft/2+1] of the DFT, from its definition X_k = sum_n x_n exp(-2 pi i n k /
    nfft): the angle reduced exactly in integers, evaluated in float64 and rounded once."""
    n = np.arange(frame_len, dtype=np.int64)[:, None]
    k = np.arange(nfft // 2 + 1, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((n * k) % nfft) / nfft
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def mk_mfb_f32(x, sample_rate=16000, nfilt=64, nfft=512, normalize="mean", use_logscale=True, winlen=0.025, winstep=0.01):
    """The same pipeline with the spectrum in float32, as a kernel that does the DFT as a float32 matrix product has it:
    float32 pre-emphasised frames times float32 cos / sin tables, the power formed from those float32 sums and stored in
    float32; then float32-rounded mel weights, floor and log in float64, the float32 store, and the normalisation in
    float64 over the stored values, stored in float32 again.  Its distance from `mk_mfb` is what float32 arithmetic costs
    this operation: it sizes the tests' bars.  Returns float32 [T, nfilt].

    The product is summed over the frame's samples in their order, every product and every sum rounded to float32: the
    plain order, and the same on every host (`fr @ cos` would sum in whatever blocks the host's BLAS build chooses for
    its processor, so the bar would depend on the machine that runs the test)."""
    fl, _ = frame_params(sample_rate, winlen, winstep)
    fr = frames(x, sample_rate, winlen, winstep, dtype=np.float32)
    assert fr.dtype == np.float32
    cos, sin = dft_table_f32(fl, nfft)
    re, im = np.zeros((len(fr), nfft // 2 + 1), np.float32), np.zeros((len(fr), nfft // 2 + 1), np.float32)
    for n in range(fl):
        col = fr[:, n, None]
        re += col * cos[n]
        im += col * sin[n]
    assert re.dtype == np.float32
    re, im = re.astype(np.float64), im.astype(np.float64)
    pw = ((re * re + im * im) / nfft).astype(np.float32)
    w = filterbank(nfilt, nfft, sample_rate).astype(np.float32)
    fb = pw.astype(np.float64) @ w.astype(np.float64).T
    fb = np.where(fb == 0, np.finfo(float).eps, fb)
    if use_logscale:
        fb = 20 * np.log10(np.maximum(fb, 1e-5))
    fb = fb.astype(np.float32)
    if normalize is None:
        return fb
    return normalize_frames(fb.astype(np.float64), scale=normalize == "mean_std").astype(np.float32)


def level_steps(seed, n, frame_step, decades=6):
    """Seeded float32 noise whose level falls by a factor of 10 every `frame_step` samples, cycling over `decades`
    decades: neighbouring frames differ by orders of magnitude, so a frame in the wrong row cannot pass for its
    neighbour."""
    rs = np.random.RandomState(seed)
    level = 10.0 ** -((np.arange(n) // frame_step) % decades)
    return (0.5 * np.clip(rs.randn(n) / 3.0, -1.0, 1.0) * level).astype(np.float32)


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
