"""TEST INFRASTRUCTURE: float64 NumPy restatement of the resampling and mono down-mix in the reference's
`librosa.load(filename, sr=16000, mono=True)` (audio_processing.py:10), as rational polyphase filtering with SciPy's
default design: it equals `scipy.signal.resample_poly(x, L, M, window=("kaiser", 5.0))` to 1e-12 where SciPy is
installed (tests/test_emul_resample.py).  With g = gcd(orig_rate, new_rate), L = new_rate / g, M = orig_rate / g,
q = max(L, M), H = zeros * q:

    h[i] = L * w[i] / sum(w),  w[i] = sinc((i - H) / q) / q * kaiser(2H + 1, beta)[i],  i = 0 .. 2H
    n_out = ceil(n * L / M)
    y[m]  = sum_k x[k] * h[H + m*M - k*L]   over 0 <= k < n with 0 <= H + m*M - k*L <= 2H

NumPy only; nothing here comes from the kernels or from features.py."""
import math

import numpy as np


def ratio(orig_rate, new_rate):
    g = math.gcd(int(orig_rate), int(new_rate))
    return int(new_rate) // g, int(orig_rate) // g


def taps(L, M, zeros=10, beta=5.0):
    q = max(L, M)
    H = zeros * q
    i = np.arange(2 * H + 1)
    w = np.sinc((i - H) / q) / q * np.kaiser(2 * H + 1, beta)
    return L * w / w.sum()


def n_taps(L, M, zeros=10):
    """taps per output, T = ceil((2H + 1) / L)"""
    return -(-(2 * zeros * max(L, M) + 1) // L)


def n_out(n, L, M):
    return -(-(int(n) * L) // M)


def resample(x, L, M, zeros=10, beta=5.0):
    """float64 y[ceil(n L / M)] of the 1-D signal x (any real dtype, taken as float64).  Vectorised over the outputs:
    step j adds every output's j-th polyphase tap, h[p + j L] with p = (H + m M) mod L, times x[(H + m M) // L - j]."""
    x = np.asarray(x, np.float64)
    n = len(x)
    h = taps(L, M, zeros, beta)
    H = zeros * max(L, M)
    m = np.arange(n_out(n, L, M), dtype=np.int64)
    c = H + m * M
    p, k_hi = c % L, c // L
    y = np.zeros(len(m))
    for j in range(n_taps(L, M, zeros)):
        i, k = p + j * L, k_hi - j
        ok = (i <= 2 * H) & (k >= 0) & (k < n)
        y[ok] += x[k[ok]] * h[i[ok]]
    return y


def resample_f32(x, L, M, zeros=10, beta=5.0):
    """The same sum as a float32 kernel has it: float32 samples times the float32-rounded taps, every product and every
    partial sum rounded to float32, each output summed in the order of ASCENDING input index (tap H + m M - k L falls as
    k rises, so j runs from the last polyphase tap down).  Its distance from `resample` is what float32 arithmetic costs
    this operation; it is not claimed bit-equal to the kernel, whose fmaf rounds once per step where this rounds twice.
    Returns float32."""
    x = np.asarray(x).astype(np.float32)
    n = len(x)
    h = taps(L, M, zeros, beta).astype(np.float32)
    H = zeros * max(L, M)
    m = np.arange(n_out(n, L, M), dtype=np.int64)
    c = H + m * M
    p, k_hi = c % L, c // L
    y = np.zeros(len(m), np.float32)
    for j in range(n_taps(L, M, zeros) - 1, -1, -1):
        i, k = p + j * L, k_hi - j
        ok = (i <= 2 * H) & (k >= 0) & (k < n)
        y[ok] = y[ok] + x[k[ok]] * h[i[ok]]
    assert y.dtype == np.float32
    return y


def to_float32(x):
    """int16 PCM scaled by 1/32768 (exact in float32); float32 unchanged"""
    x = np.asarray(x)
    return x.astype(np.float32) / np.float32(32768) if x.dtype == np.int16 else x.astype(np.float32)


def downmix(x, channels):
    """float32 mono of interleaved [n * channels] (or [n, channels]) samples in the stated float32 arithmetic: the
    channels summed in channel order, then the sum divided by `channels`."""
    f = to_float32(x).reshape(-1, channels)
    if channels == 1:
        return f[:, 0].copy()
    s = f[:, 0].copy()
    for c in range(1, channels):
        s = (s + f[:, c]).astype(np.float32)
    return (s / np.float32(channels)).astype(np.float32)


def apriori_bound(L, M, zeros=10, beta=5.0, peak=1.0):
    """Bound on |float32 kernel - this restatement| for inputs of magnitude <= peak: every one of the T products
    x * round_f32(h) carries the table's rounding (2^-24 relative), and the fmaf chain rounds T times, each by at most
    2^-24 of a partial sum that is itself at most sum_j |h| * peak: (T + 2) * 2^-24 * max_p sum_j |h[p + j L]| * peak."""
    h = np.abs(taps(L, M, zeros, beta))
    T = n_taps(L, M, zeros)
    full = np.zeros(L * T)
    full[:len(h)] = h
    return (T + 2) * 2.0 ** -24 * full.reshape(T, L).sum(axis=0).max() * peak
