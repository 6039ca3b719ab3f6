"""TEST INFRASTRUCTURE: float64 NumPy restatement of the waveform augmentation (csrc/augment.hip, features.augment):
reverberation with the direct sound kept in place, additive noise at a signal-to-noise ratio, and the output level
(Kaldi's wav-reverberate --shift-output=true, with the signal power taken over the whole reverberated utterance).  For an
utterance x of n float32 samples (int16 scaled by 1/32768):

    r[m] = sum_k h[k] x[m + p - k]   0 <= m < n, 0 <= k < K, x zero outside [0, n): np.convolve(x, h)[p : p + n],
           p = the index of the first maximum of |h|;  r = x without h
    s[m] = r[m] + sum_j g_j v_j[(s_j + m) mod len(v_j)],   g_j = sqrt(P_r / (P_vj 10^(snr_j / 10))), 0 when a power is 0
    y    = s sqrt(P_x / P_s)  (level "input"; y = s when P_s = 0)   or   y = s  (level "none")

P_x, P_r, P_s: means of the squares over the utterance; P_vj: the mean square of the WHOLE clip.  All in float64 from the
float32 samples.  NumPy only; nothing here comes from the kernels or from features.py."""
import numpy as np

MAX_NOISES = 8
U = 2.0 ** -24                                   # unit roundoff of float32


def to_float64(x):
    """the float32 samples (int16 PCM scaled by 1/32768, exact) as float64"""
    x = np.asarray(x)
    f = x.astype(np.float32) / np.float32(32768) if x.dtype == np.int16 else x.astype(np.float32)
    return f.astype(np.float64)


def delay(h):
    return int(np.argmax(np.abs(np.asarray(h))))


def mean_square(v):
    return float(np.mean(to_float64(v) ** 2))


def reverb(x, h, p=None):
    """float64 r[n]; h None: x itself"""
    x = to_float64(x)
    if h is None:
        return x
    h = to_float64(h)
    p = delay(h) if p is None else int(p)
    return np.convolve(x, h)[p:p + len(x)]


def abs_convolution(x, h, p=None):
    """(|h| conv |x|)[m + p], the scale of the a-priori bound on r"""
    h = to_float64(h)
    p = delay(h) if p is None else int(p)
    return np.convolve(np.abs(to_float64(x)), np.abs(h))[p:p + len(x)]


def gamma(K):
    """gamma_K = K u / (1 - K u): the relative error of K fused multiply-adds in any order"""
    return K * U / (1.0 - K * U)


def noise_terms(r, noises):
    """[(g_j, v_j[(s_j + m) mod len]) ...] for noises = [(clip, start, snr_db) ...]"""
    n = len(r)
    p_r = float(np.mean(r ** 2))
    out = []
    for clip, start, snr in noises:
        v = to_float64(clip)
        p_v = float(np.mean(v ** 2))
        g = np.sqrt(p_r / (p_v * 10.0 ** (snr / 10.0))) if p_r > 0.0 and p_v > 0.0 else 0.0
        out.append((g, v[(int(start) + np.arange(n)) % len(v)]))
    return out


def mix(r, noises):
    s = r.copy()
    for g, v in noise_terms(r, noises):
        s = s + g * v
    return s


def level(x, s, mode):
    if mode == "none":
        return s
    assert mode == "input"
    p_x, p_s = float(np.mean(to_float64(x) ** 2)), float(np.mean(s ** 2))
    return s * np.sqrt(p_x / p_s) if p_s > 0.0 else s


def augment(x, h=None, noises=(), mode="input", p=None):
    """float64 y[n] of one utterance"""
    assert len(noises) <= MAX_NOISES
    return level(x, mix(reverb(x, h, p), noises), mode)


def decaying_rir(seed, K, direct=None, rt=0.3):
    """float32 impulse response of K taps: noise under an exponential decay (-60 dB after rt * K taps) behind a direct
    sound of 1 at tap `direct` (default K // 16), everything before it 20 dB down"""
    rs = np.random.RandomState(seed)
    d = K // 16 if direct is None else direct
    t = np.arange(K)
    h = 0.3 * rs.randn(K) * 10.0 ** (-3.0 * np.maximum(t - d, 0) / max(1.0, rt * K))
    h[:d] *= 0.1
    h[d] = 1.0
    return h.astype(np.float32)
