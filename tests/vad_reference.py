"""TEST INFRASTRUCTURE: float64 NumPy restatement of the energy voice-activity rule of csrc/vad.hip (Kaldi's
compute-vad-energy / select-voiced-frames on the filterbank's own framing): log energy of the raw samples on the int16
scale, a threshold from the utterance's mean, a vote over a window clipped to the utterance."""
import numpy as np

import fbank_reference as FR

DEFAULTS = dict(energy_threshold=5.5, energy_mean_scale=0.5, frames_context=2, proportion_threshold=0.12,
                energy_floor=1.1920929e-07)


def log_energy(x, frame_len=400, frame_step=160, energy_floor=DEFAULTS["energy_floor"]):
    """e[t] = ln(max(sum_i (32768 x[t*step + i])^2, floor)); int16 enters as its integer value; the floor is the float32
    the kernel is handed."""
    s = np.asarray(x, np.float64) * (1.0 if np.asarray(x).dtype == np.int16 else 32768.0)
    nf = FR.n_frames(len(s), frame_len, frame_step)
    pad = np.concatenate([s, np.zeros((nf - 1) * frame_step + frame_len - len(s))])
    idx = np.arange(frame_len)[None, :] + frame_step * np.arange(nf)[:, None]
    return np.log(np.maximum((pad[idx] ** 2).sum(1), np.float64(np.float32(energy_floor))))


def threshold(e, energy_threshold=5.5, energy_mean_scale=0.5, **_):
    return energy_threshold + energy_mean_scale * e.mean()


def decide(e, energy_threshold=5.5, energy_mean_scale=0.5, frames_context=2, proportion_threshold=0.12, **_):
    """bool [T]: the clipped-window vote over e > thr"""
    above = e > threshold(e, energy_threshold, energy_mean_scale)
    T = len(e)
    out = np.zeros(T, bool)
    for t in range(T):
        lo, hi = max(0, t - frames_context), min(T - 1, t + frames_context)
        out[t] = above[lo:hi + 1].sum() >= proportion_threshold * (hi - lo + 1)
    return out


def vad(x, frame_len=400, frame_step=160, **cfg):
    cfg = {**DEFAULTS, **cfg}
    return decide(log_energy(x, frame_len, frame_step, cfg["energy_floor"]), **cfg)
