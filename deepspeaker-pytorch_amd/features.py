"""Log-mel filterbank front end on the device: waveforms -> the [T, 64] features the model consumes.

The reference makes its features offline, one utterance at a time, in float64 NumPy (`mk_MFB`,
audio_processing.py:9-36, run over the corpus by train_triplet.py --makemfb): `python_speech_features.fbank` with
nfilt=64, winlen=0.025 (pre-emphasis 0.97, rectangular window, 512-point power spectrum, triangular mel filters), then
20*log10(max(fb, 1e-5)) and `normalize_frames` (per filter over the utterance: subtract the mean; with use_scale also
divide by std + 2e-12).  Here the whole batch is one HIP call chain (csrc/fbank.hip): the DFT runs as an f32 MFMA GEMM
against a cos/sin basis built once per configuration, and the result is packed [sum T_u, nfilt] f32 on the device,
ready for `data.FeatureStore.from_waveforms`.  Frame counts follow from the host-side lengths: no read-back.

Audio at another rate, or with several channels, goes through `resample` first (csrc/resample.hip): the resampling and
mono down-mix of the reference's `librosa.load(filename, sr=16000, mono=True)` (audio_processing.py:10) as one rational
polyphase filter with SciPy's `resample_poly` design.  Decoding files stays on the host.

Recordings with silence in them go through an energy voice-activity decision (csrc/vad.hip: `voiced_frames`,
`select_frames`, the `vad=` keyword of `log_mel_fbank`): only the voiced frames become rows, and the normalisation runs
over what was kept.

Training utterances are augmented on the device (csrc/augment.hip: `SampleBank`, `AugmentPlan`, `draw_augmentation`,
`augment`, the `augment=` keyword of `log_mel_fbank`): convolved with a room impulse response and mixed with noise clips
at drawn signal-to-noise ratios, the recipe of the x-vector / ECAPA lineage (Kaldi's wav-reverberate).  Which clip, where
in it and how loud are host decisions; only indices cross to the device.
"""
from __future__ import annotations

import decimal
import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .model import get_engine

_engine_override = None
_NORMALIZE = ("mean", "mean_std", None)


def _eng():
    return _engine_override if _engine_override is not None else get_engine()


def _round_half_up(x: float) -> int:
    """python_speech_features.sigproc.round_half_up"""
    return int(decimal.Decimal(x).quantize(decimal.Decimal("1"), rounding=decimal.ROUND_HALF_UP))


@dataclass(frozen=True)
class FbankConfig:
    """The knobs of mk_MFB; the defaults are the reference's constants.py (SAMPLE_RATE=16000, FILTER_BANK=64,
    USE_LOGSCALE=True) and python_speech_features' own (winstep=0.01, nfft=512)."""
    sample_rate: int = 16000
    nfilt: int = 64
    nfft: int = 512
    winlen: float = 0.025
    winstep: float = 0.01
    use_logscale: bool = True

    @property
    def frame_len(self) -> int:
        return _round_half_up(self.winlen * self.sample_rate)

    @property
    def frame_step(self) -> int:
        return _round_half_up(self.winstep * self.sample_rate)


def mel_filterbank(config: FbankConfig) -> np.ndarray:
    """[nfilt, nfft/2+1] float64 triangular filters of python_speech_features.get_filterbanks (lowfreq 0, highfreq
    sample_rate/2)."""
    nfilt, nfft, sr = config.nfilt, config.nfft, config.sample_rate
    hz2mel = lambda hz: 2595 * np.log10(1 + hz / 700.0)
    mel2hz = lambda mel: 700 * (10 ** (mel / 2595.0) - 1)
    pts = np.linspace(hz2mel(0), hz2mel(sr / 2), nfilt + 2)
    b = np.floor((nfft + 1) * mel2hz(pts) / sr)
    fb = np.zeros((nfilt, nfft // 2 + 1))
    for j in range(nfilt):
        for i in range(int(b[j]), int(b[j + 1])):
            fb[j, i] = (i - b[j]) / (b[j + 1] - b[j])
        for i in range(int(b[j + 1]), int(b[j + 2])):
            fb[j, i] = (b[j + 2] - i) / (b[j + 2] - b[j + 1])
    return fb


def dft_basis(frame_len: int, nfft: int) -> np.ndarray:
    """[frame_len rounded up to even, nfft] float32 basis in the kernel's column order: for bin k = 32p + j, column
    64p + j is cos(2 pi n k / nfft) and column 64p + 32 + j is sin(...), except column 32 (sin_0 = 0), which holds the
    Nyquist bin's cos.  Built in float64 with the argument reduced exactly ((n k) mod nfft), rounded once."""
    kpad = (frame_len + 1) & ~1
    n = np.arange(frame_len, dtype=np.int64)[:, None]
    p, j = np.divmod(np.arange(nfft // 2), 32)
    k = 32 * p + j
    col_c = 64 * p + j
    col_s = 64 * p + 32 + j
    ang = lambda kk: 2.0 * np.pi * ((n * kk[None, :]) % nfft) / nfft
    basis = np.zeros((kpad, nfft), np.float64)
    basis[:frame_len, col_c] = np.cos(ang(k))
    basis[:frame_len, col_s] = np.sin(ang(k))
    basis[:frame_len, 32] = np.cos(ang(np.array([nfft // 2])))[:, 0]
    return basis.astype(np.float32)


_tables = {}


def _device_tables(config: FbankConfig, device: torch.device):
    """(basis, band, weights, wstride) on `device`, built once per configuration."""
    key = (config.frame_len, config.nfft, config.nfilt, config.sample_rate, str(device))
    hit = _tables.get(key)
    if hit is None:
        fb = mel_filterbank(config).astype(np.float32)
        nz = [np.nonzero(row)[0] for row in fb]
        band = np.array([[r[0], r[-1] - r[0] + 1] if len(r) else [0, 0] for r in nz], np.int32)
        wstride = max(1, int(band[:, 1].max()))
        w = np.zeros((config.nfilt, wstride), np.float32)
        for f, (b0, cnt) in enumerate(band):
            w[f, :cnt] = fb[f, b0:b0 + cnt]
        hit = (torch.from_numpy(dft_basis(config.frame_len, config.nfft)).to(device),
               torch.from_numpy(band).to(device), torch.from_numpy(w).to(device), wstride)
        _tables[key] = hit
    return hit


def _pack(waveforms, lengths, channels: int = 1):
    """(packed 1-D tensor, host int64 lengths) of either input form; with `channels` > 1 the samples are interleaved
    and the lengths count frames."""
    if isinstance(waveforms, torch.Tensor):
        if lengths is None or waveforms.dim() != 1:
            raise ValueError("a packed waveform tensor must be 1-D and come with the host `lengths` of its utterances")
        packed = waveforms.contiguous()
        lens = np.asarray(lengths, np.int64)
        if lens.ndim != 1 or int(lens.sum()) * channels != packed.numel():
            raise ValueError("lengths must sum to the packed tensor's length")
    else:
        if lengths is not None:
            raise ValueError("lengths are implied by a sequence of waveforms")
        if len(waveforms) == 0:
            raise ValueError("no waveforms")
        if any(w.dim() != 1 for w in waveforms) or len({w.dtype for w in waveforms}) != 1:
            raise ValueError("waveforms must be 1-D tensors of one dtype")
        if any(w.numel() % channels for w in waveforms):
            raise ValueError(f"every waveform must hold whole frames of {channels} interleaved channels")
        lens = np.array([w.numel() // channels for w in waveforms], np.int64)
        packed = waveforms[0].contiguous() if len(waveforms) == 1 else torch.cat(list(waveforms))
    if packed.dtype not in (torch.float32, torch.int16):
        raise ValueError(f"waveforms must be float32 or int16, got {packed.dtype}")
    return packed, lens


def _upload(table: np.ndarray, dev: torch.device) -> torch.Tensor:
    """A host plan table on `dev`: through pinned memory, without blocking the host (a pageable copy waits for the
    stream's queue)."""
    table_t = torch.from_numpy(table)
    return table_t.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else table_t


def _ragged_table(sizes: Sequence[np.ndarray], tiles: np.ndarray) -> np.ndarray:
    """The int64 tile table of csrc/ragged_tiles.h from per-utterance sizes: one column of n_utt + 1 offsets per kind of
    item, the tiles' offsets, then every tile's utterance."""
    offs = [np.concatenate([[0], np.cumsum(v)]) for v in (*sizes, tiles)]
    return np.concatenate(offs + [np.repeat(np.arange(len(tiles)), tiles)]).astype(np.int64)


def _ragged_col(table: np.ndarray, c: int, n_utt: int) -> np.ndarray:
    return table[c * (n_utt + 1):(c + 1) * (n_utt + 1)]


def _plan(eng, dev: torch.device, entry: str, host, n_utt: int, args: tuple, n_cols: int, n_counts: int = 3, tails=()):
    """A `ds_*_plan` entry's two passes over the `host` lengths or offsets, and the upload: the first pass (no table)
    gives the counts, counts[1] the tiles and with them the length of the table of `n_cols` columns; the second fills
    it.  `tails`: further int64 host tables (or None) for the same upload, every part padded to an even number of
    entries (16-byte aligned).  Returns the host table, the counts, the table on `dev` and the tails' views of it."""
    counts = np.zeros(n_counts, np.int64)
    host = np.ascontiguousarray(host, np.int64)
    call = lambda table: eng.lib.call(entry, host.ctypes.data, n_utt, *args, None if table is None else table.ctypes.data,
                                      counts.ctypes.data)
    call(None)
    even = lambda n: (n + 1) & ~1
    ends = np.cumsum([even((n_cols + 1) * (n_utt + 1) + int(counts[1]))] + [0 if t is None else even(t.size) for t in tails])
    table = np.zeros(ends[-1], np.int64)
    call(table)
    for t, at in zip(tails, ends):
        if t is not None:
            table[at:at + t.size] = t.reshape(-1)
    table_dev = _upload(table, dev)
    return table, counts, table_dev, [None if t is None else table_dev[at:] for t, at in zip(tails, ends)]


def _is_int16(packed: torch.Tensor) -> int:
    return 1 if packed.dtype == torch.int16 else 0


def _workspace(eng, entry: str, *args, dtype=torch.float64, device=None) -> torch.Tensor:
    """The workspace of 8-byte entries that a `ds_*_workspace_bytes` entry asks for."""
    return torch.empty(int(eng.lib.raw(entry)(*args)) // 8, dtype=dtype, device=device)


MAX_CHANNELS = 8


def resample_taps(L: int, M: int, zeros: int = 10, beta: float = 5.0) -> np.ndarray:
    """The float64 low-pass table h[0 .. 2H] of `scipy.signal.resample_poly(x, L, M, window=("kaiser", beta))`: with
    q = max(L, M) and H = zeros * q, h = L * w / sum(w), w[i] = sinc((i - H) / q) / q * kaiser(2H + 1, beta)[i].  The
    sinc's zero crossings (i - H a non-zero multiple of q), where np.sinc leaves a residue of 4e-17, are exact zeros: at
    L = M = 1 the table is the unit impulse and resampling returns its input's bits."""
    q = max(int(L), int(M))
    H = int(zeros) * q
    i = np.arange(2 * H + 1) - H
    w = np.sinc(i / q) / q * np.kaiser(2 * H + 1, beta)
    w[(i % q == 0) & (i != 0)] = 0.0
    return L * w / w.sum()


def polyphase_taps(h: np.ndarray, L: int) -> np.ndarray:
    """[L, T | 1] float32, T = ceil(len(h) / L): row p holds h[p], h[p + L], ... in REVERSE (the order of ascending input
    index), zero where the table has no tap and in the padding column (an odd row stride for the LDS banks)."""
    T = -(-len(h) // L)
    full = np.zeros(L * T)
    full[:len(h)] = h
    out = np.zeros((L, T | 1), np.float32)
    out[:, :T] = full.reshape(T, L).T[:, ::-1]
    return out


_taps = {}


def _device_taps(L: int, M: int, zeros: int, beta: float, device: torch.device) -> torch.Tensor:
    key = (L, M, zeros, beta, str(device))
    hit = _taps.get(key)
    if hit is None:
        hit = torch.from_numpy(polyphase_taps(resample_taps(L, M, zeros, beta), L)).to(device)
        _taps[key] = hit
    return hit


def resample(waveforms: Union[Sequence[torch.Tensor], torch.Tensor], orig_rate: int, new_rate: int = 16000,
             channels: int = 1, zeros: int = 10, beta: float = 5.0, lengths: Optional[Sequence[int]] = None
             ) -> Tuple[torch.Tensor, np.ndarray]:
    """Waveforms at `orig_rate` as mono float32 at `new_rate`, in one kernel on the waveforms' device.

    `waveforms`: as for `log_mel_fbank` (a sequence of 1-D float32 / int16 tensors, or one packed 1-D tensor with the
    host `lengths`).  With `channels` > 1 (up to 8) the samples are interleaved [frames, channels], the lengths count
    frames, and the channels are averaged first (summed in order and divided in float32: librosa's mono=True).  The
    filter is `resample_taps(new_rate / g, orig_rate / g, zeros, beta)`, g the rates' gcd: utterance u of n samples
    becomes ceil(n * new_rate / orig_rate) samples, as scipy.signal.resample_poly makes them.  Returns the packed 1-D
    float32 result on the device and the host int64 lengths, which feed `log_mel_fbank(packed, lengths=lengths)`."""
    if int(orig_rate) != orig_rate or int(new_rate) != new_rate or orig_rate < 1 or new_rate < 1:
        raise ValueError(f"sample rates must be positive integers, got {orig_rate!r} -> {new_rate!r}")
    if int(channels) != channels or not 1 <= channels <= MAX_CHANNELS:
        raise ValueError(f"channels must be 1 .. {MAX_CHANNELS}, got {channels!r}")
    if int(zeros) != zeros or zeros < 1:
        raise ValueError(f"zeros must be a positive integer, got {zeros!r}")
    orig_rate, new_rate, channels, zeros, beta = int(orig_rate), int(new_rate), int(channels), int(zeros), float(beta)
    eng = _eng()
    packed, lens = _pack(waveforms, lengths, channels)
    dev = packed.device
    n_utt = len(lens)
    g = math.gcd(orig_rate, new_rate)
    L, M = new_rate // g, orig_rate // g
    half = zeros * max(L, M)

    # output lengths, offsets and the tile table on the host (the lengths are host data)
    table, counts, table_dev, _ = _plan(eng, dev, "ds_resample_plan", lens, n_utt, (L, M, half), 2)
    n_out, n_tiles = int(counts[0]), int(counts[1])
    out_lens = np.diff(_ragged_col(table, 1, n_utt))

    taps = _device_taps(L, M, zeros, beta, dev)
    out = torch.empty(n_out, dtype=torch.float32, device=dev)
    eng.lib.call("ds_resample_poly_f32", eng._p(packed), _is_int16(packed), channels,
                 eng._p(table_dev), n_utt, n_tiles, eng._p(taps), L, M, half, eng._p(out), eng._stream(out))
    return out, out_lens


MAX_NOISES = 8
MAX_RIR_TAPS = 65536
_LEVELS = ("input", "none")


class SampleBank:
    """Noise clips, or room impulse responses, as ONE packed float32 tensor on `device`.

    `clips`: a sequence of 1-D float32 / int16 arrays or tensors (int16 is scaled by 1/32768), none empty.  Kept on the
    host: `offsets` int64 [n + 1], `mean_square` float64 [n] (the mean of x^2 over the WHOLE clip, the noise power of
    `augment`) and `delay` int64 [n] (the index of the first maximum of |x|: the direct sound of an impulse response).
    Building the bank is the one place that synchronises: clips that live on a device are copied to the host for these
    statistics."""

    def __init__(self, clips, device="cuda"):
        if isinstance(clips, (torch.Tensor, np.ndarray)) or len(clips) == 0:
            raise ValueError("a SampleBank takes a non-empty sequence of 1-D clips")
        host = []
        for i, c in enumerate(clips):
            a = c.detach().cpu().numpy() if isinstance(c, torch.Tensor) else np.asarray(c)
            if a.ndim != 1 or a.dtype not in (np.float32, np.int16):
                raise ValueError(f"clip {i} must be a 1-D float32 or int16 array, got {a.dtype} with {a.ndim} dimensions")
            if a.size == 0:
                raise ValueError(f"clip {i} is empty")
            host.append(a.astype(np.float32) / np.float32(32768) if a.dtype == np.int16 else a)
        self.offsets = np.concatenate([[0], np.cumsum([len(a) for a in host])]).astype(np.int64)
        self.mean_square = np.array([np.mean(a.astype(np.float64) ** 2) for a in host], np.float64)
        self.delay = np.array([int(np.argmax(np.abs(a))) for a in host], np.int64)
        self.samples = torch.from_numpy(np.concatenate(host)).to(device)

    def __len__(self):
        return len(self.offsets) - 1

    @property
    def lengths(self) -> np.ndarray:
        return np.diff(self.offsets)

    @property
    def device(self) -> torch.device:
        return self.samples.device


@dataclass
class AugmentPlan:
    """What `augment` does to each utterance of a batch; all of it host data.

    `rir_index` [n_utt]: the utterance's impulse response in `rir_bank`, -1 for none.  `noise_index`, `noise_start`,
    `snr_db` [n_utt, J] (J <= MAX_NOISES): the clips of `noise_bank` added to the utterance (-1 for none), the sample of
    the clip that meets the utterance's first, and the signal-to-noise ratio in dB.  `level`: "input" scales the result to
    the input's power, "none" leaves it.  A plan without tables changes nothing."""
    rir_bank: Optional[SampleBank] = None
    rir_index: Optional[np.ndarray] = None
    noise_bank: Optional[SampleBank] = None
    noise_index: Optional[np.ndarray] = None
    noise_start: Optional[np.ndarray] = None
    snr_db: Optional[np.ndarray] = None
    level: str = "input"


def draw_augmentation(rs: np.random.RandomState, n_utt: int, rir_bank: Optional[SampleBank] = None,
                      noise_bank: Optional[SampleBank] = None, p_rir: float = 0.5, p_noise: float = 0.5,
                      snr_db: Tuple[float, float] = (0.0, 15.0), noises: Tuple[int, int] = (1, 1),
                      level: str = "input") -> AugmentPlan:
    """An `AugmentPlan` drawn from the caller's `rs`: with probability `p_rir` an utterance gets an impulse response drawn
    uniformly from `rir_bank`; with probability `p_noise` it gets between noises[0] and noises[1] (inclusive) clips drawn
    uniformly from `noise_bank`, each from a uniform start at a ratio uniform in snr_db = (lo, hi) dB.  The draws are made
    in this order, whole arrays at a time: the reverberation coin and index, the noise coin, the count, then index,
    start and ratio [n_utt, J]."""
    if int(n_utt) != n_utt or n_utt < 1:
        raise ValueError(f"n_utt must be a positive integer, got {n_utt!r}")
    if not (0.0 <= p_rir <= 1.0 and 0.0 <= p_noise <= 1.0):
        raise ValueError(f"p_rir and p_noise must be probabilities, got {p_rir!r}, {p_noise!r}")
    lo, hi = (int(v) for v in noises)
    if not 1 <= lo <= hi <= MAX_NOISES:
        raise ValueError(f"noises must be (lo, hi) with 1 <= lo <= hi <= {MAX_NOISES}, got {noises!r}")
    if not (math.isfinite(snr_db[0]) and math.isfinite(snr_db[1]) and snr_db[0] <= snr_db[1]):
        raise ValueError(f"snr_db must be a finite (lo, hi), got {snr_db!r}")
    n_utt = int(n_utt)
    plan = AugmentPlan(level=level)
    if rir_bank is not None:
        coin = rs.random_sample(n_utt) < p_rir
        plan.rir_bank = rir_bank
        plan.rir_index = np.where(coin, rs.randint(0, len(rir_bank), n_utt), -1).astype(np.int64)
    if noise_bank is not None:
        coin = rs.random_sample(n_utt) < p_noise
        count = np.where(coin, rs.randint(lo, hi + 1, n_utt), 0)
        index = rs.randint(0, len(noise_bank), (n_utt, hi)).astype(np.int64)
        start = np.floor(rs.random_sample((n_utt, hi)) * noise_bank.lengths[index]).astype(np.int64)
        ratio = rs.uniform(snr_db[0], snr_db[1], (n_utt, hi))
        used = np.arange(hi)[None, :] < count[:, None]
        plan.noise_bank = noise_bank
        plan.noise_index = np.where(used, index, -1)
        plan.noise_start = np.where(used, start, 0)
        plan.snr_db = np.where(used, ratio, 0.0)
    return plan


def _augment_tables(plan: AugmentPlan, n_utt: int, dev: torch.device):
    """The validated host tables of a plan: (rir_tab [n_utt, 3] or None, largest K, noise_tab [n_utt, J, 5] or None)."""
    if not isinstance(plan, AugmentPlan):
        raise ValueError(f"augment takes an AugmentPlan, got {plan!r}")
    if plan.level not in _LEVELS:
        raise ValueError(f"level must be one of {_LEVELS}, got {plan.level!r}")

    def bank_of(bank, what):
        if not isinstance(bank, SampleBank):
            raise ValueError(f"{what} needs a SampleBank, got {bank!r}")
        if bank.device != dev:
            raise ValueError(f"the {what} bank is on {bank.device}, the waveforms are on {dev}")
        return bank

    rir_tab, max_taps = None, 0
    if plan.rir_index is not None:
        bank = bank_of(plan.rir_bank, "rir_index")
        idx = np.asarray(plan.rir_index)
        if idx.shape != (n_utt,) or idx.dtype.kind not in "iu":
            raise ValueError(f"rir_index must be {n_utt} integers, one per utterance, got shape {idx.shape} {idx.dtype}")
        idx = idx.astype(np.int64)
        if (idx < -1).any() or (idx >= len(bank)).any():
            raise ValueError(f"rir_index must be -1 or an index into the bank's {len(bank)} impulse responses")
        if (idx >= 0).any():
            at = np.maximum(idx, 0)
            rir_tab = np.stack([np.where(idx >= 0, bank.offsets[at], -1), bank.lengths[at], bank.delay[at]], 1)
            max_taps = int(bank.lengths[idx[idx >= 0]].max())

    noise_tab = None
    given = [t is not None for t in (plan.noise_index, plan.noise_start, plan.snr_db)]
    if any(given):
        if not all(given):
            raise ValueError("noise_index, noise_start and snr_db come together")
        bank = bank_of(plan.noise_bank, "noise_index")
        idx, start, snr = np.asarray(plan.noise_index), np.asarray(plan.noise_start), np.asarray(plan.snr_db, np.float64)
        if idx.ndim != 2 or idx.shape[0] != n_utt or idx.shape[1] < 1 or start.shape != idx.shape or snr.shape != idx.shape:
            raise ValueError(f"noise_index, noise_start and snr_db must share the shape [{n_utt}, J], got {idx.shape}, "
                             f"{start.shape}, {snr.shape}")
        if idx.shape[1] > MAX_NOISES:
            raise ValueError(f"at most {MAX_NOISES} noises per utterance, got {idx.shape[1]}")
        if idx.dtype.kind not in "iu" or start.dtype.kind not in "iu":
            raise ValueError("noise_index and noise_start must be integers")
        idx, start = idx.astype(np.int64), start.astype(np.int64)
        if (idx < -1).any() or (idx >= len(bank)).any():
            raise ValueError(f"noise_index must be -1 or an index into the bank's {len(bank)} clips")
        on = idx >= 0
        at = np.maximum(idx, 0)
        if (on & ((start < 0) | (start >= bank.lengths[at]))).any():
            raise ValueError("noise_start must lie inside its clip")
        if not np.isfinite(snr[on]).all():
            raise ValueError("snr_db must be finite")
        if on.any():
            if int(bank.lengths[at[on]].max()) >= 1 << 31:
                raise ValueError("a noise clip must be shorter than 2^31 samples")
            factor = 10.0 ** (np.where(on, snr, 0.0) / 10.0)
            noise_tab = np.stack([np.where(on, bank.offsets[at], -1), bank.lengths[at], np.where(on, start, 0),
                                  bank.mean_square[at].view(np.int64), factor.view(np.int64)], 2)
    return rir_tab, max_taps, noise_tab


def augment(waveforms: Union[Sequence[torch.Tensor], torch.Tensor], plan: AugmentPlan,
            lengths: Optional[Sequence[int]] = None) -> Tuple[torch.Tensor, np.ndarray]:
    """The waveforms reverberated, mixed with noise and levelled as `plan` says, on the waveforms' device.

    `waveforms` / `lengths`: as for `resample` (mono).  Utterance u with impulse response h of K taps (at most
    MAX_RIR_TAPS) and delay p becomes r = np.convolve(x, h)[p : p + n]: the direct sound stays where it was and the length
    does not change (Kaldi's wav-reverberate --shift-output=true).  Every noise clip v is then added from its start,
    wrapping around, with the gain sqrt(P_r / (P_v * 10^(snr / 10))): P_r the mean square of the whole reverberated
    utterance, P_v that of the whole clip.  With level="input" the sum is scaled to the input's mean square.  The powers
    are accumulated in float64 on the device in a fixed order and every output sample is one fixed chain of fused
    multiply-adds: the result does not depend on the batch.  Returns the packed 1-D float32 result and the host int64
    lengths (unchanged); nothing is read back."""
    eng = _eng()
    packed, lens = _pack(waveforms, lengths)
    dev = packed.device
    n_utt = len(lens)
    rir_tab, max_taps, noise_tab = _augment_tables(plan, n_utt, dev)

    # one upload: the tile table, then the plan's tables
    _, counts, table_dev, (rir_dev, noise_dev) = _plan(eng, dev, "ds_augment_plan", lens, n_utt, (), 1, n_counts=4,
                                                       tails=(rir_tab, noise_tab))
    n_total, n_tiles = int(counts[0]), int(counts[1])

    out = torch.empty(n_total, dtype=torch.float32, device=dev)
    ws = _workspace(eng, "ds_augment_workspace_bytes", n_tiles, device=dev)
    stream = eng._stream(out)
    eng.lib.call("ds_augment_reverb_f32", eng._p(packed), _is_int16(packed), eng._p(table_dev), n_utt,
                 n_tiles, None if rir_tab is None else eng._p(plan.rir_bank.samples), eng._p(rir_dev), max_taps,
                 eng._p(out), eng._p(ws), stream)
    if noise_tab is not None:
        eng.lib.call("ds_augment_mix_f32", eng._p(out), eng._p(table_dev), n_utt, n_tiles,
                     eng._p(plan.noise_bank.samples), eng._p(noise_dev), noise_tab.shape[1], eng._p(ws), stream)
    if plan.level == "input" and (rir_tab is not None or noise_tab is not None):
        eng.lib.call("ds_augment_level_f32", eng._p(out), eng._p(table_dev), n_utt, n_tiles,
                     1 if noise_tab is not None else 0, eng._p(ws), stream)
    return out, lens.copy()


_augment = augment                               # `augment=` is also a keyword of log_mel_fbank


def _fbank_plan(eng, lens: np.ndarray, config: FbankConfig, dev: torch.device):
    """Framing on the host (the lengths are host data): (table on the device, frame offsets, frames, tiles, rows per
    tile) of ds_fbank_plan."""
    n_utt = len(lens)
    table, counts, table_dev, _ = _plan(eng, dev, "ds_fbank_plan", lens, n_utt,
                                        (config.frame_len, config.frame_step, config.nfft, config.nfilt), 2)
    n_frames, n_tiles, tile_rows = (int(v) for v in counts)
    return table_dev, _ragged_col(table, 1, n_utt).copy(), n_frames, n_tiles, tile_rows


@dataclass(frozen=True)
class VadConfig:
    """The energy voice-activity rule (Kaldi's compute-vad-energy on this package's framing, csrc/vad.hip): frame t is
    voiced iff at least `proportion_threshold` of the frames t - frames_context .. t + frames_context (clipped to the
    utterance) have a log energy above energy_threshold + energy_mean_scale * (the utterance's mean log energy).  The
    energy is ln(max(sum (32768 x)^2, energy_floor)) over the raw samples of the frame: the int16 scale, so the usual
    recipe thresholds carry over."""
    energy_threshold: float = 5.5
    energy_mean_scale: float = 0.5
    frames_context: int = 2
    proportion_threshold: float = 0.12
    energy_floor: float = 1.1920929e-07

    def __post_init__(self):
        for name in ("energy_threshold", "energy_mean_scale", "proportion_threshold", "energy_floor"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"{name} must be a finite number, got {v!r}")
        if isinstance(self.frames_context, bool) or not isinstance(self.frames_context, (int, np.integer)) \
                or self.frames_context < 0:
            raise ValueError(f"frames_context must be a non-negative integer, got {self.frames_context!r}")
        if not 0.0 < self.proportion_threshold <= 1.0:
            raise ValueError(f"proportion_threshold must be in (0, 1], got {self.proportion_threshold!r}")
        if not self.energy_floor > 0.0:
            raise ValueError(f"energy_floor must be positive, got {self.energy_floor!r}")


SELECT_TILE_ROWS = 64                            # rows per workgroup of the selection and of the normalisation after it


def _log_energy(eng, packed, table_dev, n_utt, n_frames, n_tiles, tile_rows, config: FbankConfig, floor: float):
    out = torch.empty(n_frames, dtype=torch.float32, device=packed.device)
    eng.lib.call("ds_vad_log_energy_f32", eng._p(packed), _is_int16(packed), eng._p(table_dev), n_utt,
                 n_tiles, tile_rows, config.frame_len, config.frame_step, float(floor), eng._p(out), eng._stream(out))
    return out


def _vad_plan(eng, offsets: np.ndarray, dev: torch.device):
    """(decision table on the device, decision tiles) of ds_vad_plan over the host frame offsets."""
    n_utt = len(offsets) - 1
    _, counts, table_dev, _ = _plan(eng, dev, "ds_vad_plan", offsets, n_utt, (), 1)
    return table_dev, int(counts[1])


def _vad_buffers(eng, n_utt, n_frames, n_dtiles, dev):
    scan = torch.empty(n_frames, dtype=torch.int32, device=dev)
    kept = torch.empty(n_utt, dtype=torch.int64, device=dev)
    ws = _workspace(eng, "ds_vad_workspace_bytes", n_utt, n_dtiles, dtype=torch.int64, device=dev)
    return scan, kept, ws


def _voiced(eng, packed, lens, vad: VadConfig, config: FbankConfig, plan=None):
    """(mask, scan, kept, decision table, frame offsets), all but the last on the device; `plan`: the caller's
    `_fbank_plan` of the same lengths."""
    dev = packed.device
    n_utt = len(lens)
    table_dev, offsets, n_frames, n_tiles, tile_rows = _fbank_plan(eng, lens, config, dev) if plan is None else plan
    energy = _log_energy(eng, packed, table_dev, n_utt, n_frames, n_tiles, tile_rows, config, vad.energy_floor)
    vtable_dev, n_dtiles = _vad_plan(eng, offsets, dev)
    mask = torch.empty(n_frames, dtype=torch.uint8, device=dev)
    scan, kept, ws = _vad_buffers(eng, n_utt, n_frames, n_dtiles, dev)
    eng.lib.call("ds_vad_decide", eng._p(energy), eng._p(vtable_dev), n_utt, n_dtiles, float(vad.energy_threshold),
                 float(vad.energy_mean_scale), int(vad.frames_context), float(vad.proportion_threshold), eng._p(mask),
                 eng._p(scan), eng._p(kept), eng._p(ws), eng._stream(mask))
    return mask, scan, kept, vtable_dev, offsets


def _select(eng, feats, mask, scan, kept, vtable_dev):
    """(packed kept rows, new host offsets, table over the kept rows, its tiles, the workspace holding the tiles' sums).
    Reads `kept` back: the one copy to the host."""
    dev = feats.device
    n_utt, nfilt = kept.numel(), feats.shape[1]
    counts = kept.cpu().numpy()
    new_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    tiles = -(-counts // SELECT_TILE_ROWS)
    n_ktiles = int(tiles.sum())
    out = torch.empty((int(new_off[-1]), nfilt), dtype=torch.float32, device=dev)
    if n_ktiles == 0:
        return out, new_off, None, 0, None
    # ds_fbank_plan's two columns, because ds_fbank_normalize_f32 reads this table too: no samples, the kept frames
    ktable_dev = _upload(_ragged_table([np.zeros(n_utt, np.int64), counts], tiles), dev)
    ws = _workspace(eng, "ds_fbank_workspace_bytes", n_utt, n_ktiles, nfilt, device=dev)
    eng.lib.call("ds_vad_select_f32", eng._p(feats), eng._p(mask), eng._p(scan), eng._p(vtable_dev), eng._p(ktable_dev),
                 n_utt, n_ktiles, nfilt, SELECT_TILE_ROWS, eng._p(out), eng._p(ws), eng._stream(out))
    return out, new_off, ktable_dev, n_ktiles, ws


def frame_log_energy(waveforms: Union[Sequence[torch.Tensor], torch.Tensor], config: FbankConfig = FbankConfig(),
                     lengths: Optional[Sequence[int]] = None, *, energy_floor: float = VadConfig.energy_floor
                     ) -> Tuple[torch.Tensor, np.ndarray]:
    """The log energy of every frame of the filterbank's framing: ln(max(sum (32768 x)^2, energy_floor)) over the raw
    samples (int16 PCM enters as its integer value), zero past the utterance's end.  `waveforms` / `lengths`: as for
    `log_mel_fbank`.  Returns the packed float32 [sum T_u] on the device and the host int64 frame offsets [n_utt + 1].
    Every frame is summed in one fixed order: the values do not depend on the batch."""
    eng = _eng()
    packed, lens = _pack(waveforms, lengths)
    table_dev, offsets, n_frames, n_tiles, tile_rows = _fbank_plan(eng, lens, config, packed.device)
    return _log_energy(eng, packed, table_dev, len(lens), n_frames, n_tiles, tile_rows, config, energy_floor), offsets


def voiced_frames(waveforms: Union[Sequence[torch.Tensor], torch.Tensor], vad: VadConfig = VadConfig(),
                  config: FbankConfig = FbankConfig(), lengths: Optional[Sequence[int]] = None, *,
                  orig_rate: Optional[int] = None, channels: int = 1) -> Tuple[torch.Tensor, np.ndarray]:
    """The voice-activity decision of `VadConfig` for every frame of the filterbank's framing.  `waveforms`, `lengths`,
    `orig_rate`, `channels`: as for `log_mel_fbank`; audio at another rate is resampled first and the decision is that of
    the resampled mono signal.  Returns the uint8 mask [sum T_u] (1 = voiced) on the device and the host int64 frame
    offsets [n_utt + 1]: the rows of `log_mel_fbank(...)[0]`.  Nothing is read back."""
    if orig_rate is not None or channels != 1:
        waveforms, lengths = resample(waveforms, config.sample_rate if orig_rate is None else orig_rate,
                                      config.sample_rate, channels, lengths=lengths)
    packed, lens = _pack(waveforms, lengths)
    mask, _, _, _, offsets = _voiced(_eng(), packed, lens, vad, config)
    return mask, offsets


def select_frames(feats: torch.Tensor, offsets: Sequence[int], mask: torch.Tensor) -> Tuple[torch.Tensor, np.ndarray]:
    """The rows of `feats` [sum T_u, F] float32 whose `mask` entry (uint8 [sum T_u], non-zero = keep) is set, packed in
    their order, and the new host int64 offsets [n_utt + 1]; an utterance without a kept row has none
    (offsets[u] == offsets[u + 1]).

    This is the one place of the front end that READS BACK from the device: the n_utt kept counts, in one copy, because
    offsets are host data throughout this package and the result's size depends on them.  The call therefore waits for
    the stream and cannot be captured into a graph."""
    if not isinstance(feats, torch.Tensor) or feats.dim() != 2 or feats.dtype != torch.float32:
        raise ValueError("feats must be a 2-D float32 tensor")
    if not isinstance(mask, torch.Tensor) or mask.dim() != 1 or mask.dtype != torch.uint8:
        raise ValueError("mask must be a 1-D uint8 tensor")
    off = np.asarray(offsets, np.int64)
    if off.ndim != 1 or len(off) < 2 or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != feats.shape[0]:
        raise ValueError("offsets must rise from 0 to the number of rows")
    if mask.numel() != feats.shape[0]:
        raise ValueError(f"the mask has {mask.numel()} entries for {feats.shape[0]} rows")
    if mask.device != feats.device:
        raise ValueError("mask and feats must be on one device")
    eng = _eng()
    feats, mask = feats.contiguous(), mask.contiguous()
    n_utt = len(off) - 1
    vtable_dev, n_dtiles = _vad_plan(eng, off, feats.device)
    if n_dtiles == 0:
        return feats.new_empty((0, feats.shape[1])), np.zeros(n_utt + 1, np.int64)
    scan, kept, ws = _vad_buffers(eng, n_utt, feats.shape[0], n_dtiles, feats.device)
    eng.lib.call("ds_vad_scan", eng._p(mask), eng._p(vtable_dev), n_utt, n_dtiles, eng._p(scan), eng._p(kept), eng._p(ws),
                 eng._stream(mask))
    out, new_off, _, _, _ = _select(eng, feats, mask, scan, kept, vtable_dev)
    return out, new_off


def log_mel_fbank(waveforms: Union[Sequence[torch.Tensor], torch.Tensor], config: FbankConfig = FbankConfig(),
                  normalize: Optional[str] = "mean", lengths: Optional[Sequence[int]] = None, *,
                  orig_rate: Optional[int] = None, channels: int = 1, vad: Optional[VadConfig] = None,
                  augment: Optional[AugmentPlan] = None) -> Tuple[torch.Tensor, np.ndarray]:
    """mk_MFB of every waveform in one call chain on the waveforms' device.

    `waveforms`: a sequence of 1-D tensors (float32 samples, or int16 PCM, which is scaled by 1/32768), or ONE packed
    1-D tensor with the host `lengths` of its utterances.  `normalize`: "mean" (the reference's USE_SCALE=False),
    "mean_std" (USE_SCALE=True) or None (raw log filterbank; with config.use_logscale=False the raw filterbank).
    `orig_rate` / `channels`: the waveforms' own sample rate and interleaved channel count; given, they are first
    resampled to config.sample_rate and mixed down to mono on the device (`resample`), which together with this
    function is the reference's librosa.load(..., sr=16000, mono=True) followed by mk_MFB.
    `vad`: given, only the voiced frames of `voiced_frames` (decided on the same, resampled, waveform) are kept, in
    order, and the normalisation runs over the kept rows; an utterance without a voiced frame has no row.  This reads the
    kept counts back (`select_frames`), so the call waits for the stream and cannot be captured into a graph.
    `augment`: an `AugmentPlan`; the (resampled, mono) waveforms go through `augment` before the voice-activity decision
    and the filterbank.
    Returns the packed [sum T_u, nfilt] float32 features on the device and the host int64 frame offsets [n_utt + 1]:
    utterance u is rows offsets[u]:offsets[u+1].  Decoding files is the caller's; deltas are not computed (the
    reference's USE_DELTA is False)."""
    if normalize not in _NORMALIZE:
        raise ValueError(f"normalize must be one of {_NORMALIZE}, got {normalize!r}")
    if vad is not None and not isinstance(vad, VadConfig):
        raise ValueError(f"vad must be a VadConfig or None, got {vad!r}")
    if orig_rate is not None or channels != 1:
        waveforms, lengths = resample(waveforms, config.sample_rate if orig_rate is None else orig_rate,
                                      config.sample_rate, channels, lengths=lengths)
    if augment is not None:
        waveforms, lengths = _augment(waveforms, augment, lengths=lengths)
    eng = _eng()
    packed, lens = _pack(waveforms, lengths)
    dev = packed.device
    n_utt = len(lens)
    fl, fs, nfft, nfilt = config.frame_len, config.frame_step, config.nfft, config.nfilt
    table_dev, offsets, n_frames, n_tiles, tile_rows = _fbank_plan(eng, lens, config, dev)

    basis, band, weights, wstride = _device_tables(config, dev)
    out = torch.empty((n_frames, nfilt), dtype=torch.float32, device=dev)
    workspace = _workspace(eng, "ds_fbank_workspace_bytes", n_utt, n_tiles, nfilt, device=dev)
    stream = eng._stream(out)
    eng.lib.call("ds_fbank_logmel_f32", eng._p(packed), _is_int16(packed), eng._p(table_dev),
                 n_utt, n_tiles, eng._p(basis), eng._p(band), eng._p(weights), wstride, fl, fs, nfft, nfilt,
                 1 if config.use_logscale else 0, eng._p(out), eng._p(workspace), stream)
    if vad is not None:
        # the kept rows, their tiles' sums and the table over them: the normalisation below runs over what was kept
        mask, scan, kept, vtable_dev, _ = _voiced(eng, packed, lens, vad, config,
                                                  (table_dev, offsets, n_frames, n_tiles, tile_rows))
        out, offsets, table_dev, n_tiles, workspace = _select(eng, out, mask, scan, kept, vtable_dev)
        tile_rows = SELECT_TILE_ROWS
        if n_tiles == 0:
            return out, offsets
    if normalize is not None:
        eng.lib.call("ds_fbank_normalize_f32", eng._p(out), eng._p(table_dev), n_utt, n_tiles, nfilt, tile_rows,
                     1 if normalize == "mean_std" else 0, eng._p(workspace), stream)
    return out, offsets
