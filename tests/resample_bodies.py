"""TEST INFRASTRUCTURE: the resampler's cases (csrc/resample.hip, features.resample), written once and run by
tests/test_emul_resample.py through the host emulator and by tests/test_gpu_resample.py on the device.  Every body takes
a `Ctx`: the features module to call, the device the tensors live on and the loaded library.  References come from
tests/resample_reference.py (float64) and are computed once per process."""
import functools
from dataclasses import dataclass

import numpy as np
import pytest
import torch

import fbank_reference as FR
import resample_reference as R

NEW_RATE = 16000
RATES = (48000, 44100, 32000, 8000, 11025, 24000, 16000)
DTYPES = ("float32", "int16")

# End to end, waveforms at 48000 / 44100 / 8000 Hz -> resample -> log-mel features, against
# mk_mfb(float32(restatement resample)) in float64: max |feature difference| in dB over 1 s of "noise" and "ar".
# Measured through the host emulator: 2.3e-4 (8 kHz "ar": the upsampled signal's empty upper band sits near the 1e-5
# floor of the log; 48 kHz 5.5e-5, 44.1 kHz 6.0e-5); on the MI355X: 2.3e-4, every case equal to the emulator's to the
# printed digits.
# The bar is 3 x the larger, rounded up to one significant digit (the margin the filterbank's own 5e-4 bar keeps over its
# measured 2.1e-4).
E2E_TOL_DB = 7e-4
E2E_RATES = (48000, 44100, 8000)


@dataclass
class Ctx:
    features: object
    dev: str
    lib: object

    def t(self, x):
        return torch.from_numpy(np.array(x)).to(self.dev)            # a copy: the shared cases are read-only


def tile_size(lib, L, M, zeros=10):
    counts = np.zeros(3, np.int64)
    one = np.array([1], np.int64)
    assert lib.raw("ds_resample_plan")(one.ctypes.data, 1, L, M, zeros * max(L, M), None, counts.ctypes.data) == 0
    return int(counts[2])


def edge_lengths(L, M, tile, zeros=10):
    """n in {1, 2, M-1, M, M+1}, one shorter than H/L, and the n whose n_out is tile-1, tile, tile+1 and 2 tile+1 (when
    upsampling n_out moves in steps of L/M, so a target in between is met by the next one above it)."""
    H = zeros * max(L, M)
    ns = [1, 2, M - 1, M, M + 1, max(1, (H // L) // 2)]
    for target in (tile - 1, tile, tile + 1, 2 * tile + 1):
        n = target * M // L
        ns.append(n if -(-n * L // M) >= target else n + 1)
    out = []
    for n in ns:
        if n >= 1 and n not in out:
            out.append(n)
    return out


@functools.lru_cache(maxsize=None)
def value_batch(rate, tile, dtype):
    """(signals, float64 references, peak): every edge length twice, once as "noise" and once as "ar"."""
    L, M = R.ratio(rate, NEW_RATE)
    xs = []
    for i, n in enumerate(edge_lengths(L, M, tile)):
        for j, kind in enumerate(("noise", "ar")):
            x = FR.synthetic_audio(7000 + 10 * i + j, n, rate, kind)
            xs.append(FR.int16_quantised(x) if dtype == "int16" else x)
    refs = [R.resample(R.to_float32(x), L, M) for x in xs]
    peak = max(float(np.abs(R.to_float32(x)).max()) for x in xs)
    for a in xs + refs:
        a.setflags(write=False)
    return xs, refs, peak


def split(out, lens):
    y = out.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(lens)])
    assert len(y) == off[-1]
    return [y[off[u]:off[u + 1]] for u in range(len(lens))]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---- 2. values ----
def values(ctx, rate, dtype):
    L, M = R.ratio(rate, NEW_RATE)
    tile = tile_size(ctx.lib, L, M)
    xs, refs, peak = value_batch(rate, tile, dtype)
    out, lens = ctx.features.resample([ctx.t(x) for x in xs], rate)
    assert out.dtype == torch.float32 and out.dim() == 1 and lens.dtype == np.int64
    assert lens.tolist() == [-(-len(x) * L // M) for x in xs] == [len(r) for r in refs]
    n_outs = set(lens.tolist())
    if L <= M:                                   # every output count is reachable when not upsampling
        assert {tile - 1, tile, tile + 1, 2 * tile + 1} <= n_outs
    err = max(float(np.abs(y - r).max()) for y, r in zip(split(out, lens), refs))
    bound = R.apriori_bound(L, M, peak=peak)
    print(f"resample {rate} -> {NEW_RATE} ({L}/{M}, tile {tile}) {dtype}: max abs error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)


# ---- 3. identity ----
def identity(ctx):
    x = FR.synthetic_audio(1, 5000, kind="ar")
    q = FR.int16_quantised(FR.synthetic_audio(2, 5000, kind="noise"))
    out, lens = ctx.features.resample([ctx.t(x)], 16000, 16000)
    assert lens.tolist() == [5000]
    np.testing.assert_array_equal(bits(out.cpu().numpy()), bits(x))
    out, _ = ctx.features.resample([ctx.t(q)], 16000, 16000)
    np.testing.assert_array_equal(bits(out.cpu().numpy()), bits(q.astype(np.float32) / np.float32(32768)))
    for C in (2, 3):
        for make in (lambda s, n: FR.synthetic_audio(s, n, kind="noise"),
                     lambda s, n: FR.int16_quantised(FR.synthetic_audio(s, n, kind="noise"))):
            xs = [make(10 * C + i, n * C) for i, n in enumerate((1, 700, 4097))]
            out, lens = ctx.features.resample([ctx.t(v) for v in xs], 16000, 16000, channels=C)
            assert lens.tolist() == [1, 700, 4097]
            for y, v in zip(split(out, lens), xs):
                np.testing.assert_array_equal(bits(y), bits(R.downmix(v, C)))


# ---- 4. deterministic and batch-invariant ----
def deterministic(ctx, n_max=30000):
    F = ctx.features
    rs = np.random.RandomState(5)
    for rate in (48000, 44100, 8000):
        xs = [ctx.t(FR.synthetic_audio(300 + i, int(rs.randint(1, n_max)), rate, ("noise", "ar")[i % 2]))
              for i in range(20)]
        a, lens = F.resample(xs, rate)
        b, _ = F.resample(xs, rate)
        assert torch.equal(a, b)
        off = np.concatenate([[0], np.cumsum(lens)])
        for u in (0, 7, 19):
            alone, n1 = F.resample([xs[u]], rate)
            assert n1.tolist() == [lens[u]]
            assert torch.equal(alone, a[off[u]:off[u + 1]]), (rate, u)
        packed, lens2 = F.resample(torch.cat(xs), rate, lengths=[len(x) for x in xs])
        assert torch.equal(packed, a) and lens2.tolist() == lens.tolist()


# ---- 5. zero padding ----
def zero_padding(ctx):
    """An impulse at the first and at the last sample reproduces a column of the table; loud neighbours on both sides
    would show through a halo that reads past the utterance."""
    for rate in (48000, 44100, 8000):
        L, M = R.ratio(rate, NEW_RATE)
        h = R.taps(L, M)
        H = 10 * max(L, M)
        n = 3 * M + 7
        loud = (0.9 * np.sign(np.random.RandomState(3).randn(40 * max(L, M)))).astype(np.float32)
        first, last = np.zeros(n, np.float32), np.zeros(n, np.float32)
        first[0] = last[-1] = 1.0
        out, lens = ctx.features.resample([ctx.t(v) for v in (loud, first, loud, last, loud)], rate)
        ys = split(out, lens)
        bound = R.apriori_bound(L, M, peak=1.0)
        for y, k in ((ys[1], 0), (ys[3], n - 1)):
            idx = H + np.arange(len(y)) * M - k * L
            col = np.where((idx >= 0) & (idx <= 2 * H), h[np.clip(idx, 0, 2 * H)], 0.0)
            assert np.abs(col).max() > 0.1                       # the column is not all zeros
            assert np.abs(y - col).max() <= bound, (rate, k)


# ---- 6. plumbing ----
def direct_log_mel(ctx, packed, lens):
    """features.log_mel_fbank(packed, lengths=lens) with its defaults as the entry points it is made of: the call chain
    before the resampler existed."""
    F = ctx.features
    eng = F._eng()
    cfg = F.FbankConfig()
    fl, fs, nfft, nfilt = cfg.frame_len, cfg.frame_step, cfg.nfft, cfg.nfilt
    lens = np.ascontiguousarray(lens, np.int64)
    n_utt = len(lens)
    counts = np.zeros(3, np.int64)
    eng.lib.call("ds_fbank_plan", lens.ctypes.data, n_utt, fl, fs, nfft, nfilt, None, counts.ctypes.data)
    n_frames, n_tiles, tile_rows = (int(v) for v in counts)
    table = np.zeros(3 * (n_utt + 1) + n_tiles, np.int64)
    eng.lib.call("ds_fbank_plan", lens.ctypes.data, n_utt, fl, fs, nfft, nfilt, table.ctypes.data, counts.ctypes.data)
    table_dev = torch.from_numpy(table).to(packed.device)
    basis, band, weights, wstride = F._device_tables(cfg, packed.device)
    out = torch.empty((n_frames, nfilt), dtype=torch.float32, device=packed.device)
    ws = torch.empty(int(eng.lib.raw("ds_fbank_workspace_bytes")(n_utt, n_tiles, nfilt)) // 8, dtype=torch.float64,
                     device=packed.device)
    stream = eng._stream(out)
    eng.lib.call("ds_fbank_logmel_f32", eng._p(packed), 0, eng._p(table_dev), n_utt, n_tiles, eng._p(basis), eng._p(band),
                 eng._p(weights), wstride, fl, fs, nfft, nfilt, 1, eng._p(out), eng._p(ws), stream)
    eng.lib.call("ds_fbank_normalize_f32", eng._p(out), eng._p(table_dev), n_utt, n_tiles, nfilt, tile_rows, 0, eng._p(ws),
                 stream)
    return out, table[n_utt + 1:2 * (n_utt + 1)].copy()


def plumbing(ctx):
    from deepspeaker_pytorch_amd import data
    F = ctx.features
    x48 = [ctx.t(FR.synthetic_audio(40 + i, n, 48000, "ar")) for i, n in enumerate((4800, 30000))]
    a, off = F.log_mel_fbank(x48, orig_rate=48000)
    packed, lens = F.resample(x48, 48000)
    b, off_b = F.log_mel_fbank(packed, lengths=lens)
    assert torch.equal(a, b) and off.tolist() == off_b.tolist() and a.shape[0] == off[-1]
    stereo = [ctx.t(FR.int16_quantised(FR.synthetic_audio(50 + i, 2 * n, 44100, "noise"))) for i, n in enumerate((4410, 9000))]
    store = data.FeatureStore.from_waveforms(stereo, orig_rate=44100, channels=2)
    packed, lens = F.resample(stereo, 44100, channels=2)
    assert lens.tolist() == [1600, -(-9000 * 160 // 441)]
    c, off_c = F.log_mel_fbank(packed, lengths=lens)
    assert torch.equal(store.features, c) and store.offsets.tolist() == off_c.tolist() and len(store) == 2
    # channels alone: the down-mix at the configuration's own rate
    d, _ = F.log_mel_fbank(stereo, channels=2)
    packed, lens = F.resample(stereo, 16000, channels=2)
    e, _ = F.log_mel_fbank(packed, lengths=lens)
    assert torch.equal(d, e)
    # without the new keywords: the entry points called directly, as before
    x16 = [FR.synthetic_audio(60 + i, n, kind="ar") for i, n in enumerate((401, 5000))]
    f, off_f = F.log_mel_fbank([ctx.t(v) for v in x16])
    g, off_g = direct_log_mel(ctx, ctx.t(np.concatenate(x16)), [401, 5000])
    assert torch.equal(f.view(torch.int32), g.view(torch.int32)) and off_f.tolist() == off_g.tolist()
    s = data.FeatureStore.from_waveforms([ctx.t(v) for v in x16])
    assert torch.equal(s.features.view(torch.int32), g.view(torch.int32))


# ---- 7. end to end against float64 ----
@functools.lru_cache(maxsize=None)
def e2e_case(rate, kind):
    L, M = R.ratio(rate, NEW_RATE)
    x = FR.synthetic_audio(900 + rate // 1000, rate, rate, kind)
    ref = FR.mk_mfb(R.resample(x, L, M).astype(np.float32))
    x.setflags(write=False)
    ref.setflags(write=False)
    return x, ref


def end_to_end(ctx, rate):
    worst = 0.0
    for kind in ("noise", "ar"):
        x, ref = e2e_case(rate, kind)
        out, off = ctx.features.log_mel_fbank([ctx.t(x)], orig_rate=rate)
        assert off.tolist() == [0, len(ref)]
        err = float(np.abs(out.cpu().numpy() - ref).max())
        print(f"resample + fbank {rate} -> {NEW_RATE} {kind}: max abs error {err:.3e} dB")
        worst = max(worst, err)
    assert worst <= E2E_TOL_DB, worst


# ---- 8. errors ----
def abi_errors(ctx):
    lib = ctx.lib
    counts = np.zeros(3, np.int64)
    plan = lambda lens, L, M, H: lib.raw("ds_resample_plan")(lens.ctypes.data, len(lens), L, M, H, None, counts.ctypes.data)
    one = np.array([100], np.int64)
    assert plan(np.array([100, 0], np.int64), 1, 3, 30) == -1                # a zero-length utterance
    assert plan(one, 16000, 16001, 160010) == -4                             # 16001 -> 16000: the table is over the limit
    assert plan(one, 0, 3, 30) == -4 and plan(one, 1, 0, 30) == -4
    assert lib.raw("ds_resample_plan")(None, 1, 1, 3, 30, None, counts.ctypes.data) == -3
    assert plan(one, 1, 3, 30) == 0 and counts.tolist()[:2] == [34, 1]
    for rate in (8000, 11025, 16000, 22050, 32000, 44100, 48000, 96000):     # the limit admits every common rate
        L, M = R.ratio(rate, NEW_RATE)
        assert plan(one, L, M, 10 * max(L, M)) == 0, rate
    # the table entry by entry: utterances of exactly one tile of outputs, one output more, and one output
    tile = tile_size(lib, 1, 3)
    lens = np.array([3 * tile, 3 * tile + 1, 1], np.int64)
    assert plan(lens, 1, 3, 30) == 0 and counts.tolist() == [2 * tile + 2, 4, tile]
    table = np.full(3 * 4 + 4, -7, np.int64)
    counts[:] = 0
    assert lib.raw("ds_resample_plan")(lens.ctypes.data, 3, 1, 3, 30, table.ctypes.data, counts.ctypes.data) == 0
    assert counts.tolist() == [2 * tile + 2, 4, tile]
    assert table.tolist() == [0, 3 * tile, 6 * tile + 1, 6 * tile + 2,  0, tile, 2 * tile + 1, 2 * tile + 2,
                              0, 1, 3, 4,  0, 1, 1, 2]
    # the launch entry validates before it touches anything: placeholders stand for the buffers
    launch = lib.raw("ds_resample_poly_f32")
    p = np.zeros(4, np.int64).ctypes.data
    assert launch(None, 0, 1, None, 1, 1, None, 1, 3, 30, None, None) == -3
    assert launch(p, 0, 0, p, 1, 1, p, 1, 3, 30, p, None) == -4              # channels = 0
    assert launch(p, 0, 9, p, 1, 1, p, 1, 3, 30, p, None) == -4              # channels = 9
    assert launch(p, 2, 1, p, 1, 1, p, 1, 3, 30, p, None) == -4              # neither f32 nor int16
    assert launch(p, 0, 1, p, 1, 1, p, 16000, 16001, 160010, p, None) == -4
    assert launch(p, 0, 1, p, 0, 1, p, 1, 3, 30, p, None) == -1


def python_errors(ctx):
    from deepspeaker_pytorch_amd._native import DeepSpeakerHipError
    F = ctx.features
    x = ctx.t(np.zeros(1000, np.float32))
    with pytest.raises(DeepSpeakerHipError, match="bad shape"):
        F.resample([x, ctx.t(np.zeros(0, np.float32))], 48000)
    for C in (0, 9):
        with pytest.raises(ValueError):
            F.resample([x], 48000, channels=C)
    with pytest.raises(ValueError):
        F.resample([ctx.t(np.zeros(1000, np.float64))], 48000)
    with pytest.raises(ValueError):
        F.resample(x, 48000, lengths=[400, 500])
    with pytest.raises(ValueError):
        F.resample(x, 48000, channels=3, lengths=[1000])                     # 1000 samples are not 1000 frames of 3
    with pytest.raises(DeepSpeakerHipError, match="unsupported|not supported"):
        F.resample([x], 16001, 16000)
    with pytest.raises(ValueError):
        F.log_mel_fbank([x], orig_rate=48000, channels=9)
