"""TEST INFRASTRUCTURE: the filterbank front end's cases (csrc/fbank.hip, features.log_mel_fbank), written once and run by
tests/test_emul_fbank.py through the host emulator and by tests/test_gpu_fbank.py on the device.  Every body takes a
`Ctx` (resample_bodies.Ctx: the features module to call, the device the tensors live on, the loaded library).

Two kinds of bar:
  * TOL_DB, the suite's first bar, on the cases both files had before they shared this one;
  * for the configuration table below, loss_side_cases.bar_from_restatement: max(floor, 4 x the distance of the float32
    restatement fbank_reference.mk_mfb_f32 from the float64 restatement fbank_reference.mk_mfb), never the kernel's own
    output.  Floors: 1e-6 (loss_side_cases.FLOOR) for the raw filterbank (per frame, relative to the frame's largest
    value) and for "mean_std" (normalised units); 2^-17 dB for the log features, one unit in the last place of a
    float32 below 128, which the body asserts of the reference.
References are computed once per process and are read-only."""
import functools
from dataclasses import dataclass

import numpy as np
import pytest
import torch

import fbank_reference as R
from loss_side_bodies import say
from loss_side_cases import FLOOR, bar_from_restatement
from resample_bodies import Ctx  # noqa: F401  (the one definition; the backends' files build it)

TOL_DB = 5e-4
FLOOR_DB = 2.0 ** -17
GUARD = 64
DTYPES = ("float32", "int16")
LDS_MAX = 160 * 1024


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------
def as_float(x):
    return x.astype(np.float32) / np.float32(32768) if x.dtype == np.int16 else x


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def plan_counts(lib, lens, fl, fs, nfft, nfilt, table=None):
    """(return code, [frames, tiles, rows per tile]) of ds_fbank_plan"""
    lens = np.ascontiguousarray(lens, np.int64)
    counts = np.zeros(3, np.int64)
    rc = lib.raw("ds_fbank_plan")(lens.ctypes.data, len(lens), fl, fs, nfft, nfilt,
                                  None if table is None else table.ctypes.data, counts.ctypes.data)
    return rc, counts.tolist()


def lds_bytes(tm, fl, fs, nfft, nfilt):
    """One tile's LDS, restated from the kernel's layout: the statistics' partial sums [2][4][nfilt] f64, the power
    spectrum [tm][nfft/2+1] f32, and the tile's samples, (tm - 1) steps and one frame rounded up to even, as whole
    16-byte vectors."""
    span = (tm - 1) * fs + fl + (fl & 1)
    return 2 * 4 * nfilt * 8 + tm * (nfft // 2 + 1) * 4 + -(-span // 4) * 16


def restated_tile(fl, fs, nfft, nfilt):
    for tm in (64, 32):
        if lds_bytes(tm, fl, fs, nfft, nfilt) <= LDS_MAX:
            return tm
    raise AssertionError("no tile fits")


# ---------------------------------------------------------------------------------------------------------------------
# 1. the cases the two files had before: TOL_DB against the float64 restatement
# ---------------------------------------------------------------------------------------------------------------------
def restatement(ctx, xs, sr, normalize):
    """float32 and int16 signals (one call per sample type) against mk_mfb: dtype, shape, frame offsets, values"""
    F = ctx.features
    fl, fs = R.frame_params(sr)
    worst = 0.0
    for dt in (np.float32, np.int16):
        group = [x for x in xs if x.dtype == dt]
        if not group:
            continue
        out, off = F.log_mel_fbank([ctx.t(x) for x in group], F.FbankConfig(sample_rate=sr), normalize=normalize)
        out = out.cpu().numpy()
        assert out.dtype == np.float32 and out.shape[1] == 64
        assert off.tolist() == np.concatenate([[0], np.cumsum([R.n_frames(len(x), fl, fs) for x in group])]).tolist()
        for u, x in enumerate(group):
            ref = R.mk_mfb(as_float(x), sample_rate=sr, normalize=normalize)
            err = float(np.abs(out[off[u]:off[u + 1]] - ref).max())
            assert err <= TOL_DB, (str(dt), u, err)
            worst = max(worst, err)
    print(f"fbank sr={sr} normalize={normalize}: max abs error {worst:.3e}")


def int16_is_scaled_float(ctx, qs, normalize, values):
    """`values`: also against mk_mfb under TOL_DB (a bar measured on the signals of `restatement`, which holds the
    int16 values of the device's signal set)"""
    F = ctx.features
    a, off = F.log_mel_fbank([ctx.t(q) for q in qs], normalize=normalize)
    b, _ = F.log_mel_fbank([ctx.t(as_float(q)) for q in qs], normalize=normalize)
    np.testing.assert_array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy()))
    a = a.cpu().numpy()
    for u, q in enumerate(qs if values else ()):
        assert np.abs(a[off[u]:off[u + 1]] - R.mk_mfb(as_float(q), normalize=normalize)).max() <= TOL_DB


def packed_input_and_feature_store(ctx):
    from deepspeaker_pytorch_amd import data
    F = ctx.features
    xs = [R.synthetic_audio(30 + i, n, kind="noise") for i, n in enumerate((900, 2000))]
    a, off = F.log_mel_fbank(ctx.t(np.concatenate(xs)), lengths=[900, 2000])
    b, _ = F.log_mel_fbank([ctx.t(x) for x in xs])
    assert torch.equal(a, b)
    fs = data.FeatureStore.from_waveforms([ctx.t(x) for x in xs])
    assert len(fs) == 2 and fs.n_feat == 64 and fs.offsets.tolist() == off.tolist()
    assert torch.equal(fs.features, a)
    crop = fs.crops([1], [3], 8).cpu().numpy()
    np.testing.assert_array_equal(crop[0, 0], a.cpu().numpy()[off[1] + 3:off[1] + 11])


def raw_filterbank(ctx, seed, n, kind, rtol, atol):
    F = ctx.features
    x = R.synthetic_audio(seed, n, kind=kind)
    out, _ = F.log_mel_fbank([ctx.t(x)], F.FbankConfig(use_logscale=False), normalize=None)
    ref = R.mk_mfb(x, normalize=None, use_logscale=False)
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=rtol, atol=atol)


def abi_errors(ctx):
    lib = ctx.lib
    plan = lambda lens, fl, fs, nfft, nfilt: plan_counts(lib, lens, fl, fs, nfft, nfilt)
    assert plan([400, 0], 400, 160, 512, 64)[0] == -1                              # empty signal
    assert plan([400], 600, 240, 512, 64)[0] == -4                                 # frame_len > nfft
    assert plan([400], 400, 160, 512, 62)[0] == -4                                 # nfilt % 4 != 0
    assert plan([400], 400, 160, 500, 64)[0] == -4                                 # nfft not a power of two
    assert plan([400], 400, 160, 512, 64) == (0, [1, 1, 64])
    assert plan([160 * 48000 + 1], 400, 160, 512, 64) == (0, [R.n_frames(160 * 48000 + 1, 400, 160), 750, 64])  # 8 minutes
    assert lib.raw("ds_fbank_logmel_f32")(None, 0, None, 1, 1, None, None, None, 1, 400, 160, 512, 64, 1, None, None,
                                          None) == -3


def plan_table(ctx):
    """ds_fbank_plan's table entry by entry: utterances of exactly one tile of frames, one frame more, and one frame."""
    lib = ctx.lib
    fl, fs = 400, 160
    rc, counts = plan_counts(lib, [1], fl, fs, 512, 64)
    assert rc == 0
    tm = counts[2]
    a, b = fl + (tm - 1) * fs, fl + tm * fs                       # tm and tm + 1 frames (framesig)
    assert plan_counts(lib, [a, b, 1], fl, fs, 512, 64) == (0, [2 * tm + 2, 4, tm])
    table = np.full(3 * 4 + 4, -7, np.int64)
    assert plan_counts(lib, [a, b, 1], fl, fs, 512, 64, table) == (0, [2 * tm + 2, 4, tm])
    assert table.tolist() == [0, a, a + b, a + b + 1,  0, tm, 2 * tm + 1, 2 * tm + 2,  0, 1, 3, 4,  0, 1, 1, 2]


def python_errors(ctx):
    from deepspeaker_pytorch_amd._native import DeepSpeakerHipError
    F = ctx.features
    z = lambda n, dtype=np.float32: ctx.t(np.zeros(n, dtype))
    with pytest.raises(DeepSpeakerHipError, match="bad shape"):
        F.log_mel_fbank([z(400), z(0)])
    with pytest.raises(DeepSpeakerHipError, match="bad shape"):
        F.log_mel_fbank([z(1000), z(0)])
    with pytest.raises(DeepSpeakerHipError):
        F.log_mel_fbank([z(400)], F.FbankConfig(sample_rate=24000))               # frame_len 600 > nfft 512
    with pytest.raises(DeepSpeakerHipError):
        F.log_mel_fbank([z(1000)], F.FbankConfig(sample_rate=24000))
    for nfilt in (30, 66):
        with pytest.raises(DeepSpeakerHipError):
            F.log_mel_fbank([z(400)], F.FbankConfig(nfilt=nfilt))
    with pytest.raises(ValueError):
        F.log_mel_fbank([z(400)], normalize="std")
    with pytest.raises(ValueError):
        F.log_mel_fbank([z(400, np.float64)])


def other_configurations(ctx, sr, nfft, nfilt):
    """Other sample rates, FFT sizes and filter counts; nfft 1024 takes 32-frame tiles (the 64-frame tile's samples and
    power spectrum do not fit the LDS together)."""
    F = ctx.features
    cfg = F.FbankConfig(sample_rate=sr, nfft=nfft, nfilt=nfilt)
    n = 70 * cfg.frame_step + cfg.frame_len                         # more than one tile of either size
    xs = [R.synthetic_audio(50, n, sr, "ar"), R.synthetic_audio(51, n // 3, sr, "noise")]
    rc, counts = plan_counts(ctx.lib, [len(x) for x in xs], cfg.frame_len, cfg.frame_step, nfft, nfilt)
    assert rc == 0 and counts[2] == (32 if nfft == 1024 else 64)
    out, off = F.log_mel_fbank([ctx.t(x) for x in xs], cfg, normalize="mean")
    out = out.cpu().numpy()
    for u, x in enumerate(xs):
        ref = R.mk_mfb(x, sample_rate=sr, nfilt=nfilt, nfft=nfft, normalize="mean")
        assert np.abs(out[off[u]:off[u + 1]] - ref).max() <= TOL_DB


def preemphasis_bits(ctx, seed, n):
    eng = ctx.features._eng()
    x = R.synthetic_audio(seed, n, kind="ar")
    for src in (x, R.int16_quantised(x)):
        d = ctx.t(src)
        y = torch.zeros(len(src), dtype=torch.float32, device=ctx.dev)
        eng.lib.call("ds_fbank_preemphasis_f32", eng._p(d), 1 if src.dtype == np.int16 else 0, len(src), eng._p(y),
                     eng._stream(y))
        np.testing.assert_array_equal(bits(y.cpu().numpy()), bits(R.preemphasis(as_float(src))))


def deterministic(ctx, n_utt, n_max, picks):
    F = ctx.features
    rs = np.random.RandomState(11)
    kinds = ("noise", "ar", "chirp", "tone")
    xs = [ctx.t(R.synthetic_audio(1000 + i, int(rs.randint(1, n_max)), kind=kinds[i % 4])) for i in range(n_utt)]
    for normalize in ("mean", "mean_std", None):
        a, off = F.log_mel_fbank(xs, normalize=normalize)
        b, _ = F.log_mel_fbank(xs, normalize=normalize)
        assert torch.equal(a, b)
        for u in picks:
            alone, _ = F.log_mel_fbank([xs[u]], normalize=normalize)
            assert torch.equal(alone, a[off[u]:off[u + 1]]), (normalize, u)
        packed, off2 = F.log_mel_fbank(torch.cat(xs), lengths=[len(x) for x in xs], normalize=normalize)
        assert torch.equal(packed, a) and off2.tolist() == off.tolist()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the configuration table: every instantiation, odd frames, gaps, the statistics' groups, filters without a bin
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Conf:
    sample_rate: int
    winlen: float
    winstep: float
    nfft: int
    nfilt: int
    frame_len: int
    frame_step: int
    tile: int
    long: bool = False                   # also one utterance of 70 tiles and 3 frames: the small configurations

    def config(self, F, use_logscale=True):
        return F.FbankConfig(sample_rate=self.sample_rate, nfilt=self.nfilt, nfft=self.nfft, winlen=self.winlen,
                             winstep=self.winstep, use_logscale=use_logscale)

    def ref_kw(self):
        return dict(sample_rate=self.sample_rate, nfilt=self.nfilt, nfft=self.nfft, winlen=self.winlen,
                    winstep=self.winstep)


CONFS = {
    "16k": Conf(16000, 0.025, 0.01, 512, 64, 400, 160, 64),                        # baseline
    "16k_odd_len": Conf(16000, 401 / 16000, 0.01, 512, 64, 401, 160, 64),          # odd frame_len on MB = 2
    "22k": Conf(22050, 0.025, 0.01, 1024, 64, 551, 221, 32),                       # odd length and step, MB = 1
    "16k_gaps": Conf(16000, 0.025, 0.03, 512, 64, 400, 480, 32),                   # gaps; MB = 1 through the sample span
    "8k_abutting": Conf(8000, 0.025, 0.025, 256, 64, 200, 200, 64, True),          # frames that do not overlap
    "32k_128": Conf(32000, 0.025, 0.01, 1024, 128, 800, 320, 32),                  # G = 2
    "2k_12": Conf(2000, 0.025, 0.01, 64, 12, 50, 20, 64, True),                    # G = 21, 4 idle threads; one column pair
    "2k_4": Conf(2000, 0.025, 0.01, 64, 4, 50, 20, 64, True),                      # G = 64
    "2k_64": Conf(2000, 0.025, 0.01, 64, 64, 50, 20, 64, True),                    # filters without a bin
    "16k_step1": Conf(16000, 0.025, 1 / 16000, 512, 64, 400, 1, 64),               # step 1
}
MODES = ("raw", "log", "mean", "mean_std")
LAUNCHED = set()                                   # (sample type, MB) pairs this process has launched
INSTANTIATIONS = {("float", 1), ("float", 2), ("short", 1), ("short", 2)}


def frame_rel(got, ref):
    """max over frames of max |got - ref| / max |ref| within the frame"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref).max(1) / np.abs(ref).max(1)).max())


def abs_max(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max())


METRIC = {"raw": (frame_rel, FLOOR), "log": (abs_max, FLOOR_DB), "mean": (abs_max, FLOOR_DB), "mean_std": (abs_max, FLOOR)}


def lengths_of(c):
    """[(samples, frames)]: one tile, one frame more, 2 tiles + 3 frames and a started step, one sample, one sample short
    of a frame; in the small configurations 70 tiles + 3 frames"""
    tm, fl, fs = c.tile, c.frame_len, c.frame_step
    ns = [fl + (tm - 1) * fs, fl + tm * fs, fl + (2 * tm + 2) * fs + 1, 1, fl - 1]
    if c.long:
        ns.append(fl + (70 * tm + 2) * fs)
    want = [tm, tm + 1, 2 * tm + 4, 1, 1] + [70 * tm + 3] * c.long
    assert [R.n_frames(n, fl, fs) for n in ns] == want
    return list(zip(ns, want))


STEPPED = 2                                        # the utterance of a batch that is `level_steps`, the rest are "ar"


def references(x, c):
    """({mode: float64 reference}, {mode: float32 restatement}) of one float32 signal"""
    kw = c.ref_kw()
    r64, r32 = {}, {}
    for mode in MODES:
        args = dict(kw, normalize=None if mode in ("raw", "log") else mode, use_logscale=mode != "raw")
        r64[mode], r32[mode] = R.mk_mfb(x, **args), R.mk_mfb_f32(x, **args)
        r64[mode].setflags(write=False)
        r32[mode].setflags(write=False)
    return r64, r32


@functools.lru_cache(maxsize=None)
def value_batch(name, dtype):
    """(signals, [per utterance {mode: float64}], [per utterance {mode: float32 restatement}])"""
    c = CONFS[name]
    xs = []
    for i, (n, _) in enumerate(lengths_of(c)):
        seed = 100 * sorted(CONFS).index(name) + i
        x = R.level_steps(seed, n, c.frame_step) if i == STEPPED else R.synthetic_audio(seed, n, c.sample_rate, "ar")
        xs.append(R.int16_quantised(x) if dtype == "int16" else x)
    refs = [references(as_float(x), c) for x in xs]
    for x in xs:
        x.setflags(write=False)
    return xs, [r[0] for r in refs], [r[1] for r in refs]


class Direct:
    """The entry points features.log_mel_fbank is made of, on guarded buffers: the samples end in GUARD NaNs (int16: in
    -32768s), the features and the workspace are NaN-filled and end in GUARD more NaNs that must survive."""

    def __init__(self, ctx, c, xs):
        self.ctx, self.c, self.F = ctx, c, ctx.features
        self.eng = self.F._eng()
        self.cfg = c.config(self.F)
        assert (self.cfg.frame_len, self.cfg.frame_step) == (c.frame_len, c.frame_step)
        self.args = (c.frame_len, c.frame_step, c.nfft, c.nfilt)
        self.lens = np.array([len(x) for x in xs], np.int64)
        self.n_utt = len(xs)
        rc, counts = plan_counts(ctx.lib, self.lens, *self.args)
        assert rc == 0
        self.n_frames, self.n_tiles, self.tile = counts
        # the tile the planner reports, the LDS arithmetic restated here and the table of cases agree
        assert self.tile == restated_tile(*self.args) == c.tile, (self.tile, restated_tile(*self.args), c.tile)
        table = np.full(3 * (self.n_utt + 1) + self.n_tiles, -7, np.int64)
        assert plan_counts(ctx.lib, self.lens, *self.args, table) == (0, counts)
        self.offsets = table[self.n_utt + 1:2 * (self.n_utt + 1)].copy()
        assert self.offsets.tolist() == np.concatenate(
            [[0], np.cumsum([R.n_frames(n, c.frame_len, c.frame_step) for n in self.lens])]).tolist()
        assert table[2 * (self.n_utt + 1):3 * (self.n_utt + 1)].tolist() == np.concatenate(
            [[0], np.cumsum(-(-np.diff(self.offsets) // self.tile))]).tolist()
        self.table = ctx.t(table)
        dt = xs[0].dtype
        assert all(x.dtype == dt for x in xs)
        self.int16 = dt == np.int16
        tail = np.full(GUARD, -32768, np.int16) if self.int16 else np.full(GUARD, np.nan, np.float32)
        self.samples = ctx.t(np.concatenate(list(xs) + [tail]))
        self.basis, self.band, self.weights, self.wstride = self.F._device_tables(self.cfg, self.samples.device)
        self.ws_len = int(ctx.lib.raw("ds_fbank_workspace_bytes")(self.n_utt, self.n_tiles, c.nfilt)) // 8
        assert self.ws_len == 2 * c.nfilt * (self.n_tiles + self.n_utt)

    def _nan(self, n, dtype):
        return torch.full((n + GUARD,), float("nan"), dtype=dtype, device=self.ctx.dev)

    def _read(self, buf, n, what):
        a = buf.cpu().numpy()
        assert np.isnan(a[n:]).all(), f"{what}: guard tail overwritten"
        return a[:n]

    def logmel(self, log_scale):
        """(features [n_frames, nfilt] on the host, the two device buffers)"""
        eng, c = self.eng, self.c
        out, ws = self._nan(self.n_frames * c.nfilt, torch.float32), self._nan(self.ws_len, torch.float64)
        eng.lib.call("ds_fbank_logmel_f32", eng._p(self.samples), int(self.int16), eng._p(self.table), self.n_utt,
                     self.n_tiles, eng._p(self.basis), eng._p(self.band), eng._p(self.weights), self.wstride, *self.args,
                     int(log_scale), eng._p(out), eng._p(ws), eng._stream(out))
        LAUNCHED.add(("short" if self.int16 else "float", self.tile // 32))
        got = self._read(out, self.n_frames * c.nfilt, "features")
        assert not np.isnan(got).any(), "a feature was not written"
        part = self._read(ws, self.ws_len, "workspace")
        assert not np.isnan(part[:2 * c.nfilt * self.n_tiles]).any(), "a tile's statistics were not written"
        return got.reshape(self.n_frames, c.nfilt).copy(), out, ws

    def normalize(self, out, ws, use_scale):
        """on copies of logmel's buffers, so that one launch of the filterbank serves both normalisations"""
        eng, c = self.eng, self.c
        out, ws = out.clone(), ws.clone()
        eng.lib.call("ds_fbank_normalize_f32", eng._p(out), eng._p(self.table), self.n_utt, self.n_tiles, c.nfilt,
                     self.tile, int(use_scale), eng._p(ws), eng._stream(out))
        got = self._read(out, self.n_frames * c.nfilt, "normalised features")
        assert not np.isnan(self._read(ws, self.ws_len, "workspace")).any(), "an utterance's statistics were not written"
        assert not np.isnan(got).any()
        return got.reshape(self.n_frames, c.nfilt).copy()

    def all_modes(self):
        raw, _, _ = self.logmel(False)
        log, out, ws = self.logmel(True)
        return {"raw": raw, "log": log, "mean": self.normalize(out, ws, 0), "mean_std": self.normalize(out, ws, 1)}

    def split(self, a):
        return [a[self.offsets[u]:self.offsets[u + 1]] for u in range(self.n_utt)]


def empty_filters(c):
    return np.nonzero(R.filterbank(c.nfilt, c.nfft, c.sample_rate).sum(1) == 0)[0]


def configuration(ctx, name, dtype):
    """One batch of the table's lengths in one sample type, in every mode, against float64 under the restated bars"""
    c = CONFS[name]
    xs, r64, r32 = value_batch(name, dtype)
    d = Direct(ctx, c, xs)
    got = d.all_modes()
    for mode in MODES:
        metric, floor = METRIC[mode]
        for r in r64:
            assert r[mode].shape[1] == c.nfilt
            if mode in ("log", "mean"):
                assert np.abs(r[mode]).max() < 128.0           # FLOOR_DB is one unit in the last place there
        outs = d.split(got[mode])
        assert [len(o) for o in outs] == [len(r[mode]) for r in r64]
        restated = max(metric(a[mode], b[mode]) for a, b in zip(r32, r64))
        errs = [metric(o, r[mode]) for o, r in zip(outs, r64)]
        bar = bar_from_restatement(floor, restated)
        say(f"fbank {name} {c.frame_len}/{c.frame_step} nfft {c.nfft} nfilt {c.nfilt} tile {d.tile} {dtype}", mode,
            restated, bar, max(errs))
        assert max(errs) <= bar, (name, dtype, mode, errs, bar)
    # the public call is these entry points: the same bits, the same offsets
    api, off = ctx.features.log_mel_fbank([ctx.t(x) for x in xs], d.cfg, normalize="mean_std")
    assert off.tolist() == d.offsets.tolist()
    np.testing.assert_array_equal(bits(api.cpu().numpy()), bits(got["mean_std"]))
    # a filter without a bin: eps in the raw filterbank, the floor of the log, nothing after the mean is removed
    dead = empty_filters(c)
    assert len(dead) > 0 or name != "2k_64"                  # (8 kHz / 256 / 64 and 32 kHz / 1024 / 128 have some too)
    if len(dead):
        assert (got["raw"][:, dead] == np.float32(np.finfo(float).eps)).all()
        assert (got["log"][:, dead] == -100.0).all()
        assert (got["mean"][:, dead] == 0.0).all() and (got["mean_std"][:, dead] == 0.0).all()


def loud_successor(ctx, name, dtype):
    """An utterance whose last tile is part full and whose last step is only started, followed by one 1e6 times louder
    (float32) or at full scale against a few units (int16): the same bits as alone, so no frame read the successor."""
    c = CONFS[name]
    n = c.frame_len + (c.tile + 2) * c.frame_step + 1
    quiet = 1e-4 * R.synthetic_audio(7, n, c.sample_rate, "noise")           # 0.1 * randn: |quiet| about 1e-5
    loud = 1e6 * quiet[:c.frame_len + 2 * c.frame_step][::-1]
    if dtype == "int16":
        quiet, loud = np.round(quiet * 3e5).astype(np.int16), np.round(loud / np.abs(loud).max() * 32767).astype(np.int16)
        assert 1 <= np.abs(quiet).max() <= 30
    else:
        quiet, loud = quiet.astype(np.float32), loud.astype(np.float32)
    alone = Direct(ctx, c, [quiet]).logmel(False)[0]
    both = Direct(ctx, c, [quiet, loud])
    got = both.split(both.logmel(False)[0])
    np.testing.assert_array_equal(bits(got[0]), bits(alone))
    ref = R.mk_mfb(as_float(quiet), normalize=None, use_logscale=False, **c.ref_kw())
    r32 = R.mk_mfb_f32(as_float(quiet), normalize=None, use_logscale=False, **c.ref_kw())
    restated, err = frame_rel(r32, ref), frame_rel(got[0], ref)
    bar = bar_from_restatement(FLOOR, restated)
    say(f"fbank {name} {dtype} before a loud successor", "raw", restated, bar, err)
    assert err <= bar, (name, dtype, err, bar)
    assert got[1].max() > 1e6 * got[0].max()


def statistics_alone_and_last_of_five(ctx, name, dtype):
    """The long utterance (more tiles than the statistics kernel has groups, and no multiple of them) gives the same bits
    alone and as the last of a batch of five whose others have fewer tiles than groups"""
    c = CONFS[name]
    assert c.long
    xs, _, _ = value_batch(name, dtype)
    G = 256 // c.nfilt
    tiles = [-(-f // c.tile) for _, f in lengths_of(c)]
    assert tiles[-1] > G and tiles[-1] % G and all(t < G for t in tiles[:-1])
    five = [xs[0], xs[1], xs[3], xs[4], xs[5]]
    alone, batch = Direct(ctx, c, [xs[5]]), Direct(ctx, c, five)
    _, out_a, ws_a = alone.logmel(True)
    _, out_b, ws_b = batch.logmel(True)
    for use_scale in (0, 1):
        a = alone.normalize(out_a, ws_a, use_scale)
        b = batch.split(batch.normalize(out_b, ws_b, use_scale))[-1]
        np.testing.assert_array_equal(bits(a), bits(b))


def coverage(ctx):
    """every instantiation of fbank_logmel_kernel was launched by this process; one that was not is launched here"""
    for inst in sorted(INSTANTIATIONS - LAUNCHED):
        configuration(ctx, "16k" if inst[1] == 2 else "22k", "float32" if inst[0] == "float" else "int16")
    for inst in sorted(LAUNCHED):
        print("launched: fbank_logmel_kernel<%s, %d>" % inst)
    assert INSTANTIATIONS <= LAUNCHED, INSTANTIATIONS - LAUNCHED
