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

# End to end, waveforms -> resample -> log-mel features, against mk_mfb(float32(restatement resample)) in float64: max
# |feature difference| in dB over 1 s of "noise" and "ar".  The bar is the filterbank's (fbank_bodies): max(FLOOR_DB, 4 x
# the distance of the float32 chain mk_mfb_f32(resample_f32(x)) from that float64 chain), per case, and never above
# E2E_TOL_DB, the bar these cases had before (3 x the kernel's own measured 2.3e-4, which is why it is only a ceiling now).
E2E_TOL_DB = 7e-4
E2E_RATES = (48000, 44100, 8000)
E2E_22K = (44100, "22k")                         # one target that is not 16 kHz: 44100 -> 22050 under fbank_bodies.CONFS["22k"]
GUARD = 64                                       # fbank_bodies.GUARD (that module imports this one)


@dataclass(frozen=True)
class Geom:
    """One resampler configuration and the geometry it is in the table for, asserted from ds_resample_plan's tile and the
    restatement's tap count before anything is launched: `reduced` a tile of at most 2560 outputs (rs_geometry went below
    its first candidate), `ragged` a tile that is no multiple of the 512 threads (S = L * ceil(target / L) with L not a
    power of two: the last item of a thread's loop is partial), `up` one of the cases that are there for upsampling, `tile`
    / `T` / `TP` exact values."""
    orig_rate: int
    new_rate: int = 16000
    zeros: int = 10
    beta: float = 5.0
    channels: int = 1
    reduced: bool = False
    ragged: bool = False
    up: bool = False
    tile: int = 0
    T: int = 0
    TP: int = 0

    def ratio(self):
        return R.ratio(self.orig_rate, self.new_rate)

    def kw(self):
        return dict(new_rate=self.new_rate, zeros=self.zeros, beta=self.beta, channels=self.channels)


GEOMETRY = {
    "96k": Geom(96000, reduced=True, tile=2048, T=121),                                # target 512
    "192k": Geom(192000, reduced=True, tile=1024, T=241),                              # target 256
    "44k_to_8k": Geom(44100, 8000, reduced=True, ragged=True, tile=2240, T=111),       # L = 80 on a reduced tile
    "44k_zeros16": Geom(44100, zeros=16, reduced=True, tile=2560, T=89),               # reduced through the table: 85.5 KB
    "48k_zeros1": Geom(48000, zeros=1, tile=4096, T=7),                                # the span is all tile, a halo of 3
    "48k_zeros40": Geom(48000, zeros=40, beta=8.6, tile=4096, T=241),                  # T = 241 on a full tile
    "16k_to_44k": Geom(16000, 44100, ragged=True, up=True, tile=5292, T=21),           # upsampling, L = 441
    "16k_to_48k": Geom(16000, 48000, ragged=True, up=True, tile=4104, T=21),           # upsampling, L = 3
    "48k_to_44k": Geom(48000, 44100, ragged=True, tile=4116, T=22, TP=23),             # an even T padded to an odd TP
    "44k_to_22k": Geom(44100, 22050, tile=4096, T=41),                                 # L = 1, M = 2
    "44k_stereo": Geom(44100, channels=2, ragged=True, tile=4480, T=56),
    "8k_three": Geom(8000, channels=3, tile=4096, T=21),
}
DIRECT = ("48k", "96k", "16k_to_44k", "44k_stereo")                  # full tile, reduced, upsampling, multichannel
GEOMETRY_DIRECT = dict(GEOMETRY, **{"48k": Geom(48000, tile=4096, T=61)})


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
def value_batch(rate, tile, dtype, new_rate=NEW_RATE, zeros=10, beta=5.0, channels=1):
    """(signals, float64 references, peak): every edge length twice, once as "noise" and once as "ar".  With `channels`
    > 1 the signals are interleaved (n * channels samples of one seeded signal) and the reference resamples the stated
    float32 down-mix."""
    L, M = R.ratio(rate, new_rate)
    xs = []
    for i, n in enumerate(edge_lengths(L, M, tile, zeros)):
        for j, kind in enumerate(("noise", "ar")):
            x = FR.synthetic_audio(7000 + 10 * i + j, n * channels, rate, kind)
            xs.append(FR.int16_quantised(x) if dtype == "int16" else x)
    monos = [R.downmix(x, channels) for x in xs]
    refs = [R.resample(v, L, M, zeros, beta) for v in monos]
    peak = max(float(np.abs(v).max()) for v in monos)
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
def values(ctx, rate, dtype, new_rate=NEW_RATE, zeros=10, beta=5.0, channels=1):
    L, M = R.ratio(rate, new_rate)
    tile = tile_size(ctx.lib, L, M, zeros)
    xs, refs, peak = value_batch(rate, tile, dtype, new_rate, zeros, beta, channels)
    out, lens = ctx.features.resample([ctx.t(x) for x in xs], rate, new_rate, channels=channels, zeros=zeros, beta=beta)
    assert out.dtype == torch.float32 and out.dim() == 1 and lens.dtype == np.int64
    assert lens.tolist() == [-(-(len(x) // channels) * L // M) for x in xs] == [len(r) for r in refs]
    n_outs = set(lens.tolist())
    if L <= M:                                   # every output count is reachable when not upsampling
        assert {tile - 1, tile, tile + 1, 2 * tile + 1} <= n_outs
    else:                                        # a partial last tile behind a full one, and more than two tiles
        assert any(tile < n < 2 * tile for n in n_outs) and any(n > 2 * tile for n in n_outs)
    assert any(n < tile for n in n_outs) and any(n % tile for n in n_outs if n > tile)
    err = max(float(np.abs(y - r).max()) for y, r in zip(split(out, lens), refs))
    bound = R.apriori_bound(L, M, zeros, beta, peak)
    print(f"resample {rate} -> {new_rate} ({L}/{M}, zeros {zeros}, beta {beta}, channels {channels}, tile {tile}) {dtype}: "
          f"max abs error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)


def geometry(ctx, name, dtype):
    """One row of GEOMETRY: first that the planner still gives the case the geometry it is in the table for, then the
    values of every edge length under the a-priori bound"""
    g = GEOMETRY[name]
    L, M = g.ratio()
    tile, T = tile_size(ctx.lib, L, M, g.zeros), R.n_taps(L, M, g.zeros)
    assert tile == g.tile and T == g.T, (name, tile, T)
    if g.reduced:
        assert tile <= 2560, (name, tile)
    else:
        assert tile >= 4096, (name, tile)
    assert (tile % 512 != 0) == g.ragged, (name, tile)
    if g.up:                                     # the upsampling cases: a tile that is no multiple of 512
        assert L > M and tile % 512 != 0, (name, tile)
    if g.TP:
        assert T % 2 == 0 and ctx.features.polyphase_taps(ctx.features.resample_taps(L, M, g.zeros, g.beta), L).shape == (L, g.TP)
    values(ctx, g.orig_rate, dtype, **g.kw())


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
    # the three rates the case had, then a reduced tile (96 kHz) and upsampling by L = 441
    for rate, new_rate in ((48000, NEW_RATE), (44100, NEW_RATE), (8000, NEW_RATE), (96000, NEW_RATE), (16000, 44100)):
        xs = [ctx.t(FR.synthetic_audio(300 + i, int(rs.randint(1, n_max)), rate, ("noise", "ar")[i % 2]))
              for i in range(20)]
        a, lens = F.resample(xs, rate, new_rate)
        b, _ = F.resample(xs, rate, new_rate)
        assert torch.equal(a, b)
        off = np.concatenate([[0], np.cumsum(lens)])
        for u in (0, 7, 19):
            alone, n1 = F.resample([xs[u]], rate, new_rate)
            assert n1.tolist() == [lens[u]]
            assert torch.equal(alone, a[off[u]:off[u + 1]]), (rate, new_rate, u)
        packed, lens2 = F.resample(torch.cat(xs), rate, new_rate, lengths=[len(x) for x in xs])
        assert torch.equal(packed, a) and lens2.tolist() == lens.tolist()


# ---- 5. zero padding ----
def zero_padding(ctx):
    """An impulse at the first and at the last sample reproduces a column of the table; loud neighbours on both sides
    would show through a halo that reads past the utterance."""
    # the three rates the case had, then a reduced tile (96 kHz) and upsampling by L = 441
    for rate, new_rate in ((48000, NEW_RATE), (44100, NEW_RATE), (8000, NEW_RATE), (96000, NEW_RATE), (16000, 44100)):
        L, M = R.ratio(rate, new_rate)
        h = R.taps(L, M)
        H = 10 * max(L, M)
        n = 3 * M + 7
        loud = (0.9 * np.sign(np.random.RandomState(3).randn(40 * max(L, M)))).astype(np.float32)
        first, last = np.zeros(n, np.float32), np.zeros(n, np.float32)
        first[0] = last[-1] = 1.0
        out, lens = ctx.features.resample([ctx.t(v) for v in (loud, first, loud, last, loud)], rate, new_rate)
        ys = split(out, lens)
        bound = R.apriori_bound(L, M, peak=1.0)
        for y, k in ((ys[1], 0), (ys[3], n - 1)):
            idx = H + np.arange(len(y)) * M - k * L
            col = np.where((idx >= 0) & (idx <= 2 * H), h[np.clip(idx, 0, 2 * H)], 0.0)
            assert np.abs(col).max() > 0.1                       # the column is not all zeros
            assert np.abs(y - col).max() <= bound, (rate, new_rate, k)


# ---- 5a. the entry points on guarded buffers ----
class Direct:
    """ds_resample_plan / ds_resample_poly_f32 called as features.resample calls them, on buffers that show a read or a
    store outside them: the packed input lies between GUARD NaNs (int16: -32768s) inside a larger tensor, the output is
    NaN-filled between GUARD NaNs that must survive."""

    def __init__(self, ctx, g, xs):
        self.ctx, self.g, self.F = ctx, g, ctx.features
        self.eng = self.F._eng()
        self.L, self.M = g.ratio()
        self.half = g.zeros * max(self.L, self.M)
        dt = xs[0].dtype
        assert all(x.dtype == dt for x in xs)
        self.int16 = dt == np.int16
        self.lens = np.array([len(x) // g.channels for x in xs], np.int64)
        self.n_utt = len(xs)
        plan = ctx.lib.raw("ds_resample_plan")
        counts = np.zeros(3, np.int64)
        assert plan(self.lens.ctypes.data, self.n_utt, self.L, self.M, self.half, None, counts.ctypes.data) == 0
        self.n_out, self.n_tiles, self.tile = (int(v) for v in counts)
        table = np.full(3 * (self.n_utt + 1) + self.n_tiles, -7, np.int64)
        assert plan(self.lens.ctypes.data, self.n_utt, self.L, self.M, self.half, table.ctypes.data, counts.ctypes.data) == 0
        assert counts.tolist() == [self.n_out, self.n_tiles, self.tile] and (table != -7).all()
        self.out_lens = np.diff(table[self.n_utt + 1:2 * (self.n_utt + 1)])
        assert self.out_lens.tolist() == [R.n_out(n, self.L, self.M) for n in self.lens]
        assert self.n_tiles == int((-(-self.out_lens // self.tile)).sum())
        self.table = ctx.t(table)
        guard = np.full(GUARD, -32768, np.int16) if self.int16 else np.full(GUARD, np.nan, np.float32)
        self.samples = ctx.t(np.concatenate([guard] + list(xs) + [guard]))
        self.taps = self.F._device_taps(self.L, self.M, g.zeros, g.beta, self.samples.device)

    def run(self):
        eng, g = self.eng, self.g
        out = torch.full((self.n_out + 2 * GUARD,), float("nan"), dtype=torch.float32, device=self.ctx.dev)
        eng.lib.call("ds_resample_poly_f32", eng._p(self.samples[GUARD:]), int(self.int16), g.channels, eng._p(self.table),
                     self.n_utt, self.n_tiles, eng._p(self.taps), self.L, self.M, self.half, eng._p(out[GUARD:]),
                     eng._stream(out))
        a = out.cpu().numpy()
        assert np.isnan(a[:GUARD]).all(), "a store before the first output"
        assert np.isnan(a[GUARD + self.n_out:]).all(), "a store past the last output"
        got = a[GUARD:GUARD + self.n_out]
        assert not np.isnan(got).any(), "an output was not written, or a sample outside the input was read"
        return got.copy()


def direct(ctx, name, dtype):
    """the values batch of one case through the guarded entry points: no store outside the outputs, no NaN inside, under
    the a-priori bound (which a -32768 read from an int16 guard would break), and features.resample's bits"""
    g = GEOMETRY_DIRECT[name]
    L, M = g.ratio()
    tile = tile_size(ctx.lib, L, M, g.zeros)
    assert tile == g.tile
    xs, refs, peak = value_batch(g.orig_rate, tile, dtype, g.new_rate, g.zeros, g.beta, g.channels)
    d = Direct(ctx, g, xs)
    got = d.run()
    off = np.concatenate([[0], np.cumsum(d.out_lens)])
    err = max(float(np.abs(got[off[u]:off[u + 1]] - r).max()) for u, r in enumerate(refs))
    bound = R.apriori_bound(L, M, g.zeros, g.beta, peak)
    print(f"resample direct {name} {dtype}: {d.n_tiles} tiles of {d.tile}, max abs error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)
    api, lens = ctx.features.resample([ctx.t(x) for x in xs], g.orig_rate, **g.kw())
    assert lens.tolist() == d.out_lens.tolist()
    np.testing.assert_array_equal(bits(api.cpu().numpy()), bits(got))


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
def e2e_case(rate, kind, conf="16k"):
    """(1 s of signal, the float64 chain's features, the distance of the float32 chain from them in dB)"""
    import fbank_bodies as FB                                        # (imports this module: not at the top)
    c = FB.CONFS[conf]
    L, M = R.ratio(rate, c.sample_rate)
    x = FR.synthetic_audio(900 + rate // 1000, rate, rate, kind)
    ref = FR.mk_mfb(R.resample(x, L, M).astype(np.float32), **c.ref_kw())
    restated = float(np.abs(FR.mk_mfb_f32(R.resample_f32(x, L, M), **c.ref_kw()).astype(np.float64) - ref).max())
    assert np.abs(ref).max() < 128.0                                 # FLOOR_DB is one unit in the last place there
    x.setflags(write=False)
    ref.setflags(write=False)
    return x, ref, restated


def end_to_end(ctx, rate, conf="16k"):
    import fbank_bodies as FB
    c = FB.CONFS[conf]
    worst = 0.0
    for kind in ("noise", "ar"):
        x, ref, restated = e2e_case(rate, kind, conf)
        out, off = ctx.features.log_mel_fbank([ctx.t(x)], c.config(ctx.features), orig_rate=rate)
        assert off.tolist() == [0, len(ref)] and out.shape[1] == c.nfilt
        err = float(np.abs(out.cpu().numpy() - ref).max())
        bar = min(max(FB.FLOOR_DB, 4.0 * restated), E2E_TOL_DB)
        print(f"resample + fbank {rate} -> {c.sample_rate} {kind}: f32-restated {restated:.2e} bar {bar:.2e} "
              f"({'restatement' if bar < E2E_TOL_DB else 'ceiling'}) kernel {err:.2e} dB")
        assert err <= bar, (rate, conf, kind, err, bar)
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
