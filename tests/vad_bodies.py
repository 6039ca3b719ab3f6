"""TEST INFRASTRUCTURE: the cases of the energy voice-activity decision and the selection of voiced frames (csrc/vad.hip,
features.frame_log_energy / voiced_frames / select_frames, the vad= keyword of log_mel_fbank and
FeatureStore.from_waveforms), written once and run by tests/test_emul_vad.py through the host emulator and by
tests/test_gpu_vad.py on the device.  Every body takes a `Ctx`: the features module to call, the device the tensors live
on and the loaded library.  References come from tests/vad_reference.py (float64) and are computed once per process."""
import functools

import numpy as np
import pytest
import torch

import fbank_reference as FR
import resample_bodies as RB
import vad_reference as V
from resample_bodies import Ctx                                  # noqa: F401  (the same context)

FL, FS, CTX = 400, 160, V.DEFAULTS["frames_context"]
DTYPES = ("float32", "int16")
PLAIN = {"silence": False, "noise": True, "dc": True, "tone": True}      # kind -> every frame voiced?
KINDS = ("gated", "ramp") + tuple(PLAIN)

# |log energy - restatement|, a priori.  A frame's sum is frame_len squares (one rounding each) added in f32 (at most
# frame_len - 1 roundings on any one path, every term non-negative): a relative error of at most (frame_len + 1) * 2^-24
# in the sum, in whatever order, and the same absolute error in its logarithm (|ln(1 + d)| <= 1.0001 |d| here).  logf is
# good to a few ulp, taken as 4 here, and |e| < 32 (the floor is ln 2^-23 = -15.9, a full-scale frame ln(400 * 2^30) =
# 26.8), where an ulp is at most 2^-19.  Together 3.2e-5 at frame_len = 400.
# Measured worst case over every kind, length and dtype below: host emulator 1.1e-6 ("noise" int16; the host's logf is
# correctly rounded to within an ulp), MI355X 4.1e-6 ("noise" int16 and "gated" int16; two ulp of the device's logf at
# |e| >= 16); the frames at the floor ("silence") are exact on both.
def energy_tol(frame_len):
    """the bound above for a frame of `frame_len` samples (frame_len <= 800 keeps |e| < 32: ln(800 * 2^30) = 27.5)"""
    return 1.0001 * (frame_len + 1) * 2.0 ** -24 + 4 * 2.0 ** -19


def band(frame_len, energy_mean_scale):
    """a decision may differ only where some frame of the window has an energy this close to its threshold: the energy's
    own band plus the threshold's (|energy_mean_scale| times the mean's error, itself at most the energy's bound)"""
    return energy_tol(frame_len) * (1.0 + abs(energy_mean_scale))


ENERGY_TOL = energy_tol(FL)
BAND = band(FL, V.DEFAULTS["energy_mean_scale"])
TOL_DB = 5e-4                                    # the bar the default configuration's features over kept rows had: a ceiling
GUARD = RB.GUARD

# the frame configurations of fbank_bodies.CONFS the decision runs under (the 32-row tile: 22k, 16k_gaps, 32k_128) ...
VAD_CONFS = ("16k_odd_len", "22k", "16k_gaps", "8k_abutting", "32k_128", "2k_12", "16k_step1")
# ... and the rules: name -> (VadConfig keywords, the signals the rule runs on)
RULES = {
    "default": ({}, ("gated", "ramp")),
    "ctx0": (dict(frames_context=0, proportion_threshold=1.0), ("gated", "ramp")),
    "ctx7": (dict(frames_context=7, proportion_threshold=0.5), ("gated", "ramp")),
    "ctx64": (dict(frames_context=64, proportion_threshold=0.7), ("gated", "ramp")),      # (0.3 would vote every frame voiced)
    "ctx33": (dict(frames_context=33, proportion_threshold=0.75), ("gated", "ramp")),
    "fixed": (dict(energy_mean_scale=0.0, energy_threshold=14.0), ("gated", "ramp")),
    "falling": (dict(frames_context=1, proportion_threshold=1.0, energy_mean_scale=-0.25, energy_threshold=22.0),
                ("gated", "ramp")),
    "floor1": (dict(energy_floor=1.0), ("silence", "gated")),        # silence: ln 1 = 0, exactly
}
# every rule under the baseline and under a 32-row configuration, every configuration under the default rule, and the
# widest halo, an even context, no context and the long odd one once more where the frames are least like the baseline's
TABLE = tuple([(c, "default") for c in VAD_CONFS] + [
    ("16k", "ctx0"), ("22k", "ctx0"), ("16k", "ctx7"), ("16k_gaps", "ctx7"), ("16k", "ctx64"), ("32k_128", "ctx64"),
    ("16k", "ctx33"), ("22k", "ctx33"), ("16k", "fixed"), ("16k_gaps", "fixed"), ("16k", "falling"), ("32k_128", "falling"),
    ("16k", "floor1"), ("22k", "floor1"),
    ("2k_12", "ctx64"), ("8k_abutting", "ctx7"), ("16k_step1", "ctx0"), ("16k_odd_len", "ctx33")])
TABLE_CASES = tuple((c, r, kind, dtype) for c, r in TABLE for kind in RULES[r][1] for dtype in DTYPES)
ENERGY_CASES = tuple((c, kind, dtype) for c in VAD_CONFS for kind in ("gated", "ramp") for dtype in DTYPES)


def conf_of(name):
    import fbank_bodies as FB
    return FB.CONFS[name]


def rule_kw(rule):
    return {**V.DEFAULTS, **RULES[rule][0]}


def tile_frames(lib):
    return int(lib.raw("ds_vad_tile_frames")())


def samples_for(T, fl=FL, fs=FS):
    """a length that gives T frames, the last one partly zero padding (where the step leaves room for any)"""
    return fl // 2 if T == 1 else fl + (T - 1) * fs - min(37, fs - 1)


def lengths(tile):
    ns = [1, 399, 400, 401, 560, 561]
    for T in (CTX, CTX + 1, 2 * CTX + 1, 63, 64, 65, 129, tile - 1, tile, tile + 1, 2 * tile + 1):
        ns.append(samples_for(T))
    return ns


def frame_counts(tile, tm):
    """the decision tile's and the filterbank tile's boundaries"""
    return sorted({1, 2, 3, 63, 64, 65, 129, tile - 1, tile, tile + 1, 2 * tile + 1, tm - 1, tm, tm + 1, 2 * tm + 1})


def conf_lengths(tile, c):
    fl, fs = c.frame_len, c.frame_step
    return [1, fl - 1, fl + 1] + [samples_for(T, fl, fs) for T in frame_counts(tile, c.tile)]


@functools.lru_cache(maxsize=64)
def _ar(seed, n):
    """(a sample-by-sample recursion: "gated" and "ramp" of one seed share it)"""
    x = FR.synthetic_audio(seed, n, kind="ar")
    x.setflags(write=False)
    return x


def _speech(seed, n):
    rs = np.random.RandomState(seed)
    return rs, _ar(seed, n).astype(np.float64), 1e-3 * rs.randn(n)


def gated(seed, n):
    """speech-like bursts of 2000 .. 8000 samples with gaps of 1500 .. 6000 over a noise floor"""
    rs, sp, bg = _speech(seed, n)
    g = np.zeros(n)
    p = int(rs.randint(0, 3000))
    while p < n:
        b = int(rs.randint(2000, 8000))
        g[p:p + b] = 1.0
        p += b + int(rs.randint(1500, 6000))
    return (sp * g + bg).astype(np.float32)


def ramp(seed, n, fade=1.0):
    """the same speech-like signal fading linearly from full level into the noise floor over the first `fade` of the
    utterance; the rest is the floor alone"""
    _, sp, bg = _speech(seed, n)
    return (sp * np.clip(np.linspace(1.0, 1.0 - 1.0 / fade, n), 0.0, None) + bg).astype(np.float32)


# The table's "ramp" reaches the floor at 0.7 of the utterance.  Fading over the whole utterance, as the default
# configuration's cases do, leaves fewer than 2 % of the frames unvoiced under a fixed threshold of 14 (the fade crosses it
# at 1.5 % of full level), and none at all at step 1, where the last frame of the longest utterance still spans a sixth of
# the fade: "both decisions occur" would fail on the reference alone.
TABLE_FADE = 0.7


def signal(kind, seed, n, fade=1.0):
    if kind == "gated":
        return gated(seed, n)
    if kind == "ramp":
        return ramp(seed, n, fade)
    return FR.synthetic_audio(seed, n, kind=kind)


@functools.lru_cache(maxsize=None)
def _float_signals(kind, tile):
    # (the seeds: a "noise" utterance of ONE sample is voiced only if that sample is not a small one, |x| > 0.0075;
    # decisions() asserts on the reference side that these inputs are what the case assumes)
    return [signal(kind, 4001 + 100 * KINDS.index(kind) + i, n) for i, n in enumerate(lengths(tile))]


@functools.lru_cache(maxsize=None)
def _conf_signals(kind, tile, conf):
    """the table's signals of one frame configuration: "gated" and "ramp" from the same seeds"""
    c = conf_of(conf)
    seed0 = 6000 + 100 * VAD_CONFS.index(conf) if conf in VAD_CONFS else 6900
    return [signal(kind, seed0 + i, n, TABLE_FADE) for i, n in enumerate(conf_lengths(tile, c))]


@functools.lru_cache(maxsize=None)
def energies(kind, dtype, tile, conf=None, floor=V.DEFAULTS["energy_floor"]):
    """(signals, float64 energies) of every length, read-only; conf None: the default configuration's own lengths"""
    fl, fs = (FL, FS) if conf is None else (conf_of(conf).frame_len, conf_of(conf).frame_step)
    floats = _float_signals(kind, tile) if conf is None else _conf_signals(kind, tile, conf)
    xs = [FR.int16_quantised(x) if dtype == "int16" else x for x in floats]
    es = [V.log_energy(x, fl, fs, floor) for x in xs]
    for a in xs + es:
        a.setflags(write=False)
    return xs, es


@functools.lru_cache(maxsize=None)
def batch(kind, dtype, tile, conf=None, rule="default"):
    """(signals, float64 energies, thresholds, reference masks) of every length, read-only"""
    kw = rule_kw(rule)
    xs, es = energies(kind, dtype, tile, conf, kw["energy_floor"])
    thrs = [V.threshold(e, **kw) for e in es]
    masks = [V.decide(e, **kw) for e in es]
    for a in masks:
        a.setflags(write=False)
    return xs, es, thrs, masks


def split(t, off):
    a = t.cpu().numpy()
    assert len(a) == off[-1]
    return [a[off[u]:off[u + 1]] for u in range(len(off) - 1)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def exempt_frames(e, thr, ctx=CTX, band=BAND):
    """frames whose clipped window holds a frame within `band` of the threshold"""
    near = np.abs(e - thr) < band
    T = len(e)
    return np.array([near[max(0, t - ctx):min(T - 1, t + ctx) + 1].any() for t in range(T)])


# ---- 1. energy values ----
def planned_tile(ctx, c):
    """the filterbank tile ds_fbank_plan gives the configuration, which the table of cases states too"""
    import fbank_bodies as FB
    rc, counts = FB.plan_counts(ctx.lib, [1], c.frame_len, c.frame_step, c.nfft, c.nfilt)
    assert rc == 0 and counts[2] == c.tile, (counts, c.tile)
    return counts[2]


def energy_values(ctx, kind, dtype, conf=None, floor=None):
    F = ctx.features
    tile = tile_frames(ctx.lib)
    if conf is None:
        fl, fs, name, config, floor_kw = FL, FS, "", F.FbankConfig(), {}
        xs, es = energies(kind, dtype, tile, None, V.DEFAULTS["energy_floor"])
        want = {1, 2, 3, CTX, CTX + 1, 2 * CTX + 1, 63, 64, 65, 129, tile - 1, tile, tile + 1, 2 * tile + 1}
    else:
        c = conf_of(conf)
        fl, fs, name, config = c.frame_len, c.frame_step, f" {conf} {c.frame_len}/{c.frame_step} tile {c.tile}", c.config(F)
        floor_kw = {} if floor is None else dict(energy_floor=floor)
        assert (config.frame_len, config.frame_step) == (fl, fs) and fl <= 800
        xs, es = energies(kind, dtype, tile, conf, V.DEFAULTS["energy_floor"] if floor is None else floor)
        want = set(frame_counts(tile, planned_tile(ctx, c)))
    out, off = F.frame_log_energy([ctx.t(x) for x in xs], config, **floor_kw)
    assert out.dtype == torch.float32 and out.dim() == 1 and off.dtype == np.int64
    assert np.diff(off).tolist() == [len(e) for e in es] == [FR.n_frames(len(x), fl, fs) for x in xs]
    assert want <= set(np.diff(off))
    got = split(out, off)
    err = max(float(np.abs(g - e).max()) for g, e in zip(got, es))
    tol = energy_tol(fl)
    print(f"log energy{name} {kind} {dtype}: max abs error {err:.3e}, bound {tol:.3e}")
    assert err <= tol, (err, tol)
    assert max(float(np.abs(e).max()) for e in es) < 32.0            # the range the bound was derived for
    if kind == "silence":                                            # at the floor: the floor's own logarithm, exactly
        for g, e in zip(got, es):
            np.testing.assert_array_equal(bits(g), bits(e.astype(np.float32)))
            assert floor is None or (e == np.log(floor)).all()


# ---- 2. decisions ----
def decisions(ctx, kind, dtype, conf=None, rule="default"):
    F = ctx.features
    tile = tile_frames(ctx.lib)
    kw = rule_kw(rule)
    if conf is None:
        fl, name, config = FL, "", F.FbankConfig()
    else:
        c = conf_of(conf)
        fl, name, config = c.frame_len, f" {conf} {c.frame_len}/{c.frame_step} tile {planned_tile(ctx, c)} {rule}", c.config(F)
    xs, es, thrs, masks = batch(kind, dtype, tile, conf, rule)
    # the reference side first: the inputs must leave (next to) nothing to the band
    exempt = [exempt_frames(e, thr, kw["frames_context"], band(fl, kw["energy_mean_scale"])) for e, thr in zip(es, thrs)]
    n_exempt, n_all = sum(int(x.sum()) for x in exempt), sum(len(x) for x in exempt)
    assert n_exempt <= 0.01 * n_all, (kind, n_exempt, n_all)
    if kind != "ramp":
        assert n_exempt == 0, (kind, n_exempt)
    if kind in PLAIN:
        assert all(bool((m == PLAIN[kind]).all()) for m in masks), kind
    else:
        long_ones = np.concatenate([m for m in masks if len(m) >= 63])
        assert 0.02 < long_ones.mean() < 0.98, (kind, long_ones.mean())   # both decisions occur
    mask, off = F.voiced_frames([ctx.t(x) for x in xs], F.VadConfig(**kw), config)
    assert mask.dtype == torch.uint8 and mask.dim() == 1 and np.diff(off).tolist() == [len(m) for m in masks]
    bad = 0
    for g, m, x in zip(split(mask, off), masks, exempt):
        assert set(np.unique(g).tolist()) <= {0, 1}
        bad += int(((g != 0) != m)[~x].sum())
    print(f"decisions{name} {kind} {dtype}: {n_all} frames, {n_exempt} exempt, {bad} wrong, "
          f"{sum(int(m.sum()) for m in masks) / n_all:.1%} voiced")
    assert bad == 0


# ---- 3. clipping and isolation ----
def _one_loud_frame(T, last):
    x = np.zeros(FL + (T - 1) * FS, np.float32)
    rs = np.random.RandomState(T)
    if last:
        x[(T - 1) * FS + FL - FS:] = 0.5 * np.sign(rs.randn(FS))     # samples only frame T - 1 covers
    else:
        x[:FS] = 0.5 * np.sign(rs.randn(FS))                         # samples only frame 0 covers
    return x


def clipping(ctx):
    F = ctx.features
    T = 20
    loud = FR.synthetic_audio(1, 8000, kind="tone")
    first, last = _one_loud_frame(T, False), _one_loud_frame(T, True)
    silent, short = np.zeros(FL + 39 * FS, np.float32), np.zeros(FL + FS, np.float32)
    xs = [loud, first, loud, last, loud, silent, loud, short, loud]
    for cfg, reach in ((F.VadConfig(), CTX), (F.VadConfig(proportion_threshold=0.3), 0)):
        # default: one frame of 3, 4 or 5 is enough (0.12); at 0.3 only the window of 3 at the very edge is: the loud
        # frame itself votes yes, its neighbours (windows of 4 and 5 need 2) do not
        mask, off = F.voiced_frames([ctx.t(x) for x in xs], cfg)
        ms = split(mask, off)
        want_first, want_last = np.zeros(T, np.uint8), np.zeros(T, np.uint8)
        want_first[:reach + 1] = 1
        want_last[T - 1 - reach:] = 1
        kw = dict(proportion_threshold=cfg.proportion_threshold)
        assert V.vad(first, **kw).tolist() == want_first.astype(bool).tolist()         # the restatement agrees
        assert V.vad(last, **kw).tolist() == want_last.astype(bool).tolist()
        assert ms[1].tolist() == want_first.tolist() and ms[3].tolist() == want_last.tolist()
        assert all(m.all() for m in ms[0::2])                        # the loud neighbours
        assert not ms[5].any() and len(ms[5]) == 40 and not ms[7].any() and len(ms[7]) == 2
        feats = ctx.t(np.arange(off[-1] * 4, dtype=np.float32).reshape(-1, 4))
        kept, new_off = F.select_frames(feats, off, mask)
        assert np.diff(new_off).tolist() == [int(m.sum()) for m in ms]
        assert new_off[6] == new_off[5] and new_off[8] == new_off[7] and kept.shape[0] == new_off[-1]
    # the widest halo: one loud frame is one vote in a window of up to 129, so at 0.01 it lights the frames whose clipped
    # window holds it and has at most 100 frames.  20 frames: every window is the utterance.  1025 frames: the loud last
    # frame is alone in the second decision tile and lights 35 frames of the first through that tile's upper halo; its
    # own window reaches 64 frames back into the first tile
    cfg = F.VadConfig(frames_context=64, proportion_threshold=0.01)
    kw = dict(frames_context=64, proportion_threshold=0.01)
    assert tile_frames(ctx.lib) == 1024
    for T in (20, 1025):
        first, last = _one_loud_frame(T, False), _one_loud_frame(T, True)
        lit = np.array([t <= 64 and min(T - 1, t + 64) + 1 <= 100 for t in range(T)])
        assert lit.sum() == (20 if T == 20 else 36)
        assert V.vad(first, **kw).tolist() == lit.tolist() and V.vad(last, **kw).tolist() == lit[::-1].tolist()
        mask, off = F.voiced_frames([ctx.t(x) for x in (loud, first, loud, last, loud)], cfg)
        ms = split(mask, off)
        assert ms[1].tolist() == lit.astype(np.uint8).tolist() and ms[3].tolist() == lit[::-1].astype(np.uint8).tolist()
        assert all(m.all() for m in ms[0::2])


# ---- 4. selection ----
@functools.lru_cache(maxsize=None)
def selection_signals():
    """zero-row utterances first, in the middle and last; the others around the fbank tile"""
    quiet = lambda n: np.zeros(n, np.float32)
    xs = [quiet(1000)] + [gated(600 + i, samples_for(T)) for i, T in enumerate((1, 3, 63, 64))] + [quiet(401)] + \
         [gated(610 + i, samples_for(T)) for i, T in enumerate((65, 129))] + [quiet(1)]
    for x in xs:
        x.setflags(write=False)
    return xs


def selection(ctx):
    F = ctx.features
    xs = [ctx.t(x) for x in selection_signals()]
    feats, off = F.log_mel_fbank(xs, normalize=None)
    mask, off_m = F.voiced_frames(xs)
    assert off.tolist() == off_m.tolist()
    out, new_off = F.select_frames(feats, off, mask)
    m = mask.cpu().numpy().astype(bool)
    np.testing.assert_array_equal(bits(out.cpu().numpy()), bits(feats.cpu().numpy()[m]))      # values and order
    counts = [int(m[off[u]:off[u + 1]].sum()) for u in range(len(xs))]
    assert new_off.dtype == np.int64 and new_off.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert counts[0] == counts[5] == counts[-1] == 0 and sum(counts) > 100
    # every length, a narrow matrix whose entries name their row: utterances that span several decision tiles
    tile = tile_frames(ctx.lib)
    sig, _, _, masks = batch("gated", "float32", tile)
    mask, off = F.voiced_frames([ctx.t(x) for x in sig])
    rows = np.arange(off[-1] * 8, dtype=np.float32).reshape(-1, 8)
    out, new_off = F.select_frames(ctx.t(rows), off, mask)
    m = mask.cpu().numpy().astype(bool)
    np.testing.assert_array_equal(out.cpu().numpy(), rows[m])
    assert np.diff(new_off).tolist() == [int(m[off[u]:off[u + 1]].sum()) for u in range(len(sig))]
    # every row width the selection is used with (nfilt 4, 12, 64, 128): 1, 3, 16 and 32 vectors per row
    for width in (4, 12, 64, 128):
        wide = np.arange(off[-1] * width, dtype=np.float32).reshape(-1, width)
        assert wide[-1, -1] < 2.0 ** 24                              # the entries name their row exactly
        out, new_off_w = F.select_frames(ctx.t(wide), off, mask)
        np.testing.assert_array_equal(out.cpu().numpy(), wide[m])
        assert new_off_w.tolist() == new_off.tolist()
    # a mask of the caller's own: any non-zero byte keeps the row
    own = np.random.RandomState(3).randint(0, 3, off[-1]).astype(np.uint8) * 127
    out, new_off = F.select_frames(ctx.t(rows), off, ctx.t(own))
    np.testing.assert_array_equal(out.cpu().numpy(), rows[own != 0])
    # an utterance of more decision tiles than a workgroup has threads (each thread then scans a run of tile counts),
    # between two short ones
    long_off = np.array([0, 3, 3 + 2 * 256 * tile + 77, 2 * 256 * tile + 90], np.int64)
    long_rows = np.arange(long_off[-1] * 4, dtype=np.float32).reshape(-1, 4)
    long_mask = (np.random.RandomState(4).rand(long_off[-1]) < 0.3).astype(np.uint8)
    out, new_off = F.select_frames(ctx.t(long_rows), long_off, ctx.t(long_mask))
    np.testing.assert_array_equal(out.cpu().numpy(), long_rows[long_mask != 0])
    assert np.diff(new_off).tolist() == [int(long_mask[long_off[u]:long_off[u + 1]].sum()) for u in range(3)]
    none, zero_off = F.select_frames(ctx.t(rows), off, ctx.t(np.zeros(off[-1], np.uint8)))
    assert none.shape == (0, 8) and not zero_off.any() and len(zero_off) == len(off)


# ---- 5. normalisation over the kept rows ----
NORM_CONFS = ("22k", "16k_gaps", "32k_128", "2k_12")                 # 32-row tiles handed over to the selection's 64; nfilt 128, 12
KEPT_COUNTS = (0, 1, 63, 64, 65, 129)                                # around the selection's tile of 64 rows


def burst(seed, n_loud, n):
    """speech-like for the first n_loud samples, then the noise floor"""
    x = 1e-3 * np.random.RandomState(seed).randn(n)
    x[:n_loud] += _ar(seed, n)[:n_loud]
    return x.astype(np.float32)


def kept_exactly(seed, K, fl, fs):
    """an utterance of which the default rule keeps exactly K frames (asserted on the restatement): silence for none, one
    loud frame for one, else a burst at the start whose length is searched in quarter steps, before as many frames of
    floor again (at least 20), so that the threshold lies between the two levels"""
    if K == 0:
        return np.zeros(fl + 3 * fs, np.float32)
    if K == 1:
        return _ar(seed, fl // 2).copy()
    n = samples_for(2 * K + 20, fl, fs)
    for n_loud in range(max(1, K - 6) * fs, (K + 6) * fs, max(1, fs // 4)):
        x = burst(seed, n_loud, n)
        if int(V.vad(x, fl, fs).sum()) == K:
            return x
    raise AssertionError(("no burst keeps", K, fl, fs))


def mode_name(normalize):
    return "log" if normalize is None else normalize


def normalised(raw, normalize):
    return raw if normalize is None else FR.normalize_frames(raw, scale=normalize == "mean_std")


def kept_references(xs, kw, fl, fs):
    """(reference masks, float64 log filterbank over the kept rows, the float32 restatement's), asserting that the inputs
    leave nothing to the band, so that the reference mask IS the mask"""
    import fbank_bodies as FB
    masks = [V.vad(x, fl, fs) for x in xs]
    es = [V.log_energy(x, fl, fs) for x in xs]
    assert not any(exempt_frames(e, V.threshold(e), CTX, band(fl, V.DEFAULTS["energy_mean_scale"])).any() for e in es)
    raw = [FR.fbank(FB.as_float(x), **kw)[m] for x, m in zip(xs, masks)]
    raw32 = [FR.mk_mfb_f32(FB.as_float(x), normalize=None, **kw)[m] for x, m in zip(xs, masks)]
    for a in raw + raw32:
        a.setflags(write=False)
    return masks, raw, raw32


@functools.lru_cache(maxsize=None)
def normalisation_case(conf=None):
    """(signals, the float32 ones first, how many those are, kept rows in float64, kept rows of the float32 restatement)"""
    if conf is None:
        xs = [gated(700, 16000), gated(701, 48000), np.zeros(3000, np.float32), gated(702, 5000),
              FR.synthetic_audio(703, 561, kind="noise"), FR.synthetic_audio(704, 400, kind="tone"),
              FR.int16_quantised(gated(705, 16000))]
        n_float = 6
        _, raw, raw32 = kept_references(xs, {}, FL, FS)
        assert [len(r) for r in raw][2] == 0 and min(len(r) for i, r in enumerate(raw) if i != 2) >= 1
    else:
        c = conf_of(conf)
        fl, fs = c.frame_len, c.frame_step
        xs = [kept_exactly(7100 + 10 * NORM_CONFS.index(conf) + i, K, fl, fs) for i, K in enumerate(KEPT_COUNTS)]
        n_float = len(xs)
        xs += [FR.int16_quantised(x) for x in xs[3:5]]               # int16 copies of the 64 and the 65
        _, raw, raw32 = kept_references(xs, c.ref_kw(), fl, fs)
        assert [len(r) for r in raw] == list(KEPT_COUNTS) + [64, 65]
    for x in xs:
        x.setflags(write=False)
    return xs, n_float, raw, raw32


def normalisation(ctx, normalize, conf=None):
    """features over the voiced frames, normalised over what was kept, against the float64 chain under the filterbank's
    restated bar for the configuration and mode: max(floor, 4 x the float32 restatement's distance), over the kept rows"""
    import fbank_bodies as FB
    F = ctx.features
    xs, n_float, raw, raw32 = normalisation_case(conf)
    config = F.FbankConfig() if conf is None else conf_of(conf).config(F)
    if conf is not None:
        assert planned_tile(ctx, conf_of(conf)) == conf_of(conf).tile
    metric, floor = FB.METRIC[mode_name(normalize)]
    worst = restated = 0.0
    for sel in (slice(0, n_float), slice(n_float, len(xs))):         # the float32 utterances, then the int16 ones
        out, off = F.log_mel_fbank([ctx.t(x) for x in xs[sel]], config, normalize=normalize, vad=F.VadConfig())
        assert np.diff(off).tolist() == [len(r) for r in raw[sel]] and out.shape == (off[-1], config.nfilt)
        for g, r, r32 in zip(split(out, off), raw[sel], raw32[sel]):
            if len(r):
                ref = normalised(r, normalize)
                assert normalize == "mean_std" or np.abs(ref).max() < 128.0       # FLOOR_DB is one ulp there
                worst = max(worst, metric(g, ref))
                restated = max(restated, metric(normalised(r32.astype(np.float64), normalize).astype(np.float32), ref))
    bar = FB.bar_from_restatement(floor, restated)
    if conf is None:
        bar = min(bar, TOL_DB)                                       # never looser than the bar this case had
    FB.say(f"fbank over voiced frames {conf or 'default'}", mode_name(normalize), restated, bar, worst)
    assert worst <= bar, (conf, normalize, worst, bar)
    assert conf is not None or worst <= TOL_DB, worst


# ---- 5a. the entry points on guarded buffers ----
FILL = 0xAA                                      # every byte of a buffer a kernel is to write: no count, scan or 0 / 1 looks so


class Guarded:
    """A device buffer of n entries whose every byte is FILL (float: NaN), between GUARD entries of the same on both sides;
    `inside` is what the kernel is handed."""

    def __init__(self, ctx, n, dtype):
        self.n, self.dtype = n, dtype
        self.floating = dtype in (torch.float32, torch.float64)
        width = torch.empty(0, dtype=dtype).element_size()
        if self.floating:
            self.buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=ctx.dev)
        else:
            self.buf = torch.full(((n + 2 * GUARD) * width,), FILL, dtype=torch.uint8, device=ctx.dev).view(dtype)
        self.inside = self.buf[GUARD:GUARD + n]
        self.fill = None if self.floating else np.full(width, FILL, np.uint8).view(self.buf.cpu().numpy().dtype)[0]

    def untouched(self, a):
        return np.isnan(a) if self.floating else a == self.fill

    def read(self, what, written=None):
        """the inside on the host: both guards as they were, every entry (of the first `written`) overwritten"""
        a = self.buf.cpu().numpy()
        assert self.untouched(a[:GUARD]).all(), f"{what}: a store before the buffer"
        assert self.untouched(a[GUARD + self.n:]).all(), f"{what}: a store past the buffer"
        got = a[GUARD:GUARD + self.n]
        assert not self.untouched(got[:self.n if written is None else written]).any(), f"{what}: an entry was not written"
        return got.copy()


def direct(ctx, conf, dtype, max_frames=None):
    """ds_vad_log_energy_f32, ds_vad_decide, ds_vad_scan and ds_vad_select_f32 called as features.py calls them, on buffers
    that show a read past the samples or a store outside any output; the results are the public functions' bits.
    `max_frames`: leave out the longer utterances (the host emulator's filterbank is slow)"""
    import fbank_bodies as FB
    F, lib = ctx.features, ctx.lib
    eng = F._eng()
    c = conf_of(conf)
    config, vad = c.config(F), F.VadConfig()
    fl, fs, nfilt = c.frame_len, c.frame_step, c.nfilt
    tile = tile_frames(lib)
    xs = [x for x in energies("gated", dtype, tile, conf, V.DEFAULTS["energy_floor"])[0]
          if max_frames is None or FR.n_frames(len(x), fl, fs) <= max_frames]
    assert max(FR.n_frames(len(x), fl, fs) for x in xs) > tile       # more than one decision tile
    xs = xs[:3] + [np.zeros(fl + 5 * fs, xs[0].dtype)] + xs[3:]      # an utterance without a kept row among the others
    n_utt, lens = len(xs), np.array([len(x) for x in xs], np.int64)
    int16 = xs[0].dtype == np.int16
    tail = np.full(GUARD, -32768, np.int16) if int16 else np.full(GUARD, np.nan, np.float32)
    samples = ctx.t(np.concatenate(list(xs) + [tail]))
    # the filterbank's table
    rc, (n_frames, n_tiles, tm) = FB.plan_counts(lib, lens, fl, fs, c.nfft, nfilt)
    assert rc == 0 and tm == c.tile
    table = np.full(3 * (n_utt + 1) + n_tiles, -7, np.int64)
    assert FB.plan_counts(lib, lens, fl, fs, c.nfft, nfilt, table) == (0, [n_frames, n_tiles, tm])
    offsets = table[n_utt + 1:2 * (n_utt + 1)].copy()
    table_dev = ctx.t(table)
    # energies
    energy = Guarded(ctx, n_frames, torch.float32)
    eng.lib.call("ds_vad_log_energy_f32", eng._p(samples), int(int16), eng._p(table_dev), n_utt, n_tiles, tm, fl, fs,
                 float(vad.energy_floor), eng._p(energy.inside), eng._stream(energy.buf))
    e = energy.read("energy")
    # the decision
    counts = np.zeros(3, np.int64)
    assert lib.raw("ds_vad_plan")(offsets.ctypes.data, n_utt, None, counts.ctypes.data) == 0
    n_dtiles = int(counts[1])
    vtable = np.full(2 * (n_utt + 1) + n_dtiles, -7, np.int64)
    assert lib.raw("ds_vad_plan")(offsets.ctypes.data, n_utt, vtable.ctypes.data, counts.ctypes.data) == 0
    assert counts.tolist() == [n_frames, n_dtiles, tile] and (vtable != -7).all()
    vtable_dev = ctx.t(vtable)
    n_ws = int(lib.raw("ds_vad_workspace_bytes")(n_utt, n_dtiles)) // 8
    assert n_ws == n_utt + n_dtiles

    def buffers():
        return (Guarded(ctx, n_frames, torch.int32), Guarded(ctx, n_utt, torch.int64), Guarded(ctx, n_ws, torch.int64))

    mask = Guarded(ctx, n_frames, torch.uint8)
    scan, kept, ws = buffers()
    eng.lib.call("ds_vad_decide", eng._p(energy.inside), eng._p(vtable_dev), n_utt, n_dtiles, float(vad.energy_threshold),
                 float(vad.energy_mean_scale), int(vad.frames_context), float(vad.proportion_threshold),
                 eng._p(mask.inside), eng._p(scan.inside), eng._p(kept.inside), eng._p(ws.inside), eng._stream(mask.buf))
    m, sc, kp = mask.read("mask"), scan.read("scan"), kept.read("kept")
    ws.read("decision workspace")
    assert set(np.unique(m).tolist()) <= {0, 1}
    want_scan = np.concatenate([np.cumsum(m[offsets[u]:offsets[u + 1]]) - m[offsets[u]:offsets[u + 1]] for u in range(n_utt)])
    assert sc.tolist() == want_scan.tolist()
    assert kp.tolist() == [int(m[offsets[u]:offsets[u + 1]].sum()) for u in range(n_utt)] and kp[3] == 0 and kp.sum() > 100
    # the scan of a mask, alone: the same scan and counts
    scan2, kept2, ws2 = buffers()
    eng.lib.call("ds_vad_scan", eng._p(mask.inside), eng._p(vtable_dev), n_utt, n_dtiles, eng._p(scan2.inside),
                 eng._p(kept2.inside), eng._p(ws2.inside), eng._stream(mask.buf))
    assert scan2.read("scan alone").tolist() == sc.tolist() and kept2.read("kept alone").tolist() == kp.tolist()
    counts2 = ws2.read("scan workspace", written=0)[n_utt:]          # (the thresholds' part is the decision's alone)
    assert (counts2 >= 0).all(), "a tile's count was not written"
    assert mask.read("mask after the scan").tolist() == m.tolist()
    # the selection, of the public call's log features
    feats, off = F.log_mel_fbank([ctx.t(x) for x in xs], config, normalize=None)
    assert off.tolist() == offsets.tolist()
    k_tiles = -(-kp // F.SELECT_TILE_ROWS)
    n_ktiles, n_kept = int(k_tiles.sum()), int(kp.sum())
    ktable_dev = ctx.t(F._ragged_table([np.zeros(n_utt, np.int64), kp], k_tiles))
    n_stats = int(lib.raw("ds_fbank_workspace_bytes")(n_utt, n_ktiles, nfilt)) // 8
    rows, stats = Guarded(ctx, n_kept * nfilt, torch.float32), Guarded(ctx, n_stats, torch.float64)
    eng.lib.call("ds_vad_select_f32", eng._p(feats), eng._p(mask.inside), eng._p(scan.inside), eng._p(vtable_dev),
                 eng._p(ktable_dev), n_utt, n_ktiles, nfilt, F.SELECT_TILE_ROWS, eng._p(rows.inside), eng._p(stats.inside),
                 eng._stream(rows.buf))
    sel = rows.read("selected rows").reshape(n_kept, nfilt)
    part = stats.read("the tiles' statistics", written=2 * nfilt * n_ktiles)
    np.testing.assert_array_equal(bits(sel), bits(feats.cpu().numpy()[m != 0]))
    # a tile's sums are those of its rows: {sum, sum of squares} per filter, 64 rows of one utterance per tile
    koff = np.concatenate([[0], np.cumsum(kp)])
    first = [koff[u] + 64 * j for u in range(n_utt) for j in range(k_tiles[u])]
    last = [min(koff[u] + 64 * (j + 1), koff[u + 1]) for u in range(n_utt) for j in range(k_tiles[u])]
    sums = np.array([[sel[a:b].astype(np.float64).sum(0), (sel[a:b].astype(np.float64) ** 2).sum(0)] for a, b in zip(first, last)])
    np.testing.assert_allclose(part[:2 * nfilt * n_ktiles].reshape(n_ktiles, 2, nfilt), sums, rtol=1e-12, atol=1e-9)
    # the public functions: the same bits
    pe, poff = F.frame_log_energy([ctx.t(x) for x in xs], config)
    pm, _ = F.voiced_frames([ctx.t(x) for x in xs], vad, config)
    ps, pnew = F.select_frames(feats, off, pm)
    pf, pfo = F.log_mel_fbank([ctx.t(x) for x in xs], config, normalize=None, vad=vad)
    assert poff.tolist() == offsets.tolist() and pnew.tolist() == koff.tolist() == pfo.tolist()
    np.testing.assert_array_equal(bits(pe.cpu().numpy()), bits(e))
    assert pm.cpu().numpy().tolist() == m.tolist()
    np.testing.assert_array_equal(bits(ps.cpu().numpy()), bits(sel))
    np.testing.assert_array_equal(bits(pf.cpu().numpy()), bits(sel))
    print(f"vad direct {conf} {dtype}: {n_frames} frames in {n_tiles} tiles of {tm}, {n_dtiles} decision tiles, "
          f"{n_kept} kept rows of {nfilt} in {n_ktiles} tiles")


# ---- 5b. the chain ----
@functools.lru_cache(maxsize=None)
def chain_case():
    """1.5 s of stereo int16 at 44100 Hz and its float64 chain under fbank_bodies.CONFS["22k"]: down-mix -> resample ->
    decision -> filterbank over the kept rows; the float32 restatements of the resampler and the filterbank for the bar"""
    import resample_reference as R
    c = conf_of("22k")
    fl, fs = c.frame_len, c.frame_step
    rule = RULES["ctx7"][0]
    n = 66150
    g = gated(7300, n)
    stereo = FR.int16_quantised(np.stack([g, 0.5 * g], 1).reshape(-1))
    mono = R.downmix(stereo, 2)
    y = R.resample(mono, 1, 2).astype(np.float32)
    e = V.log_energy(y, fl, fs)
    m = V.decide(e, **{**V.DEFAULTS, **rule})
    assert not exempt_frames(e, V.threshold(e), rule["frames_context"], band(fl, V.DEFAULTS["energy_mean_scale"])).any()
    assert 0.1 < m.mean() < 0.9
    raw = FR.fbank(y, **c.ref_kw())[m]
    raw32 = FR.mk_mfb_f32(R.resample_f32(mono, 1, 2), normalize=None, **c.ref_kw())[m]
    for a in (stereo, raw, raw32):
        a.setflags(write=False)
    return stereo, raw, raw32


def chain(ctx):
    import fbank_bodies as FB
    F = ctx.features
    stereo, raw, raw32 = chain_case()
    out, off = F.log_mel_fbank([ctx.t(stereo)], conf_of("22k").config(F), orig_rate=44100, channels=2,
                               vad=F.VadConfig(**RULES["ctx7"][0]), normalize="mean_std")
    assert off.tolist() == [0, len(raw)] and out.shape == (len(raw), 64)
    metric, floor = FB.METRIC["mean_std"]
    ref = normalised(raw, "mean_std")
    restated = metric(normalised(raw32.astype(np.float64), "mean_std").astype(np.float32), ref)
    bar, err = FB.bar_from_restatement(floor, restated), metric(out.cpu().numpy(), ref)
    FB.say(f"44100 Hz stereo int16 -> 22050 -> vad -> fbank, {len(raw)} kept rows", "mean_std", restated, bar, err)
    assert err <= bar, (err, bar)


def vad_none_is_unchanged(ctx):
    F = ctx.features
    x16 = [FR.synthetic_audio(60 + i, n, kind="ar") for i, n in enumerate((401, 5000))]
    a, off_a = F.log_mel_fbank([ctx.t(v) for v in x16], vad=None)
    b, off_b = RB.direct_log_mel(ctx, ctx.t(np.concatenate(x16)), [401, 5000])
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and off_a.tolist() == off_b.tolist()


# ---- 6. deterministic and batch-invariant ----
def deterministic(ctx, n_max=30000):
    F = ctx.features
    rs = np.random.RandomState(9)
    xs = [ctx.t(gated(800 + i, int(rs.randint(1, n_max)))) for i in range(20)]
    mask, off = F.voiced_frames(xs)
    mask2, _ = F.voiced_frames(xs)
    e, _ = F.frame_log_energy(xs)
    e2, _ = F.frame_log_energy(xs)
    assert torch.equal(mask, mask2) and torch.equal(e.view(torch.int32), e2.view(torch.int32))
    a, koff = F.log_mel_fbank(xs, normalize="mean_std", vad=F.VadConfig())
    b, koff2 = F.log_mel_fbank(xs, normalize="mean_std", vad=F.VadConfig())
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and koff.tolist() == koff2.tolist()
    for u in (0, 7, 19):
        m1, o1 = F.voiced_frames([xs[u]])
        e1, _ = F.frame_log_energy([xs[u]])
        assert o1.tolist() == [0, off[u + 1] - off[u]]
        assert torch.equal(m1, mask[off[u]:off[u + 1]]) and torch.equal(e1.view(torch.int32), e[off[u]:off[u + 1]].view(torch.int32))
        a1, k1 = F.log_mel_fbank([xs[u]], normalize="mean_std", vad=F.VadConfig())
        assert k1.tolist() == [0, koff[u + 1] - koff[u]]
        assert torch.equal(a1.view(torch.int32), a[koff[u]:koff[u + 1]].view(torch.int32)), u
    lens = [len(x) for x in xs]
    mp, op = F.voiced_frames(torch.cat(xs), lengths=lens)
    ap, kp = F.log_mel_fbank(torch.cat(xs), normalize="mean_std", lengths=lens, vad=F.VadConfig())
    assert torch.equal(mp, mask) and op.tolist() == off.tolist()
    assert torch.equal(ap.view(torch.int32), a.view(torch.int32)) and kp.tolist() == koff.tolist()


# ---- 7. plumbing ----
def plumbing(ctx):
    from deepspeaker_pytorch_amd import data
    F = ctx.features
    vad = F.VadConfig()
    xs = [ctx.t(x) for x in (gated(900, 9000), np.zeros(2000, np.float32), gated(901, 4000))]
    a, off = F.log_mel_fbank(xs, vad=vad)
    store = data.FeatureStore.from_waveforms(xs, vad=vad)
    assert torch.equal(store.features.view(torch.int32), a.view(torch.int32)) and store.offsets.tolist() == off.tolist()
    assert len(store) == 3 and store.length(1) == 0 and store.length(0) == off[1] > 0
    crops = store.crops([1, 0, 1], [0, 0, 5], 16)
    assert crops.shape == (3, 1, 16, 64) and not crops[0].any() and not crops[2].any() and crops[1].any()
    # another rate, two channels: the decision is that of the resampled mono signal
    g48 = np.repeat(gated(902, 8000), 3)                             # 48 kHz, crudely: the gating survives
    stereo = ctx.t(np.stack([g48, 0.5 * g48], 1).reshape(-1).astype(np.float32))
    m, off_m = F.voiced_frames([stereo], vad, orig_rate=48000, channels=2)
    mono, lens = F.resample([stereo], 48000, channels=2)
    m2, off_2 = F.voiced_frames(mono, vad, lengths=lens)
    assert torch.equal(m, m2) and off_m.tolist() == off_2.tolist() and 0 < int(m.sum()) < m.numel()
    b, off_b = F.log_mel_fbank([stereo], orig_rate=48000, channels=2, vad=vad)
    c, off_c = F.log_mel_fbank(mono, lengths=lens, vad=vad)
    assert torch.equal(b.view(torch.int32), c.view(torch.int32)) and off_b.tolist() == off_c.tolist() == [0, int(m.sum())]


# ---- 8. errors ----
def abi_errors(ctx):
    lib = ctx.lib
    p = np.zeros(8, np.int64).ctypes.data                            # a placeholder: validation touches no buffer
    counts = np.zeros(3, np.int64)
    off = np.array([0, 5, 5, 2000], np.int64)
    plan = lib.raw("ds_vad_plan")
    assert plan(None, 3, None, counts.ctypes.data) == -3 and plan(off.ctypes.data, 0, None, counts.ctypes.data) == -1
    assert plan(np.array([0, 5, 4], np.int64).ctypes.data, 2, None, counts.ctypes.data) == -1         # falling offsets
    tile = tile_frames(lib)
    assert plan(off.ctypes.data, 3, None, counts.ctypes.data) == 0 and counts.tolist() == [2000, 1 + -(-1995 // tile), tile]
    # the table entry by entry: utterances of exactly one tile of frames, none, one frame more, and one frame; the
    # offsets need not start at 0
    off = np.array([5, 5 + tile, 5 + tile, 5 + 2 * tile + 1, 5 + 2 * tile + 2], np.int64)
    assert plan(off.ctypes.data, 4, None, counts.ctypes.data) == 0 and counts.tolist() == [2 * tile + 2, 4, tile]
    table = np.full(2 * 5 + 4, -7, np.int64)
    counts[:] = 0
    assert plan(off.ctypes.data, 4, table.ctypes.data, counts.ctypes.data) == 0
    assert counts.tolist() == [2 * tile + 2, 4, tile]
    assert table.tolist() == [0, tile, tile, 2 * tile + 1, 2 * tile + 2,  0, 1, 1, 3, 4,  0, 2, 2, 3]
    assert lib.raw("ds_vad_workspace_bytes")(0, 1) == -1 and lib.raw("ds_vad_workspace_bytes")(3, 4) == 56
    energy = lib.raw("ds_vad_log_energy_f32")
    assert energy(None, 0, p, 1, 1, 64, 400, 160, 1e-7, p, None) == -3
    assert energy(p, 0, p, 0, 1, 64, 400, 160, 1e-7, p, None) == -1
    assert energy(p, 2, p, 1, 1, 64, 400, 160, 1e-7, p, None) == -4          # neither f32 nor int16
    assert energy(p, 0, p, 1, 1, 64, 400, 160, 0.0, p, None) == -1           # no floor
    assert energy(p, 0, p, 1, 1, 64, 400, 160, float("nan"), p, None) == -1
    assert energy(p, 0, p, 1, 1, 64, 400, 1000, 1e-7, p, None) == -4         # a tile's samples do not fit the LDS
    decide = lambda n_utt=1, n_tiles=1, thr=5.5, scale=0.5, context=2, prop=0.12, e=p, out=p: lib.raw("ds_vad_decide")(
        e, p, n_utt, n_tiles, thr, scale, context, prop, out, p, p, p, None)
    assert decide(e=None) == -3 and decide(out=None) == -3
    assert decide(n_utt=0) == -1 and decide(n_tiles=0) == -1
    assert decide(context=-1) == -1 and decide(context=65) == -4
    assert decide(prop=0.0) == -1 and decide(prop=1.5) == -1 and decide(prop=float("nan")) == -1
    assert decide(thr=float("inf")) == -1 and decide(scale=float("nan")) == -1
    scan = lib.raw("ds_vad_scan")
    assert scan(None, p, 1, 1, p, p, p, None) == -3 and scan(p, p, 0, 1, p, p, p, None) == -1
    select = lib.raw("ds_vad_select_f32")
    assert select(None, p, p, p, p, 1, 1, 64, 64, p, p, None) == -3
    assert select(p, p, p, p, p, 0, 1, 64, 64, p, p, None) == -1 and select(p, p, p, p, p, 1, 1, 64, 48, p, p, None) == -1
    assert select(p, p, p, p, p, 1, 1, 6, 64, p, p, None) == -4              # rows of 6 floats


def python_errors(ctx):
    F = ctx.features
    for bad in (dict(frames_context=-1), dict(proportion_threshold=0.0), dict(proportion_threshold=1.01),
                dict(energy_threshold=float("nan")), dict(energy_mean_scale=float("inf")), dict(energy_floor=0.0),
                dict(frames_context=1.5)):
        with pytest.raises(ValueError):
            F.VadConfig(**bad)
    assert F.VadConfig(proportion_threshold=1.0).frames_context == 2
    with pytest.raises(Exception):
        F.VadConfig().frames_context = 3                             # frozen
    x = ctx.t(gated(1, 3000))
    feats, off = F.log_mel_fbank([x], normalize=None)
    mask, _ = F.voiced_frames([x])
    with pytest.raises(ValueError):
        F.select_frames(feats, off, mask[:-1])
    with pytest.raises(ValueError):
        F.select_frames(feats, off, mask.to(torch.int32))
    with pytest.raises(ValueError):
        F.select_frames(feats.double(), off, mask)
    with pytest.raises(ValueError):
        F.select_frames(feats, [0, 3], mask)
    with pytest.raises(ValueError):
        F.log_mel_fbank([x], vad=True)
    with pytest.raises(ValueError):
        F.voiced_frames([ctx.t(np.zeros(100, np.float64))])
