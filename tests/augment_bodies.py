"""TEST INFRASTRUCTURE: the cases of the waveform augmentation (csrc/augment.hip, features.augment), written once and run
by tests/test_emul_augment.py through the host emulator and by tests/test_gpu_augment.py on the device.  Every body takes
a `Ctx`: the features module to call, the device the tensors live on and the loaded library.  References come from
tests/augment_reference.py (float64) and are computed once per process."""
import functools
from dataclasses import dataclass

import numpy as np
import pytest
import torch

import augment_reference as A
import fbank_reference as FR

DTYPES = ("float32", "int16")
FBANK_TOL_DB = 5e-4                              # the filterbank's own bar (tests/test_emul_fbank.py, tests/test_gpu_fbank.py)

# The whole chain (reverberation, two noises, level="input") against the float64 restatement: the worst
# max |y - y64| / max |y64| over the utterances of `chain_batch`, float32 and int16.
# Measured through the host emulator: 9.7e-7 (float32; int16 8.3e-7); on the MI355X: 9.7e-7 and 8.3e-7, every utterance
# equal to the emulator's to the printed digits (the MFMA is the emulator's fmaf chain bit for bit).  No a-priori bound is
# fixed here: the float32 powers differ from the float64 ones by the convolution's own error.
# The bar is 3 x the larger, rounded up to one significant digit (the margin E2E_TOL_DB of tests/resample_bodies.py keeps).
CHAIN_TOL_REL = 3e-6


@dataclass
class Ctx:
    features: object
    dev: str
    lib: object

    def t(self, x):
        return torch.from_numpy(np.array(x)).to(self.dev)            # a copy: the shared cases are read-only

    def bank(self, clips):
        return self.features.SampleBank(clips, device=self.dev)


def plan_counts(lib):
    """(outputs per tile, taps per pass) of the plan entry"""
    counts = np.zeros(4, np.int64)
    one = np.array([1], np.int64)
    assert lib.raw("ds_augment_plan")(one.ctypes.data, 1, None, counts.ctypes.data) == 0
    assert counts[:2].tolist() == [1, 1]
    return int(counts[2]), int(counts[3])


def split(out, lens):
    y = out.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(lens)])
    assert len(y) == off[-1]
    return [y[off[u]:off[u + 1]] for u in range(len(lens))]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def with_delays(bank, delays):
    """the bank with the delays a case asks for (the bank's own is the first maximum of |h|)"""
    bank.delay = np.asarray(delays, np.int64)
    return bank


# ---- 1. exact integers ----
def integer_cases(tile, k_chunk):
    """(K, n, p) from the cross of the boundary sizes, every third combination, the delay cycling with it, plus the case
    in which all three are at their largest"""
    Ks = [1, 2, 31, 32, 33, 63, 64, 65, k_chunk - 1, k_chunk, k_chunk + 1, 2 * k_chunk + 1]
    cases = []
    for iK, K in enumerate(Ks):
        ns = [1, 2, 31, 33, K - 1, tile - 1, tile, tile + 1, 2 * tile + 1]
        ps = [0, K // 2, K - 1]
        for i_n, n in enumerate(ns):
            if (iK + i_n) % 3 == 0 and n >= 1:
                cases.append((K, n, ps[(iK + 2 * i_n) % 3]))
    cases.append((Ks[-1], 2 * tile + 1, Ks[-1] - 1))
    out = []
    for c in cases:
        if c not in out:
            out.append(c)
    return out


def exact_integers(ctx, dtype):
    F = ctx.features
    tile, k_chunk = plan_counts(ctx.lib)
    cases = integer_cases(tile, k_chunk)
    assert 24 <= len(cases) <= 60 and (2 * k_chunk + 1, 2 * tile + 1, 2 * k_chunk) in cases
    assert max(K * n for K, n, _ in cases) <= 1.1e7
    rs = np.random.RandomState(11)
    xs = [rs.randint(-8, 9, n) for _, n, _ in cases]
    hs = [rs.randint(-4, 5, K) for K, _, _ in cases]
    if dtype == "int16":
        wave, unit = [ctx.t(x.astype(np.int16)) for x in xs], 32768.0
    else:
        wave, unit = [ctx.t(x.astype(np.float32)) for x in xs], 1.0
    bank = with_delays(ctx.bank([h.astype(np.float32) for h in hs]), [p for _, _, p in cases])
    plan = F.AugmentPlan(rir_bank=bank, rir_index=np.arange(len(cases)), level="none")
    out, lens = F.augment(wave, plan)
    assert lens.tolist() == [n for _, n, _ in cases]
    for (K, n, p), x, h, y in zip(cases, xs, hs, split(out, lens)):
        want = np.convolve(x.astype(np.int64), h.astype(np.int64))[p:p + n]
        assert np.array_equal(y.astype(np.float64) * unit, want.astype(np.float64)), (K, n, p)


# ---- 2. values ----
VALUE_CASES = ((5000, 700, None, "ar"), (4173, 2048, None, "noise"), (3000, 3001, 1500, "ar"), (2500, 4000, 0, "noise"))


@functools.lru_cache(maxsize=None)
def value_case(i, dtype):
    n, K, direct, kind = VALUE_CASES[i]
    x = FR.synthetic_audio(4100 + i, n, kind=kind)
    if dtype == "int16":
        x = FR.int16_quantised(x)
    h = A.decaying_rir(4200 + i, K, direct)
    ref, scale = A.reverb(x, h), A.abs_convolution(x, h)
    for a in (x, h, ref, scale):
        a.setflags(write=False)
    return x, h, ref, scale


def values(ctx, i, dtype):
    F = ctx.features
    n, K, direct, _ = VALUE_CASES[i]
    assert n * K <= 1.0e7
    x, h, ref, scale = value_case(i, dtype)
    bank = ctx.bank([h])
    assert bank.delay.tolist() == [A.delay(h)] == [K // 16 if direct is None else direct]
    out, lens = F.augment([ctx.t(x)], F.AugmentPlan(rir_bank=bank, rir_index=np.array([0]), level="none"))
    assert out.dtype == torch.float32 and lens.tolist() == [n]
    err = np.abs(out.cpu().numpy() - ref)
    bound = A.gamma(K) * scale
    worst = int(np.argmax(err - bound))
    print(f"reverb n {n} K {K} p {bank.delay[0]} {dtype}: max abs error {err.max():.3e}, bound there "
          f"{bound[int(np.argmax(err))]:.3e}, largest error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all(), (worst, err[worst], bound[worst])


# ---- 3. mixing alone ----
@functools.lru_cache(maxsize=None)
def mix_batch(J):
    """(utterances, clips, index, start, snr): wrap-around, a start at a clip's last sample, +-0 / 20 / -5 dB, a silent
    clip, a silent utterance, entries without a noise"""
    tile = 4096
    xs = [FR.synthetic_audio(5000, 3000, kind="ar"), FR.int16_quantised(FR.synthetic_audio(5001, tile + 1, kind="noise")),
          np.zeros(700, np.float32), FR.synthetic_audio(5002, 1, kind="dc"), FR.synthetic_audio(5003, 2 * tile + 5, kind="ar")]
    xs = [x if x.dtype == np.float32 else (x.astype(np.float32) / np.float32(32768)) for x in xs]
    clips = [FR.synthetic_audio(5100, 700, kind="noise"), FR.synthetic_audio(5101, 5000, kind="chirp"),
             np.zeros(300, np.float32), FR.synthetic_audio(5102, 1, kind="dc"),
             FR.int16_quantised(FR.synthetic_audio(5103, 257, kind="tone"))]
    lens = [len(c) for c in clips]
    rs = np.random.RandomState(50 + J)
    snrs = (0.0, -0.0, 20.0, -5.0)
    index = rs.randint(0, len(clips), (len(xs), J))
    start = np.array([[rs.randint(0, lens[c]) for c in row] for row in index])
    snr = np.array(snrs)[rs.randint(0, 4, index.shape)]
    index[0, 0], start[0, 0], snr[0, 0] = 0, lens[0] - 1, 20.0          # wraps after one sample
    index[1, 0], start[1, 0], snr[1, 0] = 2, 0, 0.0                     # a silent clip
    index[4, 0], start[4, 0], snr[4, 0] = 4, lens[4] - 1, -5.0          # shorter than a pass of the kernel
    index[3, -1], snr[3, -1] = 1, -0.0
    if J > 1:
        index[0, 1] = -1                                                # no noise in this slot
        index[4, J - 1], start[4, J - 1], snr[4, J - 1] = 0, 13, 0.0
    for a in xs + clips:
        a.setflags(write=False)
    return xs, clips, index, start, snr


def mixing(ctx, J):
    F = ctx.features
    xs, clips, index, start, snr = mix_batch(J)
    bank = ctx.bank(clips)
    assert np.array_equal(bank.mean_square, [A.mean_square(c) for c in clips])
    plan = F.AugmentPlan(noise_bank=bank, noise_index=index, noise_start=np.where(index >= 0, start, 0), snr_db=snr,
                         level="none")
    out, lens = F.augment([ctx.t(x) for x in xs], plan)
    worst = 0.0
    for u, (x, y) in enumerate(zip(xs, split(out, lens))):
        noises = [(clips[index[u, j]], start[u, j], snr[u, j]) for j in range(J) if index[u, j] >= 0]
        r = A.to_float64(x)
        ref = A.mix(r, noises)
        size = np.abs(r) + sum((abs(g) * np.abs(v) for g, v in A.noise_terms(r, noises)), np.zeros(len(r)))
        bound = (J + 2) * A.U * size
        err = np.abs(y - ref)
        assert np.isfinite(y).all(), u
        assert (err <= bound).all(), (J, u, float(err.max()))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    assert not split(out, lens)[2].any()                                # the silent utterance stays silent
    print(f"mixing J {J}: largest error / bound {worst:.3f}")


def realised_snr(ctx):
    """The noise power of the rule is the WHOLE clip's: an utterance of three whole periods of the clip, from any start,
    carries exactly that power, and the ratio of the powers of r and of y - r (float64, from the outputs) is the one
    asked for up to the float32 roundings of g and of y: relative 2^-24 |y| / |y - r| on the noise, under 1e-5 dB here."""
    F = ctx.features
    clip = FR.synthetic_audio(5200, 1000, kind="noise")
    x = FR.synthetic_audio(5201, 3000, kind="ar")
    asked = np.array([[0.0], [20.0], [-5.0], [-0.0]])
    plan = F.AugmentPlan(noise_bank=ctx.bank([clip]), noise_index=np.zeros((4, 1), np.int64),
                         noise_start=np.array([[0], [999], [17], [500]]), snr_db=asked, level="none")
    out, lens = F.augment([ctx.t(x)] * 4, plan)
    r = x.astype(np.float64)
    for want, y in zip(asked[:, 0], split(out, lens)):
        got = 10.0 * np.log10(np.mean(r ** 2) / np.mean((y.astype(np.float64) - r) ** 2))
        print(f"asked for {want:+.1f} dB, realised {got:+.7f} dB")
        assert abs(got - want) <= 1e-4, (want, got)


# ---- 4. the whole chain and the level ----
@functools.lru_cache(maxsize=None)
def chain_batch(dtype):
    shapes = ((4000, 1500), (4097, 600), (2000, 33))
    xs = [FR.synthetic_audio(6000 + i, n, kind=("ar", "noise")[i % 2]) for i, (n, _) in enumerate(shapes)]
    if dtype == "int16":
        xs = [FR.int16_quantised(x) for x in xs]
    hs = [A.decaying_rir(6100 + i, K) for i, (_, K) in enumerate(shapes)]
    clips = [FR.synthetic_audio(6200, 900, kind="noise"), FR.synthetic_audio(6201, 7000, kind="ar")]
    index = np.array([[0, 1], [1, -1], [1, 0]])
    start = np.array([[899, 100], [6999, 0], [5, 450]])
    snr = np.array([[10.0, 3.0], [0.0, 0.0], [15.0, -5.0]])
    refs = []
    for u, (x, h) in enumerate(zip(xs, hs)):
        noises = [(clips[index[u, j]], start[u, j], snr[u, j]) for j in range(2) if index[u, j] >= 0]
        refs.append(A.augment(x, h, noises, "input"))
    for a in xs + hs + clips + refs:
        a.setflags(write=False)
    return xs, hs, clips, index, start, snr, refs


def chain(ctx, dtype):
    F = ctx.features
    xs, hs, clips, index, start, snr, refs = chain_batch(dtype)
    plan = F.AugmentPlan(rir_bank=ctx.bank(hs), rir_index=np.arange(3), noise_bank=ctx.bank(clips), noise_index=index,
                         noise_start=start, snr_db=snr)
    assert plan.level == "input"
    out, lens = F.augment([ctx.t(x) for x in xs], plan)
    worst = 0.0
    for x, y, ref in zip(xs, split(out, lens), refs):
        rel = float(np.abs(y - ref).max() / np.abs(ref).max())
        p_x, p_y = float(np.mean(A.to_float64(x) ** 2)), float(np.mean(y.astype(np.float64) ** 2))
        print(f"chain {dtype} n {len(x)}: max |y - y64| / max |y64| {rel:.3e}, power out / in - 1 {p_y / p_x - 1:+.2e}")
        assert abs(p_y / p_x - 1.0) <= 1e-5
        worst = max(worst, rel)
    print(f"chain {dtype}: worst relative error {worst:.3e}, bar {CHAIN_TOL_REL:.0e}")
    assert worst <= CHAIN_TOL_REL, worst


# ---- 5. identity ----
def identity(ctx):
    F = ctx.features
    x = FR.synthetic_audio(1, 5000, kind="ar")
    q = FR.int16_quantised(FR.synthetic_audio(2, 4097, kind="noise"))
    qf = q.astype(np.float32) / np.float32(32768)
    for level in ("input", "none"):
        out, lens = F.augment([ctx.t(x)], F.AugmentPlan(level=level))                    # an empty plan
        assert out.dtype == torch.float32 and lens.tolist() == [5000]
        np.testing.assert_array_equal(out.cpu().numpy(), x)
        out, _ = F.augment([ctx.t(q)], F.AugmentPlan(level=level))
        np.testing.assert_array_equal(out.cpu().numpy(), qf)
        unit = F.AugmentPlan(rir_bank=ctx.bank([np.ones(1, np.float32)]), rir_index=np.array([0]), level=level)
        out, _ = F.augment([ctx.t(x)], unit)                                             # h = [1.0]
        np.testing.assert_array_equal(out.cpu().numpy(), x)
        out, _ = F.augment([ctx.t(q)], unit)
        np.testing.assert_array_equal(out.cpu().numpy(), qf)
    # only some utterances have an impulse response: the others are their input
    xs = [FR.synthetic_audio(10 + i, n, kind="noise") for i, n in enumerate((700, 4096, 33, 5000))]
    h = A.decaying_rir(3, 200)
    for level in ("input", "none"):
        plan = F.AugmentPlan(rir_bank=ctx.bank([h]), rir_index=np.array([-1, 0, -1, 0]), level=level)
        out, lens = F.augment([ctx.t(v) for v in xs], plan)
        ys = split(out, lens)
        for u in (0, 2):
            np.testing.assert_array_equal(ys[u], xs[u])
        for u in (1, 3):
            assert np.abs(ys[u] - xs[u]).max() > 1e-3


# ---- 6. deterministic and batch-invariant ----
def subplan(F, plan, rows):
    pick = lambda a: None if a is None else np.asarray(a)[rows]
    return F.AugmentPlan(plan.rir_bank, pick(plan.rir_index), plan.noise_bank, pick(plan.noise_index),
                         pick(plan.noise_start), pick(plan.snr_db), plan.level)


def deterministic(ctx):
    F = ctx.features
    rs = np.random.RandomState(5)
    n_utt = 6
    xs = [ctx.t(FR.synthetic_audio(300 + i, int(rs.randint(1, 9000)), kind=("noise", "ar")[i % 2])) for i in range(n_utt)]
    rirs = ctx.bank([A.decaying_rir(310 + i, K) for i, K in enumerate((40, 130, 513))])
    noise = ctx.bank([FR.synthetic_audio(320 + i, n, kind="noise") for i, n in enumerate((333, 20000))])
    plan = F.draw_augmentation(np.random.RandomState(6), n_utt, rirs, noise, p_rir=0.7, p_noise=0.8, snr_db=(0, 20),
                               noises=(1, 2))
    assert (plan.rir_index >= 0).any() and (plan.noise_index >= 0).any() and plan.noise_index.shape == (n_utt, 2)
    a, lens = F.augment(xs, plan)
    b, _ = F.augment(xs, plan)
    assert torch.equal(a, b) and lens.tolist() == [len(x) for x in xs]
    off = np.concatenate([[0], np.cumsum(lens)])
    for u in range(n_utt):
        alone, n1 = F.augment([xs[u]], subplan(F, plan, [u]))
        assert n1.tolist() == [lens[u]]
        assert torch.equal(alone, a[off[u]:off[u + 1]]), u
    order = [4, 0, 5, 2]                                                 # another batch, another order
    c, lens_c = F.augment([xs[u] for u in order], subplan(F, plan, order))
    for y, u in zip(split(c, lens_c), order):
        assert np.array_equal(bits(y), bits(a[off[u]:off[u + 1]].cpu().numpy())), u
    packed, lens2 = F.augment(torch.cat(xs), plan, lengths=[len(x) for x in xs])
    assert torch.equal(packed, a) and lens2.tolist() == lens.tolist()


def drawing(ctx):
    """draw_augmentation: reproducible from the seed, inside the banks, and valid for augment"""
    F = ctx.features
    rirs = ctx.bank([A.decaying_rir(i, 50 + i) for i in range(3)])
    noise = ctx.bank([FR.synthetic_audio(i, 100 + 50 * i, kind="noise") for i in range(4)])
    p1 = F.draw_augmentation(np.random.RandomState(1), 200, rirs, noise, p_rir=0.5, p_noise=0.6, snr_db=(5, 15), noises=(1, 3))
    p2 = F.draw_augmentation(np.random.RandomState(1), 200, rirs, noise, p_rir=0.5, p_noise=0.6, snr_db=(5, 15), noises=(1, 3))
    for name in ("rir_index", "noise_index", "noise_start", "snr_db"):
        assert np.array_equal(getattr(p1, name), getattr(p2, name)), name
    assert p1.rir_index.shape == (200,) and p1.noise_index.shape == p1.noise_start.shape == p1.snr_db.shape == (200, 3)
    assert 60 <= (p1.rir_index >= 0).sum() <= 140 and set(p1.rir_index.tolist()) == {-1, 0, 1, 2}
    on = p1.noise_index >= 0
    per_utt = on.sum(1)
    assert set(per_utt.tolist()) == {0, 1, 2, 3} and 80 <= (per_utt > 0).sum() <= 160
    assert (on[:, :-1] >= on[:, 1:]).all()                               # the used slots come first
    assert ((p1.noise_start >= 0) & (p1.noise_start < noise.lengths[np.maximum(p1.noise_index, 0)]))[on].all()
    assert ((p1.snr_db >= 5) & (p1.snr_db <= 15))[on].all()
    empty = F.draw_augmentation(np.random.RandomState(1), 7)
    assert empty.rir_index is None and empty.noise_index is None and empty.level == "input"
    out, lens = F.augment([ctx.t(FR.synthetic_audio(9, 50, kind="noise"))] * 200, p1)
    assert lens.tolist() == [50] * 200 and bool(torch.isfinite(out).all())


# ---- 7. end to end ----
@functools.lru_cache(maxsize=None)
def e2e_case():
    xs = [FR.synthetic_audio(7000, 16000, kind="ar"), FR.synthetic_audio(7001, 9000, kind="noise")]
    hs = [A.decaying_rir(7100, 500), A.decaying_rir(7101, 300)]
    clips = [FR.synthetic_audio(7200, 4000, kind="noise")]
    index, start, snr = np.array([[0], [0]]), np.array([[100], [3999]]), np.array([[10.0], [5.0]])
    refs = [FR.mk_mfb(A.augment(x, h, [(clips[0], start[u, 0], snr[u, 0])], "input").astype(np.float32))
            for u, (x, h) in enumerate(zip(xs, hs))]
    for a in xs + hs + clips + refs:
        a.setflags(write=False)
    return xs, hs, clips, index, start, snr, refs


def end_to_end(ctx):
    F = ctx.features
    xs, hs, clips, index, start, snr, refs = e2e_case()
    plan = F.AugmentPlan(rir_bank=ctx.bank(hs), rir_index=np.arange(2), noise_bank=ctx.bank(clips), noise_index=index,
                         noise_start=start, snr_db=snr)
    wave = [ctx.t(x) for x in xs]
    a, off = F.log_mel_fbank(wave, augment=plan)
    packed, lens = F.augment(wave, plan)
    b, off_b = F.log_mel_fbank(packed, lengths=lens)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and off.tolist() == off_b.tolist()
    feats = a.cpu().numpy()
    for u, ref in enumerate(refs):
        err = float(np.abs(feats[off[u]:off[u + 1]] - ref).max())
        print(f"augment + fbank, utterance {u}: max abs error {err:.3e} dB, bar {FBANK_TOL_DB:.0e}")
        assert err <= FBANK_TOL_DB, (u, err)
    # without the keyword: as before
    c, _ = F.log_mel_fbank(wave)
    d, _ = F.log_mel_fbank(wave, augment=None)
    assert torch.equal(c.view(torch.int32), d.view(torch.int32)) and not torch.equal(a, c)


def store_composition(ctx):
    """FeatureStore.from_waveforms(orig_rate=, vad=, augment=) is resample, then augment, then the features with vad"""
    from deepspeaker_pytorch_amd import data
    F = ctx.features
    x48 = []
    for i, n in enumerate((24000, 30000)):
        x = FR.synthetic_audio(40 + i, n, 48000, "ar")
        x[n // 3:n // 2] *= 1e-4                                           # a pause for the voice-activity decision
        x48.append(ctx.t(x))
    plan = F.AugmentPlan(rir_bank=ctx.bank([A.decaying_rir(45, 400)]), rir_index=np.array([0, -1]),
                         noise_bank=ctx.bank([FR.synthetic_audio(46, 3000, kind="quiet_noise")]),
                         noise_index=np.array([[-1], [0]]), noise_start=np.array([[0], [7]]), snr_db=np.array([[0.0], [25.0]]))
    vad = F.VadConfig()
    store = data.FeatureStore.from_waveforms(x48, orig_rate=48000, vad=vad, augment=plan)
    packed, lens = F.resample(x48, 48000)
    packed, lens = F.augment(packed, plan, lengths=lens)
    want, off = F.log_mel_fbank(packed, lengths=lens, vad=vad)
    assert torch.equal(store.features.view(torch.int32), want.view(torch.int32)) and store.offsets.tolist() == off.tolist()
    full, off_full = F.log_mel_fbank(packed, lengths=lens)
    assert 0 < off[-1] < off_full[-1] and len(store) == 2                # the decision dropped frames, not everything
    plain = data.FeatureStore.from_waveforms(x48, orig_rate=48000, vad=vad)
    assert not torch.equal(plain.features, store.features) or plain.offsets.tolist() != store.offsets.tolist()


# ---- 8. errors ----
def abi_errors(ctx):
    lib = ctx.lib
    counts = np.zeros(4, np.int64)
    plan = lambda lens: lib.raw("ds_augment_plan")(lens.ctypes.data, len(lens), None, counts.ctypes.data)
    assert plan(np.array([100, 0], np.int64)) == -1                          # a zero-length utterance
    assert lib.raw("ds_augment_plan")(None, 1, None, counts.ctypes.data) == -3
    assert lib.raw("ds_augment_plan")(np.array([5], np.int64).ctypes.data, 1, None, None) == -3
    assert lib.raw("ds_augment_plan")(np.array([5], np.int64).ctypes.data, 0, None, counts.ctypes.data) == -1
    tile, k_chunk = plan_counts(lib)
    assert tile % 32 == 0 and k_chunk % 32 == 0
    assert plan(np.array([tile, tile + 1, 1], np.int64)) == 0 and counts.tolist() == [2 * tile + 2, 4, tile, k_chunk]
    table = np.zeros(2 * 4 + 4, np.int64)
    lens = np.array([tile, tile + 1, 1], np.int64)
    assert lib.raw("ds_augment_plan")(lens.ctypes.data, 3, table.ctypes.data, counts.ctypes.data) == 0
    assert table.tolist() == [0, tile, 2 * tile + 1, 2 * tile + 2, 0, 1, 3, 4, 0, 1, 1, 2]
    assert lib.raw("ds_augment_workspace_bytes")(4) == 4 * 3 * 8 and lib.raw("ds_augment_workspace_bytes")(0) == 0
    # the launch entries validate before they touch anything: placeholders stand for the buffers
    p = np.zeros(4, np.int64).ctypes.data
    reverb = lib.raw("ds_augment_reverb_f32")
    assert reverb(None, 0, p, 1, 1, p, p, 8, p, p, None) == -3
    assert reverb(p, 0, None, 1, 1, p, p, 8, p, p, None) == -3
    assert reverb(p, 0, p, 1, 1, p, p, 8, None, p, None) == -3
    assert reverb(p, 0, p, 1, 1, p, p, 8, p, None, None) == -3
    assert reverb(p, 0, p, 1, 1, p, None, 8, p, p, None) == -3               # a bank without its table
    assert reverb(p, 0, p, 1, 1, None, p, 8, p, p, None) == -3
    assert reverb(p, 0, p, 0, 1, p, p, 8, p, p, None) == -1                  # n_utt = 0
    assert reverb(p, 0, p, -1, 1, p, p, 8, p, p, None) == -1
    assert reverb(p, 0, p, 1, 0, p, p, 8, p, p, None) == -1
    assert reverb(p, 0, p, 1, 1, p, p, -1, p, p, None) == -1
    assert reverb(p, 2, p, 1, 1, p, p, 8, p, p, None) == -4                  # neither f32 nor int16
    assert reverb(p, 0, p, 1, 1, p, p, 65537, p, p, None) == -4              # K above the cap
    mix = lib.raw("ds_augment_mix_f32")
    assert mix(None, p, 1, 1, p, p, 1, p, None) == -3 and mix(p, p, 1, 1, None, p, 1, p, None) == -3
    assert mix(p, p, 1, 1, p, None, 1, p, None) == -3 and mix(p, p, 1, 1, p, p, 1, None, None) == -3
    assert mix(p, p, 0, 1, p, p, 1, p, None) == -1 and mix(p, p, 1, 1, p, p, 0, p, None) == -1
    assert mix(p, p, 1, 1, p, p, 9, p, None) == -4
    level = lib.raw("ds_augment_level_f32")
    assert level(None, p, 1, 1, 0, p, None) == -3 and level(p, None, 1, 1, 0, p, None) == -3
    assert level(p, p, 1, 1, 0, None, None) == -3 and level(p, p, 0, 1, 0, p, None) == -1
    assert level(p, p, 1, 1, 2, p, None) == -4


def python_errors(ctx):
    from deepspeaker_pytorch_amd._native import DeepSpeakerHipError
    F = ctx.features
    x = [ctx.t(np.zeros(1000, np.float32)), ctx.t(np.ones(500, np.float32))]
    rirs = ctx.bank([A.decaying_rir(1, 30), A.decaying_rir(2, 40)])
    noise = ctx.bank([FR.synthetic_audio(1, 100, kind="noise"), FR.synthetic_audio(2, 50, kind="noise")])
    ok = dict(noise_bank=noise, noise_index=np.array([[0], [1]]), noise_start=np.array([[99], [0]]),
              snr_db=np.array([[10.0], [0.0]]))
    F.augment(x, F.AugmentPlan(rir_bank=rirs, rir_index=np.array([1, -1]), **ok))        # the valid plan runs
    bad = [
        dict(rir_bank=rirs, rir_index=np.array([0])),                                   # wrong table shapes
        dict(rir_bank=rirs, rir_index=np.array([[0, 0]])),
        dict(rir_bank=rirs, rir_index=np.array([0.0, 1.0])),
        dict(ok, noise_index=np.array([0, 1])),
        dict(ok, noise_start=np.array([[99, 0], [0, 0]])),
        dict(ok, snr_db=np.array([10.0, 0.0])),
        dict(ok, noise_index=np.zeros((3, 1), np.int64)),
        dict(ok, snr_db=None),
        dict(rir_bank=rirs, rir_index=np.array([0, 2])),                                # an index outside its bank
        dict(rir_bank=rirs, rir_index=np.array([-2, 0])),
        dict(ok, noise_index=np.array([[0], [2]])),
        dict(ok, noise_start=np.array([[100], [0]])),                                   # a start outside its clip
        dict(ok, noise_start=np.array([[0], [-1]])),
        dict(ok, snr_db=np.array([[np.nan], [0.0]])),
        dict(noise_bank=noise, noise_index=np.zeros((2, 9), np.int64), noise_start=np.zeros((2, 9), np.int64),
             snr_db=np.zeros((2, 9))),                                                  # J > MAX_NOISES
        dict(ok, level="peak"),                                                         # an unknown level
        dict(rir_index=np.array([0, 1])),                                               # an index without a bank
        dict(ok, noise_bank=None),
    ]
    assert F.MAX_NOISES == A.MAX_NOISES == 8
    for kw in bad:
        with pytest.raises(ValueError):
            F.augment(x, F.AugmentPlan(**kw))
    with pytest.raises(ValueError):
        F.augment(x, None)
    with pytest.raises(ValueError):
        F.log_mel_fbank(x, augment="reverb")
    for clips in ([], [np.zeros(0, np.float32)], [np.ones(3, np.float32), np.zeros(0, np.float32)], [np.ones((2, 2), np.float32)],
                  [np.ones(3, np.float64)], np.ones(3, np.float32)):
        with pytest.raises(ValueError):                                                 # an empty clip, a wrong clip
            ctx.bank(clips)
    if ctx.dev != "cpu":                                                                # a bank on another device
        host = F.SampleBank([A.decaying_rir(1, 30)], device="cpu")
        with pytest.raises(ValueError, match="bank is on"):
            F.augment(x, F.AugmentPlan(rir_bank=host, rir_index=np.array([0, 0])))
    else:
        meta = F.SampleBank([A.decaying_rir(1, 30)], device="meta")
        with pytest.raises(ValueError, match="bank is on"):
            F.augment(x, F.AugmentPlan(rir_bank=meta, rir_index=np.array([0, 0])))
    with pytest.raises(DeepSpeakerHipError, match="unsupported|not supported"):         # K above the cap
        F.augment(x, F.AugmentPlan(rir_bank=ctx.bank([np.ones(F.MAX_RIR_TAPS + 1, np.float32)]), rir_index=np.array([0, -1])))
    with pytest.raises(DeepSpeakerHipError, match="bad shape"):
        F.augment([x[0], ctx.t(np.zeros(0, np.float32))], F.AugmentPlan())
    for kw in (dict(n_utt=0), dict(n_utt=3, p_rir=1.5), dict(n_utt=3, noises=(0, 1)), dict(n_utt=3, noises=(2, 9)),
               dict(n_utt=3, snr_db=(5.0, 1.0))):
        with pytest.raises(ValueError):
            F.draw_augmentation(np.random.RandomState(0), rir_bank=rirs, noise_bank=noise, **kw)
