"""CPU: the energy voice-activity decision and the selection of voiced frames (csrc/vad.hip, features.voiced_frames /
select_frames, the vad= keyword) through the host emulator of the kernels, against the float64 restatement
(tests/vad_reference.py); the restatement itself against a direct loop.  The cases are tests/vad_bodies.py, shared with
tests/test_gpu_vad.py."""
import math

import numpy as np
import pytest

import vad_bodies as B
import vad_reference as V
from emul_util import emul_lib

from deepspeaker_pytorch_amd.engine import Engine


@pytest.fixture
def ctx():
    from deepspeaker_pytorch_amd import data, features
    eng = Engine(emul_lib())
    features._engine_override = eng
    data._engine_override = eng
    try:
        yield B.Ctx(features, "cpu", emul_lib())
    finally:
        features._engine_override = None
        data._engine_override = None


# ---- the restatement alone ----
def _direct(x, thr0=5.5, scale=0.5, context=2, prop=0.12, floor=float(np.float32(1.1920929e-07))):
    """section 1 of the rule as loops over frames, samples and window positions"""
    n = len(x)
    T = 1 if n <= 400 else 1 + -(-(n - 400) // 160)
    e = []
    for t in range(T):
        s = 0.0
        for i in range(400):
            g = t * 160 + i
            if g < n:
                v = float(x[g]) * (1.0 if x.dtype == np.int16 else 32768.0)
                s += v * v
        e.append(math.log(max(s, floor)))
    thr = thr0 + scale * (sum(e) / T)
    out = []
    for t in range(T):
        count = size = 0
        for w in range(t - context, t + context + 1):
            if 0 <= w < T:
                size += 1
                count += e[w] > thr
        out.append(count >= prop * size)
    return np.array(e), np.array(out)


def test_restatement_is_the_direct_loop():
    mixed = 0
    for x, cfg in ((B.gated(11, 12000), {}), (B.FR.int16_quantised(B.ramp(12, 9000)), {}),
                   (B.gated(13, 10000), dict(frames_context=0, proportion_threshold=1.0, energy_threshold=7.0))):
        e, m = _direct(x, cfg.get("energy_threshold", 5.5), 0.5, cfg.get("frames_context", 2),
                       cfg.get("proportion_threshold", 0.12))
        assert np.abs(V.log_energy(x) - e).max() <= 1e-12
        assert V.vad(x, **cfg).tolist() == m.tolist()
        mixed += 0 < m.sum() < len(m)
    assert mixed >= 2                                                # both decisions occur


def test_signals_are_what_the_cases_assume():
    """gated: a good two thirds voiced, no frame near its threshold, the int16 copy decides alike"""
    x = B.gated(21, 48000)
    e = V.log_energy(x)
    m = V.decide(e)
    assert 0.6 <= m.mean() <= 0.8 and np.abs(e - V.threshold(e)).min() > 0.5
    assert V.vad(B.FR.int16_quantised(x)).tolist() == m.tolist()


# ---- the kernels through the emulator ----
@pytest.mark.parametrize("dtype", B.DTYPES)
@pytest.mark.parametrize("kind", B.KINDS)
def test_energy_values(ctx, kind, dtype):
    B.energy_values(ctx, kind, dtype)


@pytest.mark.parametrize("dtype", B.DTYPES)
@pytest.mark.parametrize("kind", B.KINDS)
def test_decisions(ctx, kind, dtype):
    B.decisions(ctx, kind, dtype)


@pytest.mark.parametrize("conf,kind,dtype", B.ENERGY_CASES)
def test_energy_values_of_the_table(ctx, conf, kind, dtype):
    B.energy_values(ctx, kind, dtype, conf)


@pytest.mark.parametrize("dtype", B.DTYPES)
@pytest.mark.parametrize("conf", ["16k", "22k"])
def test_energy_at_a_floor_of_one(ctx, conf, dtype):
    B.energy_values(ctx, "silence", dtype, conf, floor=1.0)


@pytest.mark.parametrize("conf,rule,kind,dtype", B.TABLE_CASES)
def test_decisions_of_the_table(ctx, conf, rule, kind, dtype):
    B.decisions(ctx, kind, dtype, conf, rule)


def test_clipping_and_isolation(ctx):
    B.clipping(ctx)


def test_selection(ctx):
    B.selection(ctx)


@pytest.mark.parametrize("normalize", ["mean", "mean_std"])
def test_normalisation_over_kept_rows(ctx, normalize):
    B.normalisation(ctx, normalize)


@pytest.mark.parametrize("normalize", ["mean", "mean_std", None])
@pytest.mark.parametrize("conf", B.NORM_CONFS)
def test_normalisation_across_the_tile_hand_over(ctx, conf, normalize):
    B.normalisation(ctx, normalize, conf)


def test_raw_features_over_kept_rows(ctx):
    B.normalisation(ctx, None)


@pytest.mark.parametrize("dtype", B.DTYPES)
@pytest.mark.parametrize("conf", ["16k", "22k"])
def test_guarded_direct_calls(ctx, conf, dtype):
    B.direct(ctx, conf, dtype, max_frames=1100)


def test_chain_from_stereo_44100(ctx):
    B.chain(ctx)


def test_vad_none_is_unchanged(ctx):
    B.vad_none_is_unchanged(ctx)


def test_deterministic_and_batch_invariant(ctx):
    B.deterministic(ctx, n_max=6000)


def test_plumbing(ctx):
    B.plumbing(ctx)


def test_abi_errors(ctx):
    B.abi_errors(ctx)


def test_python_errors(ctx):
    B.python_errors(ctx)
