"""CPU: the polyphase resampler (csrc/resample.hip, features.resample) through the host emulator of the kernels, against
the float64 restatement (tests/resample_reference.py); the restatement itself against SciPy and against the filter's
stated response.  The cases are tests/resample_bodies.py, shared with tests/test_gpu_resample.py."""
import numpy as np
import pytest

import resample_bodies as B
import resample_reference as R
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
def test_restatement_is_scipy():
    signal = pytest.importorskip("scipy.signal")
    rs = np.random.RandomState(0)
    worst = 0.0
    for L, M in ((1, 3), (2, 1), (160, 441), (3, 2), (1, 1), (320, 441), (1, 6), (160, 147)):
        for n in (1, 2, 5, 100, 1501):
            x = rs.randn(n)
            want = signal.resample_poly(x, L, M, window=("kaiser", 5.0))
            got = R.resample(x, L, M)
            assert got.shape == want.shape == (R.n_out(n, L, M),)
            worst = max(worst, float(np.abs(got - want).max()))
    print(f"restatement against scipy.signal.resample_poly: max abs difference {worst:.3e}")
    assert worst <= 1e-12


def _tone_level_db(freq):
    """level change of a 48 kHz tone through 48 -> 16 kHz, from the RMS of the middle of the signal"""
    n = 48000
    x = np.sin(2 * np.pi * freq * np.arange(n) / 48000.0)
    y = R.resample(x, 1, 3)
    return 20 * np.log10(np.sqrt(np.mean(y[2000:-2000] ** 2)) / np.sqrt(0.5))


def test_filter_sanity():
    assert abs(_tone_level_db(1000.0)) <= 0.05
    assert _tone_level_db(10000.0) <= -50.0


def test_table_lengths():
    """taps per output and table length of the ratios the design was sized for"""
    for (L, M), T, length in (((1, 3), 61, 61), ((2, 1), 21, 41), ((160, 441), 56, 8821), ((320, 441), 28, 8821),
                              ((1, 6), 121, 121), ((160, 147), 21, 3201)):
        assert R.n_taps(L, M) == T and len(R.taps(L, M)) == length


def test_product_table_is_the_restatement(ctx):
    """features.resample_taps is the restatement's table with the sinc's zero crossings made exact zeros (np.sinc leaves
    4e-17 there); the polyphase layout holds every tap once, in the order of ascending input index."""
    F = ctx.features
    for L, M in ((1, 3), (2, 1), (160, 441), (640, 441), (1, 1)):
        h, ref = F.resample_taps(L, M), R.taps(L, M)
        assert h.dtype == np.float64 and h.shape == ref.shape and np.abs(h - ref).max() <= 1e-16
        T = R.n_taps(L, M)
        poly = F.polyphase_taps(h, L)
        assert poly.dtype == np.float32 and poly.shape == (L, T | 1)
        for p in (0, L // 2, L - 1):
            want = np.zeros(T)
            col = h[p::L]
            want[:len(col)] = col
            np.testing.assert_array_equal(poly[p, :T], want[::-1].astype(np.float32))
        assert not poly[:, T:].any()
    unit = F.resample_taps(1, 1)
    assert unit[10] == 1.0 and np.count_nonzero(unit) == 1


# ---- the kernel through the emulator ----
@pytest.mark.parametrize("dtype", B.DTYPES)
@pytest.mark.parametrize("rate", B.RATES)
def test_values(ctx, rate, dtype):
    B.values(ctx, rate, dtype)


@pytest.mark.parametrize("dtype", B.DTYPES)
@pytest.mark.parametrize("name", sorted(B.GEOMETRY))
def test_geometry(ctx, name, dtype):
    B.geometry(ctx, name, dtype)


@pytest.mark.parametrize("dtype", B.DTYPES)
@pytest.mark.parametrize("name", B.DIRECT)
def test_guarded_direct_calls(ctx, name, dtype):
    B.direct(ctx, name, dtype)


def test_identity(ctx):
    B.identity(ctx)


def test_deterministic_and_batch_invariant(ctx):
    B.deterministic(ctx, n_max=30000)


def test_zero_padding(ctx):
    B.zero_padding(ctx)


def test_plumbing(ctx):
    B.plumbing(ctx)


@pytest.mark.parametrize("rate", B.E2E_RATES)
def test_end_to_end_against_float64(ctx, rate):
    B.end_to_end(ctx, rate)


def test_end_to_end_to_22050(ctx):
    B.end_to_end(ctx, *B.E2E_22K)


def test_abi_errors(ctx):
    B.abi_errors(ctx)


def test_python_errors(ctx):
    B.python_errors(ctx)
