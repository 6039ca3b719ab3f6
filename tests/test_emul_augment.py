"""CPU: the waveform augmentation (csrc/augment.hip, features.augment) through the host emulator of the kernels, against
the float64 restatement (tests/augment_reference.py); the restatement's reverberation against SciPy.  The cases are
tests/augment_bodies.py, shared with tests/test_gpu_augment.py."""
import numpy as np
import pytest
import torch

import augment_bodies as B
import augment_reference as A
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
def test_restatement_is_scipy(ctx):
    """step 1 of the restatement against scipy.signal.fftconvolve, at the delay the product's bank fixes and at the two
    extreme ones"""
    signal = pytest.importorskip("scipy.signal")
    rs = np.random.RandomState(0)
    worst = 0.0
    for n, K in ((1, 1), (5, 9), (100, 7), (1501, 400), (300, 1200)):
        x = rs.randn(n).astype(np.float32)
        h = A.decaying_rir(n + K, K)
        assert ctx.bank([h]).delay.tolist() == [A.delay(h)]
        for p in sorted({0, A.delay(h), K - 1}):
            want = signal.fftconvolve(x.astype(np.float64), h.astype(np.float64))[p:p + n]
            got = A.reverb(x, h, p)
            assert got.shape == want.shape == (n,)
            worst = max(worst, float(np.abs(got - want).max()))
    print(f"restatement against scipy.signal.fftconvolve: max abs difference {worst:.3e}")
    assert worst <= 1e-12


def test_restatement_rules(ctx):
    """the delay, the gain and the level of the restatement, on cases small enough to state by hand; the bank's host
    statistics are the restatement's"""
    h = np.array([0.1, -0.5, 1.0, -1.0, 0.2], np.float32)
    assert A.delay(h) == 2                                   # the FIRST maximum of |h|
    bank = ctx.bank([h, np.array([-3, 3, 16384], np.int16)])
    assert bank.delay.tolist() == [2, 2] and bank.offsets.tolist() == [0, 5, 8] and bank.lengths.tolist() == [5, 3]
    assert bank.mean_square.tolist() == [A.mean_square(h), (2 * (3 / 32768) ** 2 + 0.25) / 3]
    assert bank.samples.dtype == torch.float32 and bank.samples[7].item() == 0.5
    x = np.array([1.0, 2.0, 3.0], np.float32)
    assert np.array_equal(A.reverb(x, np.array([0.0, 1.0], np.float32)), x)          # a pure delay is undone
    assert np.array_equal(A.reverb(x, None), x)
    v = np.array([2.0, -2.0], np.float32)                    # power 4; x has power 14/3
    s = A.mix(x.astype(np.float64), [(v, 1, 0.0)])
    g = np.sqrt((14.0 / 3.0) / 4.0)
    np.testing.assert_allclose(s, x + g * np.array([-2.0, 2.0, -2.0]), rtol=1e-15)
    assert np.array_equal(A.mix(x.astype(np.float64), [(np.zeros(4, np.float32), 0, 5.0)]), x)   # a silent clip: gain 0
    y = A.augment(x, None, [(v, 0, 10.0)], "input")
    np.testing.assert_allclose(np.mean(y ** 2), 14.0 / 3.0, rtol=1e-15)
    assert np.array_equal(A.level(np.zeros(3, np.float32), np.zeros(3), "input"), np.zeros(3))


# ---- the kernels through the emulator ----
@pytest.mark.parametrize("dtype", B.DTYPES)
def test_exact_integers(ctx, dtype):
    B.exact_integers(ctx, dtype)


@pytest.mark.parametrize("dtype", B.DTYPES)
@pytest.mark.parametrize("case", range(len(B.VALUE_CASES)))
def test_values(ctx, case, dtype):
    B.values(ctx, case, dtype)


@pytest.mark.parametrize("J", (1, 2, 8))
def test_mixing(ctx, J):
    B.mixing(ctx, J)


def test_realised_snr(ctx):
    B.realised_snr(ctx)


@pytest.mark.parametrize("dtype", B.DTYPES)
def test_chain_and_level(ctx, dtype):
    B.chain(ctx, dtype)


def test_identity(ctx):
    B.identity(ctx)


def test_deterministic_and_batch_invariant(ctx):
    B.deterministic(ctx)


def test_draw_augmentation(ctx):
    B.drawing(ctx)


def test_end_to_end(ctx):
    B.end_to_end(ctx)


def test_store_composition(ctx):
    B.store_composition(ctx)


def test_abi_errors(ctx):
    B.abi_errors(ctx)


def test_python_errors(ctx):
    B.python_errors(ctx)
