"""MI355X: the polyphase resampler (csrc/resample.hip, features.resample, the orig_rate / channels keywords of
log_mel_fbank and FeatureStore.from_waveforms) against the float64 restatement (tests/resample_reference.py).  The cases
are tests/resample_bodies.py, the same ones tests/test_emul_resample.py runs through the host emulator."""
import pytest

import resample_bodies as B

pytestmark = pytest.mark.gpu


@pytest.fixture
def ctx():
    from deepspeaker_pytorch_amd import features
    from deepspeaker_pytorch_amd.model import get_engine
    return B.Ctx(features, "cuda", get_engine().lib)


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
    B.deterministic(ctx, n_max=160000)


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
