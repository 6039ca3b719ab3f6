"""MI355X: the waveform augmentation (csrc/augment.hip, features.augment, the augment keyword of log_mel_fbank and
FeatureStore.from_waveforms) against the float64 restatement (tests/augment_reference.py).  The cases are
tests/augment_bodies.py, the same ones tests/test_emul_augment.py runs through the host emulator."""
import pytest

import augment_bodies as B

pytestmark = pytest.mark.gpu


@pytest.fixture
def ctx():
    from deepspeaker_pytorch_amd import features
    from deepspeaker_pytorch_amd.model import get_engine
    return B.Ctx(features, "cuda", get_engine().lib)


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
