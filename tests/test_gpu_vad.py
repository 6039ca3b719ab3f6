"""MI355X: the energy voice-activity decision and the selection of voiced frames (csrc/vad.hip, features.voiced_frames /
select_frames, the vad= keyword of log_mel_fbank and FeatureStore.from_waveforms) against the float64 restatement
(tests/vad_reference.py).  The cases are tests/vad_bodies.py, the same ones tests/test_emul_vad.py runs through the host
emulator."""
import pytest

import vad_bodies as B

pytestmark = pytest.mark.gpu


@pytest.fixture
def ctx():
    from deepspeaker_pytorch_amd import features
    from deepspeaker_pytorch_amd.model import get_engine
    return B.Ctx(features, "cuda", get_engine().lib)


@pytest.mark.parametrize("dtype", B.DTYPES)
@pytest.mark.parametrize("kind", B.KINDS)
def test_energy_values(ctx, kind, dtype):
    B.energy_values(ctx, kind, dtype)


@pytest.mark.parametrize("dtype", B.DTYPES)
@pytest.mark.parametrize("kind", B.KINDS)
def test_decisions(ctx, kind, dtype):
    B.decisions(ctx, kind, dtype)


def test_clipping_and_isolation(ctx):
    B.clipping(ctx)


def test_selection(ctx):
    B.selection(ctx)


@pytest.mark.parametrize("normalize", ["mean", "mean_std"])
def test_normalisation_over_kept_rows(ctx, normalize):
    B.normalisation(ctx, normalize)


def test_vad_none_is_unchanged(ctx):
    B.vad_none_is_unchanged(ctx)


def test_deterministic_and_batch_invariant(ctx):
    B.deterministic(ctx, n_max=60000)


def test_plumbing(ctx):
    B.plumbing(ctx)


def test_abi_errors(ctx):
    B.abi_errors(ctx)


def test_python_errors(ctx):
    B.python_errors(ctx)
