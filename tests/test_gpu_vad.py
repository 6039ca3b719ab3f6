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
    B.direct(ctx, conf, dtype)


def test_chain_from_stereo_44100(ctx):
    B.chain(ctx)


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
