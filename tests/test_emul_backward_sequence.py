"""The launch sequence of every backward pass, on the host emulator, against the committed record
(tests/golden/backward_launch_sequences.json; see backward_sequence_cases.py for what is recorded and why)."""
import pytest

from backward_sequence_cases import PASSES, load_fixture, run_pass
from emul_util import emul_lib
from deepspeaker_pytorch_amd.engine import Engine


@pytest.fixture(scope="module")
def fixture_rows():
    return load_fixture()


def test_fixture_has_exactly_the_recorded_passes(fixture_rows):
    assert list(fixture_rows) == list(PASSES)


@pytest.mark.parametrize("name", list(PASSES))
def test_backward_launch_sequence_is_the_recorded_one(name, fixture_rows):
    seq, grads = run_pass(Engine(emul_lib()), name)
    want = fixture_rows[name]
    for k, (got, exp) in enumerate(zip(seq, want)):
        assert got == exp, (name, k, got, exp)
    assert len(seq) == len(want), (name, len(seq), len(want))
    assert len(grads) == 2 + 9 * PASSES[name][2]       # fc weight + bias; per stage 3 filters, 3 x (gamma, beta)


def test_recorder_leaves_the_trace_working():
    lib = emul_lib()
    lib.trace = {}
    try:
        seq, _ = run_pass(Engine(lib), "bf16x3_group_fused")
        counted = dict(lib.trace)
    finally:
        lib.trace = None
    assert "call" not in vars(lib)                     # the instance is as it was
    for name in ("ds_l2norm_scale_bwd_f32", "ds_conv_dgrad_bnbwd_bf16", "ds_bn_bwd_group_finish_f32", "ds_conv_wgrad_bf16"):
        assert counted.get(name, 0) == sum(c[0] == name for c in seq) > 0, name        # (entry points of no forward)
