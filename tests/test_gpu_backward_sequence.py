"""The launch sequence of the backward pass on the device: the one the host emulator recorded
(tests/golden/backward_launch_sequences.json, backward_sequence_cases.py), and which stream every launch goes to."""
import pytest
import torch

from backward_sequence_cases import load_fixture, run_pass

pytestmark = pytest.mark.gpu

# the leaves of the pass that the filter-gradient lane takes off the main stream (backward._FilterGradLane); the fc
# filter gradient (ds_conv_wgrad_f32 over a 1x1 shape, enqueued before the lane's first fork) stays on the main stream
CONV_FILTER_GRADIENTS = ("ds_conv_wgrad_bf16", "ds_conv_wgrad_f16", "ds_conv_wgrad_c1_f16", "ds_conv_wgrad_f32")


@pytest.mark.parametrize("name,lane", [("bf16x3_group_fused", True), ("f16_group", True), ("bf16x3_group_fused", False)])
def test_device_backward_is_the_recorded_sequence_on_the_right_streams(name, lane):
    from deepspeaker_pytorch_amd.model import get_engine
    seq, grads = run_pass(get_engine(), name, device="cuda", overlap_filter_gradients=lane, tag_streams=True)
    want = load_fixture()[name]
    assert [c[1:] for c in seq] == want
    for tag, entry, *args in seq:
        conv = entry in CONV_FILTER_GRADIENTS and args[0][5] in (3, 5)      # ConvShape.KS; the fc gradient's shape has 1
        side = lane and conv
        assert tag == ("side" if side else "main"), (tag, entry, args[0])
    if lane:
        on_side = {c[1] for c in seq if c[0] == "side"}
        assert on_side == ({"ds_conv_wgrad_bf16", "ds_conv_wgrad_f32"} if name.startswith("bf16x3")
                           else {"ds_conv_wgrad_f16", "ds_conv_wgrad_c1_f16"})
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
