"""The latency plan mode of the bf16x3 forward convolution on the device: the bodies of bf16_latency_cases.py (shared with
test_emul_bf16_latency.py) plus the end-to-end checks that need a GPU.  All checks are bitwise.

    - ds_conv_fwd_bf16 with DS_CONV_PLAN_LATENCY == without, for the network's seven stage convolutions at B = 1 and 3
    - each latency row (64 x 64, 32 x 128) forced, 3x3 and 5x5, ragged and image-spanning tiles included
    - the plan mode: 12 rows of the 512-channel layer -> a latency row, 768 rows -> today's plan
    - forward_eval_planned(bf16x3) of 12 utterances with low_latency == without
    - select_triplets on 8 triplets of 32 frames: indices, d_p, d_n and the observed fp16 error identical whether the
      slot forward is planned for latency or not"""
import numpy as np
import pytest
import torch

import bf16_latency_cases as LC
import deepspeaker_oracle as O
from test_gpu_bf16_train_kernels import GpuBackend
from test_gpu_train_f16_kernels import eng     # noqa: F401  (the module-scoped engine fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be(eng):
    return GpuBackend(eng)


@pytest.mark.parametrize("b", LC.BATCHES)
@pytest.mark.parametrize("geom", LC.GEOMETRIES)
def test_flag_is_bit_identical(be, geom, b):
    LC.body_flag_is_bit_identical(be, geom, b)


@pytest.mark.parametrize("cfg", sorted(LC.LAT_ROWS))
@pytest.mark.parametrize("geom,b", LC.FORCED_CASES)
def test_forced_latency_row_is_bit_identical(be, geom, b, cfg):
    LC.body_forced_row_is_bit_identical(be, geom, b, cfg)


def test_plan_mode(be):
    LC.body_plan_mode(be.lib)


def test_forward_eval_low_latency_is_bit_identical(eng):
    from deepspeaker_pytorch_amd.engine import Engine
    sd = O.make_state_dict(seed=23, num_classes=4)
    tsd = {k: torch.from_numpy(np.array(v)).cuda() for k, v in sd.items()}
    x = torch.from_numpy(O.make_input(seed=3, batch=12, frames=160)).cuda()
    LC.body_forward_eval(Engine(eng.lib), x, tsd)        # (an engine of its own: the body counts its cached plans)


def test_select_triplets_same_with_and_without():
    """8 triplets of 32 frames, 4 refinement slots (a 12-row slot forward), two models from the same weights (each with
    a fresh refinement policy, so both calls place their probes alike)"""
    from deepspeaker_pytorch_amd import mining
    from deepspeaker_pytorch_amd.model import DeepSpeakerModel
    sd = O.make_state_dict(seed=31, num_classes=8)
    xs = [torch.from_numpy(O.make_input(seed=40 + i, batch=8, frames=32)).cuda() for i in range(3)]
    got = {}
    saved = mining.REFINE_LOW_LATENCY
    try:
        for low in (False, True):
            mining.REFINE_LOW_LATENCY = low
            m = DeepSpeakerModel(512, 8, precision="f16")
            m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
            m = m.cuda().eval()
            with torch.no_grad():
                e = [m(x).clone() for x in xs]
                # a band wide enough that near ties fill the slots: re-embedded rows decide the distances handed out
                sel = mining.select_triplets(*e, margin=0.1, model=m, inputs=xs, cap=4, band=0.05)
            got[low] = (sel.indices.cpu(), sel.d_p.cpu(), sel.d_n.cpu(), sel.observed_error, sel.n_near_ties,
                        sel.refined_all)
            print(f"low_latency={low}: {len(got[low][0])} selected, {got[low][4]} near ties, fell back {got[low][5]}, "
                  f"observed error {got[low][3]}")
    finally:
        mining.REFINE_LOW_LATENCY = saved
    a, b = got[False], got[True]
    # the slot forward decided the distances handed out: near ties within the 4 slots, no whole-batch fallback (which
    # never asks for the latency mode), and probe slots whose fp16 error was read back
    for g in (a, b):
        assert not g[5] and 0 < g[4] <= 4 and g[3][1] > 0, g[3:]
    assert torch.equal(a[0], b[0])
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
    assert a[3] == b[3] and a[4:] == b[4:]
