"""The pipelined walk of the bf16x3 forward convolution on the device: the bodies of bf16_walk_cases.py (shared with
test_emul_bf16_walk.py).  Pipelined against classic is bitwise on every output element; every pipelined output is also
held to the bf16x3 bar against float64.

    - every row with a pipelined instantiation forced in turn (128 x 64, 64 x 64, 32 x 128), 3x3 stride 1 and 5x5
      stride 2, 1 / 2 / 3 (/ 4) chunks, one and several N tiles, ragged / image-spanning / single-workgroup maps, three
      epilogues
    - selection: classic without DS_CONV_PLAN_LATENCY and at a chip-filling batch, pipelined at B = 1 and 12 with it; the
      pipelined walk forced onto a row without an instantiation is an error
    - forward_eval_planned(bf16x3, low_latency=True) of 12 utterances of 32 frames: classic == pipelined == low_latency=False"""
import numpy as np
import pytest
import torch

import bf16_walk_cases as WC
import deepspeaker_oracle as O
from test_gpu_bf16_train_kernels import GpuBackend
from test_gpu_train_f16_kernels import eng     # noqa: F401  (the module-scoped engine fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be(eng):
    return GpuBackend(eng)


@pytest.mark.parametrize("bhw", WC.MAPS)
@pytest.mark.parametrize("k,s", WC.KERNELS)
@pytest.mark.parametrize("cfg", sorted(WC.PIPE_ROWS))
def test_walks_are_bit_identical(be, cfg, k, s, bhw):
    WC.body_walks_are_bit_identical(be, cfg, k, s, bhw)


def test_selection(be):
    WC.body_selection(be.lib)


def test_forward_eval_walks_are_bit_identical(eng):
    from deepspeaker_pytorch_amd.engine import Engine
    sd = O.make_state_dict(seed=23, num_classes=4)
    tsd = {k: torch.from_numpy(np.array(v)).cuda() for k, v in sd.items()}
    x = torch.from_numpy(O.make_input(seed=3, batch=12, frames=32)).cuda()
    WC.body_forward_eval(lambda: Engine(eng.lib), x, tsd)
