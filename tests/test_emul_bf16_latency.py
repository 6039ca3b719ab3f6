"""The latency plan mode of the bf16x3 forward convolution on the host emulator (no GPU): the bodies of
bf16_latency_cases.py, shared with test_gpu_bf16_latency.py.  All checks are bitwise; `-s` prints the plans.
(`select_triplets` needs a device: its with / without comparison is in the GPU file only.)"""
import numpy as np
import pytest
import torch

import bf16_latency_cases as LC
import deepspeaker_oracle as O
from emul_util import emul_lib
from test_emul_bf16_train import EmulBackend


@pytest.fixture(scope="module")
def be():
    return EmulBackend()


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


def test_forward_eval_low_latency_is_bit_identical():
    """12 rows through the whole network (16 frames: the emulator runs one lane at a time)"""
    from deepspeaker_pytorch_amd.engine import Engine
    eng = Engine(emul_lib())
    sd = O.make_state_dict(seed=23, num_classes=4)
    tsd = {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
    x = torch.from_numpy(O.make_input(seed=3, batch=12, frames=16))
    LC.body_forward_eval(eng, x, tsd)
