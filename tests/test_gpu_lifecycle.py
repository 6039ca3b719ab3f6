"""The lifecycle suite (lifecycle_bodies.py) on a real MI355X: the bodies the host emulator runs (test_emul_lifecycle.py) on
device memory, and the two that need a HIP graph -- a replayed step that overflows, and captures with the scheduler
pool nearly used up.

Geometry: n_stages = 2, 16 classes, members of 4 utterances x 32 frames (stage 1: 16 x 32 pixels of 64 channels, stage 2:
8 x 16 of 128: both BasicBlocks run the fused persistent block kernel, every stage convolution the persistent fp16 one).

Every test prints what it measured (`-s`): the slots one captured step keeps, the guard's check counts, build and drain
times.  Figures of the MI355X are in DESIGN_LOG.md."""
import numpy as np
import pytest
import torch

import deepspeaker_oracle as O
import lifecycle_bodies as LB

pytestmark = pytest.mark.gpu


class DeviceEnv:
    name, is_device = "gpu", True
    batch, frames, classes = 4, 32, 16

    def __init__(self):
        from deepspeaker_pytorch_amd.model import get_engine
        self.eng = get_engine()
        self.lib = self.eng.lib
        self.device = torch.device("cuda", torch.cuda.current_device())

    def tensor(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def model(self, seed=3, **kw):
        from deepspeaker_pytorch_amd.model import DeepSpeakerModel
        sd = O.make_state_dict(seed=seed, num_classes=self.classes, n_stages=LB.N_STAGES)
        m = DeepSpeakerModel(512, self.classes, n_stages=LB.N_STAGES, **kw)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
        return m.to(self.device)


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return DeviceEnv()


@pytest.mark.parametrize("way", LB.WAYS)
def test_overflow_sequence(env, way):
    LB.body_overflow_sequence(env, way)
    torch.cuda.synchronize()


@pytest.mark.parametrize("per_generation", [1, 2, 3])
def test_guard_cadence(env, per_generation):
    LB.body_guard_cadence(env, per_generation)


def test_workspace_outlives_its_instance(env):
    LB.body_workspace_outlives_its_instance(env)


def test_replayed_step_that_overflows(env):
    LB.body_replayed_overflow(env)


def test_capture_with_the_pool_nearly_used_up(env):
    LB.body_capture_with_drained_pool(env)
