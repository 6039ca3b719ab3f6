"""The lifecycle suite (lifecycle_bodies.py) on the host emulator: the host-side state around the kernels across several
steps of a loop, with the unmodified kernels computing underneath.  CPU tensors reach the emulated library here ONLY to
test host logic without a GPU (the product refuses them).  Everything that needs no HIP graph and no second stream runs
here and on the device (test_gpu_lifecycle.py); the graph and slot cases are the device's.

Geometry: n_stages = 2, 4 classes, members of 2 utterances x 16 frames.

What each test caught before its fix (the same bodies against the files of the commit before):
  * overflow sequence: with a model.py in which only the fused optimizers consume the flag, `torch_sgd` fails at the first
    clean step after the O (`_overflow_state` is still [1, 0]: update_loss_scale() returns True and backs off again),
    `fused_by_hand` and `torch_sgd_accumulate` have no consume_overflow() to call; `fused` passes, as it should;
  * guard cadence, 2 and 3 forwards per generation: 12 synchronous checks where the bounds are 7 and 10;
  * workspace lifetime: the buffer died with the second NativeLib.

Time: the emulator takes 0.6 s per eval forward and 1.8 s per training pass at this geometry, the smallest the kernels'
paths allow; the counts of passes are the cases' (10 scripted steps four ways, 12 generations of 1, 2 and 3 forwards)."""
import numpy as np
import pytest
import torch

import deepspeaker_oracle as O
import lifecycle_bodies as LB
from emul_util import emul_lib


class EmulEnv:
    name, is_device = "emul", False
    batch, frames, classes = 2, 16, 4

    def __init__(self, M, eng):
        self.M, self.eng, self.lib = M, eng, eng.lib

    def tensor(self, a):
        return torch.from_numpy(np.ascontiguousarray(a))

    def model(self, seed=3, **kw):
        sd = O.make_state_dict(seed=seed, num_classes=self.classes, n_stages=LB.N_STAGES)
        m = self.M.DeepSpeakerModel(512, self.classes, n_stages=LB.N_STAGES, **kw)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
        return m


@pytest.fixture()
def env(monkeypatch):
    """the `emul_model` pattern of test_emul_guard.py: the package's engine bound to the emulated library"""
    from deepspeaker_pytorch_amd import model as M
    from deepspeaker_pytorch_amd.engine import Engine
    eng = Engine(emul_lib())
    monkeypatch.setattr(M, "_engine", eng)
    monkeypatch.setattr(M, "_require_cuda", lambda t, what: None)
    return EmulEnv(M, eng)


def test_scaler_restatement_visits_growth_backoff_floor_and_cap():
    scales = LB.scripted_scales()
    assert scales == [2.0, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0]


@pytest.mark.parametrize("way", LB.WAYS)
def test_overflow_sequence(env, way):
    LB.body_overflow_sequence(env, way)


@pytest.mark.parametrize("per_generation", [1, 2, 3])
def test_guard_cadence(env, per_generation):
    LB.body_guard_cadence(env, per_generation)


def test_workspace_outlives_its_instance(env):
    LB.body_workspace_outlives_its_instance(env)
