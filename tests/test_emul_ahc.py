"""CPU: speaker diarisation (csrc/ahc.hip, deepspeaker_pytorch_amd.diarisation) through the host emulator of the
kernels, against the restatements in tests/ahc_reference.py.  The same cases run on the device in test_gpu_ahc.py."""
import pytest
import torch

import ahc_cases as C
from emul_util import emul_lib

from deepspeaker_pytorch_amd.engine import Engine


@pytest.fixture
def env():
    from deepspeaker_pytorch_amd import diarisation
    eng = Engine(emul_lib())
    diarisation._engine_override = eng
    try:
        yield C.Env(diarisation, eng, torch.device("cpu"))
    finally:
        diarisation._engine_override = None


@pytest.mark.parametrize("method", C.METHODS)
def test_linkage_is_the_float32_restatement_bit_for_bit(env, method):
    C.case_linkage_bit_exact(env, method)


@pytest.mark.parametrize("method", C.METHODS)
def test_ties_go_to_the_lowest_slots(env, method):
    C.case_ties(env, method)


def test_result_does_not_depend_on_the_batch(env):
    C.case_independence(env)


@pytest.mark.parametrize("dim", (512, 40))
def test_distances_are_pairwise_distance_bits(env, dim):
    C.case_distances(env, dim)


def test_cut(env):
    C.case_cut(env)


@pytest.mark.parametrize("k,n,seed", C.SCIPY_CASES)
def test_against_scipy_end_to_end(env, k, n, seed):
    C.case_against_scipy(env, k, n, seed)


def test_errors(env):
    C.case_errors(env)


def test_sliding_windows():
    from deepspeaker_pytorch_amd import diarisation
    C.case_sliding_windows(diarisation)


def test_turn_assembly():
    from deepspeaker_pytorch_amd import diarisation
    C.case_turns(diarisation)
