"""CPU: speaker identification (csrc/identify.hip, scoring.nearest / speaker_models / identify) through the host
emulator of the kernels, against the float64 restatement (tests/identify_reference.py).  The same cases run on the
device in test_gpu_identify.py."""
import pytest
import torch

import identify_cases as C
from emul_util import emul_lib

from deepspeaker_pytorch_amd.engine import Engine


@pytest.fixture
def env():
    from deepspeaker_pytorch_amd import scoring
    eng = Engine(emul_lib())
    scoring._engine_override = eng
    try:
        yield C.Env(scoring, eng, torch.device("cpu"))
    finally:
        scoring._engine_override = None


@pytest.mark.parametrize("splits", C.INT_SPLITS)
@pytest.mark.parametrize("k", C.INT_KS)
@pytest.mark.parametrize("D", C.INT_DS)
def test_integer_data_indices_are_exact(env, D, k, splits):
    C.case_integer_identity(env, D, k, splits)


def test_real_valued_distances_and_membership(env):
    C.case_real_valued(env)


def test_result_does_not_depend_on_the_batch(env):
    C.case_batch_independence(env)


def test_screening_bits_do_not_move(env):
    C.case_screening_bits_do_not_move(env)


@pytest.mark.parametrize("splits", (0, 3))
def test_label_filter(env, splits):
    C.case_label_filter(env, splits)


def test_label_filter_nothing_eligible(env):
    C.case_label_filter_nothing_eligible(env)


def test_speaker_models(env):
    C.case_speaker_models(env)


def test_identify_and_rank_hits(env):
    C.case_identify(env)


def test_rank_hits_many_queries(env):
    C.case_rank_hits_many_queries(env)


def test_errors(env):
    C.case_errors(env)
