"""CPU: score normalisation (csrc/score_norm.hip, scoring.cohort_stats / normalise_scores / min_dcf) through the host
emulator of the kernels, against the float64 restatement (tests/score_norm_reference.py).  The same cases run on the
device in test_gpu_score_norm.py."""
import pytest
import torch

import score_norm_cases as C
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


@pytest.mark.parametrize("row_block", C.ROW_BLOCKS)
@pytest.mark.parametrize("K", C.INT_KS)
@pytest.mark.parametrize("D", C.INT_DS)
def test_integer_data_selection_is_exact(env, D, K, row_block):
    C.case_integer_selection(env, D, K, row_block)


def test_tie_is_cut_in_index_order(env):
    C.case_tie_cut(env)


def test_lds_capacity_edge(env):
    C.case_capacity_edge(env)


def test_real_valued_statistics_and_membership(env):
    C.case_real_valued(env)


def test_duplicate_row_signed_keys(env):
    C.case_duplicate_row(env)


def test_result_does_not_depend_on_the_batch(env):
    C.case_independence(env)


def test_agrees_with_nearest(env):
    C.case_agrees_with_nearest(env)


def test_statistics_are_the_fixed_order_reduction_of_pairwise_distance_bits(env):
    C.case_statistics_bits(env)


@pytest.mark.parametrize("exclude", ("same", "other"))
def test_label_filter(env, exclude):
    C.case_labels(env, exclude)


@pytest.mark.parametrize("T", (1, 1000, 5000))
def test_apply(env, T):
    C.case_apply(env, T)


@pytest.mark.parametrize("kind", ("z", "t", "as"))
def test_end_to_end(env, kind):
    C.case_end_to_end(env, kind)


def test_min_dcf(env):
    C.case_min_dcf(env)


def test_signed_threshold_grid(env):
    C.case_signed_grid(env)


def test_errors(env):
    C.case_errors(env)
