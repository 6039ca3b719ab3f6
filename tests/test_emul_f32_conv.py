"""The f32 convolution family on the host emulator (no GPU): the test bodies of f32_conv_cases.py -- shared with
test_gpu_f32_conv_kernels.py -- on numpy memory.  Every tile configuration of conv_mfma_f32.hip is LAUNCHED here (forced
through ds_conv_f32_set_forced_cfg), forward and both data gradients, and every instantiation of the filter gradient.  `-s`
prints every launch with its errors and bars, and the two coverage tests the instantiations launched.

Figures of this suite (max-norm relative error / relative L2 error; bar in brackets).  Forward, 30 forced launches
(configurations 0 - 2 on ten cases) and 8 of the planner's choice: fused 7.1e-8 .. 1.6e-7 / 2.6e-8 .. 3.1e-8, raw 1.3e-7 .. 6.1e-7 /
8.8e-8 .. 3.1e-7 (2e-6); column sums within 1.8e-5 absolute (atol 1e-4), sums of squares 8.8e-8 .. 5.4e-7 relative (rtol 1e-4); the
statistics of the fused and the raw launch, and the raw y of the three configurations, bit for bit.  Data gradient, 15
launches: 1.0e-7 .. 4.6e-7 / 7.5e-8 .. 1.8e-7 (2e-6), bit for bit among the configurations.  Filter gradient: float32
restatement 2.1e-7 .. 9.4e-7 -> bar 3.0e-6 .. 3.8e-6 -> kernel 9.9e-8 .. 2.2e-7.  37 tests in 8 s, the slowest 1 s.

Seeded faults (each built into a copy of the emulator, nothing of it kept): the `live` select dropped from the statistics,
the filter ring of RING == 3 refilled one tap late, the row offset of a_off off by one sub-tile for MSUB == 4 -- the forward
tests here fail under all three, the data-gradient tests under the last two; test_emul_kernels.py notices only the first."""
import pytest

import f32_conv_cases as FC
from test_emul_bf16_train import EmulBackend

STATS_ATOL = 1e-4                       # the emulator suite's bar for the statistics rows (test_emul_kernels.py)


@pytest.fixture(scope="module")
def be():
    return EmulBackend()


# ---- a. forward convolution, every tile configuration ----
@pytest.mark.parametrize("case", list(FC.FWD_CFG_CASES))
def test_conv_fwd_every_configuration(be, case):
    FC.body_conv_fwd(be, case, FC.CFGS, STATS_ATOL, FC.FWD_CFG_CASES[case])


@pytest.mark.parametrize("case", list(FC.FWD_WIDE_CASES))
def test_conv_fwd_several_n_tiles(be, case):
    FC.body_fwd_wide(be, case, STATS_ATOL)


@pytest.mark.parametrize("case", FC.CASES)
def test_conv_fwd_planner_choice(be, case):
    FC.body_conv_fwd(be, case, (-1,), STATS_ATOL)


# ---- b. data gradient, every tile configuration ----
@pytest.mark.parametrize("case", FC.DGRAD_CFG_CASES)
def test_conv_dgrad_every_configuration(be, case):
    FC.body_conv_dgrad(be, case, FC.CFGS)


# ---- c. filter gradient ----
@pytest.mark.parametrize("case", list(FC.WGRAD_CASES))
def test_conv_wgrad(be, case):
    FC.body_conv_wgrad(be, case, FC.WGRAD_CASES[case])


@pytest.mark.parametrize("case", list(FC.WGRAD_CASES_DEVICE))
def test_conv_wgrad_device_case_plans(case):
    """the two cases only the device launches: their plans, from the restated arithmetic (no launch here)"""
    inst, S, tiles = FC.WGRAD_CASES_DEVICE[case]
    plan = FC.plan_wgrad(case)
    assert (plan["inst"], plan["S"], plan["n_tiles"], plan["ni"]) == (inst, S, tiles, 3), plan
    assert max(plan["shares"]) == 2 and min(plan["shares"]) == 1


def test_fc_wgrad_feature_permutation(be):
    FC.body_fc_wgrad_permutation(be)


# ---- d. refusals ----
def test_forced_configuration_refusals(be):
    FC.body_refusals(be)


# ---- coverage ----
def test_every_forward_instantiation_is_launched(be):
    FC.body_fwd_coverage(be, STATS_ATOL)


def test_every_data_gradient_schedule_is_launched(be):
    FC.body_dgrad_coverage(be)


def test_every_filter_gradient_instantiation_is_launched(be):
    FC.body_wgrad_coverage(be)
