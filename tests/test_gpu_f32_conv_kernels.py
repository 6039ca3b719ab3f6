"""The f32 convolution family, one kernel at a time, on the device (through the C ABI on device tensors) against float64
references of the same operation: the test bodies of f32_conv_cases.py, shared with test_emul_f32_conv.py.

    a. ds_conv_fwd_f32 LAUNCHED under every tile configuration of kCfg (128x64, 160x128, 256x64; forced through
       ds_conv_f32_set_forced_cfg): 3x3, 5x5 stride 2 and 1x1, every staging depth each reaches (19 instantiations), fused
       epilogue (affine + residual + clip on both edges + statistics) and raw, the raw outputs bit for bit among the tiles
    b. ds_conv_dgrad_f32 under the three configurations: stride 1, and the four parity classes of stride 2 on the
       table-driven tap schedule (odd maps, a one-row map with empty classes)
    c. ds_conv_wgrad_f32: <9,false>, <5,true>, <5,false>, <1,false>, the fc form with its feature permutation, and two cases
       with three images per tile and an uneven share of the tiles per split
    d. the shapes a forced configuration must still refuse

Bars: f32_conv_cases.py (y and gx 2e-6 on the max-norm relative and the relative L2 error; statistics rtol 1e-4 beyond atol
1e-3; filter gradient max(3e-6, 4 x the float32 restatement)).

Measured on one MI355X (every run prints its own under -s; emulator figures in test_emul_f32_conv.py), max-norm / L2:
  forward, 30 forced launches and 8 of the planner's choice: fused 7.1e-8 .. 1.6e-7 / 2.6e-8 .. 3.1e-8, raw 1.3e-7 .. 6.1e-7 /
    8.8e-8 .. 3.1e-7 -- the forced launches to the digit of the emulator's; column sums within 1.8e-5 absolute, sums of squares
    within 5.4e-7 relative; fused and raw statistics, and the raw y of the three configurations, bit for bit
  data gradient, 15 launches: 1.0e-7 .. 4.6e-7 / 7.5e-8 .. 1.8e-7, bit for bit among the configurations
  filter gradient, 10 cases: float32 restatement 2.1e-7 .. 1.0e-6 -> bar 3.0e-6 .. 4.1e-6 -> kernel 9.9e-8 .. 2.2e-7.  The two
    device-only plans are as derived: (24,256,512,10,4,5,2) <5,true>, 24 segments, 3 per tile, 8 tiles over S = 7;
    (52,512,512,5,4,3,1) <9,false>, 52 segments, 3 per tile, 18 tiles over S = 16 (1 .. 2 tiles per split in both)
  the whole file: 37 tests in 2.8 s, the slowest 0.3 s"""
import pytest

import f32_conv_cases as FC
from test_gpu_bf16_train_kernels import GpuBackend
from test_gpu_train_f16_kernels import eng                     # noqa: F401  (the module-scoped engine fixture)

pytestmark = pytest.mark.gpu

STATS_ATOL = 1e-3                       # the device suite's bar for the statistics rows (test_gpu_parity.py)


@pytest.fixture(scope="module")
def be(eng):
    return GpuBackend(eng)


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
@pytest.mark.parametrize("case", list(FC.WGRAD_CASES) + list(FC.WGRAD_CASES_DEVICE))
def test_conv_wgrad(be, case):
    plan = FC.body_conv_wgrad(be, case, FC.WGRAD_CASES.get(case) or FC.WGRAD_CASES_DEVICE[case])
    if case in FC.WGRAD_CASES_DEVICE:                           # three images per tile, one split owns two tiles
        assert plan["ni"] == 3 and max(plan["shares"]) == 2 and min(plan["shares"]) == 1, plan
        assert plan["n_segs"] % 3 == (0 if case[0] == 24 else 1)                # 52 images: the last tile one-third full


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
