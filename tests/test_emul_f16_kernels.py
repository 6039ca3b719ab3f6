"""The fp16 forward convolutions on the host emulator (no GPU): the test bodies of f16_kernel_cases.py -- shared with
test_gpu_f16_kernels.py -- on numpy memory.  Every tile configuration of kCfgH is LAUNCHED here (forced through
ds_conv_f16_set_forced_cfg), persistent and one tile per workgroup, single-buffered, in 16-channel chunks and from the
plane-major input, each with the raw, the fp16 and the plane-major epilogue.  `-s` prints every launch with its plan, errors
and bars, and the coverage test the instantiations launched.

The emulator is slow, so this file runs a subset of part a: every form on the two cheapest maps (FK.EMUL_ALL_FORMS) and the
default and one-tile forms on two more (FK.EMUL_TWO_FORMS) -- enough for the coverage assert minus its NIT > 8 rows; the
device file runs all seven shapes in every form.  Part b (workgroups that walk several tiles) and part d (the block kernel)
launch on the device only; here the walk batches are checked against the planner as a 256-CU device sees it.

The emulator models none of the hardware hazards (MFMA lane layout, scheduling barriers, buffer range checks, cross-wave LDS
races): what it checks is the index arithmetic of every instantiation, the layouts, and the planner's hand-over to each.

Figures of this suite (bar in brackets).  Part a, 384 launches: raw f32 at most 2.3e-7 max-norm relative (2e-6), fp16 at most
7.81e-3 absolute (9.78e-3: half an fp16 step at 16 .. 20 is 7.8125e-3), everything else bit for bit.  Split-K: raw at most
4.1e-7, the f32 store of the epilogue 2.1e-7, fp16 7.81e-3.  16 tests in 68 s of wall time, the slowest (eight forms x eight
configurations of the 5x5 case) 33 s.

Seeded faults (each built into a scratch copy of the emulator, nothing of it kept): the plane stride of DS_EPI_OUT_PLANES16 in
conv_fwd_f16 doubled -- both part-a tests with every form and all six split-K tests fail; the pixel stride of
DS_CONV_IN_PLANES16 doubled -- the 5x5 part-a test fails, and no other test of the fp16 emulator files (test_emul_f16.py,
test_emul_f16_plans.py) does."""
import pytest

import f16_kernel_cases as FK
from test_emul_bf16_train import EmulBackend


@pytest.fixture(scope="module")
def be():
    return EmulBackend()


# ---- a. every tile configuration, every form of a launch ----
@pytest.mark.parametrize("case", FK.EMUL_ALL_FORMS)
def test_conv_fwd_every_configuration_every_form(be, case):
    FK.body_conv_fwd(be, case)


@pytest.mark.parametrize("case", FK.EMUL_TWO_FORMS)
def test_conv_fwd_every_configuration_persistent_and_one_tile(be, case):
    FK.body_conv_fwd(be, case, FK.TWO_FORMS)


# ---- b. the walk batches, as a 256-CU device plans them (describe only) ----
@pytest.mark.parametrize("base", list(FK.WALK_BASES))
def test_walk_batches_plan_persistent_with_more_tiles_than_workgroups(be, base, monkeypatch):
    monkeypatch.setenv("DS_EMUL_CUS", "256")
    FK.body_walk_plans(be.lib, base, 256)


# ---- c. split-K ----
@pytest.mark.parametrize("case", list(FK.SPLITK_CASES))
def test_split_k(be, case):
    FK.body_splitk(be, case)


# ---- e. refusals ----
def test_refusals(be):
    FK.body_refusals(be)


# ---- coverage ----
def test_every_instantiation_is_launched(be):
    """a selection or a worker of a parallel run has not run every case above: what is missing is run here"""
    for case in FK.EMUL_ALL_FORMS:
        if case not in FK.FWD_RAN:
            FK.body_conv_fwd(be, case)
    FK.body_fwd_coverage(nit_rows=False)


def test_the_hook_is_back_at_the_planners_choice(be):
    FK.body_hook_is_back(be.lib)
