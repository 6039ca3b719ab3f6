"""The fp16 forward convolutions, one kernel at a time, on the device (through the C ABI on device tensors) against float64
references of the same operation on the same fp16-rounded operands: the test bodies of f16_kernel_cases.py, shared with
test_emul_f16_kernels.py.

    a. ds_conv_fwd_f16 LAUNCHED under configurations 0 .. 6 of kCfgH (forced through ds_conv_f16_set_forced_cfg) and the
       planner's choice on seven shapes, in every form (persistent, one tile per workgroup, single-buffered, 64-wide, 16-channel
       chunks, plane-major input) with the raw f32, the fp16 and the plane-major epilogue: the first output of each kind against
       float64, every other one bit for bit the first, the un-permuted planes bit for bit the channels-last output
    b. persistent workgroups that walk several tiles under every configuration (batches from the CU count): XCD queues, one
       queue, one tile per workgroup and the plane-major input, bit for bit over the whole tensor
    c. ds_conv_fwd_f16_splitk 8, 4 and 2 ways, an uneven split, f32 output and residual through the reduce kernel, and the
       three ways to one pass (a workspace one byte short, plane-major output, the chunk-width switch)
    d. ds_conv_block_f16 with its output flags, and the XCD-dealt tile order (more tiles than 2 x CUs workgroups, a batch that
       is no multiple of 8), plain and masked, bit for bit two ds_conv_fwd_f16 calls
    e. refusals

Bars: f16_kernel_cases.py (raw f32 2e-6 max-norm relative; fp16 epilogue 20 * 2^-11 + 1e-5 absolute; everything else bit
for bit).

Measured on one MI355X (256 CUs; every run prints its own under -s; emulator figures in test_emul_f16_kernels.py):
  a. 960 launches (seven shapes x eight configurations x four or eight forms x three epilogues): raw 1.6e-7 .. 6.4e-7, fp16
     7.80e-3 .. 7.81e-3 (half an fp16 step at 16 .. 20); every other launch bit for bit the first, every plane-major output bit
     for bit the channels-last one.  The coverage test lists 175 distinct plans (tile, kernel, buffering, chunk width, NIT)
  b. 148 launches, 416 .. 1344 tiles on 256 or 512 resident workgroups: raw 2.5e-7 .. 4.7e-7, fp16 7.81e-3, all bit for bit
  c. split-K raw 1.3e-7 .. 6.6e-7, fp16 7.73e-3 .. 7.81e-3, the f32 store of the epilogue 6.8e-8 .. 2.7e-7
  d. 9 + 4 block launches bit for bit two convolution calls; (67, 59, 32, 64) and (67, 59, 16, 128): 536 tiles on 512 workgroups
  the whole file: 32 tests in 4.2 s, the slowest (the 96-image walk) 0.4 s"""
import numpy as np
import pytest
import torch

import f16_kernel_cases as FK
from test_gpu_bf16_train_kernels import GpuBackend
from test_gpu_train_f16_kernels import eng, full                # noqa: F401  (eng: the module-scoped engine fixture)

pytestmark = pytest.mark.gpu


class F16GpuBackend(GpuBackend):
    """... with fp16 outputs"""

    @staticmethod
    def nan(shape, dtype=np.float32):
        if np.dtype(dtype) == np.float16:
            return full(tuple(shape) if np.ndim(shape) else (int(shape),), torch.float16)
        return GpuBackend.nan(shape, dtype)


@pytest.fixture(scope="module")
def be(eng):
    return F16GpuBackend(eng)


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- a. every tile configuration, every form of a launch ----
@pytest.mark.parametrize("case", FK.FWD_CASES)
def test_conv_fwd_every_configuration_every_form(be, case):
    FK.body_conv_fwd(be, case)


# ---- b. persistent workgroups that walk several tiles ----
@pytest.mark.parametrize("base", list(FK.WALK_BASES))
def test_persistent_workgroups_walk_several_tiles(be, cus, base):
    FK.body_walk(be, base, cus)


# ---- c. split-K ----
@pytest.mark.parametrize("case", list(FK.SPLITK_CASES))
def test_split_k(be, case):
    FK.body_splitk(be, case)


# ---- d. the BasicBlock kernel ----
@pytest.mark.parametrize("out", list(FK.BLOCK_FLAGS))
@pytest.mark.parametrize("geom", FK.BLOCK_FLAG_GEOMS)
def test_block_kernel_output_flags(be, geom, out):
    FK.body_block(be, geom, FK.BLOCK_FLAGS[out])


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("w,c", FK.BLOCK_XCD_WIDTHS)
def test_block_kernel_xcd_dealt_tile_order(be, cus, w, c, masked):
    geom = FK.block_xcd_geom(cus, w, c)
    b, h = geom[:2]
    # the condition of conv_block_f16.hip for dealing images to XCDs, restated
    assert b >= 8 and b % 8 != 0 and b * -(-h // FK.BLOCK_ROWS) > 2 * cus and (2 * cus) % 8 == 0, (geom, cus)
    FK.body_block(be, geom, 0, masked)


# ---- e. refusals ----
def test_refusals(be):
    FK.body_refusals(be)


# ---- coverage ----
def test_every_instantiation_is_launched(be):
    """a selection or a worker of a parallel run has not run every case above: what is missing is run here"""
    for case in FK.FWD_CASES:
        if case not in FK.FWD_RAN:
            FK.body_conv_fwd(be, case)
    FK.body_fwd_coverage(nit_rows=True)


def test_the_hook_is_back_at_the_planners_choice(be):
    FK.body_hook_is_back(be.lib)
