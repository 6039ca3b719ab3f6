"""The kernels of the default (bf16x3) training step, one at a time, on the device (through the C ABI on device tensors)
against float64 references of the same operation: the test bodies of bf16_train_cases.py, shared with
test_emul_bf16_train.py.

    a. ds_conv_fwd_bf16 LAUNCHED under every tile configuration of kCfgB (0 - 8 bf16x3, 0 - 2 plain bf16; 3x3 and 5x5
       stride 2), fused epilogue (affine + residual + clip on both edges + statistics) and raw; the batched weight pack
    b. ds_conv_dgrad_bnbwd_bf16 / ds_conv_dgrad_s2_bnbwd_bf16 (the fused instantiation of all nine configurations; one
       and three members; parity classes of different sizes, empty classes; the refusals the callers fall back on) and
       ds_bn_bwd_group_finish_f32 -- the mask re-derived from the pre-activation by whatever fma the device compiler emitted
    c. ds_conv5x5s2_c1_fwd_f32 / _bf16
    d. ds_bn_stats_finalize_f32 (on the rows of a real ds_conv_fwd_f32 launch), ds_partial_sum_f64 +
       ds_bn_stats_from_sums_f32, ds_bn_apply_f32, ds_bn_fold_f32; ds_bn_bwd_f32 up to the 2048-row cap, its split form
       (ds_bn_bwd_reduce_f32 / ds_bn_bwd_apply_f32) and ds_bn_bwd_group_f32 + ds_colsum_f32 bit for bit; the grouped entry
       points with G = 1 and the split / finish forms with G = 3 bit for bit; the calls the nine entry points refuse

Bars (the emulator suite's own; max-norm relative errors).  Forward: bf16x3 2e-5, plain bf16 in (1e-4, 2e-2); statistics
rtol 1e-4 beyond atol 1e-3 (plain: 2e-2 beyond 0.5).  Fused data gradient: gy 3e-5; gz, dgamma, dbeta 1e-4; the partial
sums max(3e-5, 4 x the error of the float32 restatement -- torch's float32 convolution backward, float32 sums per M
tile).  First layer: f32 1e-5 absolute, bf16 3e-4 absolute and 3e-5 relative; statistics 1e-4 / 1e-4 and 1e-3 / 2e-3.
BatchNorm backward: gy 1e-6, the rest 1e-4; forward tables max(1e-5, 4 x float32 restatement); normalise: three float32
roundings of the largest value.

Measured on one MI355X (every run prints its own under -s; emulator figures in test_emul_bf16_train.py):
  forward, 42 bf16x3 launches (configurations 0 - 8, both kernel sizes): fused 9.7e-7 .. 1.6e-6, raw 3.7e-6 .. 5.7e-6; sums within
    atol, sums of squares at most 7.5e-7 of rtol.  18 plain bf16 launches: fused 4.8e-4 .. 8.3e-4, raw 2.1e-3 .. 2.8e-3
  fused data gradient, 25 launches: gy 2.9e-6 .. 5.0e-6; sum gy: float32 restatement 1.2e-7 .. 3.8e-7 -> bar 3e-5 -> kernel
    2.6e-6 .. 5.0e-6; sum gy * xhat: 1.4e-7 .. 5.5e-7 -> 3e-5 -> 2.2e-6 .. 4.3e-6; gz 2.7e-6 .. 4.9e-6, dgamma 2.2e-6 .. 4.9e-6,
    dbeta 2.6e-6 .. 4.6e-6
  first layer: f32 1.1e-6 .. 2.4e-6 absolute; bf16 4.4e-5 .. 6.8e-5 absolute, 5.0e-6 .. 6.2e-6 relative
  forward tables: invstd restatement 7.3e-8 .. 2.8e-7 -> bar 1e-5 -> kernel 8.4e-8 .. 3.2e-7 (mean, running statistics
    within atol 1e-6); normalise 9.5e-7 .. 1.9e-6 absolute under bars of 6.9e-6 .. 9.0e-6; fold 5.4e-8
  BatchNorm backward (2048 rows included): gy at most 5.8e-8, gz 7.8e-8 .. 1.7e-7, dgamma / dbeta 5.5e-8 .. 1.4e-7
  the whole file: 45 tests in 3.1 s, the slowest (300000 pixels of 64 channels) 0.7 s
"""
import numpy as np
import pytest
import torch

import bf16_train_cases as BC
from test_gpu_train_f16_kernels import dev, eng, full, host     # noqa: F401  (eng: the module-scoped engine fixture)

pytestmark = pytest.mark.gpu

_TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.uint16): torch.bfloat16}


class GpuBackend:
    def __init__(self, engine):
        self.eng, self.lib, self.p = engine, engine.lib, engine._p

    @property
    def stream(self):
        import ctypes
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def put(a):
        return dev(np.array(a))                                      # (a copy: the cached inputs are read-only)

    @staticmethod
    def nan(shape, dtype=np.float32):
        shape = tuple(shape) if np.ndim(shape) else (int(shape),)
        return full(shape, _TORCH[np.dtype(dtype)])                   # (a bf16 NaN is 0x7FC0: still "never written")

    @staticmethod
    def get(h):
        if h.dtype == torch.bfloat16:
            return host(h.view(torch.int16)).view(np.uint16)
        return host(h)

    @staticmethod
    def part(h, row0, rows):
        return h[row0:row0 + rows]

    @staticmethod
    def same(a, b):
        bits = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(bits), b.view(bits))


@pytest.fixture(scope="module")
def be(eng):
    return GpuBackend(eng)


# ---- a. forward convolution, every tile configuration ----
@pytest.mark.parametrize("x3", [True, False])
@pytest.mark.parametrize("case", BC.FWD_CFG_CASES)
def test_conv_fwd_every_configuration(be, case, x3):
    BC.body_conv_fwd(be, case, x3, BC.X3_CFGS if x3 else BC.PLAIN_CFGS)


@pytest.mark.parametrize("x3", [True, False])
@pytest.mark.parametrize("case", BC.BF16_CASES)
def test_conv_fwd_planner_choice(be, case, x3):
    BC.body_conv_fwd(be, case, x3, (-1,))


def test_pack_batch_equals_single_calls(be):
    BC.body_pack_batch(be)


# ---- b. fused data gradient + BatchNorm backward ----
@pytest.mark.parametrize("case,G,cfgs", BC.DGRAD_BN_CASES)
def test_dgrad_bnbwd(be, case, G, cfgs):
    BC.body_dgrad_bn(be, case, G, cfgs)


def test_dgrad_bnbwd_refusals(be):
    BC.body_dgrad_bn_refusals(be)


# ---- c. first layer ----
@pytest.mark.parametrize("shape", BC.C1_CASES)
def test_conv1(be, shape):
    BC.body_conv1(be, shape)


# ---- d. f32 BatchNorm family ----
@pytest.mark.parametrize("case", BC.BN_FWD_CASES)
def test_bn_forward_chain(be, case):
    BC.body_bn_forward(be, case)


@pytest.mark.parametrize("C,n_pix,with_g2,with_act", BC.BN_BWD_CASES)
def test_bn_bwd(be, C, n_pix, with_g2, with_act):
    BC.body_bn_bwd(be, C, n_pix, with_g2, with_act)


def test_bn_bwd_refusals(be):
    BC.body_bn_bwd_refusals(be)


@pytest.mark.parametrize("R,C", BC.COLSUM_CASES)
def test_colsum(be, R, C):
    BC.body_colsum(be, R, C)


def test_forced_configuration_is_restored(be):
    """the hook is process-global and later tests plan through it: the planner chooses again after every use, also after
    a body that raised"""
    from deepspeaker_pytorch_amd._native import ConvShape
    shp = ConvShape(2, 9, 32, 16, 64, 3, 1)
    with BC.forced_cfg(be.lib, 6):
        assert BC.describe(be.lib, shp, False)[0] == BC.DS_ERR_UNSUPPORTED      # plain bf16 has no 320x64 kernel
    with pytest.raises(RuntimeError):
        with BC.forced_cfg(be.lib, 6):
            raise RuntimeError("a failing test body")
    rc, out8 = BC.describe(be.lib, shp, False)
    assert rc == 0 and (out8[0], out8[1]) == (128, 64)
