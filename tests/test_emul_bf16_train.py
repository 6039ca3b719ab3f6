"""The kernels of the default (bf16x3) training step on the host emulator (no GPU): the test bodies of
bf16_train_cases.py -- shared with test_gpu_bf16_train_kernels.py -- on numpy memory, at the shapes small enough for it.
Every tile configuration of the bf16 convolution is LAUNCHED here (forced through ds_conv_bf16_set_forced_cfg), not only
described: 0 - 8 for bf16x3, forward (3x3 and 5x5) and fused with the BatchNorm backward, 0 - 2 for plain bf16.  `-s`
prints every launch with its errors and bars, and the last test the table of what the case lists launch.

Figures of this suite (max-norm relative errors; bar in brackets): bf16x3 forward fused 9.7e-7 .. 1.6e-6, raw 3.7e-6 ..
5.7e-6 (2e-5), its sums within atol 1e-3 and sums of squares at most 7.4e-7 of rtol (1e-4); plain bf16 fused 4.8e-4 ..
8.3e-4, raw 2.1e-3 .. 2.8e-3 (1e-4 .. 2e-2); fused data gradient gy 2.9e-6 .. 5.0e-6 (3e-5), its partial sums at most 4.9e-6
(3e-5: the float32 restatement is at 1.2e-7 .. 5.5e-7); gz, dgamma, dbeta at most 5.1e-6 (1e-4).  About a minute in all."""
import numpy as np
import pytest

import bf16_train_cases as BC
from emul_util import aligned, emul_lib, ptr, to_aligned


class EmulBackend:
    stream = None

    def __init__(self):
        self.lib = emul_lib()

    @staticmethod
    def put(a):
        a = np.asarray(a)
        return to_aligned(a, a.dtype)

    @staticmethod
    def nan(shape, dtype=np.float32):
        return aligned(shape, dtype, fill=0xFFFF if np.dtype(dtype) == np.uint16 else np.nan)

    @staticmethod
    def p(h):
        return ptr(h)

    @staticmethod
    def get(h):
        return h

    @staticmethod
    def part(h, row0, rows):
        return h[row0:row0 + rows]

    @staticmethod
    def same(a, b):
        return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def be():
    return EmulBackend()


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


# ---- d. f32 BatchNorm family: the cases small enough for the emulator (the device suite runs all of them) ----
@pytest.mark.parametrize("case", BC.BN_FWD_CASES[:2])
def test_bn_forward_chain(be, case):
    BC.body_bn_forward(be, case)


@pytest.mark.parametrize("C,n_pix,with_g2,with_act", [c for c in BC.BN_BWD_CASES if c[1] <= BC.BN_BWD_GROUP_MAX_PIX])
def test_bn_bwd(be, C, n_pix, with_g2, with_act):
    BC.body_bn_bwd(be, C, n_pix, with_g2, with_act)


def test_bn_bwd_refusals(be):
    BC.body_bn_bwd_refusals(be)


@pytest.mark.parametrize("R,C", BC.COLSUM_CASES)
def test_colsum(be, R, C):
    BC.body_colsum(be, R, C)


def test_forced_configuration_is_restored(be):
    """the hook is process-global: after every use the planner chooses again (a forced configuration 6 would refuse
    plain bf16, which has no such kernel)"""
    import ctypes
    from deepspeaker_pytorch_amd._native import ConvShape
    shp = ConvShape(2, 9, 32, 16, 64, 3, 1)
    with BC.forced_cfg(be.lib, 6):
        assert BC.describe(be.lib, shp, False)[0] == BC.DS_ERR_UNSUPPORTED
    with pytest.raises(RuntimeError):
        with BC.forced_cfg(be.lib, 6):
            raise RuntimeError("a failing test body")
    rc, out8 = BC.describe(be.lib, shp, False)
    assert rc == 0 and (out8[0], out8[1]) == (128, 64)
    assert ctypes.sizeof(shp) == 28


def test_case_lists_launch_every_configuration(be):
    """what the case lists above launch: (kernel size, arithmetic, plain / fused with the BatchNorm backward,
    configuration).  Every body asserts that a forced configuration is feasible and that its plan has the
    configuration's tile, so a row of this table is a launch of that instantiation."""
    table = set()
    for case in BC.FWD_CFG_CASES:
        table |= {(case[5], "bf16x3", "plain", c) for c in BC.X3_CFGS} | {(case[5], "bf16", "plain", c) for c in BC.PLAIN_CFGS}
    for case, _, cfgs in BC.DGRAD_BN_CASES:
        table |= {(3, "bf16x3", "fused", c) for c in cfgs if c >= 0}        # (the 5x5 layer's classes run the 3x3 kernel)
    for row in sorted(table):
        print("launches: KS %d %-6s %-5s configuration %d (%dx%d, %d threads)" % (row + BC.CFG_TILES[row[3]]))
    ran = sorted((r for r in BC.LAUNCHED), key=str)
    for row in ran:
        print("launched by this process:", row)
    for ks in (3, 5):
        assert {c for k, a, f, c in table if (k, a, f) == (ks, "bf16x3", "plain")} == set(range(9))
        assert {c for k, a, f, c in table if (k, a, f) == (ks, "bf16", "plain")} == {0, 1, 2}
    assert {c for k, a, f, c in table if f == "fused"} == set(range(9))
