"""The kernels around the convolution stack, one entry point at a time, on the device (through the C ABI on device tensors)
against float64 references of the same operation (tests/loss_side_cases.py): the row kernels of the loss side, the triplet
scan family, the near-tie refinement, the semi-hard search, the row movers, the pools and masks, cross entropy
(tail_loss.hip, scoring.hip), the split-K projection head and the small-batch tail (fc_mfma_f32.hip), verification scoring
(scoring.hip).  The bodies are loss_side_bodies.py's, the same the host emulator runs (test_emul_loss_side.py); here they
see what only the device compiler decides -- fma contraction, powf / expf / logf, 64-lane ballots and xor shuffles, the
dynamic-LDS aliasing of the search, the f32 MFMA of the split-K GEMM -- and the cases the emulator leaves out: the search's
<8> / <4> / <2> instantiations as the device's own compute-unit count selects them (printed), the LDS-driven reduction at
D = 1024 / 2048 / 3584 with 1500 candidates, the grid-stride loops past 2048 / 4096 workgroups, 768-row GEMMs, 5994 classes.

Bars.  Bit-exact where the operation is a move, a compaction, a count or a decision on given numbers (filter and near-tie
lists, probes, gathers, the scatter's sequential sum, masks, crops, tp / fp, maxima).  Elsewhere max(floor, 4 x the error of
the plain float32 restatement against float64), floors from the emulator suite: distances / loss / mean difference 1e-6,
any-norm distance 2e-6 (gradient 5e-6), search distances 2e-6, projection and small tail 2e-6, cross entropy 1e-6, 1e-6
where it has none.  Every test prints the restatement's error, the bar and the kernel's error (`-s`).

Figures of the same bodies on the host emulator (restatement error -> bar -> kernel):
  row kernels, rows=257 D=512: distance 4.1e-08 -> 1e-06 -> 3.8e-08; any-norm p=0.5 8.4e-08 -> 2e-06 -> 8.6e-08;
    triplet loss (absolute) 8.2e-09 -> 1e-06 -> 6.7e-09
  scan N=1000: loss 6.6e-10 -> 1e-06 -> 6.6e-10; near ties 666 against cap 5 (overflow), 17 against cap 64 at N=768
  refinement cap=64 D=512: patched distances 1.0e-07 -> 1e-06 -> 8.5e-08; err[0] 1.9e-06 -> 2.4e-05 -> 1.9e-06
  search N=300 M=512 D=2048: out_dist 1.6e-06 -> 6.2e-06 -> 9.3e-07 (D=64: 2.9e-07 -> 2e-06 -> 2.1e-07); no anchor of any
    case takes the tie escape
  cross entropy M=770 n_cls=65 spread 1e4: lse 6.5e-09 -> 1e-06 -> 6.5e-09; dlogits 1.4e-07 -> 1e-06 -> 1.2e-07
  projection B=33 K=2048: f 5.2e-07 -> 2.1e-06 -> 4.2e-07; small tail B=3 K=2048: f 1.0e-06 -> 4.0e-06 -> 1.8e-07
The device's own figures are printed by every run."""
import ctypes

import numpy as np
import pytest
import torch

import loss_side_bodies as LB
import loss_side_cases as LC

pytestmark = pytest.mark.gpu

_TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.int64): torch.int64, np.dtype(np.int32): torch.int32}


class DeviceBackend:
    name, is_device = "gpu", True

    def __init__(self, eng):
        self.lib = eng.lib
        self.cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count

    @staticmethod
    def _stream():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def full(self, n, dtype, fill):
        return torch.full((n,), fill, dtype=_TORCH[np.dtype(dtype)], device="cuda")

    def put(self, h, a):
        h[:a.size].copy_(torch.from_numpy(a))

    def get(self, h):
        torch.cuda.synchronize()
        return h.cpu().numpy()

    def p(self, h, off=0):
        return ctypes.c_void_p(h.data_ptr() + off * h.element_size())

    def call(self, name, *args):
        return self.lib.call(name, *args, self._stream())

    def rc(self, name, *args):
        return self.lib.raw(name)(*args, self._stream())

    def plain(self, name, *args):
        return self.lib.raw(name)(*args)


@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    from deepspeaker_pytorch_amd.model import get_engine
    b = DeviceBackend(get_engine())
    print(f"device: {b.cus} compute units")
    return b


def cases(table):
    return pytest.mark.parametrize("case", table, ids=["-".join(str(v) for v in c[:-1]) for c in table])


@cases(LC.ROW_CASES)
def test_row_kernels(be, case):
    LB.body_rows(be, *case[:-1])


@cases(LC.SCAN_CASES)
def test_scan_family(be, case):
    LB.body_scan(be, *case[:-1])


@cases(LC.REFINE_CASES)
def test_refinement(be, case):
    LB.body_refine(be, *case[:-1])


@cases(LC.MINE_CASES)
def test_mine_semihard(be, case):
    LB.body_mine(be, *case[:-1])


@pytest.mark.parametrize("plant", ["same_label", "no_semihard", "dup_in_tile", "dup_across_tiles", "equals_positive"])
def test_mine_semihard_planted(be, plant):
    LB.body_mine_planted(be, plant)


def test_mine_semihard_refuses_rows_past_the_lds_budget(be):
    LB.body_mine_refused(be)


@cases(LC.MOVER_CASES)
def test_row_movers(be, case):
    LB.body_movers(be, *case[:-1])


@cases(LC.POOL_CASES)
def test_pools(be, case):
    LB.body_pools(be, *case[:-1])


@pytest.mark.parametrize("row_bytes", LC.MASK_ROW_BYTES)
def test_mask_rows(be, row_bytes):
    LB.body_mask_rows(be, row_bytes)


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 3 * 1024 * 1024])
def test_max_abs_diff(be, n):
    LB.body_max_abs_diff(be, n)


@cases(LC.CE_CASES)
def test_cross_entropy(be, case):
    LB.body_ce(be, *case[:-1])


@cases(LC.FC_CASES)
def test_fc_l2norm(be, case):
    LB.body_fc(be, *case[:-1])


@cases(LC.FC_CE_CASES)
def test_fc_ce(be, case):
    LB.body_fc_ce(be, *case[:-1])


@cases(LC.TAIL_SMALL_CASES)
def test_tail_small(be, case):
    LB.body_tail_small(be, *case[:-1])


def test_tail_small_refusals(be):
    LB.body_tail_small_refused(be)


@cases(LC.GROUP_CASES)
def test_group_and_segment_mean(be, case):
    LB.body_group_mean(be, *case[:-1])


def test_assemble_crops(be):
    LB.body_assemble_crops(be)


@cases(LC.ROC_CASES)
def test_roc_sweep(be, case):
    LB.body_roc(be, *case[:-1])
