"""The loss-side, head and scoring kernels (tail_loss.hip, fc_mfma_f32.hip, scoring.hip), one entry point at a time, on the
host emulator: the bodies of loss_side_bodies.py on numpy memory, every case of loss_side_cases.py the emulator can hold in
reasonable time (the rest is marked "gpu" in the tables and runs in test_gpu_loss_side_kernels.py).  What this suite
checks is the kernels' logic -- indexing, tails, ordered compaction, tie rules, refusals; what only the device compiler
decides (fma contraction, powf / expf / logf, 64-lane ballots, dynamic-LDS aliasing, the MFMA) is the device suite's.

Also here, CPU only: the input conditions of the device-only cases that need no kernel (the mining tables' classes and
their 2 % cap of ambiguous anchors, the ROC distances' clearance from the thresholds)."""
import ctypes
import os

import numpy as np
import pytest

import loss_side_bodies as LB
import loss_side_cases as LC
from emul_util import aligned, emul_lib


class EmulBackend:
    name, is_device = "emul", False

    def __init__(self):
        self.lib = emul_lib()

    @property
    def cus(self):
        e = os.environ.get("DS_EMUL_CUS")
        return int(e) if e else 2

    def full(self, n, dtype, fill):
        return aligned(n, dtype, fill)

    def put(self, h, a):
        h[:a.size] = a

    def get(self, h):
        return h.copy()

    def p(self, h, off=0):
        return ctypes.c_void_p(h.ctypes.data + off * h.itemsize)

    def call(self, name, *args):
        return self.lib.call(name, *args, None)

    def rc(self, name, *args):
        return self.lib.raw(name)(*args, None)

    def plain(self, name, *args):
        return self.lib.raw(name)(*args)


@pytest.fixture(scope="module")
def be():
    return EmulBackend()


def ids(table):
    return ["-".join(str(v) for v in c[:-1]) for c in table]


def cases(table):
    t = LC.emul_cases(table)
    return pytest.mark.parametrize("case", t, ids=ids(t))


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
def test_mine_semihard(be, case, monkeypatch):
    monkeypatch.setenv("DS_EMUL_CUS", "256")        # the launcher's choice of anchors per workgroup as on a 256-unit device
    LB.body_mine(be, *case[:-1])


@pytest.mark.parametrize("plant", ["same_label", "no_semihard", "dup_in_tile", "dup_across_tiles", "equals_positive"])
@pytest.mark.parametrize("cus", [2, 256])
def test_mine_semihard_planted(be, plant, cus, monkeypatch):
    monkeypatch.setenv("DS_EMUL_CUS", str(cus))     # 8 anchors per workgroup, and 2
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


# ---- CPU-only conditions on the case tables (no kernel): they hold for the device-only cases too ----
@pytest.mark.parametrize("case", LC.MINE_CASES, ids=ids(LC.MINE_CASES))
def test_mine_case_inputs_stay_under_the_escape_cap(case):
    N, M, D, cls, _ = case
    assert LC.mine_anchors_per_group(N, M, D, 256) == {"lds4": 4, "lds2": 2}.get(cls, cls)
    anchor, cand, alab, clab, d_p, d64 = LC.mine_inputs(N, M, D, N + 3 * M + D)
    d32 = LC.mine_dist(anchor, cand, LC.F32)
    gap = LC.bar_from_restatement(LC.FLOOR_MINE_DIST, float((np.abs(d32 - d64) / d64).max()))
    win, _, accept = LC.mine_ref(d64, d_p, alab, clab, gap)
    escapes = sum(a is not None for a in accept)
    print(f"mine N={N} M={M} D={D}: gap {gap:.2e}, {escapes} of {N} anchors ambiguous, {int((win < 0).sum())} without a candidate")
    assert escapes <= LC.MINE_ESCAPE_CAP * N or (escapes <= 1 and N < 50)


def test_case_tables_name_every_listed_edge():
    assert {c[1] for c in LC.ROW_CASES} >= {1, 63, 64, 65, 512, 1000} and {c[0] for c in LC.ROW_CASES} >= {1, 3, 4, 5, 257}
    assert {c[0] for c in LC.SCAN_CASES} >= set(LC.SCAN_N) and {c[2] for c in LC.SCAN_CASES} >= {"0", "1", "5", "N+7"}
    assert {c[0] for c in LC.REFINE_CASES} >= {1, 3, 4, 6, 64} and {c[1] for c in LC.REFINE_CASES} == {"0", "lt", "eq", "gt"}
    assert {c[2] for c in LC.MINE_CASES} >= {4, 36, 64, 100, 512, 1024, 2048} and {c[1] for c in LC.MINE_CASES} >= {1, 255, 256, 257, 1500}
    assert {c[0] for c in LC.MINE_CASES} >= {1, 2, 5, 9, 64, 300} and {c[3] for c in LC.MINE_CASES} >= {2, 4, 8, "lds4", "lds2"}
    assert {c[2] for c in LC.MOVER_CASES} >= {4, 100, 4096, 4100, 10240} and {c[1] for c in LC.POOL_CASES} >= {1, 10, 50}
    assert {c[0] for c in LC.CE_CASES} >= {1, 3, 4, 5, 770} and {c[1] for c in LC.CE_CASES} >= {1, 2, 63, 64, 65, 1000, 5994}
    assert {c[1] for c in LC.FC_CASES} >= {32, 64, 96, 128, 192, 2048} and {c[2] for c in LC.FC_CASES} >= {128, 256, 512, 640, 1024}
    assert {c[0] for c in LC.FC_CASES} >= {1, 31, 32, 33, 100, 768}
    assert {c[0] for c in LC.ROC_CASES} >= {1, 1023, 1024, 1025, 5000} and {c[1] for c in LC.ROC_CASES} >= {1, 255, 256, 257, 3000}
    assert any(c[0] * c[2] * c[3] // 4 > 2048 * 256 for c in LC.POOL_CASES) and any(c[0] * c[1] * c[2] * c[3] // 4 > 4096 * 256 for c in LC.POOL_CASES)
