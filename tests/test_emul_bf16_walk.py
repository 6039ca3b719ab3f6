"""The pipelined walk of the bf16x3 forward convolution on the host emulator (no GPU): the bodies of bf16_walk_cases.py,
shared with test_gpu_bf16_walk.py; `-s` prints the cases and errors.  The emulator runs the unmodified kernel source with
__syncthreads() / the LDS barrier as rendezvous points of a workgroup's threads: a wave that executed another number of
barriers than its neighbours would hang or fail HERE, on the CPU.

Also here, because it needs a compiler and no GPU: the resources of every pipelined instantiation (no scratch, no
spills, no static LDS next to the launch's dynamic request), read from the compiler's own remarks."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import bf16_walk_cases as WC
import deepspeaker_oracle as O
from emul_util import emul_lib
from test_emul_bf16_train import EmulBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def be():
    return EmulBackend()


@pytest.mark.parametrize("bhw", WC.MAPS)
@pytest.mark.parametrize("k,s", WC.KERNELS)
@pytest.mark.parametrize("cfg", sorted(WC.PIPE_ROWS))
def test_walks_are_bit_identical(be, cfg, k, s, bhw):
    WC.body_walks_are_bit_identical(be, cfg, k, s, bhw)


def test_selection(be):
    WC.body_selection(be.lib)


def test_forward_eval_walks_are_bit_identical():
    """12 rows through the whole network (16 frames: the emulator runs one lane at a time; the device test runs 32)"""
    from deepspeaker_pytorch_amd.engine import Engine
    sd = O.make_state_dict(seed=23, num_classes=4)
    tsd = {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
    x = torch.from_numpy(O.make_input(seed=3, batch=12, frames=16))
    WC.body_forward_eval(lambda: Engine(emul_lib()), x, tsd)


# ---------------------------------------------------------------------------------------------------------------------
# resources of the pipelined instantiations (the Makefile's flags + -Rpass-analysis=kernel-resource-usage, device only)
# ---------------------------------------------------------------------------------------------------------------------
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PIPE_TUS = ("conv_mfma_bf16_k3x3p", "conv_mfma_bf16_k5x3p")
# <KS, MSUB, NSUB, WM, WN, X3 = true, NIT, PREF = true, BNB = false, PIPE = true> of every row of WC.PIPE_ROWS
ROW_TEMPLATE_ARGS = {0: (2, 1, 2, 2), 9: (1, 1, 2, 2), 10: (1, 1, 1, 4)}
NITS = (4, 8, 16)


def _makefile_flags(tu):
    """the flags `make` compiles this translation unit with (dry run: nothing is built)"""
    out = subprocess.run(["make", "-C", ROOT, "-n", "-B", f"build/obj/{tu}.o"], check=True, capture_output=True, text=True).stdout
    line = next(l for l in out.splitlines() if f"{tu}.hip" in l and " -c " in l)
    args = line.split()[1:]
    drop = {"-c", "-o", f"build/obj/{tu}.o", f"deepspeaker-pytorch_amd/csrc/{tu}.hip"}
    return [a for a in args if a not in drop]


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("make") is None, reason="needs hipcc and make")
@pytest.mark.parametrize("tu", PIPE_TUS)
def test_pipelined_instantiations_use_no_scratch(tu, tmp_path):
    ks = int(tu[len("conv_mfma_bf16_k")])
    cmd = [HIPCC] + _makefile_flags(tu) + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-o",
                                            str(tmp_path / "k.o"), f"deepspeaker-pytorch_amd/csrc/{tu}.hip"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s*([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+))", line)
        if not m:
            continue
        if m.group(1):
            name = m.group(1)
            kernels[name] = {}
        elif name:
            kernels[name][m.group(2).strip()] = int(m.group(3))
    want = {f"conv_mfma_bf16_kernelILi{ks}ELi{a}ELi{b}ELi{c}ELi{d}ELb1ELi{nit}ELb1ELb0ELb1EE": (cfg, nit)
            for cfg, (a, b, c, d) in ROW_TEMPLATE_ARGS.items() for nit in NITS}
    seen = set()
    for name, res in kernels.items():
        key = next((w for w in want if w in name), None)
        assert key is not None, f"{tu} holds a kernel that is no pipelined instantiation: {name}"
        seen.add(key)
        print(f"{tu} row {want[key][0]} NIT {want[key][1]}: {res}")
        assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, (name, res)
        # all LDS is the launch's dynamic request (sized by the plan, at most 160 KiB - 64): nothing static beside it
        assert res["LDS Size"] == 0, (name, res)
        assert res["VGPRs"] + res["AGPRs"] <= 512 and res["Occupancy"] >= 1, (name, res)
    assert seen == set(want), sorted(set(want) - seen)
