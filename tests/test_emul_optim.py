"""The fused optimizers (optim.hip) on the host emulator: the bodies of optim_bodies.py on host memory.  What this suite
checks is the kernels' logic -- chunk and element indexing, the tables, the first-step rule, the skip flag, the device-side
step count, refusals -- and the Python layer (optim.py: the device counter across load_state_dict and state_dict, tables of
more than 256 parameters); what only the device compiler decides (fma contraction in s + g*g and p - clr*q, sqrtf, the
double-precision pow and division of the `_dev` kernels, the by-value 2 KiB kernel argument of ds_fill_bytes) is the
device suite's (test_gpu_optim_kernels.py).

Also here, CPU only: the float64 restatement the bars rest on against torch.optim on float64 parameters."""
import ctypes

import numpy as np
import pytest
import torch

import optim_bodies as OB
import optim_cases as OC
from emul_util import aligned, emul_lib
from deepspeaker_pytorch_amd.engine import Engine


class EmulBackend:
    name, is_device, device = "emul", False, torch.device("cpu")

    def __init__(self):
        self.lib = emul_lib()
        self.eng = Engine(self.lib)

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

    def tensor(self, a):
        return torch.from_numpy(np.ascontiguousarray(a))


@pytest.fixture(scope="module")
def be():
    return EmulBackend()


@pytest.mark.parametrize("set_name", OC.SETS)
@pytest.mark.parametrize("kind", OC.KINDS)
def test_step(be, kind, set_name):
    OB.body_step(be, kind, set_name)


@pytest.mark.parametrize("kind", OC.KINDS)
def test_skip_flag(be, kind):
    OB.body_skip_flag(be, kind)


def test_step_inc(be):
    OB.body_step_inc(be)


def test_fill_bytes(be):
    OB.body_fill_bytes(be)


def test_refusals(be):
    OB.body_refusals(be)


@pytest.mark.parametrize("kind", ["adagrad", "sgd", "adam"])
def test_load_state_dict_refills_the_device_counter(be, kind):
    OB.body_py_load_state_dict(be, kind)


@pytest.mark.parametrize("kind", ["adagrad", "adam"])
def test_state_dict_reports_the_device_count_after_a_skipped_step(be, kind):
    OB.body_py_state_dict_after_skip(be, kind)


def test_more_than_256_parameters(be):
    OB.body_py_many_params(be)


@pytest.mark.parametrize("kind", ["adagrad", "sgd", "adam"])
def test_skipped_step_neither_updates_nor_counts(be, kind):
    OB.body_py_skipped_step(be, kind)


# ---- CPU only: the restatement, the tensor sets ----
@pytest.mark.parametrize("wd", [0.0, 1e-3])
@pytest.mark.parametrize("kind", OC.KINDS)
def test_float64_restatement_equals_torch_optimizers(kind, wd):
    """three steps of optim_cases.step_ref in float64, each from the state the last left, against torch.optim.{Adagrad,
    SGD,Adam} on float64 parameters with create_optimizer's hyper-parameters: parameters and every state tensor to 1e-12"""
    hp = OC.hyper(kind, wd)
    rs = np.random.RandomState(7)
    n = 1000
    p0 = 0.5 * rs.randn(n)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = OB.make_torch(kind, [tp], hp)
    cur = dict(p=p0, s1=np.zeros(n), s2=np.zeros(n))
    for t in (1, 2, 3):
        g = rs.randn(n)
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        cur = OC.step_ref(kind, hp, t, cur["p"], g, cur["s1"], cur["s2"], OC.F64)
        want = dict(p=tp.detach().numpy())
        for k, name in zip(("s1", "s2"), OC.STATE_KEYS[kind]):
            want[k] = opt.state[tp][name].numpy()
        assert [k for k in cur if cur[k] is not None] == list(want)
        for k, w in want.items():
            err = float(np.abs(cur[k] - w).max() / np.abs(w).max())
            print(f"{kind} wd={wd:g} step {t}: {k} restatement against torch float64 {err:.2e}")
            assert err <= 1e-12, (kind, t, k, err)
    if kind in ("adagrad", "adam"):
        assert float(opt.state[tp]["step"]) == 3.0


def test_tensor_sets_reach_every_index_path():
    C = 16384
    e, m, o, lg = (OC.tensor_set(s, C) for s in OC.SETS)
    assert e.sizes == [1, 255, 256, 257, C - 1, C, C + 1, 2 * C + 232]
    assert len(m.sizes) == 301 and m.chunks(C)[0].max() == 300 and m.sizes[-1] == C + 3
    assert sorted({off % 4 for off in o.offs}) == [1, 2, 3] and o.offs == sorted(o.offs, reverse=True)
    assert lg.chunks(C)[1].max() == 40 and lg.sizes == [40 * C + 5]
    assert sum(a.total for a in (e, m, o, lg)) < 1_000_000
    for a in (e, m, o, lg):
        gap = np.ones(a.total, bool)
        gap[a.live] = False
        assert gap[:OC.GAP].all() and gap[-OC.GAP:].all()
        starts = sorted(zip(a.offs, a.sizes))
        assert all(s1 + n1 + OC.GAP <= s2 for (s1, n1), (s2, _) in zip(starts, starts[1:])), "poison between any two tensors"
