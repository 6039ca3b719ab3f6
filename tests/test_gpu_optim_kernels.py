"""The fused optimizers (optim.hip) on the device: the bodies of optim_bodies.py, the same the host emulator runs
(test_emul_optim.py), on device memory through the C ABI and through optim.py.  Here they see what only the device
compiler decides -- fma contraction in s + g*g and p - clr*q, sqrtf, the double-precision pow and division of the `_dev`
kernels, the by-value 2 KiB kernel argument of ds_fill_bytes.  Device only as well: ds_optim_step_inc + a `_dev` step
captured into one linear graph and replayed with the count of each replay, and a captured ds_fill_bytes that re-writes its
table on replay.

Bars: max(1e-6, 4 x the error of the plain float32 restatement against float64) in max |d| / max |ref|, on the update
p_new - p_old and on every state tensor.  Every test prints the restatement's error, the bar and the kernel's error (`-s`).

Figures on the MI355X (restatement error -> bar -> kernel; the host emulator's figure in brackets where it differs -- the
emulator reproduces the restatement bit for bit, the device contracts s + g*g and p - clr*q into fma), on the long set (one
tensor of 40C+5 elements) at weight decay 1e-3; the `_dev` entry gave the host-scalar entry's figures in every line:
  Adagrad host t=2 decay=0.5:     update 3.84e-07 -> 1.54e-06 -> 3.41e-07 [3.84e-07]; sum 1.22e-07 -> 1e-06 -> 7.13e-08 [1.22e-07]
  Adagrad _dev t=2 decay=0.5:     update 3.84e-07 -> 1.54e-06 -> 3.41e-07 [3.84e-07]; sum 1.22e-07 -> 1e-06 -> 7.13e-08 [1.22e-07]
  Adagrad host t=1000 decay=1e-4: update 2.79e-07 -> 1.12e-06 -> 2.65e-07 [2.79e-07]; sum 1.36e-07 -> 1e-06 -> 9.37e-08 [1.36e-07]
  Adagrad _dev t=1000 decay=1e-4: update 2.79e-07 -> 1.12e-06 -> 2.65e-07 [2.79e-07]; sum 1.36e-07 -> 1e-06 -> 9.37e-08 [1.36e-07]
  Adagrad host and _dev t=1000 decay=0.5 (clr = 2e-4: the updates are a few ulps of p): update 7.46e-05 -> 2.99e-04 ->
    7.46e-05; there the tiny-gradient elements (p = 0) hold clr itself: 7.53e-08 -> 1e-06 -> 7.53e-08
  SGD momentum 0.9 host t=1 (NaN buffer, first_step=1): update 1.19e-07 -> 1e-06 -> 8.18e-08 [1.19e-07]; momentum_buffer
    4.53e-08 -> 1e-06 -> 4.53e-08
  SGD momentum 0.9 _dev t=1 (NaN buffer, count 1):      update 1.19e-07 -> 1e-06 -> 8.18e-08 [1.19e-07]; momentum_buffer
    4.53e-08 -> 1e-06 -> 4.53e-08
  SGD momentum 0.9 host t=1000: update 1.96e-07 -> 1e-06 -> 1.79e-07 [1.96e-07]; momentum_buffer 1.20e-07 -> 1e-06 -> 1.20e-07
  SGD momentum 0.9 _dev t=1000: update 1.96e-07 -> 1e-06 -> 1.79e-07 [1.96e-07]; momentum_buffer 1.20e-07 -> 1e-06 -> 1.20e-07
  SGD momentum 0 (null state1) host t=2: update 1.16e-07 -> 1e-06 -> 8.46e-08 [1.16e-07]
  SGD momentum 0 (null state1) _dev t=2: update 1.16e-07 -> 1e-06 -> 8.46e-08 [1.16e-07]
  Adam host t=1 (bc1 = 0.1): update 4.56e-06 -> 1.83e-05 -> 4.49e-06 [4.56e-06]; exp_avg 1.10e-07 -> 1e-06 -> 1.10e-07;
    exp_avg_sq 3.16e-07 -> 1.26e-06 -> 3.16e-07; tiny gradient (g = 1e-9 on zero state) 7.37e-07 -> 2.95e-06 -> 7.37e-07
  Adam _dev t=1 (bc1 = 0.1): update 4.56e-06 -> 1.83e-05 -> 4.49e-06 [4.56e-06]; exp_avg 1.10e-07 -> 1e-06 -> 1.10e-07;
    exp_avg_sq 3.16e-07 -> 1.26e-06 -> 3.16e-07; tiny gradient 7.37e-07 -> 2.95e-06 -> 7.37e-07
  Adam host t=1000: update 4.61e-06 -> 1.84e-05 -> 4.61e-06; exp_avg 1.14e-07 -> 1e-06 -> 1.14e-07; exp_avg_sq 2.86e-07 ->
    1.14e-06 -> 2.86e-07
  Adam _dev t=1000: update 4.61e-06 -> 1.84e-05 -> 4.61e-06; exp_avg 1.14e-07 -> 1e-06 -> 1.14e-07; exp_avg_sq 2.86e-07 ->
    1.14e-06 -> 2.86e-07
  the largest share of a bar any case takes: Adam, the many set, t=1: update 5.01e-06 -> 2.01e-05 -> 5.29e-06
  third replay of one graph (edges set, count 3): Adagrad update 3.61e-07 -> 1.45e-06 -> 3.61e-07, sum 5.65e-08 -> 1e-06 ->
    7.86e-08; Adam update 2.30e-06 -> 9.21e-06 -> 2.30e-06, exp_avg_sq 2.42e-07 -> 1e-06 -> 2.42e-07
  optim.py: Adagrad, second step after load_state_dict (count 10): update 3.61e-06 -> 1.44e-05 -> 3.61e-06; 301 parameters,
    new gradient tensors: update 9.72e-07 -> 3.89e-06 -> 9.72e-07; Adam from zero state, count 5: exp_avg_sq 8.41e-06 ->
    3.36e-05 -> 8.41e-06 (1.0f - b2 is taken in float32, 1.3e-5 off 1 - b2: it shows while v is young)
The device's own figures are printed by every run."""
import ctypes

import numpy as np
import pytest
import torch

import optim_bodies as OB
import optim_cases as OC
from loss_side_bodies import out, same_bits

pytestmark = pytest.mark.gpu

_TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.int64): torch.int64, np.dtype(np.int32): torch.int32}


class DeviceBackend:
    name, is_device = "gpu", True

    def __init__(self, eng):
        self.eng, self.lib = eng, eng.lib
        self.device = torch.device("cuda", torch.cuda.current_device())

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

    def tensor(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)


@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    from deepspeaker_pytorch_amd.model import get_engine
    return DeviceBackend(get_engine())


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


# ---- device only: captured replays (one linear capture: every launch on the one capturing stream, no side stream, no
# parallel branch) ----
@pytest.mark.parametrize("kind", ["adagrad", "adam"])
def test_counter_and_step_replay_with_the_count_of_the_replay(be, kind):
    """ds_optim_step_inc followed by the `_dev` step, captured once on the edges set and replayed three times with new
    gradients in the same buffers: after replay k the counter reads k + 1 and parameters and state hold their bar against
    the float64 step with THAT count applied to the kernel's own previous state"""
    C = OB.chunk_elems(be)
    ar = OC.tensor_set("edges", C)
    hp = OC.hyper(kind, 1e-3, 0.5) if kind == "adagrad" else OC.hyper(kind, 1e-3)
    p, g, s1, s2 = OC.step_inputs(kind, ar.n_live, 1e-3, 61, plant=False)
    warm = OB.Launch(be, ar, C, p, g, s1, s2)                 # the kernels' code is loaded before the capture, not in it
    warm_cnt = OB.counter(be, 0)
    L, cnt = OB.Launch(be, ar, C, p, g, s1, s2), OB.counter(be, 0)

    def enqueue(launch, count):
        be.call("ds_optim_step_inc", count.p(1), None)
        be.call(OB.entry(kind, True), *launch.args(), *OB.step_args(kind, hp, 1, True, count), None)

    enqueue(warm, warm_cnt)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue(L, cnt)
    assert OB.count_of(cnt) == 0 and L.untouched("captured, not run"), "a capture runs nothing"
    before = dict(p=p, s1=s1, s2=s2)
    rs = np.random.RandomState(62)
    for k in range(3):
        gk = rs.randn(ar.n_live).astype(np.float32)
        L.set_grads(gk)
        graph.replay()
        assert OB.count_of(cnt) == k + 1
        got = L.read(f"replay {k}")
        OB.check_step(f"{kind} edges replay {k} (count {k + 1})", kind, hp, k + 1, before, gk, got, planted=False)
        before = dict(got, s1=got.get("s1"), s2=got.get("s2"))


def test_fill_bytes_replay_rewrites_the_table(be):
    """a captured ds_fill_bytes carries its values as kernel arguments: after the destination is overwritten and the host
    source cleared, a replay brings the table back bit for bit"""
    for n_bytes in (1028, 2048):
        words = OB.fill_words(n_bytes, 3)
        src = words.copy()
        dst = out(be, n_bytes // 4, np.int32)
        warm = out(be, n_bytes // 4, np.int32)
        be.call("ds_fill_bytes", warm.p(), ctypes.c_void_p(src.ctypes.data), n_bytes)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            be.call("ds_fill_bytes", dst.p(), ctypes.c_void_p(src.ctypes.data), n_bytes)
        src[:] = 0
        dst.h[:n_bytes // 4].fill_(-1)
        graph.replay()
        got = dst.get(f"replayed fill of {n_bytes} bytes")
        assert same_bits(got, words), np.flatnonzero(got != words)[:4]
