"""The angular-margin softmax head (margin_head.hip) on the device: the bodies of margin_head_bodies.py, the same the host
emulator runs (test_emul_margin_head.py), on device memory through the C ABI and through DeepSpeakerModel.  Here they see
what only the device compiler decides -- fma contraction, expf / logf / sqrtf, the 64-lane xor trees, the f32 MFMA of the
split-K GEMM (1, 2, 4 and 8 K-slices) -- and the two cases the emulator leaves out: 768 rows against 1211 and 5994 classes.  Device only as well:
margin_loss forward + backward captured into one graph and replayed, and the refusal of host tensors.

Bars: max(floor, 4 x the error of the plain float32 restatement against float64); floors 1e-6 for loss and log-sum-exp
(the plain head's), 1e-5 for c, the gradients and the sums they are built from (max |d| / max |ref|).  Every test prints
the restatement's error, the bar and the kernel's error (`-s`).

Figures on the MI355X (restatement error -> bar -> kernel; the host emulator's figure in brackets where it differs):
  M=768 n_cls=1211 aam m=0.2 s=30: c 5.4e-07 -> 1e-05 -> 2.5e-07; lse 3.1e-08 -> 1e-06 -> 4.0e-08; row_loss 2.9e-07 ->
    1.2e-06 -> 2.5e-07; loss 3.7e-08 -> 1e-06 -> 3.7e-08; gx 1.3e-06 -> 1e-05 -> 6.1e-07; gw 7.0e-07 -> 1e-05 -> 4.8e-07
  M=768 n_cls=5994 aam m=0.2 s=30: c 5.6e-07 -> 1e-05 -> 2.9e-07; lse 3.8e-08 -> 1e-06 -> 4.7e-08; loss 3.5e-08 -> 1e-06
    -> 6.4e-08; gx 9.1e-07 -> 1e-05 -> 1.6e-06; gw 9.5e-07 -> 1e-05 -> 8.5e-07
  M=33 n_cls=129 K=512 aam m=0.2 s=64: c 3.8e-07 -> 1e-05 -> 2.1e-07; lse 1.1e-07 -> 1e-06 -> 6.4e-08 [6.1e-08];
    gx 9.0e-07 -> 1e-05 -> 3.1e-07; gw 5.5e-07 -> 1e-05 -> 2.4e-07 [2.3e-07]
  fallback plant (c = -0.97 on the fallback branch, +0.89), aam m=0.5 s=30: gc 1.7e-06 -> 1e-05 -> 1.4e-06 [1.6e-06];
    gx 2.6e-06 -> 1.02e-05 -> 2.2e-06 [2.4e-06]
  the same plant at m=0.2 s=64 (c = -0.97 on the main branch, where dphi/dc = 0.19 is a difference of 0.98 and 0.79):
    gc 2.7e-07 -> 1e-05 -> 1.2e-06; r 7.9e-07 -> 1e-05 -> 3.5e-06; q 1.4e-06 -> 1e-05 -> 6.2e-06 -- the largest share of
    a bar any case takes
  saturated row: c 2.6e-08 -> 1e-05 -> 6.0e-08; loss 1.0e-09 -> 1e-06 -> 1.5e-08; gradients finite
  all-negative rows at s = 128 (a pad column in the maximum would give lse = -inf): lse 4.1e-08 -> 1e-06 -> 4.4e-08;
    gx 5.1e-06 -> 2.1e-05 -> 6.4e-06 (aam), 2.2e-06 -> 1e-05 -> 2.4e-06 (am)
  forward alone, one and two K-slices: K=32 M=33 n_cls=129: c 2.7e-07 -> 1e-05 -> 1.7e-07, lse 1.1e-07 -> 1e-06 -> 8.6e-08;
    K=64 M=5 n_cls=129: c 1.4e-07 -> 1e-05 -> 2.2e-07, loss 2.5e-08 -> 1e-06 -> 2.5e-08; K=192: loss 3.7e-08 -> 1e-06 -> 1.6e-07
  margin 0: aam and am bit-identical; against ds_cross_entropy_fwd_f32 on classify_cosine's logits lse 7.1e-08, loss 0
The device's own figures are printed by every run."""
import ctypes

import numpy as np
import pytest
import torch

import margin_head_bodies as MB
import margin_head_cases as MC

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


def case_id(c):
    return "-".join(str(v) for v in c[:-1] if v != "")


@pytest.mark.parametrize("case", MC.MARGIN_CASES, ids=[case_id(c) for c in MC.MARGIN_CASES])
def test_margin_head(be, case):
    MB.body_margin(be, *case[:-1])


@pytest.mark.parametrize("case", MC.FORWARD_CASES, ids=[case_id(c) for c in MC.FORWARD_CASES])
def test_forward_at_one_and_two_k_slices(be, case):
    MB.body_forward_only(be, *case[:-1])


@pytest.mark.parametrize("M,n,K,s", [(5, 129, 512, 30.0), (3, 21, 128, 64.0), (1, 2, 512, 1.0)])
def test_margin_zero_is_the_cosine_head_under_plain_cross_entropy(be, M, n, K, s):
    MB.body_margin_zero_equals_cosine_ce(be, M, n, K, s)


@pytest.mark.parametrize("M,n,K,s", [(5, 129, 512, 30.0), (33, 21, 128, 1.0)])
def test_cosine_backward(be, M, n, K, s):
    MB.body_cosine_bwd(be, M, n, K, s)


def test_abi_refusals(be):
    MB.body_abi_errors(be)


@pytest.mark.parametrize("kind", ["aam", "am"])
def test_margin_loss_autograd_and_pack_cache(be, kind):
    MB.body_autograd(be, kind)


def test_classify_cosine_autograd(be):
    MB.body_cosine_autograd(be)


def test_python_argument_checks(be):
    MB.body_python_errors(be)


def test_host_tensors_are_refused(be):
    model = MB.make_model(be, 21)
    x, _, labels = MC.margin_inputs(4, 21, 512, "", 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.margin_loss(torch.from_numpy(x), be.tensor(labels))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.margin_loss(be.tensor(x), torch.from_numpy(labels))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.classify_cosine(torch.from_numpy(x))


def test_margin_loss_forward_and_backward_replay_from_one_graph(be):
    """forward + backward captured into one graph the way train_graph.GraphedTripletStep captures its step (warm-up on a
    side stream, thread-local capture mode: the backward kernels are enqueued by autograd's worker thread), with the
    default queue count and nothing about replay configured: one replay on new contents of the static inputs gives the
    eager result bit for bit"""
    M, n = 33, 129
    model = MB.make_model(be, n)
    cls = model.model.classifier
    x0, _, lab0 = MC.margin_inputs(M, n, 512, "", 1)
    x1, _, lab1 = MC.margin_inputs(M, n, 512, "", 2)

    def step(emb, lab):
        emb.grad = cls.weight.grad = None
        loss = model.margin_loss(emb, lab, margin=0.2, scale=30.0, kind="aam")
        loss.backward()
        return loss.detach()

    emb = be.tensor(x1).requires_grad_(True)
    eager = (step(emb, be.tensor(lab1)).clone(), emb.grad.clone(), cls.weight.grad.clone())
    s_emb, s_lab = be.tensor(x0).requires_grad_(True), be.tensor(lab0)
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        step(s_emb, s_lab)
    cur.wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        s_loss = step(s_emb, s_lab)
    with torch.no_grad():
        s_emb.copy_(be.tensor(x1))
        s_lab.copy_(be.tensor(lab1))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(s_loss, eager[0]) and torch.equal(s_emb.grad, eager[1])
    assert torch.equal(cls.weight.grad, eager[2]) and cls.bias.grad is None
