"""The angular-margin softmax head (margin_head.hip) on the host emulator: the bodies of margin_head_bodies.py on host
memory, every case of margin_head_cases.py but the two pre-training sizes (marked "gpu": test_gpu_margin_head.py).  What
this suite checks is the kernels' logic -- indexing, padding, the label column, branch selection, fixed summation orders,
refusals -- and the Python layer (autograd, the pack cache, argument checks); what only the device compiler decides (fma
contraction, expf / logf, the f32 MFMA) is the device suite's.

Also here, CPU only: the float64 restatement the bars rest on against torch float64 autograd, the one constant shared by
header, binding and restatement, and the fused optimizers with a classifier bias that has no gradient."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import margin_head_bodies as MB
import margin_head_cases as MC
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


@pytest.fixture
def model_be(be, monkeypatch):
    """DeepSpeakerModel's head methods on the emulator: the module's engine is the emulator's, host tensors are let in"""
    from deepspeaker_pytorch_amd import model as M
    monkeypatch.setattr(M, "_engine", be.eng)
    monkeypatch.setattr(M, "_require_cuda", lambda t, what: None)
    return be


def case_id(c):
    return "-".join(str(v) for v in c[:-1] if v != "")


_EMUL = MC.emul_cases(MC.MARGIN_CASES)


@pytest.mark.parametrize("case", _EMUL, ids=[case_id(c) for c in _EMUL])
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
def test_margin_loss_autograd_and_pack_cache(model_be, kind):
    MB.body_autograd(model_be, kind)


def test_classify_cosine_autograd(model_be):
    MB.body_cosine_autograd(model_be)


def test_python_argument_checks(model_be):
    MB.body_python_errors(model_be)


def test_fused_optimizers_step_a_head_whose_bias_has_no_gradient(model_be):
    """margin_loss leaves classifier.bias.grad None: the fused optimizers update the weight (visibly to the pack's version
    key) and neither touch nor count the bias"""
    from deepspeaker_pytorch_amd import optim as fo
    be = model_be
    x, _, labels = MC.margin_inputs(6, 21, 512, "", 9)
    for make in (lambda p: fo.FusedAdagrad(p, lr=0.1), lambda p: fo.FusedSGD(p, lr=0.1, momentum=0.9),
                 lambda p: fo.FusedAdam(p, lr=0.01)):
        model = MB.make_model(be, 21)
        cls = model.model.classifier
        opt = make([cls.weight, cls.bias])
        opt._engine = be.eng
        w0, b0, bver = cls.weight.detach().clone(), cls.bias.detach().clone(), cls.bias._version
        pack = model._margin_head()
        model.margin_loss(be.tensor(x), be.tensor(labels)).backward()
        assert cls.bias.grad is None and cls.weight.grad is not None
        opt.step()
        assert not torch.equal(cls.weight.detach(), w0) and torch.equal(cls.bias.detach(), b0) and cls.bias._version == bver
        assert cls.bias not in opt.state or "step" not in opt.state[cls.bias]
        assert model._margin_head() is not pack, "the update is visible to the pack's key"


# ---- CPU only: the restatement, the constant, the tables ----
@pytest.mark.parametrize("kind", ["aam", "am"])
@pytest.mark.parametrize("m,s", [(0.2, 30.0), (0.5, 64.0), (0.0, 1.0)])
def test_float64_restatement_equals_torch_autograd(kind, m, s):
    """the closed-form backward of margin_head_cases.margin_ref against torch float64 autograd of the forward written with
    torch's own operators; row 0 on ArcFace's fallback side of the plants (c = -0.97), row 1 at c = 0.89"""
    M, n, K = 5, 21, 512
    x, w, labels = MC.margin_inputs(M, n, K, "fallback", 11)
    ref = MC.margin_ref(x, w, labels, s, m, kind, gloss=1.7)
    assert ref["label_cos"][0] < -0.96 and ref["label_cos"][1] > 0.88
    tx, tw = torch.from_numpy(x).double().requires_grad_(True), torch.from_numpy(w).double().requires_grad_(True)
    tl = torch.from_numpy(labels)
    c = torch.nn.functional.linear(torch.nn.functional.normalize(tx, dim=1, eps=0), torch.nn.functional.normalize(tw, dim=1, eps=0))
    cy = c[torch.arange(M), tl]
    if kind == "am":
        phi = cy - m
    else:
        sn = torch.sqrt(torch.clamp(1 - cy * cy, min=MC.SIN2_FLOOR))
        phi = torch.where(cy > -np.cos(m), cy * np.cos(m) - sn * np.sin(m), cy - m * np.sin(m))
    z = (s * c).scatter(1, tl[:, None], (s * phi)[:, None])
    loss = torch.nn.functional.cross_entropy(z, tl)
    (loss * 1.7).backward()
    for name, got, want in (("c", ref["c"], c.detach().numpy()), ("loss", ref["loss"], loss.item()),
                            ("gx", ref["gx"], tx.grad.numpy()), ("gw", ref["gw"], tw.grad.numpy())):
        err = float(np.abs(np.asarray(got) - np.asarray(want)).max())
        print(f"{kind} m={m} s={s}: {name} restatement against torch float64 {err:.2e}")
        assert err <= 1e-12, (name, err)


def test_sin2_floor_is_one_constant():
    from deepspeaker_pytorch_amd import _native
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "deepspeaker_hip.h")).read()
    (value,) = re.findall(r"#define\s+DS_MARGIN_SIN2_FLOOR\s+([0-9.eE+-]+)f", header)
    assert float(value) == _native.DS_MARGIN_SIN2_FLOOR == MC.SIN2_FLOOR == 1e-6
    assert (_native.DS_MARGIN_AAM, _native.DS_MARGIN_AM) == (0, 1) == (MC.KINDS["aam"], MC.KINDS["am"])
    assert re.search(r"#define\s+DS_MARGIN_AAM\s+0\b", header) and re.search(r"#define\s+DS_MARGIN_AM\s+1\b", header)
    source = open(os.path.join(root, "deepspeaker-pytorch_amd", "csrc", "margin_head.hip")).read()
    assert "DS_MARGIN_SIN2_FLOOR" in source and "1e-6" not in source, "the kernels name the constant, they do not repeat it"


def test_case_tables_name_every_listed_edge():
    t = MC.MARGIN_CASES
    assert {c[0] for c in t} >= {1, 3, 4, 5, 33, 768} and {c[1] for c in t} >= {2, 21, 64, 65, 127, 128, 129, 1211, 5994}
    assert {c[2] for c in t} == {128, 256, 384, 512} and {c[2] for c in MC.FORWARD_CASES} == {32, 64, 96, 192}
    assert {c[2] for c in t} | {c[2] for c in MC.FORWARD_CASES} == set(MC.EXPECTED_S)
    from loss_side_cases import fc_splits
    assert all(fc_splits(K) == S for K, S in MC.EXPECTED_S.items()) and set(MC.EXPECTED_S.values()) == {1, 2, 4, 8}
    assert {c[3] for c in MC.FORWARD_CASES} == {"aam", "am"} and {MC.EXPECTED_S[c[2]] for c in MC.FORWARD_CASES} == {1, 2}
    assert {(c[3], c[4], c[5]) for c in t} >= {(k, m, s) for k in ("aam", "am") for m in (0.0, 0.2, 0.5) for s in (1.0, 30.0, 64.0)}
    assert {(c[3], c[6]) for c in t} >= {(k, p) for k in ("aam", "am") for p in ("fallback", "saturated", "zero", "padwin", "padwin_deep")}
    for M, n in ((5, 129), (33, 129)):
        labels = MC.label_plan(M, n, np.random.RandomState(0))
        assert labels[0] == 0 and labels[M - 1] == n - 1 and labels[1] == 128
    assert len(MC.emul_cases(t)) == len(t) - 2
