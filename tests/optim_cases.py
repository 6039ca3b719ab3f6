"""The fused optimizers (optim.hip) restated in NumPy, and the tensor sets of their two suites (test_emul_optim.py on the
host emulator, test_gpu_optim_kernels.py on the device, through optim_bodies.py).  A plain helper module: host arrays in,
host arrays out; no GPU, no emulator, no fixtures.

`step_ref` is ONE step of Adagrad / SGD / Adam from a given state, in the operation order the comments of optim.hip state,
and takes `dtype`: np.float64 is the reference, np.float32 the plain restatement (every intermediate rounded to float32,
no fma) whose distance from the reference sizes the bar -- loss_side_cases.bar_from_restatement: max(FLOOR, 4 x that
distance), never the kernel's own output.  The per-step scalars (Adagrad's decayed learning rate, Adam's 1 - b1^t and
sqrt(1 - b2^t)) are computed in Python double by `step_scalars`, the way optim.py computes what it hands the host-scalar
entry points.  test_emul_optim.py checks the float64 restatement against torch.optim on float64 parameters.

Metric: max_rel (max |d| / max |ref|) over all tensors of one launch together, applied to every state tensor the step
writes and to the UPDATE p_new - p_old taken in float64 -- not to p_new, whose magnitude would hide an error in the update.
(One figure per launch, not per tensor: a one-element tensor's figure is the rounding of that one parameter, up to half an
ulp of |p| against an update a hundred times smaller, which no restatement of one element sizes reliably; every tensor of
a launch is drawn from the same distributions, so the launch-wide maximum is the same scale for all of them.)

Each comparison is one step from a given state; where steps are chained the reference for step k starts from the kernel's
own state after step k - 1 (Adagrad's first steps are sign-like and amplify last-bit differences: test_gpu_next_rows.py)."""
import math

import numpy as np

from loss_side_cases import FLOOR, bar_from_restatement, max_rel  # noqa: F401  (one definition for every suite)

F32, F64 = np.float32, np.float64
DS_ERR_BAD_SHAPE, DS_ERR_ALIGNMENT, DS_ERR_NULL = -1, -2, -3
KINDS = ("adagrad", "sgd", "sgd_plain", "adam")
STATE_KEYS = {"adagrad": ("sum",), "sgd": ("momentum_buffer",), "sgd_plain": (), "adam": ("exp_avg", "exp_avg_sq")}
GAP = 8                 # elements before, between and after the tensors of an arena, all GAP_VALUE
GAP_VALUE = 3.0         # finite, so that a step applied one element too far CHANGES it (NaN in, NaN out would not show)
TINY_G = {"adagrad": 1e-12, "adam": 1e-9}


def hyper(kind, wd=0.0, lr_decay=1e-4):
    """create_optimizer's hyper-parameters (train_triplet.py:369-383)"""
    if kind == "adagrad":
        return dict(lr=0.1, lr_decay=lr_decay, weight_decay=wd, eps=1e-10)
    if kind == "sgd":
        return dict(lr=0.1, momentum=0.9, dampening=0.9, weight_decay=wd)
    if kind == "sgd_plain":
        return dict(lr=0.1, momentum=0.0, dampening=0.0, weight_decay=wd)
    assert kind == "adam", kind
    return dict(lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)


def step_scalars(kind, hp, t):
    """what depends on the step count t (1-based: the count of the step being taken), in Python double"""
    if kind == "adagrad":
        return dict(clr=hp["lr"] / (1 + (t - 1) * hp["lr_decay"]))
    if kind == "adam":
        b1, b2 = hp["betas"]
        return dict(bc1=1 - b1 ** t, bc2_sqrt=math.sqrt(1 - b2 ** t))
    return dict(first=t == 1)


def adagrad_step(p, g, s, clr, wd, eps, dtype=F64):
    """grad += wd*p; sum += grad*grad; p -= clr * (grad / (sqrt(sum) + eps))"""
    p, g, s = p.astype(dtype), g.astype(dtype), s.astype(dtype)
    if wd != 0:
        g = g + dtype(wd) * p
    s = s + g * g
    return p - dtype(clr) * (g / (np.sqrt(s) + dtype(eps))), s


def sgd_step(p, g, buf, lr, momentum, dampening, wd, first, dtype=F64):
    """grad += wd*p; buf = first ? grad : momentum*buf + (1-dampening)*grad; p -= lr*buf (momentum 0: p -= lr*grad, no buf)"""
    p, g = p.astype(dtype), g.astype(dtype)
    if wd != 0:
        g = g + dtype(wd) * p
    if momentum != 0:
        buf = g if first else dtype(momentum) * buf.astype(dtype) + (dtype(1) - dtype(dampening)) * g
        g = buf
    else:
        buf = None
    return p - dtype(lr) * g, buf


def adam_step(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2_sqrt, dtype=F64):
    """grad += wd*p; m += (grad - m)*(1-b1); v = b2*v + (1-b2)*grad*grad; p -= (lr/bc1) * (m / (sqrt(v)/bc2_sqrt + eps))"""
    p, g, m, v = p.astype(dtype), g.astype(dtype), m.astype(dtype), v.astype(dtype)
    if wd != 0:
        g = g + dtype(wd) * p
    m = m + (g - m) * (dtype(1) - dtype(b1))
    v = dtype(b2) * v + (dtype(1) - dtype(b2)) * g * g
    denom = np.sqrt(v) / dtype(bc2_sqrt) + dtype(eps)
    return p - (dtype(lr) / dtype(bc1)) * (m / denom), m, v


def step_ref(kind, hp, t, p, g, s1=None, s2=None, dtype=F64):
    """one step with count t from (p, s1, s2): dict(p=, s1=, s2=), absent states None"""
    sc = step_scalars(kind, hp, t)
    with np.errstate(all="ignore"):
        if kind == "adagrad":
            pn, s = adagrad_step(p, g, s1, sc["clr"], hp["weight_decay"], hp["eps"], dtype)
            return dict(p=pn, s1=s, s2=None)
        if kind in ("sgd", "sgd_plain"):
            pn, b = sgd_step(p, g, s1, hp["lr"], hp["momentum"], hp["dampening"], hp["weight_decay"], sc["first"], dtype)
            return dict(p=pn, s1=b, s2=None)
        pn, m, v = adam_step(p, g, s1, s2, hp["lr"], hp["betas"][0], hp["betas"][1], hp["eps"], hp["weight_decay"], sc["bc1"],
                             sc["bc2_sqrt"], dtype)
        return dict(p=pn, s1=m, s2=v)


# ---------------------------------------------------------------------------------------------------------------------
# tensor sets: where every tensor of a launch lies in one arena per role (parameters, gradients, each state)
# ---------------------------------------------------------------------------------------------------------------------
class Arena:
    """`sizes[i]` elements for tensor i of the table, GAP or more elements of GAP_VALUE around each.  A tensor starts `mods[i]`
    elements past a 16-byte boundary (default 0); `descending`: table order is descending address order."""

    def __init__(self, sizes, mods=None, descending=False):
        self.sizes = [int(n) for n in sizes]
        mods = list(mods) if mods is not None else [0] * len(self.sizes)
        order = range(len(self.sizes) - 1, -1, -1) if descending else range(len(self.sizes))
        self.offs = [0] * len(self.sizes)
        cur = GAP
        for i in order:
            cur = -(-cur // 4) * 4 + mods[i]
            self.offs[i] = cur
            cur += self.sizes[i] + GAP
        self.total = cur
        self.live = np.concatenate([np.arange(o, o + n, dtype=np.int64) for o, n in zip(self.offs, self.sizes)])
        self.n_live = int(self.live.size)
        assert np.unique(self.live).size == self.n_live and self.live.min() >= GAP and self.live.max() < self.total - GAP

    def spread(self, vec, dtype=F32):
        a = np.full(self.total, GAP_VALUE, dtype)
        a[self.live] = vec
        return a

    def chunks(self, C):
        ct, ci = [], []
        for i, n in enumerate(self.sizes):
            for c in range(-(-n // C)):
                ct.append(i)
                ci.append(c)
        return np.array(ct, np.int32), np.array(ci, np.int32)


def tensor_set(name, C):
    """The smallest sizes that reach every index path of a chunk size C (ds_optim_chunk_elems):
    edges:  1, 255, 256, 257 (the 256-thread sweep), C-1, C, C+1 (one chunk and its neighbours), 2C+232 (three chunks);
    many:   300 tensors of 1..7 elements and one of C+3: more than 256 table entries, chunk_tensor above 255;
    offset: tensors that start 1, 2 and 3 elements past a 16-byte boundary (the kernels promise 4-byte alignment only, what
            a contiguous slice has), listed in descending address order;
    long:   one tensor of 40C+5: chunk_index runs to 40."""
    if name == "edges":
        return Arena([1, 255, 256, 257, C - 1, C, C + 1, 2 * C + 232])
    if name == "many":
        return Arena([1 + i % 7 for i in range(300)] + [C + 3])
    if name == "offset":
        return Arena([C + 1, 257, 5, 1, 2 * C + 3, 64], mods=[1, 2, 3, 1, 3, 2], descending=True)
    assert name == "long", name
    return Arena([40 * C + 5])


SETS = ("edges", "many", "offset", "long")


def plants(n_live):
    """live positions of the planted elements: zero (g = 0 on zero state), tiny (a gradient far below sqrt(eps) on zero
    state), inf and NaN gradients; the last live element (the end of a partial chunk) is a tiny one"""
    assert n_live >= 16
    return dict(zero=[0, n_live // 2], tiny=[1, n_live - 1], inf=[2, n_live // 3], nan=[3, (2 * n_live) // 3])


def step_inputs(kind, n_live, wd, seed, first=False, plant=True):
    """p, g, s1, s2 (absent states None) as live vectors, float32.  States are planted mid-trajectory, not zero: sum and
    exp_avg_sq non-negative, momentum_buffer and exp_avg signed; `first` (SGD): the momentum buffer is NaN, which the
    first step must not read.  Planted elements (`plant`): see plants(); the tiny and (under weight decay) the zero
    elements have p = 0, so that the gradient the step sees is the planted one and the update is not rounded into a
    large p."""
    rs = np.random.RandomState(seed)
    p = (0.1 * rs.randn(n_live)).astype(F32)
    g = rs.randn(n_live).astype(F32)
    s1 = s2 = None
    if kind == "adagrad":
        s1 = (3.0 * rs.rand(n_live)).astype(F32)
    elif kind == "sgd":
        s1 = np.full(n_live, np.nan, F32) if first else (0.3 * rs.randn(n_live)).astype(F32)
    elif kind == "adam":
        s1, s2 = (0.3 * rs.randn(n_live)).astype(F32), rs.rand(n_live).astype(F32)
    if not plant:
        return p, g, s1, s2
    pl = plants(n_live)
    g[pl["zero"]] = 0
    g[pl["inf"]], g[pl["nan"]] = np.inf, np.nan
    if wd != 0:
        p[pl["zero"]] = 0
    if kind in TINY_G:
        g[pl["tiny"]] = TINY_G[kind]
        p[pl["tiny"]] = 0
    for s in (s1, s2):
        if s is not None and not first:
            s[pl["zero"]] = 0
            if kind in TINY_G:
                s[pl["tiny"]] = 0
    return p, g, s1, s2
