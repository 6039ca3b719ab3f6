"""The test bodies of the fused optimizers' suites, written once against the backend adapter of loss_side_bodies.py
(be.full / put / get / p / call / rc / plain) plus, for the Python-layer bodies, be.eng (an Engine on the backend's library)
and be.tensor(host array) -> a torch tensor in the backend's memory.  Run by test_emul_optim.py (host emulator) and
test_gpu_optim_kernels.py (MI355X).

The kernel bodies drive the C ABI of optim.hip directly: they build the pointer tables, `numel`, `chunk_tensor` and
`chunk_index` themselves (class Launch) and do not go through optim.py.  Every parameter, gradient and state tensor of a
launch lies in one arena per role (optim_cases.Arena) inside a loss_side_bodies.Buf: a finite marker between the tensors
(a step applied one element too far changes it) and the NaN guard tail, all of which must survive; gradients must come
back bit-identical.  Bars: optim_cases -- max(FLOOR, 4 x the float32 restatement's error against float64) in max_rel, on
the update p_new - p_old and on every state tensor, printed with the kernel's error; no case is exempt."""
import copy
import ctypes

import numpy as np
import torch

import optim_cases as OC
from loss_side_bodies import SENTINEL, hold, inp, out, same_bits
from optim_cases import F32, F64, FLOOR, max_rel

ENTRY = {"adagrad": "ds_adagrad_step", "sgd": "ds_sgd_step", "sgd_plain": "ds_sgd_step", "adam": "ds_adam_step"}
DEV_COUNTS = (1, 2, 1000)


def entry(kind, dev):
    return ENTRY[kind] + ("_dev_f32" if dev else "_f32")


def chunk_elems(be):
    C = int(be.plain("ds_optim_chunk_elems"))
    assert C >= 512 and C % 256 == 0, C
    return C


def counter(be, t):
    """the device-side step count with a sentinel word on either side; the count is at .p(1)"""
    return inp(be, np.array([SENTINEL, t, SENTINEL], np.int32))


def count_of(cnt):
    a = cnt.get("step count")
    assert a[0] == SENTINEL and a[2] == SENTINEL, "the words on both sides of the counter keep their sentinel"
    return int(a[1])


class Launch:
    """one tensor set in the backend's memory with its tables; `perm`: an order of the chunk table"""

    def __init__(self, be, ar, C, p, g, s1=None, s2=None, perm=None):
        self.be, self.ar = be, ar
        self.host = dict(p=p, g=g, s1=s1, s2=s2)
        self.buf = {k: inp(be, ar.spread(v)) for k, v in self.host.items() if v is not None}
        self.before = {k: ar.spread(v) for k, v in self.host.items() if v is not None}
        self.tab = {k: inp(be, np.array([b.p(o).value for o in ar.offs], np.int64)) for k, b in self.buf.items()}
        self.numel = inp(be, np.array(ar.sizes, np.int64))
        ct, ci = ar.chunks(C)
        if perm is not None:
            ct, ci = ct[perm], ci[perm]
        self.n_chunks = int(ct.size)
        self.ct, self.ci = inp(be, ct), inp(be, ci)
        self.tables_before = [t.get() for t in self._tables()]

    def _tables(self):
        return [self.tab[k] for k in ("p", "g", "s1", "s2") if k in self.tab] + [self.numel, self.ct, self.ci]

    def args(self, **replace):
        """the eight leading arguments of every step entry; replace= a table by None (or n_chunks by a number)"""
        a = dict(p=self.tab["p"].p(), g=self.tab["g"].p(), s1=self.tab["s1"].p() if "s1" in self.tab else None,
                 s2=self.tab["s2"].p() if "s2" in self.tab else None, numel=self.numel.p(), ct=self.ct.p(), ci=self.ci.p(),
                 n_chunks=self.n_chunks)
        a.update(replace)
        return tuple(a[k] for k in ("p", "g", "s1", "s2", "numel", "ct", "ci", "n_chunks"))

    def set_grads(self, g):
        self.host["g"] = g
        self.before["g"] = self.ar.spread(g)
        self.be.put(self.buf["g"].h, self.before["g"])

    def read(self, what=""):
        """live vectors of p, s1, s2 now; the gaps between tensors, the guard tails, the gradients and the tables intact"""
        got = {}
        gap = np.ones(self.ar.total, bool)
        gap[self.ar.live] = False
        for k, b in self.buf.items():
            a = b.get(f"{what} {k}")
            assert same_bits(a[gap], self.before[k][gap]), (what, k, "written between the tensors")
            if k == "g":
                assert same_bits(a, self.before[k]), (what, "gradients come back bit-identical")
            else:
                got[k] = a[self.ar.live]
        for t, was in zip(self._tables(), self.tables_before):
            assert (t.get(f"{what} table") == was).all(), (what, "a table was written")
        return got

    def untouched(self, what=""):
        got = self.read(what)
        return all(same_bits(got[k], self.host[k]) for k in got)


def step_args(kind, hp, t, dev, cnt):
    """the scalars of a step entry after the tables: host-side scalars for step count t, or the counter"""
    sc, wd = OC.step_scalars(kind, hp, t), hp["weight_decay"]
    if kind == "adagrad":
        return (hp["lr"], hp["lr_decay"], wd, hp["eps"], cnt.p(1)) if dev else (sc["clr"], wd, hp["eps"])
    if kind in ("sgd", "sgd_plain"):
        return (hp["lr"], hp["momentum"], hp["dampening"], wd, cnt.p(1) if dev else int(sc["first"]))
    b1, b2 = hp["betas"]
    return (hp["lr"], b1, b2, hp["eps"], wd) + ((cnt.p(1),) if dev else (sc["bc1"], sc["bc2_sqrt"]))


def run_step(be, L, kind, hp, t, dev, flag=None, what=""):
    cnt = counter(be, t) if dev else None
    be.call(entry(kind, dev), *L.args(), *step_args(kind, hp, t, dev, cnt), flag.p() if flag is not None else None)
    got = L.read(what)
    if dev:
        assert count_of(cnt) == t, "a step kernel reads the counter, it does not write it"
    return got


def check_step(tag, kind, hp, t, before, g, got, planted=True):
    """`got` against one float64 step with count t from `before` (live vectors p, s1, s2), under the restatement's bar"""
    p0 = before["p"]
    r64 = OC.step_ref(kind, hp, t, p0, g, before.get("s1"), before.get("s2"), F64)
    r32 = OC.step_ref(kind, hp, t, p0, g, before.get("s1"), before.get("s2"), F32)
    n = p0.size
    bad = ~np.isfinite(g)
    pl = OC.plants(n) if planted else None
    if planted:
        want = np.zeros(n, bool)
        want[pl["inf"] + pl["nan"]] = True
        assert (bad == want).all(), "input condition: exactly the planted gradients are non-finite"
    ok = ~bad
    keys = [k for k in ("p", "s1", "s2") if r64[k] is not None]
    assert sorted(got) == sorted(keys), (tag, sorted(got))
    for k in keys:
        assert r64[k].dtype == F64 and r32[k].dtype == F32, (k, r64[k].dtype, r32[k].dtype)
        assert not np.isfinite(r64[k][bad]).any() and np.isfinite(r64[k][ok]).all(), "the restatement itself"
        assert not np.isfinite(got[k][bad]).any(), (tag, k, "a non-finite gradient makes its own element non-finite")
        assert np.isfinite(got[k][ok]).all(), (tag, k, "and no other element")
    d64 = p0[ok].astype(F64)
    hold(tag, "update", got["p"][ok].astype(F64) - d64, r64["p"][ok] - d64, r32["p"][ok].astype(F64) - d64, FLOOR, max_rel)
    names = dict(zip(("s1", "s2"), OC.STATE_KEYS[kind]))
    for k in keys[1:]:
        hold(tag, names[k], got[k][ok], r64[k][ok], r32[k][ok], FLOOR, max_rel)
    if not planted:
        return
    z = pl["zero"]
    assert same_bits(got["p"][z], p0[z]), (tag, "g = 0 on zero state: an update of exactly 0")
    for k in keys[1:]:
        assert (got[k][z] == 0).all(), (tag, k, "g = 0 on zero state leaves the state 0")
    if kind in OC.TINY_G:
        for i in pl["tiny"]:
            assert p0[i] == 0 and r64["p"][i] != 0
            restated = abs(float(r32["p"][i]) - r64["p"][i]) / abs(r64["p"][i])
            err = abs(float(got["p"][i]) - r64["p"][i]) / abs(r64["p"][i])
            bar = OC.bar_from_restatement(FLOOR, restated)
            print(f"{tag}: tiny gradient at {i}: update {float(got['p'][i]):.6e} reference {r64['p'][i]:.6e} f32-restated "
                  f"{restated:.2e} bar {bar:.2e} kernel {err:.2e}")
            assert err <= bar, (tag, "tiny gradient", i, err, bar)
        if kind == "adagrad":               # eps outside the square root: clr g / (|g| + eps), about 1% of clr; inside: ~0
            clr, gt = OC.step_scalars(kind, hp, t)["clr"], OC.TINY_G[kind]
            assert abs(-r64["p"][pl["tiny"][0]] / (clr * gt / (gt + hp["eps"])) - 1) < 1e-6 and 0.009 < gt / (gt + hp["eps"]) < 0.011
    if kind == "sgd" and t == 1:
        assert np.isnan(before["s1"]).all(), "input condition: the first step finds a NaN momentum buffer"
        if hp["weight_decay"] == 0:
            assert same_bits(got["s1"][ok], g[ok]), (tag, "the first momentum buffer is the gradient")


def step_combos(kind):
    """(step count, lr_decay): the counts of the `_dev` variants; Adagrad's two decays where the count lets them show"""
    if kind == "adagrad":
        return [(1, 1e-4), (2, 1e-4), (2, 0.5), (1000, 1e-4), (1000, 0.5)]
    return [(t, None) for t in DEV_COUNTS]


def body_step(be, kind, set_name):
    """one step of `kind` on a tensor set, weight decay 0 and 1e-3, step counts 1, 2 and 1000: the host-scalar entry and the
    `_dev` entry (counter on the device) each against float64 under the SAME bar -- not bit for bit against each other, the
    device may contract 1 + (t-1) decay.  The offset set also runs with its chunk table shuffled: bit-identical."""
    C = chunk_elems(be)
    ar = OC.tensor_set(set_name, C)
    for wd in (0.0, 1e-3):
        for t, decay in step_combos(kind):
            hp = OC.hyper(kind, wd, decay) if decay is not None else OC.hyper(kind, wd)
            p, g, s1, s2 = OC.step_inputs(kind, ar.n_live, wd, 13 * t + len(set_name), first=kind == "sgd" and t == 1)
            before = dict(p=p, s1=s1, s2=s2)
            results = []
            for dev in (False, True):
                tag = f"{kind} {set_name} wd={wd:g} t={t}" + (f" decay={decay:g}" if decay is not None else "") + (" dev" if dev else " host")
                got = run_step(be, Launch(be, ar, C, p, g, s1, s2), kind, hp, t, dev, what=tag)
                check_step(tag, kind, hp, t, before, g, got)
                results.append(got)
            if set_name == "offset":
                perm = np.random.RandomState(t).permutation(ar.chunks(C)[0].size)
                assert (perm != np.arange(perm.size)).any()
                shuf = run_step(be, Launch(be, ar, C, p, g, s1, s2, perm=perm), kind, hp, t, False, what="shuffled")
                for k in shuf:
                    assert same_bits(shuf[k], results[0][k]), (kind, t, k, "a shuffled chunk table gives identical bits")


def body_skip_flag(be, kind):
    """*skip_flag = 1, -1 or 2: parameters and every state tensor bit-identical to before, both entries; 0: bit-identical to
    a null flag"""
    C = chunk_elems(be)
    ar = OC.tensor_set("edges", C)
    hp, t = OC.hyper(kind, 1e-3), 2
    p, g, s1, s2 = OC.step_inputs(kind, ar.n_live, 1e-3, 99)
    for dev in (False, True):
        for v in (1, -1, 2):
            flag = inp(be, np.array([v], np.int32))
            got = run_step(be, Launch(be, ar, C, p, g, s1, s2), kind, hp, t, dev, flag)
            for k in got:
                assert same_bits(got[k], dict(p=p, s1=s1, s2=s2)[k]), (kind, dev, v, k, "a skipped step writes nothing")
            assert flag.get("flag")[0] == v, "the step kernels read the flag, the optimizer clears it"
        flag = inp(be, np.array([0], np.int32))
        with_flag = run_step(be, Launch(be, ar, C, p, g, s1, s2), kind, hp, t, dev, flag)
        without = run_step(be, Launch(be, ar, C, p, g, s1, s2), kind, hp, t, dev, None)
        assert not same_bits(without["p"], p), "input condition: the step changes the parameters"
        for k in without:
            assert same_bits(with_flag[k], without[k]), (kind, dev, k, "flag 0 is no flag")


def body_step_inc(be):
    """ds_optim_step_inc adds exactly 1, not under a raised flag; the neighbouring words keep their sentinel"""
    for start in (0, 5, 999):
        cnt = counter(be, start)
        be.call("ds_optim_step_inc", cnt.p(1), None)
        assert count_of(cnt) == start + 1
        zero = inp(be, np.array([0], np.int32))
        be.call("ds_optim_step_inc", cnt.p(1), zero.p())
        assert count_of(cnt) == start + 2
        for v in (1, -1, 2):
            flag = inp(be, np.array([v], np.int32))
            be.call("ds_optim_step_inc", cnt.p(1), flag.p())
            assert count_of(cnt) == start + 2 and flag.get("flag")[0] == v, (v, "a skipped step does not count")


FILL_BYTES = (4, 1020, 1024, 1028, 2044, 2048)      # 1028: one word past the first 256-thread sweep; 2048: the whole argument


def fill_words(n_bytes, seed=0):
    return np.random.RandomState(n_bytes + seed).randint(-2 ** 31, 2 ** 31, n_bytes // 4, dtype=np.int64).astype(np.int32)


def body_fill_bytes(be):
    """random words arrive bit-exact, at a 16-byte aligned destination and one word past it; nothing else is written"""
    for n_bytes in FILL_BYTES:
        for off in (0, 1):
            words = fill_words(n_bytes, off)
            dst = out(be, off + n_bytes // 4, np.int32)
            assert dst.p().value % 16 == 0
            be.call("ds_fill_bytes", dst.p(off), ctypes.c_void_p(words.ctypes.data), n_bytes)
            got = dst.get(f"fill {n_bytes} bytes at word {off}")
            assert (got[off:] == words).all(), (n_bytes, off, np.flatnonzero(got[off:] != words)[:4])
            assert (got[:off] == SENTINEL).all(), "the word before the destination"


def body_refusals(be):
    """every refusal returns its documented code before any launch: all outputs untouched"""
    C = chunk_elems(be)
    ar = OC.Arena([5, 300])
    p, g, s1, s2 = OC.step_inputs("adam", ar.n_live, 0.0, 4)
    L = Launch(be, ar, C, p, g, s1, s2)
    cnt = counter(be, 3)
    flagless = (None,)

    def rc(kind, dev, counter_=cnt, **replace):
        return be.rc(entry(kind, dev), *L.args(**replace), *step_args(kind, OC.hyper(kind), 3, dev, counter_), *flagless)

    class _Null:                                    # a counter that is not there
        @staticmethod
        def p(off=0):
            return None

    for kind in OC.KINDS:
        for dev in (False, True):
            for k in ("p", "g", "numel", "ct", "ci"):
                assert rc(kind, dev, **{k: None}) == OC.DS_ERR_NULL, (kind, dev, k)
            assert rc(kind, dev, n_chunks=0) == OC.DS_ERR_BAD_SHAPE and rc(kind, dev, n_chunks=-1) == OC.DS_ERR_BAD_SHAPE
        assert rc(kind, True, counter_=_Null) == OC.DS_ERR_NULL, (kind, "a _dev entry without step_count")
    for dev in (False, True):
        assert rc("adagrad", dev, s1=None) == OC.DS_ERR_NULL, "Adagrad without state1"
        assert rc("sgd", dev, s1=None) == OC.DS_ERR_NULL, "SGD with momentum and without state1"
        assert rc("adam", dev, s2=None) == OC.DS_ERR_NULL and rc("adam", dev, s1=None) == OC.DS_ERR_NULL, "Adam without a state"
    assert be.rc("ds_optim_step_inc", None, None) == OC.DS_ERR_NULL
    assert L.untouched("refused step") and count_of(cnt) == 3

    words = fill_words(2048)
    src = ctypes.c_void_p(words.ctypes.data)
    dst = out(be, 520, np.int32)
    for n_bytes in (0, 2052, 6, -4):
        assert be.rc("ds_fill_bytes", dst.p(), src, n_bytes) == OC.DS_ERR_BAD_SHAPE, n_bytes
    assert be.rc("ds_fill_bytes", None, src, 64) == OC.DS_ERR_NULL
    assert be.rc("ds_fill_bytes", dst.p(), None, 64) == OC.DS_ERR_NULL
    assert be.rc("ds_fill_bytes", ctypes.c_void_p(dst.p().value + 2), src, 64) == OC.DS_ERR_ALIGNMENT
    assert (dst.get("refused fill") == SENTINEL).all(), "a refused call launches nothing"


# ---------------------------------------------------------------------------------------------------------------------
# the Python layer (optim.py on the backend's engine)
# ---------------------------------------------------------------------------------------------------------------------
def make_ours(be, kind, params, hp):
    from deepspeaker_pytorch_amd import optim as fo
    if kind == "adagrad":
        opt = fo.FusedAdagrad(params, **hp)
    elif kind in ("sgd", "sgd_plain"):
        opt = fo.FusedSGD(params, **hp)
    else:
        opt = fo.FusedAdam(params, **hp)
    opt._engine = be.eng
    return opt


def make_torch(kind, params, hp):
    cls = {"adagrad": torch.optim.Adagrad, "sgd": torch.optim.SGD, "sgd_plain": torch.optim.SGD, "adam": torch.optim.Adam}[kind]
    return cls(params, foreach=False, **hp)


def new_params(be, shapes, seed):
    rs = np.random.RandomState(seed)
    return [torch.nn.Parameter(be.tensor((0.5 * rs.randn(*s)).astype(F32))) for s in shapes]


def _cat(tensors):
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in tensors])


def _state(opt, params, key):
    return _cat([opt.state[p][key] if key in opt.state.get(p, {}) else torch.zeros_like(p) for p in params])


def set_grads(be, params, rs):
    """fresh gradient tensors (new allocations; the caller may keep the old ones alive); the live vector"""
    g = rs.randn(sum(p.numel() for p in params)).astype(F32)
    o = 0
    for p in params:
        p.grad = be.tensor(g[o:o + p.numel()].reshape(tuple(p.shape)))
        o += p.numel()
    return g


def checked_step(be, tag, kind, hp, t, opt, params, rs):
    """opt.step() on fresh random gradients against ONE float64 step with count t from the optimizer's own state before"""
    keys = OC.STATE_KEYS[kind]
    before = dict(p=_cat(params), **{f"s{i + 1}": _state(opt, params, k) for i, k in enumerate(keys)})
    g = set_grads(be, params, rs)
    opt.step()
    got = dict(p=_cat(params), **{f"s{i + 1}": _state(opt, params, k) for i, k in enumerate(keys)})
    check_step(tag, kind, hp, t, before, g, got, planted=False)


PY_SHAPES = [(17,), (64, 5), (300,)]


def body_py_load_state_dict(be, kind):
    """load_state_dict into an optimizer that has already stepped in device-step mode: the device counter takes the loaded
    count IN PLACE (a captured step replays with that tensor's address), and the steps after it are the checkpoint's next"""
    hp = OC.hyper(kind, 1e-3, 0.5) if kind == "adagrad" else OC.hyper(kind, 1e-3)
    rs = np.random.RandomState(21)
    ref_p = [torch.nn.Parameter(torch.from_numpy((0.5 * rs.randn(*s)).astype(F32))) for s in PY_SHAPES]
    ref = make_torch(kind, ref_p, hp)
    for _ in range(8):
        for q in ref_p:
            q.grad = torch.from_numpy(rs.randn(*q.shape).astype(F32))
        ref.step()
    ckpt = ref.state_dict()
    params = new_params(be, PY_SHAPES, 22)
    ours = make_ours(be, kind, params, hp).enable_device_step()
    for _ in range(2):
        set_grads(be, params, rs)
        ours.step()
    assert int(ours._dev_step) == 2
    addr = ours._dev_step.data_ptr()
    with torch.no_grad():
        for p, q in zip(params, ref_p):
            p.copy_(be.tensor(q.detach().numpy()))
    ours.load_state_dict(copy.deepcopy(ckpt))
    loaded = 1 if kind == "sgd" else 8               # SGD keeps no count: buffers that exist are past their first step
    assert int(ours._dev_step) == loaded, ("the device counter after load_state_dict", int(ours._dev_step), loaded)
    assert ours._dev_step.data_ptr() == addr, "refilled in place, not replaced"
    for k in (1, 2):
        checked_step(be, f"{kind} after load_state_dict, step {loaded + k}", kind, hp, loaded + k, ours, params, rs)
        assert int(ours._dev_step) == loaded + k and ours._dev_step.data_ptr() == addr


def body_py_state_dict_after_skip(be, kind):
    """device-step mode with a skip flag, three counted steps and one skipped: state_dict() reports the device's 3, and a
    fresh optimizer that loads it takes its next step with count 4"""
    hp = OC.hyper(kind, 0.0, 0.5) if kind == "adagrad" else OC.hyper(kind)
    rs = np.random.RandomState(31)
    params = new_params(be, PY_SHAPES, 32)
    ours = make_ours(be, kind, params, hp).enable_device_step()
    flag = be.tensor(np.zeros(1, np.int32))
    ours.skip_flag = flag
    for t in (1, 2, 3):
        checked_step(be, f"{kind} counted step {t}", kind, hp, t, ours, params, rs)
    flag.fill_(1)
    held = _cat(params)
    set_grads(be, params, rs)
    ours.step()
    assert same_bits(_cat(params), held) and int(ours._dev_step) == 3 and int(flag) == 0
    sd = ours.state_dict()
    steps = [float(s["step"]) for s in sd["state"].values()]
    assert steps == [3.0] * len(params), ("state_dict() after a skipped step", steps)
    fresh_p = [torch.nn.Parameter(p.detach().clone()) for p in params]
    fresh = make_ours(be, kind, fresh_p, hp).enable_device_step()
    fresh.load_state_dict(copy.deepcopy(sd))
    checked_step(be, f"{kind} fresh optimizer, step 4", kind, hp, 4, fresh, fresh_p, rs)
    assert int(fresh._dev_step) == 4


def body_py_many_params(be):
    """FusedAdagrad over 300 tiny parameters and one of C+3 elements: pointer tables of 2408 bytes, which fill() splits at
    2048 and writes at data_ptr() + off; then the same after every gradient tensor is a new allocation (the gkey path)"""
    C = chunk_elems(be)
    shapes = [(1 + i % 7,) for i in range(300)] + [(C + 3,)]
    hp = OC.hyper("adagrad", 1e-3)
    rs = np.random.RandomState(41)
    params = new_params(be, shapes, 42)
    ours = make_ours(be, "adagrad", params, hp)
    checked_step(be, "adagrad 301 parameters, step 1", "adagrad", hp, 1, ours, params, rs)
    cache = ours.param_groups[0]["_ds_cache"][len(params)]
    assert cache["params"].numel() * 8 > 2048 and cache["n_chunks"] == 302
    old = [p.grad for p in params]                  # kept alive: the next gradients cannot land on the same addresses
    gkey = cache["gkey"]
    checked_step(be, "adagrad 301 parameters, step 2, new gradient tensors", "adagrad", hp, 2, ours, params, rs)
    assert ours.param_groups[0]["_ds_cache"][len(params)] is cache, "the static tables are kept"
    assert all(a != b for a, b in zip(cache["gkey"], gkey)) and len(old) == len(params), "every gradient pointer is new"


def body_py_skipped_step(be, kind):
    """test_emul_engine.test_fused_optimizers_device_side_step_count with the per-step float64 reference: six steps, the
    third skipped by the overflow flag -- it neither updates nor counts; sync_host_steps() brings state[p]['step'] up to date"""
    hp = OC.hyper(kind, 0.0, 1e-2) if kind == "adagrad" else OC.hyper(kind)
    rs = np.random.RandomState(5)
    params = new_params(be, [(64, 1, 5, 5), (17,), (20000,)], 6)
    ours = make_ours(be, kind, params, hp).enable_device_step()
    flag = be.tensor(np.zeros(1, np.int32))
    ours.skip_flag = flag
    t = 0
    for it in range(6):
        if it == 2:
            flag.fill_(1)
            held = {k: _state(ours, params, k) for k in OC.STATE_KEYS[kind]}
            held_p = _cat(params)
            set_grads(be, params, rs)
            ours.step()
            assert same_bits(_cat(params), held_p) and int(ours._dev_step) == 2 and int(flag) == 0
            assert all(same_bits(_state(ours, params, k), v) for k, v in held.items())
            continue
        t += 1
        checked_step(be, f"{kind} step {it} (count {t})", kind, hp, t, ours, params, rs)
    assert int(ours._dev_step) == 5
    ours.sync_host_steps()
    if kind != "sgd":
        assert all(float(ours.state[p]["step"]) == 5.0 for p in params)
