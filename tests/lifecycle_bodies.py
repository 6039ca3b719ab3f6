"""Bodies of the lifecycle suite: the HOST-side state around the kernels across several steps of a loop -- the fp16 step's
overflow latch and loss scale, the precision guard's cadence, the scheduler workspace the persistent kernels draw their
tile counters from.  test_emul_lifecycle.py runs them on the host emulator, test_gpu_lifecycle.py on the device; the
bodies that need a HIP graph (`body_replayed_overflow`, `body_capture_with_drained_pool`) are the device's alone.

An environment `env` has: `name`, `is_device`, `lib` (the NativeLib), `eng` (its Engine), `tensor(numpy) -> torch tensor`
where the kernels compute, `model(**kw) -> DeepSpeakerModel` there with seeded weights (n_stages = 2), `batch` / `frames`
(the geometry of one member's input) and `classes`.

References are plain Python: `scaler_rule` restates the GradScaler rule `update_loss_scale` documents; parameters that a
skipped step must leave alone are compared bit for bit; everything else the bodies assert is a count."""
import ctypes
import gc
import os
import time

import numpy as np
import torch

import deepspeaker_oracle as O

N_STAGES = 2
MARGIN = 30.0                   # above any distance between x10-normalised embeddings: every hinge of a batch of 4 is
                                # active, so no step's gradient is zero by chance and "a clean step updates" can be asserted
MIN_GAP = 4
GENERATIONS = 12


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def inputs(env, seed, members=1):
    xs = [env.tensor(O.make_input(seed=seed + i, batch=env.batch, frames=env.frames)) for i in range(members)]
    return xs if members > 1 else xs[0]


# ---- 1. overflow latch and loss scale ------------------------------------------------------------------------
SEQUENCE = "COCCOOCCCC"         # C clean, O overflow
SCALE0, MAX_SCALE, GROWTH_INTERVAL = 2.0, 2.0, 2
WAYS = ("fused", "fused_by_hand", "torch_sgd", "torch_sgd_accumulate")


def scaler_rule(scale, clean, overflow, backoff=0.5, growth=2.0, growth_interval=GROWTH_INTERVAL, max_scale=MAX_SCALE,
                floor=1.0):
    """torch.amp.GradScaler.update as update_loss_scale documents it, restated: (new scale, new count of clean steps)"""
    if overflow:
        return max(floor, scale * backoff), 0
    clean += 1
    if clean >= growth_interval:
        return min(max_scale, scale * growth), 0
    return scale, clean


def scripted_scales():
    """the restatement over SEQUENCE; it must itself visit growth, back-off, the floor and the cap"""
    scale, clean, out, seen = SCALE0, 0, [], set()
    for c in SEQUENCE:
        new, clean = scaler_rule(scale, clean, c == "O")
        if c == "O":
            seen.add("floor" if scale * 0.5 < 1.0 and new == 1.0 else "backoff")
        elif new > scale:
            seen.add("growth")
        elif clean == 0:
            seen.add("cap")                     # the interval ran out and the scale stayed: min(max_scale, .)
        scale = new
        out.append(scale)
    assert seen == {"growth", "backoff", "floor", "cap"} and len(SEQUENCE) >= 10, seen
    return out


class _Boost(torch.autograd.Function):          # identity forward; backward multiplies dL/de by 1e9 (test_gpu_train_f16.py):
    @staticmethod                                # the scaled gradients of that pass leave fp16's range
    def forward(ctx, e):
        return e.view_as(e)

    @staticmethod
    def backward(ctx, g):
        return g * 1e9


def _flat(tensors):
    return torch.cat([t.detach().reshape(-1).float() for t in tensors]).clone()


def _opt_state(opt, params):
    keep = []
    for p in params:
        for k, v in sorted(opt.state.get(p, {}).items()):
            if torch.is_tensor(v) and v.numel() > 1:
                keep.append(v)
    return _flat(keep) if keep else torch.zeros(0)


def body_overflow_sequence(env, way):
    """SEQUENCE stepped `way`; after every step the value update_loss_scale() returns and model.loss_scale equal the
    restatement exactly, a clean step reads clean, and (where the loop has a step that can be skipped: the fused
    optimizers, and every loop that gates on consume_overflow()) an O step leaves parameters and optimizer state bit for
    bit alone while a C step changes them.

    Overflows are PLANTED two ways: `_Boost` on one member of the pass (a real overflow: inf / NaN gradients) where the
    step is skipped, the pending flag raised by hand (passes only OR into it, so it reads as an earlier pass that
    overflowed; the gradients stay finite) where the loop steps regardless, as the reference loop does."""
    from deepspeaker_pytorch_amd.model import TripletMarginLoss
    from deepspeaker_pytorch_amd.optim import FusedSGD, create_optimizer
    m = env.model(precision="f16", train_precision="f16", loss_scale=SCALE0).train()
    params = [p for n, p in m.named_parameters() if not n.startswith("model.classifier")]
    if way == "fused":
        opt = create_optimizer(m, 0.01, "adagrad", lr_decay=1e-2)
    elif way == "fused_by_hand":
        opt = FusedSGD(m.parameters(), lr=0.01, momentum=0.9, dampening=0.9)        # no skip_flag, no skip_source
        assert opt.skip_flag is None
    else:
        opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9)
    if way.startswith("fused") and not env.is_device:
        opt._engine = env.eng
    xs = inputs(env, 300, members=3)
    weight = env.tensor(np.random.RandomState(5).randn(env.batch, 512).astype(np.float32) * 0.1)
    loss_fn = TripletMarginLoss(MARGIN)
    flag = m.grad_overflow_flag()
    want = scripted_scales()
    counted = 0
    for it, c in enumerate(SEQUENCE):
        bad = c == "O"
        before_p, before_s = _flat(params), _opt_state(opt, params)
        opt.zero_grad(set_to_none=True)
        if way == "fused":                                      # the whole step is the fused path's: nothing for the loop to call
            if env.is_device:                                   # the triplet step, the overflow in ONE member's gradient
                out = m.forward_triplet(*xs)
                if bad:
                    out = (out[0], out[1], _Boost.apply(out[2]))
                loss_fn.forward(*out).backward()
            else:                                               # (the emulator takes seconds per pass: one member)
                e = m(xs[0])
                ((_Boost.apply(e) if bad else e) * weight).sum().backward()
            assert int(flag) == int(bad)
            opt.step()
            assert int(flag) == 0                               # consumed on the device by the step that honoured it
            stepped = not bad
        elif way == "torch_sgd":                                # the reference loop: it steps whatever happened
            (m(xs[0]) * weight).sum().backward()
            if bad:
                flag.fill_(1)
            opt.step()
            stepped = None
        else:                                                   # loops that gate their step on consume_overflow()
            passes = 2 if way == "torch_sgd_accumulate" else 1
            for k in range(passes):
                e = m(xs[k])
                if bad and k == 0:
                    if way == "torch_sgd_accumulate":
                        e = _Boost.apply(e)                     # the overflow is in the FIRST of the two passes
                (e * weight).sum().backward()
                if bad and k == 0 and way == "fused_by_hand":
                    flag.fill_(1)
            assert int(flag) == int(bad), "a clean later pass must not hide an earlier overflow"
            stepped = not m.consume_overflow()
            assert stepped == (not bad) and int(flag) == 0
            assert m.grad_overflow == bad                       # the verdict stays readable until update_loss_scale()
            if stepped:
                opt.step()
        got = m.update_loss_scale(growth_interval=GROWTH_INTERVAL, max_scale=MAX_SCALE)
        assert got == bad, (way, it, c, got)
        assert m.loss_scale == want[it], (way, it, c, m.loss_scale, want[it])
        if not bad:
            assert not m.grad_overflow, (way, it, c, "a clean step reads clean, whatever the steps before it did")
        if stepped is not None:
            after_p, after_s = _flat(params), _opt_state(opt, params)
            if stepped:
                counted += 1
                assert not same_bits(after_p, before_p), (way, it, c)
                assert after_s.numel() and not same_bits(after_s, before_s), (way, it, c)
            else:
                assert same_bits(after_p, before_p), (way, it, c, "a skipped step must leave every parameter alone")
                assert same_bits(after_s, before_s), (way, it, c, "... and the optimizer state")
            assert bool(torch.isfinite(after_p).all())
        if way == "fused":
            assert int(opt._dev_step) == counted, (it, int(opt._dev_step), counted)
    assert m.loss_scale == MAX_SCALE
    if way not in ("fused", "torch_sgd"):       # a loop with a static scale: consume_overflow() alone, never update_loss_scale()
        flag.fill_(1)
        assert m.consume_overflow() and m.grad_overflow and int(flag) == 0
        assert not m.consume_overflow() and not m.grad_overflow, "the next consumed clean step reads clean"


# ---- 3. guard cadence ------------------------------------------------------------------------------------------
def body_guard_cadence(env, per_generation):
    """min_gap = 4; after the first check, 12 weight generations with `per_generation` eval forwards each: the synchronous
    checks added are at most forwards // min_gap + 1 (each is a double-path forward plus a host synchronisation), at
    least one (the first change after a stable stretch is measured at once), the verdict and the embeddings stay those of
    an unguarded fp16 model; and a change after min_gap stable forwards is measured at once again."""
    m = env.model(precision="f16", f16_guard=0.5).eval()
    plain = env.model(precision="f16", f16_guard=None).eval()
    assert plain.f16_guard is None
    g = m.f16_guard
    g.min_gap = MIN_GAP
    x = inputs(env, 400)

    def bump():
        with torch.no_grad():
            m.model.conv1.weight.mul_(1.0)      # a new weight generation (test_emul_guard.py), the same values

    with torch.no_grad():
        want = plain(x).clone()
        assert same_bits(m(x), want) and g.checks == 1
        first, forwards = g.checks, 0
        t0 = time.perf_counter()
        for _ in range(GENERATIONS):
            bump()
            for _ in range(per_generation):
                e = m(x)
                forwards += 1
                assert g.verdict == "f16" and same_bits(e, want)
        dt = time.perf_counter() - t0
        added = g.checks - first
        print(f"[{env.name}] guard cadence: {per_generation} forward(s) per generation, {forwards} forwards, "
              f"{added} synchronous checks (bound {forwards // MIN_GAP + 1}), {1e3 * dt / forwards:.2f} ms per forward")
        assert 1 <= added <= forwards // MIN_GAP + 1, (per_generation, added, forwards)
        assert g.calls == 1 + forwards and g.escalations == 0
        for _ in range(MIN_GAP):                # a stable stretch ...
            m(x)
        n = g.checks
        bump()                                  # ... then ONE change: measured at once
        assert same_bits(m(x), want) and g.checks == n + 1


# ---- 4(a). the scheduler workspace outlives the instance that allocated it ---------------------------------------
def _block_launch(env):
    """a ds_conv_block_f16 launch on a supported geometry: returns (run() -> output tensor, what it keeps alive)"""
    lib, eng = env.lib, env.eng
    b, h, w, c = 2, 8, 32, 64
    assert lib.raw("ds_conv_block_f16_supported")(b, h, w, c) == 1
    rs = np.random.RandomState(17)

    def dev(a):
        if env.is_device:
            return env.tensor(a)
        from emul_util import aligned
        h_ = aligned(a.shape, a.dtype)          # 64-byte aligned host memory (the kernels do 16-byte accesses)
        h_[...] = a
        return torch.from_numpy(h_)

    x = dev((np.abs(rs.randn(b, h, w, c)) * 2).astype(np.float16))
    packs, folds = [], []
    for _ in range(2):
        wt = dev((rs.randn(c, c, 3, 3) / np.sqrt(c * 9)).astype(np.float32))
        wp = dev(np.zeros(wt.numel(), np.float16))
        lib.call("ds_pack_conv_weight_f16", eng._p(wt), eng._p(wp), c, c, 3, eng._stream(wt))
        packs.append(wp)
        folds.append((dev(rs.uniform(0.5, 1.5, c).astype(np.float32)), dev((rs.randn(c) * 0.5).astype(np.float32))))
    y = dev(np.zeros((b, h, w, c), np.float16))

    def run():
        lib.call("ds_conv_block_f16", eng._p(x), eng._p(packs[0]), eng._p(packs[1]), eng._p(folds[0][0]), eng._p(folds[0][1]),
                 eng._p(folds[1][0]), eng._p(folds[1][1]), eng._p(y), b, h, w, c, 0, eng._stream(x))
        return y
    return run, (x, packs, folds, y)


def body_workspace_outlives_its_instance(env):
    """A second NativeLib on the same path hands the library a workspace and is garbage-collected: the pool inside the
    shared library is process-wide and goes on carving slots from that buffer, so the buffer must still be referenced from
    `_native` (a registry keyed by library path and device).  On the emulator a persistent launch through the FIRST
    instance afterwards equals its result before; on the device only the retention is asserted."""
    from deepspeaker_pytorch_amd import _native
    lib = env.lib
    run = None
    if not env.is_device:
        run, keep = _block_launch(env)
        before = run().clone()
        assert float(before.float().abs().max()) > 0
    second = _native.NativeLib(lib.path, host_memory=lib.host_memory)
    handed = []
    raw = second._ds_sched_set_workspace

    def spy(ptr, nbytes):
        handed.append((ptr.value if isinstance(ptr, ctypes.c_void_p) else int(ptr), int(nbytes)))
        return raw(ptr, nbytes)
    second._ds_sched_set_workspace = spy
    free0 = int(lib.raw("ds_sched_free_slots")())
    second.add_sched_workspace("cuda" if env.is_device else None)       # (no index: the registry's key must carry one)
    assert len(handed) == 1 and handed[0][1] == int(lib.raw("ds_sched_workspace_bytes")())
    assert int(lib.raw("ds_sched_free_slots")()) == free0 + handed[0][1] // 64       # the ONE pool both instances share
    del second, raw, spy
    gc.collect()
    registry = getattr(_native, "_SCHED_WORKSPACES", {})
    held = {b.data_ptr(): (key, b) for key, bufs in registry.items() for b in bufs}
    assert handed[0][0] in held, "the buffer the library still carves slots from died with the instance that allocated it"
    key, buf = held[handed[0][0]]
    assert key[0] == os.path.realpath(lib.path) and buf.numel() * buf.element_size() == handed[0][1]
    assert key[1] == (str(env.device) if env.is_device else "cpu"), key      # the canonical name: "cuda:0", never "cuda"
    assert any(b is buf for b in _native.sched_workspaces(lib.path))
    if run is not None:
        assert not bool(buf.any())              # slots are zero between launches
        assert same_bits(run(), before)


# ---- 2. a replayed step that overflows (device only) -------------------------------------------------------------
def _train_pair(env):
    from deepspeaker_pytorch_amd.optim import create_optimizer
    m = env.model(precision="f16", train_precision="f16").train()
    return m, create_optimizer(m, 0.01, "adagrad", lr_decay=1e-2)


def _state_tensors(opt):
    return [v for st in opt.state.values() for k, v in sorted(st.items()) if torch.is_tensor(v) and v.numel() > 1]


def body_replayed_overflow(env):
    """GraphedTripletStep at fp16 with Adagrad and lr_decay over 5 replays, the pending flag raised by hand before replay
    3: that replay leaves parameters, optimizer state and the device step count bit for bit alone, clears the flag and
    latches it; replays 4 and 5 update; the run equals an eager loop treated the same way."""
    from deepspeaker_pytorch_amd.model import TripletMarginLoss
    from deepspeaker_pytorch_amd.train_graph import GraphedTripletStep
    assert env.is_device
    batches = [inputs(env, 500 + 10 * b, members=3) for b in range(2)]
    steps, planted = 5, 2                       # (0-based: the third step)
    loss_fn = TripletMarginLoss(MARGIN)
    m, opt = _train_pair(env)
    eager = []
    for it in range(steps):
        if it == planted:
            m.grad_overflow_flag().fill_(1)
        loss = loss_fn.forward(*m.forward_triplet(*batches[it % 2]))
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        eager.append(float(loss))
    p_eager = {n: p.detach().clone() for n, p in m.named_parameters()}
    b_eager = {n: b.detach().clone() for n, b in m.named_buffers()}
    assert int(opt._dev_step) == steps - 1

    m2, opt2 = _train_pair(env)
    graphed = []
    t0 = time.perf_counter()
    with GraphedTripletStep(m2, opt2, margin=MARGIN, example=batches[0]) as gstep:
        build_s = time.perf_counter() - t0
        params = [p for n, p in m2.named_parameters() if not n.startswith("model.classifier")]
        flag, state = m2.grad_overflow_flag(), m2.__dict__["_overflow_state"]
        for it in range(steps):
            if it == planted:
                flag.fill_(1)
            held_p, held_s, held_n = _flat(params), _flat(_state_tensors(opt2)), int(opt2._dev_step)
            graphed.append(float(gstep(*batches[it % 2])))
            torch.cuda.synchronize()
            now_p, now_s = _flat(params), _flat(_state_tensors(opt2))
            if it == planted:
                assert same_bits(now_p, held_p), "the replay that overflowed must leave every parameter alone"
                assert same_bits(now_s, held_s) and int(opt2._dev_step) == held_n
                assert state.tolist() == [0, 1] and m2.grad_overflow        # cleared, and latched
            else:
                assert not same_bits(now_p, held_p) and not same_bits(now_s, held_s), it
                assert int(opt2._dev_step) == held_n + 1
                assert state.tolist() == [0, 0] and not m2.grad_overflow
    print(f"[{env.name}] replayed overflow: GraphedTripletStep built in {build_s:.2f} s; eager  ", " ".join(f"{v:.6f}" for v in eager))
    print(f"[{env.name}]                                                           graphed", " ".join(f"{v:.6f}" for v in graphed))
    np.testing.assert_allclose(graphed, eager, rtol=2e-5, atol=1e-7)
    worst = max(float((p.detach() - p_eager[n]).abs().max() / p_eager[n].abs().max().clamp_min(1e-12))
                for n, p in m2.named_parameters() if not n.startswith("model.classifier"))
    assert worst < 1e-5, worst
    for n, b in m2.named_buffers():             # running statistics (and batch counts) advanced on all five steps
        assert torch.allclose(b.float(), b_eager[n].float(), rtol=1e-5, atol=1e-6), n
        if n.endswith("num_batches_tracked"):
            assert int(b) == 3 * steps, (n, int(b))
    assert all(float(st["step"]) == steps - 1 for st in opt2.state.values() if "step" in st)     # after close()
    assert sum("step" in st for st in opt2.state.values()) >= len(params)


# ---- 4(b). capture with the pool nearly used up (device only) ----------------------------------------------------
def _drain(env, leave, graphs):
    """Take scheduler slots out of the pool until `leave` are free: ds_conv_block_f16 draws one per launch unconditionally,
    and a launch that is CAPTURED keeps its slot for good.  The throwaway graphs are never replayed: capturing executes
    nothing."""
    lib = env.lib
    run, keep = _block_launch(env)
    run()                                       # eager once: the kernel's LDS opt-in, this stream's ring
    torch.cuda.synchronize()
    free = int(lib.raw("ds_sched_free_slots")())
    assert free >= leave, (free, leave)
    todo = free - leave
    while todo > 0:
        n = min(todo, 300)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(n):
                run()
        graphs.append((g, keep))
        todo -= n
    assert int(lib.raw("ds_sched_free_slots")()) == leave


def _ring_every_stream(env):
    """An eager persistent launch on every stream torch hands out (its pool deals them round robin), so that each owns
    its 8-slot eager ring BEFORE anything is drained.  A warm-up on a stream WITHOUT a ring would carve one, fail on a
    drained pool, and have `_with_workspace` add a buffer eagerly -- the capture after it would then find its slots with
    or without the reservation under test.  Returns the number of distinct streams."""
    run, keep = _block_launch(env)
    cur = torch.cuda.current_stream()
    handles = set()
    for _ in range(128):                        # (four times the 32 streams of torch's pool; the premise is asserted below)
        s = torch.cuda.Stream()
        s.wait_stream(cur)
        with torch.cuda.stream(s):
            run()
        handles.add(s.cuda_stream)
    torch.cuda.synchronize()
    return len(handles)


class _AddSpy:
    """records every add_sched_workspace() of `lib`: was a capture under way, and how many persistent launches had been
    made by then"""

    def __init__(self, lib):
        self.lib, self.calls = lib, []
        self.inner = lib.add_sched_workspace

    def __enter__(self):
        def spy(*a, **kw):
            self.calls.append((bool(torch.cuda.is_current_stream_capturing()), self.lib.persistent_launches))
            return self.inner(*a, **kw)
        self.lib.add_sched_workspace = spy
        return self

    def __exit__(self, *exc):
        del self.lib.add_sched_workspace        # (the instance attribute: the class's method is back)
        return False

    def check(self, what, launches_of_the_capture):
        """the pool was topped up, outside any capture, and AFTER the warm-up: nothing but the captured launches followed"""
        assert self.calls, f"{what}: the pool had fewer slots than the capture keeps, and nothing was added"
        assert not any(capturing for capturing, _ in self.calls), (what, self.calls)
        after = [self.lib.persistent_launches - n for _, n in self.calls]
        assert all(k == launches_of_the_capture for k in after), \
            (what, "a buffer was added DURING the warm-up (a launch found no slot), not by the reservation before the "
             "capture", after, launches_of_the_capture)


def body_capture_with_drained_pool(env):
    """One GraphedTripletStep build says how many slots a captured step keeps.  With ONE FEWER left in the pool a second
    GraphedTripletStep must still build, and with one fewer than an eval forward launches a GraphedEmbedder: they top the
    pool up BEFORE capturing, outside the capture, where add_sched_workspace is allowed -- seen by a spy on that method:
    called outside a capture, after the warm-up's last launch.  Their replays equal the eager results.

    Every stream owns its eager ring beforehand (`_ring_every_stream`), so a warm-up draws nothing from the pool and the
    slots left are exactly what the capture finds: without the reservation both captures run out (add_sched_workspace
    raises inside a capture), whatever margin the reservation adds."""
    from deepspeaker_pytorch_amd.model import TripletMarginLoss
    from deepspeaker_pytorch_amd.train_graph import GraphedTripletStep
    assert env.is_device
    lib = env.lib
    free = lambda: int(lib.raw("ds_sched_free_slots")())
    batches = [inputs(env, 600 + 10 * b, members=3) for b in range(2)]
    # every model is built (and moved to the device: that tops the pool up to 64 free slots) BEFORE the pool is drained
    m1, opt1 = _train_pair(env)
    m, opt = _train_pair(env)
    m2, opt2 = _train_pair(env)
    me = env.model(precision="f16").eval()
    streams = _ring_every_stream(env)
    # the eager results, and what one step / one forward launches
    loss_fn = TripletMarginLoss(MARGIN)
    eager, per_step = [], None
    for it in range(3):
        n = lib.persistent_launches
        loss = loss_fn.forward(*m.forward_triplet(*batches[it % 2]))
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        eager.append(float(loss))
        assert per_step in (None, lib.persistent_launches - n)
        per_step = lib.persistent_launches - n
    x, x2 = inputs(env, 700), inputs(env, 710)
    with torch.no_grad():
        want = me(x).clone()                            # (the guard's first check runs here, eagerly)
        n = lib.persistent_launches
        want2 = me(x2).clone()
        per_forward = lib.persistent_launches - n
    # what one capture keeps: the pool before and after one build (enough slots are secured first, so that no buffer is
    # added in between)
    lib.reserve_sched_slots(env.device, 4 * per_step + 64)
    f0 = free()
    t0 = time.perf_counter()
    first = GraphedTripletStep(m1, opt1, margin=MARGIN, example=batches[0])
    build_s = time.perf_counter() - t0
    need = f0 - free()
    print(f"[{env.name}] one captured fp16 triplet step keeps {need} scheduler slots ({env.batch} x {env.frames} frames, "
          f"{N_STAGES} stages; {per_step} persistent launches per eager step, {per_forward} per eval forward; "
          f"{streams} streams own a ring); built in {build_s:.2f} s")
    assert need == per_step > 1 and per_forward > 1, "one slot per captured launch; the warm-up's streams had their rings"
    first.close()
    graphs = []
    # ---- the step, with one slot fewer than it keeps ----
    t0 = time.perf_counter()
    _drain(env, per_step - 1, graphs)
    print(f"[{env.name}] pool drained to {per_step - 1} free slots in {time.perf_counter() - t0:.2f} s "
          f"({len(graphs)} throwaway graphs)")
    with _AddSpy(lib) as spy:
        gstep = GraphedTripletStep(m2, opt2, margin=MARGIN, example=batches[0])
        spy.check("GraphedTripletStep", per_step)
    with gstep:
        graphed = [float(gstep(*batches[it % 2])) for it in range(3)]
    np.testing.assert_allclose(graphed, eager, rtol=2e-5, atol=1e-7)
    worst = max(float((p.detach() - q.detach()).abs().max() / q.detach().abs().max().clamp_min(1e-12))
                for (n, p), q in zip(m2.named_parameters(), m.parameters()) if not n.startswith("model.classifier"))
    assert worst < 1e-5, worst
    # ---- the eval forward, with one slot fewer than it launches ----
    _drain(env, per_forward - 1, graphs)
    with _AddSpy(lib) as spy:
        ge = me.graphed(x)
        spy.check("GraphedEmbedder", per_forward)
    with torch.no_grad():
        assert same_bits(ge(x).clone(), want)
        assert same_bits(ge(x2).clone(), want2) and same_bits(me(x2), want2)
    return need
