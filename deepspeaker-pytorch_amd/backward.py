"""Backward pass of the train-mode ResCNN as a sequence of C-ABI launches.

Restates what torch autograd derives for `loss.backward()` (reference train_triplet.py:223,290) over
`DeepSpeakerModel.forward` (model.py:185-218): l2-norm, fc, temporal mean, and per stage
clip / BatchNorm(train) / 3x3 conv x2 with the identity residual, then clip / BatchNorm / 5x5 s2 conv.
Every op is a HIP kernel (include/deepspeaker_hip.h, "backward" sections); this file only orders them.
"""
from __future__ import annotations

import ctypes
from typing import Dict


import torch

from ._native import ConvShape
from .engine import ALPHA, L2_EPS, STAGE_CHANNELS, Engine, PackedWeights, SavedForward


def _stats_table(stats, c: int):
    """(G, mean table, invstd table): the members' mean / invstd as consecutive rows of one [G][C] table each.  The
    statistics of one member (a tuple) are a table of one row; a list of members whose rows already lie consecutively
    (Engine.forward_train_group lays them out so) is used in place; any other list is stacked first."""
    members = stats if isinstance(stats, list) else [stats]
    G, step = len(members), c * 4
    if all(m_[k].data_ptr() == members[0][k].data_ptr() + g * step for g, m_ in enumerate(members) for k in (0, 1)):
        return G, members[0][0], members[0][1]
    return G, torch.stack([m_[0] for m_ in members]), torch.stack([m_[1] for m_ in members])


def _bn_bwd(eng: Engine, g1, g2, act, z, stats, gamma, reducer=None, fused_launch=None, rows=None):
    """(masked upstream gradient gy, gz = dL/d(conv output), dgamma, dbeta) of one BatchNorm + clip layer over a batch
    made of G members with their own batch statistics (`stats`: one member's tuple, or a list of them -- the three
    forwards of a triplet step run as one batch): ds_bn_bwd_group_f32, G = 1 included.  dgamma / dbeta are summed over
    the members (the reference accumulates them over its three backward passes).  With an active `reducer` the float64
    sums of ALL members travel in one all-reduce between the reduction and the application (global-batch BatchNorm);
    dgamma / dbeta then already are the global gradients.  `fused_launch(gy, partial, stream)`: a data-gradient kernel
    whose epilogue is the reduction (`rows` partial rows per member) runs in place of the reduce step."""
    c = z.shape[-1]
    dev = z.device
    G, mean, invstd = _stats_table(stats, c)
    n_pix = (z.numel() // c) // G
    if fused_launch is None:
        rows = eng.lib.raw("ds_bn_bwd_partial_rows")(n_pix, c)
    st = eng._stream(z)
    gy, gz = torch.empty_like(z), torch.empty_like(z)
    partial = torch.empty((G, rows, c, 2), dtype=torch.float32, device=dev)
    coef = torch.empty((G, 3 * c), dtype=torch.float32, device=dev)
    member_sums = torch.empty((2, G, c), dtype=torch.float32, device=dev)      # dgamma / dbeta per member
    gg, gb = torch.empty(c, dtype=torch.float32, device=dev), torch.empty(c, dtype=torch.float32, device=dev)
    tail = (eng._p(z), eng._p(mean), eng._p(invstd), eng._p(gamma.detach()), eng._p(coef), eng._p(member_sums),
            eng._p(gg), eng._p(gb), eng._p(gz), n_pix, c, G, st)
    if fused_launch is not None:
        fused_launch(gy, partial, st)
    if reducer is not None and reducer.active:
        # split where the sums of ALL members travel in one all-reduce (2 + 3 launches)
        sums = torch.empty((G, 2 * c + 1), dtype=torch.float64, device=dev)
        if fused_launch is not None:
            eng.lib.call("ds_partial_sum_f64_group", eng._p(partial), rows, eng._p(sums), n_pix, c, G, st)
        else:
            eng.lib.call("ds_bn_bwd_group_reduce_f32", eng._p(g1), eng._p(g2), eng._p(act), eng._p(z), eng._p(mean),
                         eng._p(invstd), eng._p(gy), eng._p(partial), eng._p(sums), n_pix, c, G, st)
        reducer.all_reduce_sum_(sums)                               # every member of this layer in ONE collective
        eng.lib.call("ds_bn_bwd_group_apply_f32", eng._p(sums), eng._p(gy), *tail)
    elif fused_launch is not None:
        eng.lib.call("ds_bn_bwd_group_finish_f32", eng._p(partial), rows, eng._p(gy), *tail)
    else:
        eng.lib.call("ds_bn_bwd_group_f32", eng._p(g1), eng._p(g2), eng._p(act), eng._p(z), eng._p(mean), eng._p(invstd),
                     eng._p(gamma.detach()), eng._p(gy), eng._p(partial), eng._p(coef), eng._p(member_sums), eng._p(gg),
                     eng._p(gb), eng._p(gz), n_pix, c, G, st)
    return gy, gz, gg, gb


FUSE_DGRAD_BN_BWD = True       # module switch for A/B runs and tests of the unfused sequence


def _fused_plan(eng: Engine, rows_entry: str, shp: ConvShape, bank_bf16, stats, c: int, n_tables: int):
    """(members' statistics, partial rows per member) if a fused data gradient + BatchNorm backward applies, else None:
    the switch is on, the bf16x3 bank exists, the first `n_tables` statistics of the members are rows of one table each
    and the kernel's planner (`rows_entry`) keeps every tile of the launch inside one member."""
    if not FUSE_DGRAD_BN_BWD or bank_bf16 is None:
        return None
    members = stats if isinstance(stats, list) else [stats]
    G = len(members)
    step = c * 4
    if any(len(m_) < n_tables for m_ in members):
        return None
    if not all(m_[k].data_ptr() == members[0][k].data_ptr() + g * step for g, m_ in enumerate(members) for k in range(n_tables)):
        return None
    rows = eng.lib.raw(rows_entry)(ctypes.byref(shp), G)
    return (members, rows) if rows > 0 else None


def _dgrad_bn_bwd(eng: Engine, shp: ConvShape, gz_up, bank_bf16, g2, z, stats, gamma, reducer=None):
    """`_dgrad` of a 3x3 layer followed by `_bn_bwd` of the BatchNorm + clipped-ReLU layer it feeds, with the first half
    of the latter inside the data-gradient kernel's epilogue (ds_conv_dgrad_bnbwd_bf16): the gradient never makes the
    round trip through HBM between the two, and the mask comes from the layer's own pre-activation `z` instead of a
    third tensor.  Returns (gy, gz, dgamma, dbeta) like `_bn_bwd`, or None where the fused kernel does not apply (a tile
    of the launch would straddle two members, statistics not laid out as tables): the caller then runs the two steps."""
    plan = _fused_plan(eng, "ds_conv_dgrad_bnbwd_bf16_rows", shp, bank_bf16, stats, z.shape[-1], 4)
    if plan is None:
        return None
    members, rows = plan
    G = len(members)
    mean, invstd, sc, sh = members[0]

    def fused_launch(gy, partial, st):
        eng.lib.call("ds_conv_dgrad_bnbwd_bf16", ctypes.byref(shp), eng._p(gz_up), eng._p(bank_bf16[0]), eng._p(bank_bf16[1]),
                     eng._p(g2), eng._p(z), eng._p(mean), eng._p(invstd), eng._p(sc), eng._p(sh), G, eng._p(gy),
                     eng._p(partial), st)
    return _bn_bwd(eng, None, None, None, z, stats, gamma, reducer, fused_launch, rows)


def _dgrad_s2_bn_bwd(eng: Engine, shp: ConvShape, gz_up, bank_bf16, act, z, stats, gamma, reducer=None):
    """`_dgrad` of a 5x5 stride-2 layer followed by `_bn_bwd` of the BasicBlock output it feeds (bn2 + residual + clip of
    the previous stage), fused like `_dgrad_bn_bwd` (ds_conv_dgrad_s2_bnbwd_bf16): the four parity-class launches mask
    with the stored activation `act`, sum and write gy.  Returns (gy, gz, dgamma, dbeta) or None (not applicable)."""
    plan = _fused_plan(eng, "ds_conv_dgrad_s2_bnbwd_bf16_rows", shp, bank_bf16, stats, z.shape[-1], 2)
    if plan is None:
        return None
    members, rows = plan
    G = len(members)
    mean, invstd = members[0][0], members[0][1]

    def fused_launch(gy, partial, st):
        eng.lib.call("ds_conv_dgrad_s2_bnbwd_bf16", ctypes.byref(shp), eng._p(gz_up), eng._p(bank_bf16[0]),
                     eng._p(bank_bf16[1]), eng._p(act), eng._p(z), eng._p(mean), eng._p(invstd), G, eng._p(gy),
                     eng._p(partial), st)
    return _bn_bwd(eng, None, None, None, z, stats, gamma, reducer, fused_launch, rows)


def _wgrad_call(eng: Engine, workspace_entry: str, entry: str, shp: ConvShape, x, gz, out, *tail):
    """One filter-gradient launch into `out`: the kernel's workspace is asked for, checked and allocated here.  `tail`:
    the entry point's arguments between the output and the stream (fc bins, 1 / loss scale)."""
    n_ws = eng.lib.raw(workspace_entry)(ctypes.byref(shp))
    if n_ws <= 0:
        raise RuntimeError(f"{workspace_entry} failed: {n_ws}")
    ws = torch.empty(n_ws, dtype=torch.float32, device=x.device)
    eng.lib.call(entry, ctypes.byref(shp), eng._p(x), eng._p(gz), eng._p(ws), eng._p(out), *tail, eng._stream(x))
    return out


def _wgrad(eng: Engine, shp: ConvShape, x, gz, out_shape, fc_f: int = 0, x3: bool = False, out=None):
    """filter gradient into `out` (a contiguous view of a gradient bucket) or a fresh tensor"""
    gw = out if out is not None else torch.empty(out_shape, dtype=torch.float32, device=x.device)
    if x3 and shp.KS in (3, 5) and shp.Cin % 64 == 0:      # split-operand bf16 matrix cores
        return _wgrad_call(eng, "ds_conv_wgrad_bf16_workspace_floats", "ds_conv_wgrad_bf16", shp, x, gz, gw)
    return _wgrad_call(eng, "ds_conv_wgrad_workspace_floats", "ds_conv_wgrad_f32", shp, x, gz, gw, fc_f)


def _dgrad(eng: Engine, shp: ConvShape, gz, w_dgrad, w_dgrad_bf16=None):
    gx = torch.empty((shp.B, shp.H, shp.W, shp.Cin), dtype=torch.float32, device=gz.device)
    if w_dgrad_bf16 is not None:       # bf16x3 data gradient (3x3 stride 1 / 5x5 stride 2)
        eng.lib.call("ds_conv_dgrad_bf16", ctypes.byref(shp), eng._p(gz), eng._p(w_dgrad_bf16[0]),
                     eng._p(w_dgrad_bf16[1]), eng._p(gx), eng._stream(gz))
        return gx
    eng.lib.call("ds_conv_dgrad_f32", ctypes.byref(shp), eng._p(gz), eng._p(w_dgrad), eng._p(gx), eng._stream(gz))
    return gx


_wgrad_streams: Dict[tuple, "torch.cuda.Stream"] = {}
OVERLAP_FILTER_GRADIENTS = True        # module default of backward_train(overlap_filter_gradients=None); tools flip it for A/B runs


class _FilterGradLane:
    """Where the filter-gradient kernels run.  A layer's filter gradient is a leaf of the backward pass: nothing
    downstream waits for it, while the data gradient -> BatchNorm-backward chain next to it is what the earlier
    layers wait for, and that chain is half HBM-bound element-wise passes.  On the GPU the filter gradients are
    therefore enqueued on a second HIP stream (fork after the kernel that produced dL/d(conv output), join at the end
    of the pass): the matrix-core-bound gradient kernels and the HBM-bound BatchNorm passes then share the chip
    instead of queueing behind each other.  Results are those of the one-stream order (same kernels, same inputs).
    On the host emulator (CPU tensors) everything stays in program order."""

    def __init__(self, device: torch.device, enabled: bool = True, priority: int = 0):
        """`priority` -1: a high-priority stream (tuning probe).  HIP deals normal-priority streams to its (4) hardware
        queues round-robin in creation order, so whether this lane shares a queue -- and then serialises -- with the
        caller's stream depends on how many streams the process made before (fp16 step: 8.8 ms in three alignments of
        four, 9.6 in the fourth; `bench.py --pad-streams`).  A high-priority lane lives on queues of its own and measured
        8.77 - 8.79 ms in all four alignments of a fresh process -- but 13.0 ms inside the full bench process (after the
        bf16x3 legs), and 23.5 ms for the bf16x3 step in one alignment: priority also reorders dispatch.  Default 0."""
        self.main = self.side = None
        self.keep = []                  # main-stream tensors the side stream reads: alive until the join
        if device.type == "cuda" and enabled:
            self.main = torch.cuda.current_stream(device)
            side = _wgrad_streams.get((device, priority))
            if side is None:
                side = _wgrad_streams[(device, priority)] = torch.cuda.Stream(device=device, priority=priority)
            self.side = side
            side.wait_stream(self.main)

    def run(self, fn, *inputs):
        """fn() on the side stream, ordered after everything enqueued on the main stream so far; `inputs` are the
        main-stream tensors it reads.  They are kept alive until join() -- after which the main stream is ordered
        behind the side stream, so their memory can be recycled the ordinary way.  (Tensor.record_stream instead
        made the caching allocator hold every such block back until the side stream had caught up: 54 GiB reserved
        for a 14 GiB working set.)"""
        if self.side is None:
            return fn()
        self.side.wait_event(self.main.record_event())
        self.keep.extend(t for t in inputs if t is not None)
        with torch.cuda.stream(self.side):
            return fn()

    def join(self):
        if self.side is not None:
            self.main.wait_stream(self.side)
        self.keep.clear()


class _GradBuckets:
    """The filter / fc gradients of one backward pass, laid out as one flat buffer per stage (+ one for fc): the
    gradient kernels write straight into views of their bucket.  Under data parallelism each bucket is summed over
    the ranks either the moment its last gradient kernel has been enqueued -- it then travels over xGMI while the
    earlier stages' backward kernels execute; needs the buckets' own communicator, Reducer(grad_comm="separate") --
    or, on the shared communicator (default), right after the pass.  BatchNorm affine gradients come out of the
    (already global) statistic sums and are not reduced."""

    def __init__(self, shapes: Dict[int, Dict[str, tuple]], device, reducer=None):
        self.reducer = reducer if (reducer is not None and reducer.active) else None
        self.views: Dict[str, torch.Tensor] = {}
        self.flat: Dict[int, torch.Tensor] = {}
        self.work = []
        self.deferred = []              # buckets whose exchange waits for finish() (Reducer.overlap_gradients False)
        for b, names in shapes.items():
            n = sum(int(torch.Size(shp).numel()) for shp in names.values())
            flat = torch.empty(n, dtype=torch.float32, device=device)
            self.flat[b] = flat
            off = 0
            for name, shp in names.items():
                k = int(torch.Size(shp).numel())
                self.views[name] = flat[off:off + k].view(shp)
                off += k

    def done(self, bucket: int):
        """the bucket's last gradient kernel has been enqueued (on the current stream)"""
        if self.reducer is None:
            return
        if self.reducer.overlap_gradients:      # own communicator: reduce now, under the earlier stages' kernels
            self.work.append(self.reducer.all_reduce_sum_(self.flat[bucket], async_op=True, gradients=True))
        else:                                   # shared communicator: after the pass's last BatchNorm collective
            self.deferred.append(bucket)

    def finish(self):
        """called on the main stream after the filter-gradient stream has joined it"""
        for b in self.deferred:
            self.work.append(self.reducer.all_reduce_sum_(self.flat[b], async_op=True, gradients=True))
        self.deferred = []
        for h in self.work:
            if h is not None:
                h.wait()
        self.work = []


def _backward_walk(eng: Engine, ar, bn_weights: Dict[str, torch.Tensor], pw: PackedWeights, saved: SavedForward,
                   ge: torch.Tensor, reducer, reduce_gradients: bool, overlap_filter_gradients):
    """The layer sequence of every backward pass, the counterpart of Engine._train_walk: the f32 tail (l2-norm, fc,
    temporal mean), then per stage, last first, bn2 -> conv2's filter gradient -> conv2's data gradient + bn1 -> conv1's
    filter gradient -> conv1's data gradient + bn_i (the residual's gradient joins there) -> conv_i's filter gradient ->
    conv_i's data gradient towards the stage below.  This loop owns the order, the shapes, the saved-tensor lookups, the
    gradient buckets with their exchange and the filter-gradient lane; `ar` is the pass's arithmetic (_F32Class here,
    train_f16._F16):

      ar.head(g)                                    the f32 gradient of the last stage's output -> what its bn2 step takes
      ar.bn2(handed, z, stats, gamma, hw)           -> (g_out, gz, dgamma, dbeta); `handed` comes from head / dgrad_s2
      ar.dgrad_bn(shp, gz, sw, conv, g_out, act, z, stats, gamma)   the 3x3 data gradient of `sw.<conv>` and the BatchNorm
                                                    backward of the layer it feeds (+ g_out) -> (gz, dgamma, dbeta)
      ar.wgrad(shp, x, gz, out)                     one layer's filter gradient into its bucket view
      ar.dgrad_s2(shp, gz, sw, x_in, z, stats, gamma)   the 5x5 stride-2 data gradient -> what the bn2 step of the stage
                                                    below takes (x_in IS that stage's output: the mask of its clip)
      ar.exchange_before_dgrad_s2                   on which side of that launch a stage's bucket goes to the reducer

    Returns (parameter gradients, the buckets)."""
    lane = _FilterGradLane(ge.device, OVERLAP_FILTER_GRADIENTS if overlap_filter_gradients is None else overlap_filter_gradients)
    lib = eng.lib
    grads: Dict[str, torch.Tensor] = {}
    n_stages = len(pw.stages)
    shapes = {n_stages: {"model.fc.weight": tuple(saved.fc_out.shape[1:]) + (saved.pooled.shape[1],),
                         "model.fc.bias": (saved.fc_out.shape[1],)}}
    for s_ in range(n_stages):
        i_, c_ = s_ + 1, STAGE_CHANNELS[s_]
        cin_ = 1 if s_ == 0 else STAGE_CHANNELS[s_ - 1]
        shapes[s_] = {f"model.layer{i_}.0.conv2.weight": (c_, c_, 3, 3), f"model.layer{i_}.0.conv1.weight": (c_, c_, 3, 3),
                      f"model.conv{i_}.weight": (c_, cin_, 5, 5)}
    buckets = _GradBuckets(shapes, ge.device, reducer if reduce_gradients else None)
    f = saved.fc_out
    B, n_out = f.shape
    st = eng._stream(f)
    # ---- l2-norm x alpha (model.py:210-213) ----
    gf = torch.empty_like(f)
    lib.call("ds_l2norm_scale_bwd_f32", eng._p(f), eng._p(ge), eng._p(gf), B, n_out, ALPHA, L2_EPS, st)
    # ---- fc (model.py:209): bias, weight, input ----
    pooled = saved.pooled
    k = pooled.shape[1]
    gb = buckets.views["model.fc.bias"]
    lib.call("ds_colsum_f32", eng._p(gf), eng._p(gb), B, n_out, st)
    grads["model.fc.bias"] = gb
    f_bins = k // STAGE_CHANNELS[n_stages - 1]
    grads["model.fc.weight"] = _wgrad(eng, ConvShape(1, B, 1, k, n_out, 1, 1), pooled, gf, (n_out, k), f_bins,
                                      out=buckets.views["model.fc.weight"])
    buckets.done(n_stages)
    ws = torch.empty(lib.raw("ds_fc_workspace_floats")(B, n_out, k), dtype=torch.float32, device=f.device)
    gpooled = torch.empty((B, k), dtype=torch.float32, device=f.device)
    lib.call("ds_fc_l2norm_fwd_f32", eng._p(gf), eng._p(pw.fc_dgrad), None, eng._p(ws), eng._p(gpooled), None, B,
             n_out, k, 1.0, 0.0, st)
    # ---- temporal mean + the clip of the last stage output (model.py:205-207) ----
    out = saved.acts[f"stage{n_stages}.c"]
    _, hr, wc, c = out.shape
    g = torch.empty_like(out)
    lib.call("ds_avgpool_time_bwd_f32", eng._p(gpooled), eng._p(out), eng._p(g), B, hr, wc, c, st)
    handed = ar.head(g)

    def bn(name):
        return saved.raws[name], saved.stats[name], bn_weights[name]

    def filter_gradient(name, shp, x, gz):
        grads[name] = lane.run(lambda: ar.wgrad(shp, x, gz, buckets.views[name]), gz)

    for s in reversed(range(n_stages)):
        i, c = s + 1, STAGE_CHANNELS[s]
        h, w = saved.dims[s]
        cin = 1 if s == 0 else STAGE_CHANNELS[s - 1]
        sw = pw.stages[s]
        a_act, b_act = saved.acts[f"stage{i}.a"], saved.acts[f"stage{i}.b"]
        shp3 = ConvShape(B, h, w, c, c, 3, 1)
        # out = clip(bn2(conv2(y)) + r)            (model.py:73-80)
        name = f"model.layer{i}.0.bn2"
        g_out, gz, grads[name + ".weight"], grads[name + ".bias"] = ar.bn2(handed, *bn(name), (h, w))
        filter_gradient(f"model.layer{i}.0.conv2.weight", shp3, b_act, gz)
        # y = clip(bn1(conv1(r)))                  (model.py:69-71): conv2's data gradient + bn1's backward
        name = f"model.layer{i}.0.bn1"
        gz, grads[name + ".weight"], grads[name + ".bias"] = ar.dgrad_bn(shp3, gz, sw, "l_conv2", None, b_act, *bn(name))
        filter_gradient(f"model.layer{i}.0.conv1.weight", shp3, a_act, gz)
        # r = clip(bn_i(conv_i(x)));  dL/dr = conv-path + residual path   (model.py:187-189, 67, 79)
        name = f"model.bn{i}"
        gz, grads[name + ".weight"], grads[name + ".bias"] = ar.dgrad_bn(shp3, gz, sw, "l_conv1", g_out, a_act, *bn(name))
        h_in, w_in = (saved.x.shape[2], saved.x.shape[3]) if s == 0 else saved.dims[s - 1]
        shp5 = ConvShape(B, h_in, w_in, cin, c, 5, 2)
        x_in = saved.x if s == 0 else saved.acts[f"stage{s}.c"]
        filter_gradient(f"model.conv{i}.weight", shp5, x_in, gz)
        # this stage's three filter gradients are enqueued: reduce them now.  (The f32-class pass forks the exchange off
        # before the stride-2 data gradient is enqueued, the fp16 pass after it -- the lane orders the exchange behind
        # whatever the main stream holds at the fork, so the side is part of each pass's schedule and is kept.)
        if ar.exchange_before_dgrad_s2:
            lane.run(lambda: buckets.done(s))
        if s > 0:
            handed = ar.dgrad_s2(shp5, gz, sw, x_in, *bn(f"model.layer{s}.0.bn2"))
        if not ar.exchange_before_dgrad_s2:
            lane.run(lambda: buckets.done(s))
    lane.join()
    buckets.finish()
    return grads, buckets


class _F32Class:
    """The f32-class arithmetic of `_backward_walk` (f32, or bf16x3: data and filter gradients of the 3x3 / 5x5 layers on
    the bf16 matrix cores with split operands).  A stage hands the bn2 step below it either the finished
    (gy, gz, dgamma, dbeta) of the fused stride-2 kernel or (gradient, the activation that still has to mask it)."""
    exchange_before_dgrad_s2 = True

    def __init__(self, eng: Engine, x3: bool, reducer):
        self.eng, self.x3, self.reducer = eng, x3, reducer

    def head(self, g):
        return g, None                  # ds_avgpool_time_bwd_f32 applied the last clip's mask

    def bn2(self, handed, z, stats, gamma, hw):
        if len(handed) == 4:            # the stage above already ran this step inside its 5x5 data gradient
            return handed
        g, mask_act = handed
        return _bn_bwd(self.eng, g, None, mask_act, z, stats, gamma, self.reducer)

    def dgrad_bn(self, shp, gz, sw, conv, g_out, act, z, stats, gamma):
        bank = getattr(sw, conv + "_dgrad_bf16") if self.x3 else None
        fused = _dgrad_bn_bwd(self.eng, shp, gz, bank, g_out, z, stats, gamma, self.reducer)
        if fused is None:
            g = _dgrad(self.eng, shp, gz, getattr(sw, conv + "_dgrad"), bank)
            fused = _bn_bwd(self.eng, g, g_out, act, z, stats, gamma, self.reducer)
        return fused[1:]

    def wgrad(self, shp, x, gz, out):
        return _wgrad(self.eng, shp, x, gz, None, x3=self.x3, out=out)

    def dgrad_s2(self, shp, gz, sw, x_in, z, stats, gamma):
        bank = sw.conv_dgrad_bf16 if self.x3 else None
        fused = _dgrad_s2_bn_bwd(self.eng, shp, gz, bank, x_in, z, stats, gamma, self.reducer)
        if fused is not None:
            return fused
        return _dgrad(self.eng, shp, gz, sw.conv_dgrad, bank), x_in        # unmasked: the next bn2 step masks it


def backward_train(eng: Engine, bn_weights: Dict[str, torch.Tensor], pw: PackedWeights, saved: SavedForward,
                   ge: torch.Tensor, reducer=None, precision: str = "f32",
                   reduce_gradients: bool = False, overlap_filter_gradients=None) -> Dict[str, torch.Tensor]:
    """Parameter gradients (reference key names, reference shapes) given dL/d(embedding) `ge` [B,512].
    precision "bf16x3": data and filter gradients of the 3x3 / 5x5 layers run on the bf16 matrix cores with
    split operands; conv1 and fc stay on the f32 matrix cores.  `reduce_gradients` (data parallelism): the
    per-stage gradient buckets are all-reduced over `reducer` as the pass produces them, overlapped with the rest
    of the pass; the returned gradients are then the global sums.  `overlap_filter_gradients`: see _FilterGradLane."""
    grads, _ = _backward_walk(eng, _F32Class(eng, precision == "bf16x3", reducer), bn_weights, pw, saved, ge, reducer,
                              reduce_gradients, overlap_filter_gradients)
    return grads
