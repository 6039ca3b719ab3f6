"""The OPT-IN fp16 training step: `DeepSpeakerModel(..., train_precision="f16")`.

Same function as the f32-class step (`Engine.forward_train_group` + `backward.backward_train`, i.e. the reference's
`out_a, out_p, out_n = model(data_a), model(data_p), model(data_n)`; `loss.backward()` -- train_triplet.py:215-223), other
arithmetic and other bytes (the layer walks are shared: `Engine._train_walk`, `backward._backward_walk`; this file supplies
the per-layer routines):

* every activation, pre-activation and gradient tensor is fp16 in HBM (the network input, the last stage's output and
  everything behind it -- pooling, projection, l2-norm, loss -- stay f32);
* forward convolutions AND data gradients run on the eval path's fp16 matrix-core kernels (`ds_conv_fwd_f16`: persistent
  workgroups, one MFMA per product, f32 accumulate) -- a 3x3 data gradient is that kernel over dL/dz with the flipped
  bank, a 5x5 stride-2 data gradient is ONE 3x3 convolution whose 4 Cin output channels are the four parity classes of
  dX (read in place by the BatchNorm backward of the layer below);
* BatchNorm statistics come from a pass of their own over the fp16 pre-activation, BatchNorm / clip passes move half
  the bytes of the f32 step's; filter gradients contract fp16 operands (`ds_conv_wgrad_f16`), f32 accumulate;
* gradient tensors hold `loss_scale` * g (a constant power of two; the small gradients of the early layers then sit in
  fp16's normal range); parameter gradients leave in f32, un-scaled.

Stated tolerance (tests/test_gpu_train_f16.py; measured at the 768-row bench batch in brackets): loss within 1e-3 (3.5e-4)
and train-mode embeddings within 2e-3 (1.15e-3) of the reference's recorded step, every parameter gradient within 8e-3
rel-L2 (4.0e-3 worst, 1.4e-3 median) of the oracle evaluated with this forward's clip masks and dL/de -- the order of the
4e-3 the reference's own float32 run is from its float64 run.  The f32-class step (bf16x3, 1e-4) stays the default.

Data parallelism (`enable_data_parallel`): the same exchange pattern as the f32-class step -- one float64 all-reduce per
BatchNorm layer and direction carrying all members' sums, f32 gradient buckets per stage (tests/test_distributed_gloo.py).
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from ._native import DS_EPI_OUT_F16, DS_EPI_OUT_F32
from .backward import _backward_walk, _wgrad_call
from .engine import BN_EPS, BN_MOMENTUM, BNParams, Engine, PackedWeights, SavedForward, _clip_flags

DEFAULT_LOSS_SCALE = 1024.0


def _bn_stats(eng: Engine, z16: torch.Tensor, bn: BNParams, G: int, update_running: bool = True, reducer=None, tables=None):
    """[G][C] tables (mean, invstd, scale, shift) of a train-mode BatchNorm over the G members of z16 [B,h,w,C] fp16.
    With an active `reducer` (data parallelism) the members' float64 sums travel in ONE all-reduce, so every rank
    normalises with the statistics of the global batch."""
    c = z16.shape[-1]
    n_pix = (z16.numel() // c) // G
    rows = eng.lib.raw("ds_bn_f16_partial_rows")(n_pix, c)
    partial = torch.empty((G, rows, c, 2), dtype=torch.float32, device=z16.device)
    if tables is None:
        tables = torch.empty((4, G, c), dtype=torch.float32, device=z16.device)
    st = eng._stream(z16)
    if reducer is not None and reducer.active:
        sums = torch.empty((G, 2 * c + 1), dtype=torch.float64, device=z16.device)
        eng.lib.call("ds_bn_stats_partial_f16", eng._p(z16), eng._p(partial), n_pix, c, G, st)
        eng.lib.call("ds_partial_sum_f64_group", eng._p(partial), rows, eng._p(sums), n_pix, c, G, st)
        reducer.all_reduce_sum_(sums)
        eng.lib.call("ds_bn_stats_from_sums_group_f32", eng._p(sums), eng._p(bn.weight.detach()), eng._p(bn.bias.detach()),
                     BN_EPS, BN_MOMENTUM, eng._p(bn.running_mean) if update_running else None,
                     eng._p(bn.running_var) if update_running else None, eng._p(tables[0]), eng._p(tables[1]),
                     eng._p(tables[2]), eng._p(tables[3]), c, G, st)      # members in call order inside the kernel
        return tables
    eng.lib.call("ds_bn_stats_group_f16", eng._p(z16), eng._p(partial), n_pix, eng._p(bn.weight.detach()),
                 eng._p(bn.bias.detach()), BN_EPS, BN_MOMENTUM, eng._p(bn.running_mean) if update_running else None,
                 eng._p(bn.running_var) if update_running else None, eng._p(tables[0]), eng._p(tables[1]),
                 eng._p(tables[2]), eng._p(tables[3]), c, G, st)
    return tables


def _bn_apply(eng: Engine, z16, tables, residual16, G: int, flags: int, out=None):
    c = z16.shape[-1]
    n_pix = (z16.numel() // c) // G
    y = out if out is not None else torch.empty(z16.shape, dtype=torch.float32 if flags & DS_EPI_OUT_F32 else torch.float16,
                                                device=z16.device)
    eng.lib.call("ds_bn_apply_group_f16", eng._p(z16), eng._p(tables[2]), eng._p(tables[3]), eng._p(residual16), eng._p(y),
                 n_pix, c, G, flags, eng._stream(z16))
    return y


def forward_train_group_f16(eng: Engine, xs: List[torch.Tensor], pw: PackedWeights, bns: Dict[str, BNParams],
                            save: bool = True, reducer=None):
    """The train-mode forwards of the G = len(xs) members in lock-step over one concatenated batch, fp16 tensors between
    the layers.  One convolution launch per layer over ALL members (the statistics are a separate pass, so tiles may
    straddle members), one statistics launch pair, one normalise + clip launch.  (Measured and dropped: one HIP stream per
    member, as the f32-class forward runs -- bitwise the same results, 8.89 against 8.86 ms per step and 5.4 instead of 3.8
    ms of host enqueue: the fp16 passes are short enough that three times the launches cost what the overlap gains; the
    same for the backward chain, 9.9 ms.)  `reducer` (data parallelism): one
    float64 all-reduce per BatchNorm layer carrying all members' sums.  Returns ([embeddings per member],
    SavedForward with fp16 `raws` / `acts` -- the last stage's output is f32 -- and `stats[name]` = the [4][G][C] tables)."""
    G = len(xs)
    x, Bm = eng._members(xs)
    if pw.stages[0].l_conv1_f16 is None:
        raise ValueError("pack_weights(..., with_f16=True) is required for the fp16 training step")
    B = G * Bm

    def layer(src, sw, conv, name, geom, residual, last):
        h, w, cin = geom[:3]
        if cin == 1:        # the split-operand kernel of the eval path, raw fp16 output
            z, _ = eng.conv1(src, sw.conv, B, h, w, flags=DS_EPI_OUT_F16, lowp=True)
        else:
            z = eng.conv_f16(src, getattr(sw, conv + "_f16"), B, *geom)
        tb = _bn_stats(eng, z, bns[name], G, reducer=reducer)
        return z, _bn_apply(eng, z, tb, residual, G, _clip_flags(residual) | (DS_EPI_OUT_F32 if last else 0)), tb

    a, saved = eng._train_walk(x, pw, save, layer)
    e = eng.tail(a, pw, saved)
    return [e[g * Bm:(g + 1) * Bm] for g in range(G)], saved


def _bn_bwd(eng: Engine, g1, g1_parity, g2, act, z16, tables, gamma, G: int, hw, inv_scale: float, mask_from_z: bool = False,
            want_gy: bool = True, reducer=None):
    """(gy16 or None, gz16, dgamma, dbeta) of one BatchNorm + clip layer; see ds_bn_bwd_group_f16.  mask_from_z: the clip
    mask is re-derived from the pre-activation z16 and the forward's scale / shift tables instead of being read from a
    stored activation; want_gy=False (then also: no g2, no parity layout): the masked gradient is not stored."""
    c = z16.shape[-1]
    n_pix = (z16.numel() // c) // G
    dev = z16.device
    rows = eng.lib.raw("ds_bn_f16_partial_rows")(n_pix, c)
    partial = torch.empty((G, rows, c, 2), dtype=torch.float32, device=dev)
    coef = torch.empty((G, 3 * c), dtype=torch.float32, device=dev)
    gz = torch.empty_like(z16)
    gy = torch.empty_like(z16) if want_gy else None
    gg, gb = torch.empty(c, dtype=torch.float32, device=dev), torch.empty(c, dtype=torch.float32, device=dev)
    act_p = None if mask_from_z else eng._p(act)
    act32 = int(act is not None and act.dtype == torch.float32)
    msc, msh = (eng._p(tables[2]), eng._p(tables[3])) if mask_from_z else (None, None)
    st = eng._stream(z16)
    if reducer is not None and reducer.active:
        # the grouped launches split where the sums of ALL members travel in one all-reduce
        eng.lib.call("ds_bn_bwd_group_reduce_f16", eng._p(g1), int(g1_parity), eng._p(g2), act_p, act32, msc, msh, eng._p(z16),
                     eng._p(tables[0]), eng._p(tables[1]), eng._p(gy), eng._p(partial), n_pix, hw[0], hw[1], c, G, st)
        sums = torch.empty((G, 2 * c + 1), dtype=torch.float64, device=dev)
        eng.lib.call("ds_partial_sum_f64_group", eng._p(partial), rows, eng._p(sums), n_pix, c, G, st)
        reducer.all_reduce_sum_(sums)
        eng.lib.call("ds_bn_bwd_group_apply_f16", eng._p(sums), eng._p(gy if gy is not None else g1), int(gy is None), msc, msh,
                     eng._p(z16), eng._p(tables[0]), eng._p(tables[1]), eng._p(gamma.detach()), eng._p(coef), eng._p(gg),
                     eng._p(gb), eng._p(gz), n_pix, c, G, float(inv_scale), st)
        return gy, gz, gg, gb
    eng.lib.call("ds_bn_bwd_group_f16", eng._p(g1), int(g1_parity), eng._p(g2), act_p, act32, msc, msh, eng._p(z16),
                 eng._p(tables[0]), eng._p(tables[1]), eng._p(gamma.detach()), eng._p(gy), eng._p(partial), eng._p(coef),
                 eng._p(gg), eng._p(gb), eng._p(gz), n_pix, hw[0], hw[1], c, G, float(inv_scale), st)
    return gy, gz, gg, gb


class _F16:
    """The fp16 arithmetic of `backward._backward_walk`: fp16 gradient tensors holding `loss_scale` * g, data gradients on
    the forward's fp16 convolution kernel over the flipped banks.  A stage hands the bn2 step below it (gradient, parity
    layout?, the activation that still has to mask it)."""
    exchange_before_dgrad_s2 = False

    def __init__(self, eng: Engine, G: int, loss_scale: float, reducer):
        self.eng, self.G, self.loss_scale, self.inv, self.reducer = eng, G, float(loss_scale), 1.0 / float(loss_scale), reducer

    def head(self, g32):
        g = torch.empty(g32.shape, dtype=torch.float16, device=g32.device)
        self.eng.lib.call("ds_scale_cast_f32_to_f16", self.eng._p(g32), self.eng._p(g), g32.numel(), self.loss_scale,
                          self.eng._stream(g32))
        return g, False, None           # ds_avgpool_time_bwd_f32 applied the last clip's mask

    def bn2(self, handed, z, tables, gamma, hw):
        g, parity, mask_act = handed
        return _bn_bwd(self.eng, g, parity, None, mask_act, z, tables, gamma, self.G, hw, self.inv, reducer=self.reducer)

    def dgrad_bn(self, shp, gz, sw, conv, g_out, act, z, tables, gamma):
        g = self.eng.conv_f16(gz, getattr(sw, conv + "_dgrad_f16"), shp.B, shp.H, shp.W, shp.Cout, shp.Cin, 3, 1)
        # (no residual was added before this clip: its mask is re-derived from z; the masked gradient is stored only where
        # the residual's gradient g_out has to be added to it)
        return _bn_bwd(self.eng, g, False, g_out, None, z, tables, gamma, self.G, (shp.H, shp.W), self.inv, mask_from_z=True,
                       want_gy=g_out is not None, reducer=self.reducer)[1:]

    def wgrad(self, shp, x, gz16, out):
        if shp.Cin == 1:                # conv1: f32 input
            return _wgrad_call(self.eng, "ds_conv_wgrad_workspace_floats", "ds_conv_wgrad_c1_f16", shp, x, gz16, out, self.inv)
        return _wgrad_call(self.eng, "ds_conv_wgrad_f16_workspace_floats", "ds_conv_wgrad_f16", shp, x, gz16, out, self.inv)

    def dgrad_s2(self, shp, gz, sw, x_in, z, tables, gamma):
        # dL/d(stage-below output): ONE 3x3 convolution over dL/dz whose 4 cin output channels are the parity classes
        # of the stride-2 data gradient; the layer below reads that layout in place and masks it itself
        B, h, w, c = gz.shape
        return self.eng.conv_f16(gz, sw.conv_dgrad_f16, B, h, w, c, 4 * shp.Cin, 3, 1), True, x_in


def backward_train_f16(eng: Engine, bn_weights: Dict[str, torch.Tensor], pw: PackedWeights, saved: SavedForward,
                       ge: torch.Tensor, loss_scale: float = DEFAULT_LOSS_SCALE,
                       overlap_filter_gradients=None, reducer=None, reduce_gradients: bool = False,
                       overflow_flag: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """Parameter gradients (reference key names and shapes, f32, un-scaled) given dL/d(embedding) `ge` [B,512] f32, from
    the fp16 tensors `forward_train_group_f16` saved.  Filter gradients run on the second stream like the f32-class
    pass's (backward._FilterGradLane); the main chain stays on ONE stream over the whole batch (measured: every member's
    BatchNorm-backward / data-gradient chain on a stream of its own, as the forward does, is bitwise the same and SLOWER --
    9.9 against 8.9 ms per step: three times the launches, and 256-utterance convolutions fill the persistent grids
    worse than one 768-utterance launch).  `reducer` / `reduce_gradients` (data parallelism): global BatchNorm sums (one
    all-reduce per layer) and the per-stage f32 gradient buckets summed over the ranks, as backward.backward_train does.
    `overflow_flag` (int32 device tensor [1]): set to 1 at the end of the pass if any filter / fc gradient is inf or NaN
    (the static loss scale was too large for this step); never cleared and never read by the host here -- a step may be
    several passes (three `model(x)` calls, gradient accumulation), so the flag is cleared where it is CONSUMED: by the
    fused optimizer after its update (optim._FusedBase._consume_skip) or, in a loop stepped by any other optimizer, by the
    `DeepSpeakerModel.consume_overflow()` / `update_loss_scale()` that loop must call once per step."""
    G = saved.stats["model.bn1"].shape[1]
    grads, buckets = _backward_walk(eng, _F16(eng, G, loss_scale, reducer), bn_weights, pw, saved, ge, reducer,
                                    reduce_gradients, overlap_filter_gradients)
    if overflow_flag is not None:
        # Loss scaling is STATIC (`loss_scale`), and ds_scale_cast_f32_to_f16 does not saturate: a scaled gradient beyond
        # fp16's 65504 is an inf in the gradient tensors, then NaN in the BatchNorm-backward sums and in every filter
        # gradient downstream.  Any such value reaches the filter gradients of its own layer (the sums feed dL/dz, which
        # the filter gradient contracts), so one pass over the f32 gradient buckets (46 MB: ~10 us each at HBM rate) sees
        # it; under data parallelism the buckets are already the global sums, so every rank raises the same flag.  The
        # flag stays on the device: the fused optimizers read it there (optim._FusedBase.skip_flag).
        for flat in buckets.flat.values():
            eng.lib.call("ds_nonfinite_flag_f32", eng._p(flat), flat.numel(), eng._p(overflow_flag), eng._stream(flat))
    return grads
