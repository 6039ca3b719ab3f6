#!/usr/bin/env python3
"""The classic against the pipelined walk of the bf16x3 forward convolution (ds_conv_bf16_set_walk; PIPE of
conv_mfma_bf16_kernel.h) under DS_CONV_PLAN_LATENCY, in one process, the two walks taking turns:

  1. per stage convolution at B rows (default 12): us per launch (10 launches between two events per call), median, min
     and max of N calls after 3 warm-up turns, next to the MFMA issue floor of one wave: (KS^2 * Cin / 16) taps x
     3 * MSUB * NSUB MFMAs x 32 cycles at 1.9 GHz.  A layer's pipelined walk "holds" when its median is no worse than the
     classic one beyond the layer's own larger (max - min) spread.  Outputs compared bitwise.
  2. the whole bf16x3 `forward_eval_planned(low_latency=True)` of B rows, each call between its own pair of events; the
     margin next to the larger (max - min) spread of the two series.

    python tools/bf16_walk_ab.py [--calls 30] [--rows 12]"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np
import torch

import deepspeaker_oracle as O
from deepspeaker_pytorch_amd._native import ConvShape, DS_CONV_PLAN_LATENCY, DS_EPI_AFFINE, DS_EPI_CLIP
from deepspeaker_pytorch_amd.model import DeepSpeakerModel, get_engine

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--rows", type=int, nargs="+", default=[12])
args = ap.parse_args()

eng = get_engine()
lib = eng.lib
dev = torch.device("cuda:0")
setwalk = lib.raw("ds_conv_bf16_set_walk")
WALKS = [("classic", 1), ("pipelined", 2)]
MFMAS_PER_KSTEP = {(128, 64): 6, (64, 64): 3, (32, 128): 3}       # 3 * MSUB * NSUB of the rows the latency plan picks
CLOCK_GHZ = 1.9


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, out


def stats(ts):
    t = np.array(ts)
    return float(np.median(t)), float(t.min()), float(t.max())


# ---- 1. per stage convolution ----
GEOMETRIES = [(64, 64, 80, 32, 3, 1, 2), (64, 128, 80, 32, 5, 2, 1), (128, 128, 40, 16, 3, 1, 2), (128, 256, 40, 16, 5, 2, 1),
              (256, 256, 20, 8, 3, 1, 2), (256, 512, 20, 8, 5, 2, 1), (512, 512, 10, 4, 3, 1, 2)]      # last: launches per forward
FL = DS_EPI_AFFINE | DS_EPI_CLIP | DS_CONV_PLAN_LATENCY
st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
print(f"== ds_conv_fwd_bf16 (x3, affine + clip, DS_CONV_PLAN_LATENCY), us per launch: median [min .. max] of {args.calls} calls "
      f"of 10 launches, 3 warm-up turns ==")
try:
    for B in args.rows:
        tot = {"classic": 0.0, "pipelined": 0.0, "floor": 0.0}
        for ci, co, h, w, k, s, per_fwd in GEOMETRIES:
            shp = ConvShape(B, h, w, ci, co, k, s)
            ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
            x = torch.randn(B, h, w, ci, device=dev)
            bank = eng._pack_bf16(torch.randn(co, ci, k, k, device=dev) * 0.05, k)
            sc, sh = torch.rand(co, device=dev) + 0.5, torch.randn(co, device=dev)
            y = torch.empty(B, ho, wo, co, device=dev)

            def launch():
                lib.call("ds_conv_fwd_bf16", ctypes.byref(shp), eng._p(x), eng._p(bank[0]), eng._p(bank[1]), eng._p(sc), eng._p(sh),
                         None, eng._p(y), None, FL, st)

            series, outs, plan = {n: [] for n, _ in WALKS}, {}, {}
            for turn in range(3 + args.calls):
                for name, wk in WALKS:
                    setwalk(wk)
                    if turn == 0:
                        out8 = (ctypes.c_int * 8)()
                        assert lib.raw("ds_conv_bf16_plan_describe_hinted")(ctypes.byref(shp), 1, FL, out8) == 0
                        assert lib.raw("ds_conv_bf16_plan_walk")(ctypes.byref(shp), 1, FL) == wk
                        plan[name] = list(out8)
                        y.fill_(float("nan"))
                    t, _ = timed(lambda: [launch() for _ in range(10)])
                    if turn == 0:
                        outs[name] = y.clone()
                    if turn >= 3:
                        series[name].append(t / 10)
            d = plan["pipelined"]
            floor = (k * k * ci // 16) * MFMAS_PER_KSTEP[(d[0], d[1])] * 32 / (CLOCK_GHZ * 1e3)
            (m0, lo0, hi0), (m1, lo1, hi1) = stats(series["classic"]), stats(series["pipelined"])
            spread = max(hi0 - lo0, hi1 - lo1)
            same = torch.equal(outs["classic"].view(torch.int32), outs["pipelined"].view(torch.int32))
            verdict = "faster beyond the spread" if m0 - m1 > spread else ("holds" if m1 - m0 <= spread else "LOSES")
            print(f"  B = {B:3d}  conv{k}x{k}s{s} {ci:3d}->{co:3d} on {h}x{w} (x{per_fwd})  tile {d[0]}x{d[1]} workgroups {d[4]:3d} "
                  f"LDS {plan['classic'][5]} -> {d[5]}\n"
                  f"      classic {m0:6.1f} [{lo0:6.1f} .. {hi0:6.1f}]  pipelined {m1:6.1f} [{lo1:6.1f} .. {hi1:6.1f}]  "
                  f"spread {spread:4.1f}  floor {floor:5.1f}  pipelined / floor {m1 / floor:4.2f} (classic {m0 / floor:4.2f})  "
                  f"{verdict}  {'bitwise equal' if same else 'DIFFERS'}")
            tot["classic"] += per_fwd * m0
            tot["pipelined"] += per_fwd * m1
            tot["floor"] += per_fwd * floor
        print(f"  B = {B:3d}  the eleven launches of a forward: classic {tot['classic']:.1f} us, pipelined {tot['pipelined']:.1f} us, "
              f"floors {tot['floor']:.1f} us")

    # ---- 2. the whole forward ----
    sd = O.make_state_dict(seed=1, num_classes=8)
    model = DeepSpeakerModel(512, 8, precision="bf16x3")
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    model = model.cuda().eval()
    pw, folded = model._packed(with_bf16=True), model._folded()
    print(f"== bf16x3 forward_eval_planned(low_latency=True), us per call: median [min .. max] of {args.calls} calls, 3 warm-up turns ==")
    for B in args.rows:
        x = torch.from_numpy(O.make_input(seed=7, batch=B)).to(dev)
        series, outs = {n: [] for n, _ in WALKS}, {}
        for turn in range(3 + args.calls):
            for name, wk in WALKS:
                setwalk(wk)
                t, e = timed(lambda: eng.forward_eval_planned(x, pw, folded, precision="bf16x3", low_latency=True))
                if turn >= 3:
                    series[name].append(t)
                outs[name] = e.clone()
        for name, _ in WALKS:
            med, lo, hi = stats(series[name])
            print(f"  {B:3d} rows  {name:10s} {med:7.1f} [{lo:7.1f} .. {hi:7.1f}]  spread {hi - lo:6.1f}")
        (m0, lo0, hi0), (m1, lo1, hi1) = stats(series["classic"]), stats(series["pipelined"])
        spread = max(hi0 - lo0, hi1 - lo1)
        same = torch.equal(outs["classic"].view(torch.int32), outs["pipelined"].view(torch.int32))
        print(f"  {B:3d} rows  margin of the pipelined walk: {m0 - m1:+.1f} us ({100 * (m0 - m1) / m0:+.1f} %), larger spread {spread:.1f} us"
              f" -> {'faster by more than the spread' if m0 - m1 > spread else 'NOT faster by more than the spread'}; "
              f"{'bitwise equal' if same else 'DIFFERS'}")
        for name, _ in WALKS:
            print(f"            series {name}: {' '.join('%.0f' % t for t in series[name])}")
finally:
    setwalk(0)
