#!/usr/bin/env python3
"""The small f32-class forward behind the near-tie refinement, planned as always against planned for latency
(DS_CONV_PLAN_LATENCY: the one-sub-tile rows kCfgBLat of conv_mfma_bf16_kernel.h), in one process:

  1. the bf16x3 `forward_eval_planned` of 12 rows [12,1,160,64] and of 96 rows: the default plan, every stage convolution
     forced onto the 64 x 64 latency row (ds_conv_bf16_set_forced_cfg(9)), and the plan mode (low_latency=True).  Each
     call is timed by its own pair of events; 3 warm-ups, then the variants take turns; median, min and max of N calls,
     and the margin of the plan mode over the default next to the (max - min) spread of either series.
  2. per stage convolution at the same batch sizes: the default plan, the plan mode's choice and each latency row
     forced (10 launches between two events).  Outputs compared bitwise.

    python tools/refine_latency_ab.py [--calls 30] [--rows 12 96]"""
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
ap.add_argument("--rows", type=int, nargs="+", default=[12, 96])
args = ap.parse_args()
assert args.calls >= 20

eng = get_engine()
lib = eng.lib
dev = torch.device("cuda:0")
setcfg = lib.raw("ds_conv_bf16_set_forced_cfg")
LAT = {9: "64x64", 10: "32x128"}


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


# ---- 1. the whole forward ----
sd = O.make_state_dict(seed=1, num_classes=8)
model = DeepSpeakerModel(512, 8, precision="bf16x3")
model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
model = model.cuda().eval()
pw, folded = model._packed(with_bf16=True), model._folded()
VARIANTS = [("default plan", -1, False), ("forced 64x64", 9, False), ("plan mode", -1, True)]
print(f"== bf16x3 forward_eval_planned, us per call: median [min .. max] of {args.calls} calls, 3 warm-ups ==")
for B in args.rows:
    x = torch.from_numpy(O.make_input(seed=7, batch=B)).to(dev)
    series = {name: [] for name, _, _ in VARIANTS}
    outs = {}
    try:
        for turn in range(3 + args.calls):
            for name, cfg, low in VARIANTS:
                setcfg(cfg)
                t, e = timed(lambda: eng.forward_eval_planned(x, pw, folded, precision="bf16x3", low_latency=low))
                if turn >= 3:
                    series[name].append(t)
                outs[name] = e.clone()
    finally:
        setcfg(-1)
    for name, _, _ in VARIANTS:
        med, lo, hi = stats(series[name])
        same = torch.equal(outs[name].view(torch.int32), outs["default plan"].view(torch.int32))
        print(f"  {B:3d} rows  {name:13s} {med:7.1f} [{lo:7.1f} .. {hi:7.1f}]  spread {hi - lo:6.1f}  "
              f"{'bitwise equal' if same else 'DIFFERS'}")
    m0, lo0, hi0 = stats(series["default plan"])
    m1, lo1, hi1 = stats(series["plan mode"])
    spread = max(hi0 - lo0, hi1 - lo1)
    print(f"  {B:3d} rows  margin of the plan mode: {m0 - m1:+.1f} us ({100 * (m0 - m1) / m0:+.1f} %), larger spread {spread:.1f} us"
          f" -> {'faster by more than the spread' if m0 - m1 > spread else 'NOT faster by more than the spread'}")
    print(f"            series default: {' '.join('%.0f' % t for t in series['default plan'])}")
    print(f"            series plan mode: {' '.join('%.0f' % t for t in series['plan mode'])}")

# ---- 2. per stage convolution ----
GEOMETRIES = [(64, 64, 80, 32, 3, 1), (64, 128, 80, 32, 5, 2), (128, 128, 40, 16, 3, 1), (128, 256, 40, 16, 5, 2),
              (256, 256, 20, 8, 3, 1), (256, 512, 20, 8, 5, 2), (512, 512, 10, 4, 3, 1)]
AC = DS_EPI_AFFINE | DS_EPI_CLIP
st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
print("== ds_conv_fwd_bf16 (x3, affine + clip), us per launch: median of 8 rounds of 10 launches ==")
for B in args.rows:
    for ci, co, h, w, k, s in GEOMETRIES:
        shp = ConvShape(B, h, w, ci, co, k, s)
        ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
        x = torch.randn(B, h, w, ci, device=dev)
        bank = eng._pack_bf16(torch.randn(co, ci, k, k, device=dev) * 0.05, k)
        sc, sh = torch.rand(co, device=dev) + 0.5, torch.randn(co, device=dev)
        y = torch.empty(B, ho, wo, co, device=dev)

        def launch(flags):
            lib.call("ds_conv_fwd_bf16", ctypes.byref(shp), eng._p(x), eng._p(bank[0]), eng._p(bank[1]), eng._p(sc), eng._p(sh),
                     None, eng._p(y), None, flags, st)

        variants = [("default", -1, AC), ("plan mode", -1, AC | DS_CONV_PLAN_LATENCY)] + [(LAT[c], c, AC) for c in LAT if co % int(LAT[c].split("x")[1]) == 0]
        rows, ref = [], None
        try:
            for name, cfg, flags in variants:
                setcfg(cfg)
                out8 = (ctypes.c_int * 8)()
                if lib.raw("ds_conv_bf16_plan_describe_hinted")(ctypes.byref(shp), 1, flags, out8) != 0:
                    continue
                launch(flags)
                torch.cuda.synchronize()
                got = y.clone()
                ref = got if ref is None else ref
                rows.append([name, cfg, flags, list(out8), [], torch.equal(got, ref)])
            for rd in range(9):
                for row in rows:
                    setcfg(row[1])
                    t, _ = timed(lambda: [launch(row[2]) for _ in range(10)])
                    if rd:
                        row[4].append(t / 10)
        finally:
            setcfg(-1)
        print(f"  B = {B:3d}  conv{k}x{k}s{s} {ci}->{co} on {h}x{w}")
        for name, cfg, flags, d, ts, same in rows:
            print(f"      {name:10s} {np.median(ts):7.1f} us  tile {d[0]}x{d[1]} RT {d[2]} NI {d[3]} workgroups {d[4]:4d}  "
                  f"{'=' if same else 'DIFFERS'}")
