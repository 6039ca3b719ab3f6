#!/usr/bin/env python3
"""Same-process A/B of the waveform front end (features.log_mel_fbank: plain, with vad=, with augment=, and from 48 kHz
stereo) between library builds tools/_ab/libds_ab_<name>.so, from float32 and from int16 input.
    python tools/frontend_ab.py [--utts 256] [--rounds 7] base other ...
Every chain's features and offsets must be bitwise those of the first library; the calls are timed with device events in
interleaved rounds (the first round is the warm-up).  One JSON line per chain and input type."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from deepspeaker_pytorch_amd import features as F
from deepspeaker_pytorch_amd._native import NativeLib
from deepspeaker_pytorch_amd.engine import Engine

RATE = 16000


def gated_noise(n, seed, dev):
    """noise in bursts of a quarter second with near-silence between them: the voice-activity decision keeps a part"""
    g = torch.Generator(dev).manual_seed(seed)
    x = torch.empty(n, dtype=torch.float32, device=dev).normal_(0.0, 0.1, generator=g)
    on = (torch.arange(n, device=dev) // (RATE // 4)) % 3 != 2
    return x * torch.where(on, 1.0, 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--min-s", type=float, default=2.0)
    ap.add_argument("--max-s", type=float, default=6.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("names", nargs="+")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frontend_ab needs an MI355X: nothing is timed on the host alone")
    dev = "cuda"
    engs = [Engine(NativeLib(os.path.join(ROOT, "tools", "_ab", f"libds_ab_{n}.so"))) for n in args.names]
    rs = np.random.RandomState(0)
    lens = rs.randint(int(args.min_s * RATE), int(args.max_s * RATE) + 1, size=args.utts).astype(np.int64)
    x = gated_noise(int(lens.sum()), 0, dev)
    lens48 = 3 * lens
    mono48 = gated_noise(int(lens48.sum()), 1, dev)
    x48 = torch.stack([mono48, 0.5 * mono48], 1).reshape(-1).contiguous()
    rirs = F.SampleBank([(np.random.RandomState(200 + i).randn(2048) * np.exp(-np.arange(2048) / 300.0)).astype(np.float32)
                         for i in range(8)], dev)
    noise = F.SampleBank([(0.05 * np.random.RandomState(100 + i).randn(5 * RATE)).astype(np.float32) for i in range(4)], dev)
    plan = F.draw_augmentation(np.random.RandomState(1), args.utts, rirs, noise, p_rir=0.75, p_noise=0.75, noises=(1, 2))
    as_i16 = lambda t: (t * 29000.0).clamp(-32768, 32767).to(torch.int16)
    chains = {"plain": (x, lens, {}), "vad": (x, lens, dict(vad=F.VadConfig())), "augment": (x, lens, dict(augment=plan)),
              "48k_stereo": (x48, lens48, dict(orig_rate=48000, channels=2))}
    ok = True
    for name, (wave, wl, kw) in chains.items():
        for dtype, w in (("float32", wave), ("int16", as_i16(wave))):
            times, outs = [[] for _ in engs], [None] * len(engs)
            for rnd in range(args.rounds):
                for i, e in enumerate(engs):
                    F._engine_override = e
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    out, off = F.log_mel_fbank(w, lengths=wl, **kw)
                    b.record()
                    b.synchronize()
                    if rnd:
                        times[i].append(a.elapsed_time(b))
                    outs[i] = (out, off)
            F._engine_override = None
            same = [torch.equal(o.view(torch.int32), outs[0][0].view(torch.int32)) and f.tolist() == outs[0][1].tolist()
                    for o, f in outs]
            ok = ok and all(same)
            print(json.dumps({"chain": name, "input": dtype, "utterances": args.utts, "rows": int(outs[0][1][-1]),
                              "libraries": args.names, "bitwise_equal_to_first": same,
                              "call_ms_median": [round(float(np.median(t)), 4) for t in times],
                              "call_ms_all": [[round(v, 4) for v in t] for t in times]}), flush=True)
    if not ok:
        raise SystemExit("outputs differ between the libraries")


if __name__ == "__main__":
    main()
