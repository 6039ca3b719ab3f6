"""Throughput of the polyphase resampler (features.resample) on a corpus-sized call.

    python tools/resample_bench.py [--utts 2000] [--min-s 2] [--max-s 10] [--reps 7] [--rates 48000 44100 8000]

For every source rate and both sample formats (int16 PCM, float32): device events around whole calls (host planning,
table upload and the kernel) on seeded noise of uniformly random length, median of `--reps` calls after a warm-up.
Prints one JSON line per case: ms per call, hours of audio per second, the bytes the call must move (samples in, samples
out) over its time as a share of HBM bandwidth, the time of `log_mel_fbank` on the resampled audio next to it, and -- in
the same run, on the same device, float32 only -- what torch offers for the job: one `torch.nn.functional.conv1d` per
polyphase branch (stride M, that branch's T taps) over the packed signal as one long utterance (the utterance
boundaries, which the kernel respects, are ignored there: timing only)."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BW = 8.0e12                   # spec (6.3 TB/s achievable)


def timed(fn, reps):
    import torch
    fn()                                                              # warm-up: code objects, tables, allocator
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), [round(t, 3) for t in times]


def conv1d_per_phase(x, poly, L, M, T, half):
    """Every polyphase branch as one strided conv1d over the whole packed signal (float32)."""
    import torch
    import torch.nn.functional as F
    n = x.numel()
    per_phase = (n - 2 * (half // L) - 2 * T) // M - T - 4           # outputs every branch can produce from inside x
    xin = x.view(1, 1, -1)
    span = (per_phase - 1) * M + T
    outs = []
    for j in range(L):                                                # output m = j + i L, i = 0 .. per_phase - 1
        c = half + (j + L * (T + 1)) * M                              # start far enough in that no tap is before x[0]
        k_first, p = c // L - T + 1, c % L
        outs.append(F.conv1d(xin[:, :, k_first:k_first + span], poly[p, :T].view(1, 1, T), stride=M))
    return torch.cat(outs, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=2000)
    ap.add_argument("--min-s", type=float, default=2.0)
    ap.add_argument("--max-s", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rates", type=int, nargs="+", default=[48000, 44100, 8000])
    ap.add_argument("--new-rate", type=int, default=16000)
    ap.add_argument("--no-comparator", action="store_true")
    args = ap.parse_args()

    import torch
    from deepspeaker_pytorch_amd import features as F
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench needs an MI355X: nothing is timed on the host alone")
    for rate in args.rates:
        g = math.gcd(rate, args.new_rate)
        L, M = args.new_rate // g, rate // g
        half = 10 * max(L, M)
        T = -(-(2 * half + 1) // L)
        rs = np.random.RandomState(0)
        lens = rs.randint(int(args.min_s * rate), int(args.max_s * rate) + 1, size=args.utts)
        n_in = int(lens.sum())
        x32 = torch.empty(n_in, dtype=torch.float32, device="cuda").normal_(0.0, 0.1, generator=torch.Generator("cuda").manual_seed(0))
        x16 = (x32 * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
        comparator = None
        if not args.no_comparator:
            poly = F._device_taps(L, M, 10, 5.0, x32.device)
            try:
                ms, _ = timed(lambda: conv1d_per_phase(x32, poly, L, M, T, half), args.reps)
                comparator = {"conv1d_per_phase_ms": ms, "conv1d_calls": L}
            except RuntimeError as e:                                 # reported, never hidden: the figure is then absent
                comparator = {"conv1d_per_phase_error": str(e).splitlines()[0][:200]}
        for name, x in (("int16", x16), ("float32", x32)):
            ms, every = timed(lambda: F.resample(x, rate, args.new_rate, lengths=lens), args.reps)
            y, out_lens = F.resample(x, rate, args.new_rate, lengths=lens)
            fb_ms, _ = timed(lambda: F.log_mel_fbank(y, lengths=out_lens), args.reps)
            n_out = int(out_lens.sum())
            moved = x.element_size() * n_in + 4 * n_out
            res = {"orig_rate": rate, "new_rate": args.new_rate, "L": L, "M": M, "taps_per_output": T, "dtype": name,
                   "utterances": args.utts, "audio_hours": n_in / rate / 3600, "samples_in": n_in, "samples_out": n_out,
                   "call_ms_median": ms, "call_ms_all": every, "audio_hours_per_s": n_in / rate / 3600 / (ms * 1e-3),
                   "fma_per_s": n_out * T / (ms * 1e-3), "min_bytes": moved,
                   "hbm_fraction_of_spec": moved / (ms * 1e-3) / HBM_BW,
                   "log_mel_fbank_ms_on_the_resampled_audio": fb_ms}
            if name == "float32" and comparator is not None:
                res.update(comparator)
            print(json.dumps(res), flush=True)
        del x32, x16


if __name__ == "__main__":
    main()
