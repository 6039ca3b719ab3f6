"""Cost of the waveform augmentation (features.augment) on a batch of training utterances, next to torch's own operators.

    python tools/augment_bench.py [--utts 768] [--min-s 2] [--max-s 6] [--reps 7] [--taps 512 2048 8192]
                                  [--out profiles/augment_mi355x.txt]

The workload: `--utts` float32 utterances of uniformly random length at 16 kHz, every one with an impulse response of the
given number of taps (a bank of 16 decaying-noise responses) and one noise clip (a bank of 8 clips of 10 s) at a drawn
ratio, level="input".  Device events around whole calls (host tables, their upload and the kernels), median of `--reps`
calls after a warm-up.  One JSON line per number of taps, printed and appended to `--out`:
  * augment_ms: `features.augment`; reverb_kernel_ms: ds_augment_reverb_f32 alone on tables already on the device, its
    useful TFLOP/s (2 n K per utterance) and that as a share of the 157 TFLOP/s f32 MFMA peak
  * fbank_ms / fbank_augment_ms: `log_mel_fbank` without and with `augment=`
  * fft_*: the same augmentation from torch's operators on the same device -- the batch padded to its longest utterance
    plus the taps, rounded up to a power of two, torch.fft.rfft of signals and responses, their product, irfft, the
    shifted slice, masked powers, the noise gathered by index, gains and level as tensor operations -- its time, its
    peak allocated memory next to the packed path's, and its largest difference from the packed result."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32_MFMA_PEAK = 157.0e12
RATE = 16000


def timed(fn, reps):
    import torch
    fn()                                                              # warm-up: code objects, plans, allocator
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


def peak_bytes(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return int(torch.cuda.max_memory_allocated() - base)


def decaying_rir(seed, K):
    rs = np.random.RandomState(seed)
    d = K // 16
    t = np.arange(K)
    h = 0.3 * rs.randn(K) * 10.0 ** (-3.0 * np.maximum(t - d, 0) / (0.3 * K))
    h[:d] *= 0.1
    h[d] = 1.0
    return h.astype(np.float32)


def fft_augment(x, lens, plan):
    """features.augment(x, plan, lengths=lens) with level="input" from torch's operators; returns the padded [n_utt, Lmax]
    result (zero past each utterance's end)."""
    import torch
    dev = x.device
    n_utt, l_max = len(lens), int(lens.max())
    rb, nb = plan.rir_bank, plan.noise_bank
    k_max = int(rb.lengths.max())
    n_fft = 1 << int(l_max + k_max - 1).bit_length()
    lens_t = torch.from_numpy(lens).to(dev)
    col = torch.arange(l_max, device=dev)
    mask = col[None, :] < lens_t[:, None]
    xp = torch.zeros((n_utt, l_max), dtype=torch.float32, device=dev)
    xp[mask] = x                                                      # the packed samples in row-major order
    # impulse responses [n_utt, k_max] by index
    roff = torch.from_numpy(rb.offsets[plan.rir_index]).to(dev)
    rlen = torch.from_numpy(rb.lengths[plan.rir_index]).to(dev)
    kcol = torch.arange(k_max, device=dev)
    h = torch.where(kcol[None, :] < rlen[:, None], rb.samples[(roff[:, None] + kcol[None, :]).clamp_(max=rb.samples.numel() - 1)],
                    torch.zeros((), device=dev))
    full = torch.fft.irfft(torch.fft.rfft(xp, n_fft) * torch.fft.rfft(h, n_fft), n_fft)
    delay = torch.from_numpy(rb.delay[plan.rir_index]).to(dev)
    r = torch.gather(full, 1, delay[:, None] + col[None, :]) * mask
    n_f = lens_t.to(torch.float64)
    p_x = (xp.double() ** 2).sum(1) / n_f
    p_r = (r.double() ** 2).sum(1) / n_f
    s = r
    for j in range(plan.noise_index.shape[1]):
        idx = plan.noise_index[:, j]
        noff = torch.from_numpy(nb.offsets[idx]).to(dev)
        nlen = torch.from_numpy(nb.lengths[idx]).to(dev)
        start = torch.from_numpy(plan.noise_start[:, j]).to(dev)
        v = nb.samples[noff[:, None] + (start[:, None] + col[None, :]) % nlen[:, None]]
        p_v = torch.from_numpy(nb.mean_square[idx] * 10.0 ** (plan.snr_db[:, j] / 10.0)).to(dev)
        g = torch.sqrt(p_r / p_v).float()
        s = s + g[:, None] * v * mask
    p_s = (s.double() ** 2).sum(1) / n_f
    return s * torch.sqrt(p_x / p_s).float()[:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=768)
    ap.add_argument("--min-s", type=float, default=2.0)
    ap.add_argument("--max-s", type=float, default=6.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--taps", type=int, nargs="+", default=[512, 2048, 8192])
    ap.add_argument("--no-comparator", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_mi355x.txt"))
    args = ap.parse_args()

    import torch
    from deepspeaker_pytorch_amd import features as F
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs an MI355X: nothing is timed on the host alone")
    eng = F._eng()
    rs = np.random.RandomState(0)
    lens = rs.randint(int(args.min_s * RATE), int(args.max_s * RATE) + 1, size=args.utts).astype(np.int64)
    n_in = int(lens.sum())
    x = torch.empty(n_in, dtype=torch.float32, device="cuda").normal_(0.0, 0.1, generator=torch.Generator("cuda").manual_seed(0))
    noise = F.SampleBank([(0.05 * np.random.RandomState(100 + i).randn(10 * RATE)).astype(np.float32) for i in range(8)], "cuda")
    lines = []
    for K in args.taps:
        rirs = F.SampleBank([decaying_rir(200 + i, K) for i in range(16)], "cuda")
        plan = F.draw_augmentation(np.random.RandomState(1), args.utts, rirs, noise, p_rir=1.0, p_noise=1.0, snr_db=(0.0, 15.0))
        ms, every = timed(lambda: F.augment(x, plan, lengths=lens), args.reps)
        packed_peak = peak_bytes(lambda: F.augment(x, plan, lengths=lens))

        # the reverberation kernel alone, on tables already on the device
        rir_tab, max_taps, _ = F._augment_tables(plan, args.utts, x.device)
        _, counts, table_dev, (rir_dev,) = F._plan(eng, x.device, "ds_augment_plan", lens, args.utts, (), 1, n_counts=4,
                                                   tails=(rir_tab,))
        n_tiles = int(counts[1])
        out = torch.empty(n_in, dtype=torch.float32, device="cuda")
        ws = torch.empty(3 * n_tiles, dtype=torch.float64, device="cuda")
        kernel = lambda: eng.lib.call("ds_augment_reverb_f32", eng._p(x), 0, eng._p(table_dev), args.utts, n_tiles,
                                      eng._p(rirs.samples), eng._p(rir_dev), max_taps, eng._p(out), eng._p(ws), eng._stream(out))
        k_ms, _ = timed(kernel, args.reps)
        flop = 2.0 * float((lens * rirs.lengths[plan.rir_index]).sum())

        fb_ms, _ = timed(lambda: F.log_mel_fbank(x, lengths=lens), args.reps)
        fba_ms, _ = timed(lambda: F.log_mel_fbank(x, lengths=lens, augment=plan), args.reps)
        res = {"taps": K, "utterances": args.utts, "audio_hours": n_in / RATE / 3600, "samples": n_in, "tiles": n_tiles,
               "tile": int(counts[2]), "k_chunk": int(counts[3]), "augment_ms": ms, "augment_ms_all": every,
               "reverb_kernel_ms": k_ms, "reverb_useful_tflop": flop / 1e12, "reverb_tflops": flop / (k_ms * 1e-3) / 1e12,
               "reverb_fraction_of_f32_mfma_peak": flop / (k_ms * 1e-3) / F32_MFMA_PEAK,
               "augment_peak_bytes": packed_peak, "fbank_ms": fb_ms, "fbank_augment_ms": fba_ms,
               "augment_adds_to_fbank_ms": fba_ms - fb_ms}
        if not args.no_comparator:
            try:
                f_ms, f_every = timed(lambda: fft_augment(x, lens, plan), args.reps)
                res.update({"fft_ms": f_ms, "fft_ms_all": f_every, "fft_peak_bytes": peak_bytes(lambda: fft_augment(x, lens, plan))})
                y, _ = F.augment(x, plan, lengths=lens)
                pad = fft_augment(x, lens, plan)
                mask = torch.arange(pad.shape[1], device="cuda")[None, :] < torch.from_numpy(lens).cuda()[:, None]
                res["fft_max_abs_difference"] = float((pad[mask] - y).abs().max())
                res["packed_over_fft_time"] = ms / f_ms
                del pad, y, mask
            except RuntimeError as e:                                 # reported, never hidden: the figure is then absent
                res["fft_error"] = str(e).splitlines()[0][:200]
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        del rirs, plan, table_dev, rir_dev, out, ws
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
