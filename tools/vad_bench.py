"""Cost of the energy voice-activity decision (features.voiced_frames / select_frames, the vad= keyword of
features.log_mel_fbank) on a corpus-sized call.

    python tools/vad_bench.py [--utts 2000] [--min-s 2] [--max-s 10] [--reps 7]

The corpus is seeded: `--utts` utterances of uniformly random length, noise at speech level switched on and off in bursts
of 0.125 .. 0.5 s with gaps of 0.1 .. 0.375 s over a noise floor, as int16 PCM and as float32.  Device events around whole
calls (host planning, table uploads, every kernel and -- with vad= -- the read-back of the kept counts), median of
`--reps` calls after a warm-up, every single time printed next to it.  One JSON line per sample format:
`log_mel_fbank` without, with and again without vad= in the same run on the same device (the difference is the feature's
cost, the two baselines show the drift), the
calls it is made of on their own (`voiced_frames`, `select_frames`), the bytes the voice-activity kernels must move
(samples in; per frame the energy out and in, the mask out and in, the scan out and in; every kept row in and out for the
selection and again for the normalisation over the kept rows) over the added time as a share of HBM bandwidth, and --
float32 only -- what torch offers for the job: `unfold` + `sum` + `log` over the packed signal (the utterance boundaries,
which the kernels respect, are ignored there: timing only), a per-utterance loop for the mean, `cumsum` for the vote
and the scan, `index_select` for the rows."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BW = 8.0e12                   # spec (6.3 TB/s achievable)
RATE = 16000


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


def gate(n, rs):
    """0 / 1 per sample: bursts of 2000 .. 8000 samples, gaps of 1500 .. 6000"""
    pairs = n // 3500 + 2                                             # the shortest burst + gap is 3500 samples
    runs = np.stack([rs.randint(1500, 6000, pairs), rs.randint(2000, 8000, pairs)], 1).reshape(-1)
    return np.repeat(np.tile(np.array([0, 1], np.uint8), pairs), runs)[:n]


def torch_vad(x, feats, offsets, vad, frame_len, frame_step):
    """The rule with torch's own operators (boundaries between utterances ignored by the framing and the vote)."""
    import torch
    # (framing the packed signal as one utterance gives a few more frames than the utterances have rows: cut to the rows)
    frames = x.unfold(0, frame_len, frame_step)[:feats.shape[0]]
    e = torch.log(torch.clamp((frames * 32768.0).square().sum(1), min=vad.energy_floor))
    n = e.numel()
    thr = torch.empty_like(e)
    for u in range(len(offsets) - 1):
        a, b = int(offsets[u]), min(int(offsets[u + 1]), n)
        if a < b:
            thr[a:b] = vad.energy_threshold + vad.energy_mean_scale * e[a:b].mean()
    c = torch.cumsum(torch.nn.functional.pad((e > thr).to(torch.int32), (vad.frames_context + 1, vad.frames_context)), 0)
    width = 2 * vad.frames_context + 1
    voiced = (c[width:] - c[:-width]).to(torch.float64) >= vad.proportion_threshold * width
    scan = torch.cumsum(voiced.to(torch.int32), 0)                    # the positions of the kept rows
    rows = torch.nonzero(voiced).view(-1)                             # (reads the count back, as select_frames does)
    assert voiced.numel() <= feats.shape[0]                           # every index names a row
    return feats.index_select(0, rows), scan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=2000)
    ap.add_argument("--min-s", type=float, default=2.0)
    ap.add_argument("--max-s", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-comparator", action="store_true")
    args = ap.parse_args()

    import torch
    from deepspeaker_pytorch_amd import features as F
    if not torch.cuda.is_available():
        raise SystemExit("vad_bench needs an MI355X: nothing is timed on the host alone")
    cfg, vad = F.FbankConfig(), F.VadConfig()
    rs = np.random.RandomState(0)
    lens = rs.randint(int(args.min_s * RATE), int(args.max_s * RATE) + 1, size=args.utts)
    n = int(lens.sum())
    gen = torch.Generator("cuda").manual_seed(0)
    g = torch.from_numpy(gate(n, rs)).cuda().to(torch.float32)
    x32 = torch.empty(n, dtype=torch.float32, device="cuda").normal_(0.0, 0.1, generator=gen) * g
    x32 += torch.empty(n, dtype=torch.float32, device="cuda").normal_(0.0, 1e-3, generator=gen)
    del g
    x16 = (x32 * 32768.0).round().clamp(-32768, 32767).to(torch.int16)

    for name, x in (("int16", x16), ("float32", x32)):
        plain_ms, plain_all = timed(lambda: F.log_mel_fbank(x, lengths=lens), args.reps)
        vad_ms, vad_all = timed(lambda: F.log_mel_fbank(x, lengths=lens, vad=vad), args.reps)
        again_ms, again_all = timed(lambda: F.log_mel_fbank(x, lengths=lens), args.reps)     # the drift of the baseline
        mask_ms, mask_all = timed(lambda: F.voiced_frames(x, vad, lengths=lens), args.reps)
        feats, off = F.log_mel_fbank(x, normalize=None, lengths=lens)
        mask, _ = F.voiced_frames(x, vad, lengths=lens)
        select_ms, select_all = timed(lambda: F.select_frames(feats, off, mask), args.reps)
        kept, new_off = F.select_frames(feats, off, mask)
        n_frames, n_kept, row = int(off[-1]), int(new_off[-1]), 4 * cfg.nfilt
        moved = x.element_size() * n + n_frames * (4 + 4 + 1 + 1 + 4 + 4) + n_kept * 4 * row
        added = vad_ms - plain_ms
        res = {"dtype": name, "utterances": args.utts, "audio_hours": n / RATE / 3600, "samples": n, "frames": n_frames,
               "voiced_frames": n_kept, "voiced_share": n_kept / n_frames,
               "utterances_without_voiced_frames": int((np.diff(new_off) == 0).sum()),
               "log_mel_fbank_ms_median": plain_ms, "log_mel_fbank_ms_all": plain_all,
               "log_mel_fbank_ms_median_after": again_ms, "log_mel_fbank_ms_all_after": again_all,
               "log_mel_fbank_vad_ms_median": vad_ms, "log_mel_fbank_vad_ms_all": vad_all,
               "vad_added_ms": added, "vad_added_share_of_log_mel_fbank": added / plain_ms,
               "vad_added_ms_spread": [round(min(vad_all) - max(plain_all), 3), round(max(vad_all) - min(plain_all), 3)],
               "audio_hours_per_s": n / RATE / 3600 / (plain_ms * 1e-3),
               "audio_hours_per_s_with_vad": n / RATE / 3600 / (vad_ms * 1e-3),
               "voiced_frames_ms_median": mask_ms, "voiced_frames_ms_all": mask_all,
               "select_frames_ms_median": select_ms, "select_frames_ms_all": select_all,
               "vad_min_bytes": moved, "vad_hbm_fraction_of_spec": moved / (added * 1e-3) / HBM_BW}
        if name == "float32" and not args.no_comparator:
            ms, every = timed(lambda: torch_vad(x, feats, off, vad, cfg.frame_len, cfg.frame_step), args.reps)
            res.update({"torch_operators_ms_median": ms, "torch_operators_ms_all": every,
                        "torch_operators_over_voiced_plus_select": ms / (mask_ms + select_ms)})
        print(json.dumps(res), flush=True)
        del feats, mask, kept


if __name__ == "__main__":
    main()
