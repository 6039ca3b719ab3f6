"""Throughput of the log-mel filterbank front end (features.log_mel_fbank) on a corpus-sized call.

    python tools/fbank_bench.py [--utts 2000] [--min-s 2] [--max-s 10] [--reps 5] [--normalize mean]

Device events around whole calls (host framing, table upload, the filterbank kernel and the normalisation) on seeded
noise of uniformly random length.  Prints frames/s and hours of audio per second, the DFT GEMM's FLOP rate against the
f32 MFMA peak, the bytes the call must move against HBM bandwidth, and -- for scale only -- the speed of the float64
NumPy restatement of the reference (tests/fbank_reference.py) on this host's CPU: the reference's own libraries
(librosa, python_speech_features) are not available to time."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F32_MFMA_PEAK = 157.3e12          # v_mfma_f32_32x32x2_f32, spec (MI355X_MICROARCH: 155 TF measured)
HBM_BW = 8.0e12                   # spec (6.3 TB/s achievable)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=2000)
    ap.add_argument("--min-s", type=float, default=2.0)
    ap.add_argument("--max-s", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--normalize", default="mean", choices=["mean", "mean_std", "none"])
    ap.add_argument("--host-utts", type=int, default=20, help="utterances timed through the NumPy restatement")
    args = ap.parse_args()

    import torch
    from deepspeaker_pytorch_amd.features import FbankConfig, log_mel_fbank
    if not torch.cuda.is_available():
        raise SystemExit("fbank_bench needs an MI355X: nothing is timed on the host alone")
    cfg = FbankConfig()
    sr = cfg.sample_rate
    norm = None if args.normalize == "none" else args.normalize
    rs = np.random.RandomState(0)
    lens = rs.randint(int(args.min_s * sr), int(args.max_s * sr) + 1, size=args.utts)
    packed = torch.empty(int(lens.sum()), dtype=torch.float32, device="cuda").normal_(0.0, 0.1,
                                                                                      generator=torch.Generator("cuda").manual_seed(0))
    out, off = log_mel_fbank(packed, cfg, norm, lengths=lens)          # warm-up: code objects, basis tables
    torch.cuda.synchronize()
    frames = int(off[-1])
    times = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out, off = log_mel_fbank(packed, cfg, norm, lengths=lens)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    t = float(np.median(times))
    kpad = (cfg.frame_len + 1) & ~1
    tiles = int(sum((int(off[u + 1] - off[u]) + 63) // 64 for u in range(args.utts)))
    flop_useful = 2.0 * frames * kpad * cfg.nfft
    flop_issued = 2.0 * tiles * 64 * kpad * cfg.nfft                    # every tile runs 64 rows
    bytes_min = 4 * packed.numel() + 4 * frames * cfg.nfilt * (3 if norm else 1)   # samples in, features out (+ r/w)
    audio_s = float(lens.sum()) / sr

    # the float64 restatement on this host, for scale (single-threaded NumPy, like the reference's --makemfb loop)
    import fbank_reference as R
    host_x = [rs.randn(int(n)).astype(np.float32) * 0.1 for n in lens[:args.host_utts]]
    t0 = time.perf_counter()
    host_frames = sum(len(R.mk_mfb(x)) for x in host_x)
    host_t = time.perf_counter() - t0

    res = {
        "utterances": args.utts, "frames": frames, "audio_hours": audio_s / 3600, "normalize": args.normalize,
        "call_ms_median": t * 1e3, "call_ms_all": [round(x * 1e3, 3) for x in times],
        "frames_per_s": frames / t, "audio_hours_per_s": audio_s / 3600 / t,
        "dft_tflops_useful": flop_useful / t / 1e12, "dft_fraction_of_f32_mfma_peak": flop_useful / t / F32_MFMA_PEAK,
        "dft_tflops_issued": flop_issued / t / 1e12,
        "min_bytes": bytes_min, "hbm_fraction_of_spec": bytes_min / t / HBM_BW,
        "host_restatement_frames_per_s": host_frames / host_t,
        "host_restatement_note": "float64 NumPy restatement of mk_MFB on the host CPU (the reference's libraries are absent)",
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
