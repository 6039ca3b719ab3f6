#!/usr/bin/env python
"""Times the three device steps of diarisation (diarisation.pairwise_distances / linkage / cut, csrc/ahc.hip) on two
batches -- 256 recordings of 600 windows, 16 recordings of 4096 (the cap) -- against what a user would otherwise run:
torch.cdist per recording on the same device in the same run for the distances, scipy.cluster.hierarchy.linkage on the
host, one recording at a time, for the linkage.

    python tools/diarise_bench.py [--repeats 7] [--small] [--out profiles/diarise_mi355x.txt]

Every device time is the median of `repeats` event-timed whole calls after a warm-up (the linkage call includes the
clone of the matrices it consumes).  The per-step time is the linkage time over n - 1: the recordings of a batch run
side by side, one workgroup each, so the call lasts as long as one workgroup's steps.  SciPy is timed on the first few
recordings of the batch (their number is printed) and scaled to the batch; the host's core count and thread setting
are recorded with it.  One JSON object per batch, on stdout and in `--out`."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def embeddings(n_rec, n, d, seed):
    """rows on the radius-10 sphere around four "speakers" per recording"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    centres = torch.randn((n_rec, 4, d), device="cuda", generator=gen)
    who = torch.randint(0, 4, (n_rec, n), device="cuda", generator=gen)
    x = centres[torch.arange(n_rec, device="cuda")[:, None], who] + 0.5 * torch.randn((n_rec, n, d), device="cuda", generator=gen)
    return (10.0 * x / x.norm(dim=2, keepdim=True)).reshape(n_rec * n, d).contiguous()


def bench(n_rec, n, d, repeats, scipy_recs):
    from scipy.cluster.hierarchy import linkage as scipy_linkage
    from deepspeaker_pytorch_amd import diarisation as dia
    emb = embeddings(n_rec, n, d, 7)
    off = np.arange(n_rec + 1, dtype=np.int64) * n
    out = {"recordings": n_rec, "windows": n, "D": d}
    out["distances_ms"] = timed(lambda: dia.pairwise_distances(emb, off), repeats)
    out["torch_cdist_per_recording_ms"] = timed(lambda: [torch.cdist(emb[r * n:(r + 1) * n], emb[r * n:(r + 1) * n])
                                                        for r in range(n_rec)], repeats)
    x3 = emb.view(n_rec, n, d)
    out["torch_cdist_batched_ms"] = timed(lambda: torch.cdist(x3, x3), repeats)
    dist = dia.pairwise_distances(emb, off)
    cd = torch.cdist(x3[0], x3[0])
    ours = dist.matrix(0)
    mask = ~torch.eye(n, dtype=torch.bool, device="cuda")
    out["cdist_max_rel_difference"] = float(((cd - ours)[mask].abs() / ours[mask]).max())
    for method in ("average", "complete", "single"):
        ms = timed(lambda: dia.linkage(dist, method), repeats)
        out[f"linkage_{method}_ms"] = ms
        out[f"linkage_{method}_us_per_step"] = 1e3 * ms / (n - 1)
    out["matrix_clone_ms"] = timed(lambda: dist.data.clone(), repeats)
    dend = dia.linkage(dist, "average")
    h = dend.height[:n - 1].sort().values
    thr = float(h[n - 5] + h[n - 4]) / 2
    out["cut_ms"] = timed(lambda: dia.cut(dend, threshold=thr), repeats)
    out["n_found_first"] = int(dia.cut(dend, threshold=thr)[1][0])
    host = dist.data.cpu().numpy()
    iu = np.triu_indices(n, 1)
    t = []
    for r in range(min(scipy_recs, n_rec)):
        y = host[r * n * n:(r + 1) * n * n].reshape(n, n)[iu].astype(np.float64)
        t0 = time.perf_counter()
        scipy_linkage(y, "average")
        t.append(1e3 * (time.perf_counter() - t0))
    out["scipy_linkage_recordings_timed"] = len(t)
    out["scipy_linkage_ms_per_recording"] = statistics.median(t)
    out["scipy_linkage_ms_batch_scaled"] = statistics.median(t) * n_rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diarise_mi355x.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("diarise_bench.py measures on an MI355X: no ROCm device")
    from deepspeaker_pytorch_amd import diarisation as dia
    cases = ((8, 100, 64, 2), (2, 300, 64, 1)) if args.small else ((256, 600, 512, 16), (16, dia.AHC_MAX_N, 512, 2))
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "host_cores": os.cpu_count(),
                         "OMP_NUM_THREADS": os.environ.get("OMP_NUM_THREADS"), "torch_threads": torch.get_num_threads(),
                         "repeats": args.repeats})]
    print(lines[0], flush=True)
    for n_rec, n, d, scipy_recs in cases:
        lines.append(json.dumps(bench(n_rec, n, d, args.repeats, scipy_recs)))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
