#!/usr/bin/env python
"""Times the cohort statistics of score normalisation (scoring.cohort_stats, csrc/score_norm.hip) on the device against
the torch composition on the same device in the same run: a chunked torch.cdist (chunks of at most 1 GiB), then
torch.topk(K, largest=False), then mean and std(unbiased=False).

    python tools/score_norm_bench.py [--repeats 7] [--small] [--no-phases]

Every time is the median of `repeats` event-timed calls after a warm-up.  One JSON object per case on stdout: the two
times in ms, the kernels' time per phase (screening tiles; select plus rescoring -- from a profiler pass of its own,
after the timed ones), the screening GEMM's share of the 157.3 TFLOP/s f32-MFMA peak (2 N M D flop over the screening
kernels' time), the workspace held, what an unchunked N x M matrix would take and the agreement of the means with
torch's.  The last lines time candidate `row_block` sizes against the library's choice."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32_MFMA_PEAK = 157.3e12


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


def torch_cohort_stats(q, g, k, chunk_bytes=1 << 30):
    """The baseline: the distance matrix in row chunks of at most `chunk_bytes`, the K smallest of each row, their mean
    and population standard deviation."""
    rows = max(1, min(q.shape[0], chunk_bytes // (4 * g.shape[0])))
    mean, std = [], []
    for r0 in range(0, q.shape[0], rows):
        d = torch.cdist(q[r0:r0 + rows], g)
        if k < g.shape[0]:
            d = torch.topk(d, k, dim=1, largest=False).values
        mean.append(d.mean(dim=1))
        std.append(d.std(dim=1, unbiased=False))
    return torch.cat(mean), torch.cat(std)


def sphere_rows(n, d, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((n, d), device="cuda", generator=gen)
    return (10.0 * x / x.norm(dim=1, keepdim=True)).contiguous()


def phase_times(fn, calls):
    """Kernel time per call of the two phases, from the profiler's device events (None where it reports none)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    us = {"cohort_screen_kernel": 0.0, "cohort_select_kernel": 0.0}
    seen = 0
    for ev in prof.events():
        for name in us:
            if name in ev.name:
                us[name] += getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0)
                seen += 1
    if not seen or min(us.values()) <= 0.0:
        return None, None
    return us["cohort_screen_kernel"] / calls / 1e3, us["cohort_select_kernel"] / calls / 1e3


def case(name, n, m, d, k, repeats, phases):
    from deepspeaker_pytorch_amd import scoring
    from deepspeaker_pytorch_amd.model import get_engine
    q, g = sphere_rows(n, d, 1), sphere_rows(m, d, 2)
    ours = timed(lambda: scoring.cohort_stats(q, g, k), repeats)
    base = timed(lambda: torch_cohort_stats(q, g, k), repeats)
    st = scoring.cohort_stats(q, g, k)
    mean_t, std_t = torch_cohort_stats(q, g, k)
    screen_ms = select_ms = None
    if phases:
        screen_ms, select_ms = phase_times(lambda: scoring.cohort_stats(q, g, k), 3)
    ws = int(get_engine().lib.raw("ds_cohort_workspace_bytes")(n, m, d, k, 0))
    out = {"case": name, "N": n, "M": m, "D": d, "K": k, "cohort_stats_ms": round(ours, 4),
           "torch_cdist_topk_mean_std_ms": round(base, 4), "speedup_vs_torch": round(base / ours, 3),
           "screen_kernels_ms": None if screen_ms is None else round(screen_ms, 4),
           "select_rescore_kernels_ms": None if select_ms is None else round(select_ms, 4),
           "screen_fraction_of_f32_mfma_peak": None if screen_ms is None else
           round(2.0 * n * m * d / (screen_ms * 1e-3) / F32_MFMA_PEAK, 4),
           "whole_call_fraction_of_f32_mfma_peak": round(2.0 * n * m * d / (ours * 1e-3) / F32_MFMA_PEAK, 4),
           "workspace_bytes": ws, "unchunked_matrix_bytes": 4 * n * m,
           "mean_max_abs_diff_vs_torch": float((st.mean - mean_t).abs().max()),
           "std_max_abs_diff_vs_torch": float((st.std - std_t).abs().max())}
    print(json.dumps(out), flush=True)


def case_row_block(n, m, d, k, repeats):
    """The library's row_block (0) against smaller and larger blocks of screening values, alternating within one run."""
    from deepspeaker_pytorch_amd import scoring
    q, g = sphere_rows(n, d, 1), sphere_rows(m, d, 2)
    pitch = 4 * ((m + 3) // 4 * 4)
    cands = {"library": 0}
    for mib in (8, 32, 128):
        cands[f"{mib}MiB"] = max(64, (mib << 20) // pitch // 64 * 64)
    times = {name: [] for name in cands}
    for _ in range(3):
        for name, rb in cands.items():
            times[name].append(timed(lambda: scoring.cohort_stats(q, g, k, row_block=rb), repeats, warmup=1))
    print(json.dumps({"case": "row_block", "N": n, "M": m, "D": d, "K": k, "rows": cands,
                      "cohort_stats_ms": {name: round(statistics.median(v), 4) for name, v in times.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="an eighth of the rows (a quick look)")
    ap.add_argument("--no-phases", action="store_true", help="skip the profiler pass")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("score_norm_bench needs an MI355X")
    s = 8 if args.small else 1
    phases = not args.no_phases
    case("voxceleb1_o_speaker_means", 4708 // s, 5994, 512, 300, args.repeats, phases)
    case("large_cohort", 32768 // s, 16384, 512, 400, args.repeats, phases)
    case("all_rows_s_norm", 4708 // s, 5994, 512, 5994, args.repeats, phases)
    case_row_block(32768 // s, 16384, 512, 400, max(3, args.repeats // 2))
    case_row_block(4708 // s, 5994, 512, 300, max(3, args.repeats // 2))


if __name__ == "__main__":
    main()
