#!/usr/bin/env python
"""Times the identification path (scoring.nearest / identify, csrc/identify.hip) on the device against a chunked
torch.cdist + torch.topk on the same device in the same run, and (at the mining shape) against ds_mine_semihard_f32.

    python tools/identify_bench.py [--repeats 7] [--small]

Every figure is the median of `repeats` event-timed calls after a warm-up.  One JSON object per case on stdout:
times in ms, the search's share of the 157.3 TFLOP/s f32-MFMA peak (2 N M D flop of the distance GEMM over the whole
`nearest` call, rescoring included), the workspace the search holds and what an unchunked N x M matrix would take."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
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


def torch_nearest(q, g, k, chunk_bytes=1 << 30):
    """The baseline: the distance matrix in row chunks of at most `chunk_bytes`, top-k of each chunk."""
    rows = max(1, min(q.shape[0], chunk_bytes // (4 * g.shape[0])))
    d, i = [], []
    for r0 in range(0, q.shape[0], rows):
        dd, ii = torch.topk(torch.cdist(q[r0:r0 + rows], g), k, dim=1, largest=False)
        d.append(dd)
        i.append(ii)
    return torch.cat(d), torch.cat(i)


def unit_rows(n, d, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((n, d), device="cuda", generator=gen)
    return (10.0 * x / x.norm(dim=1, keepdim=True)).contiguous()


def case_nearest(name, n, m, d, k, repeats):
    from deepspeaker_pytorch_amd import scoring
    from deepspeaker_pytorch_amd.model import get_engine
    q, g = unit_rows(n, d, 1), unit_rows(m, d, 2)
    ours = timed(lambda: scoring.nearest(q, g, k), repeats)
    base = timed(lambda: torch_nearest(q, g, k), repeats)
    _, i_ours = scoring.nearest(q, g, k)
    _, i_base = torch_nearest(q, g, k)
    agree = float((i_ours == i_base).float().mean())
    ws = int(get_engine().lib.raw("ds_nearest_workspace_bytes")(n, m, d, k, 0))
    return {"case": name, "N": n, "M": m, "D": d, "k": k, "nearest_ms": round(ours, 4), "torch_cdist_topk_ms": round(base, 4),
            "speedup_vs_torch": round(base / ours, 3), "fraction_of_f32_mfma_peak": round(2.0 * n * m * d / (ours * 1e-3) / F32_MFMA_PEAK, 4),
            "workspace_bytes": ws, "unchunked_matrix_bytes": 4 * n * m, "index_agreement_with_torch": round(agree, 6)}


def case_mine(n, m, d, repeats):
    from deepspeaker_pytorch_amd.model import get_engine
    eng = get_engine()
    a, c = unit_rows(n, d, 3), unit_rows(m, d, 4)
    la = torch.arange(n, device="cuda", dtype=torch.int64)
    lc = torch.arange(m, device="cuda", dtype=torch.int64) % 997 + n
    d_p = torch.zeros(n, device="cuda")
    ws = torch.empty(int(eng.lib.raw("ds_mine_workspace_floats")(n, m)), device="cuda")
    out_i = torch.empty(n, dtype=torch.int64, device="cuda")
    out_d = torch.empty(n, device="cuda")
    call = lambda: eng.lib.call("ds_mine_semihard_f32", eng._p(a), eng._p(d_p), eng._p(la), eng._p(c), eng._p(lc), eng._p(ws),
                                eng._p(out_i), eng._p(out_d), n, m, d, eng._stream(a))
    return {"case": "ds_mine_semihard_f32", "N": n, "M": m, "D": d, "ms": round(timed(call, repeats), 4)}


def case_identify(n, s, d, k, repeats):
    from deepspeaker_pytorch_amd import scoring
    test, models = unit_rows(n, d, 5), unit_rows(s, d, 6)
    ml = torch.arange(s, device="cuda", dtype=torch.int64)
    tl = torch.arange(n, device="cuda", dtype=torch.int64) % s
    ours = timed(lambda: scoring.identify(test, models, ml, tl, k=k), repeats)
    base = timed(lambda: torch_nearest(test, models, k), repeats)
    return {"case": "identify", "N": n, "S": s, "D": d, "k": k, "identify_ms": round(ours, 4), "torch_cdist_topk_ms": round(base, 4),
            "speedup_vs_torch": round(base / ours, 3), "fraction_of_f32_mfma_peak": round(2.0 * n * s * d / (ours * 1e-3) / F32_MFMA_PEAK, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="a tenth of the sizes (a quick look)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("identify_bench needs an MI355X")
    big = (4096, 131072) if not args.small else (512, 16384)
    print(json.dumps(case_nearest("nearest_large", big[0], big[1], 512, 10, args.repeats)), flush=True)
    print(json.dumps(case_nearest("nearest_mining_shape", 256, 6144, 512, 1, args.repeats)), flush=True)
    print(json.dumps(case_mine(256, 6144, 512, args.repeats)), flush=True)
    print(json.dumps(case_identify(100000 if not args.small else 10000, 1251, 512, 5, args.repeats)), flush=True)


if __name__ == "__main__":
    main()
