#!/usr/bin/env python
"""Times the angular-margin softmax head (DeepSpeakerModel.margin_loss, csrc/margin_head.hip), forward + backward, on the
device against two things in the same run:
  (b) the same loss composed from torch's own device operators -- F.normalize, F.linear, clamp, the margin on the whole
      matrix, torch.where on a one-hot mask, F.cross_entropy, autograd -- the usual ArcFace / CosFace module;
  (c) the plain softmax head of the same model, DeepSpeakerModel.classifier_loss.

    python tools/margin_head_bench.py [--repeats 21] [--kind aam]

M = 768 rows (3 x 256 embeddings of norm 10), K = 512, n_cls = 1211 and 5994.  Every figure is the median of `repeats`
event-timed calls after a warm-up: `*_ms` has one forward + backward between the two events (what an eager training
step sees, host enqueue included), `*_stream_ms` ten of them back to back divided by ten (the queue stays full).
`margin_loss_repack_ms` bumps the weight's version before every call, as an optimizer step does: the normalised and
packed copies of the classifier are then rebuilt inside the timed call.  One JSON object per shape on stdout."""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, repeats, warmup=3, inner=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return statistics.median(ms)


def torch_margin_loss(x, w, labels, margin, scale, kind, sin2_floor):
    c = F.linear(F.normalize(x, dim=1), F.normalize(w, dim=1)).clamp(-1.0, 1.0)
    if kind == "am":
        phi = c - margin
    else:
        sn = torch.sqrt(torch.clamp(1.0 - c * c, min=sin2_floor))
        phi = torch.where(c > -math.cos(margin), c * math.cos(margin) - sn * math.sin(margin), c - margin * math.sin(margin))
    mask = F.one_hot(labels, w.shape[0]).bool()
    return F.cross_entropy(scale * torch.where(mask, phi, c), labels)


def case(m, n_cls, kind, margin, scale, repeats):
    from deepspeaker_pytorch_amd._native import DS_MARGIN_SIN2_FLOOR
    from deepspeaker_pytorch_amd.model import DeepSpeakerModel
    gen = torch.Generator(device="cuda").manual_seed(n_cls)
    model = DeepSpeakerModel(512, n_cls).cuda()
    cls = model.model.classifier
    x = torch.randn((m, 512), device="cuda", generator=gen)
    emb = (10.0 * x / x.norm(dim=1, keepdim=True)).contiguous().requires_grad_(True)
    labels = torch.randint(0, n_cls, (m,), device="cuda", generator=gen)

    def run(loss_fn, repack=False):
        def step():
            emb.grad = cls.weight.grad = cls.bias.grad = None
            if repack:
                torch.autograd.graph.increment_version(cls.weight)
            loss_fn().backward()
        return step

    ours = run(lambda: model.margin_loss(emb, labels, margin=margin, scale=scale, kind=kind))
    ours_repack = run(lambda: model.margin_loss(emb, labels, margin=margin, scale=scale, kind=kind), repack=True)
    composed = run(lambda: torch_margin_loss(emb, cls.weight, labels, margin, scale, kind, DS_MARGIN_SIN2_FLOOR))
    plain = run(lambda: model.classifier_loss(emb, labels))

    # the three compute what they claim: the same loss and gradients from (a) and (b)
    ours()
    la, ga, gwa = model.margin_loss(emb, labels, margin=margin, scale=scale, kind=kind).item(), emb.grad.clone(), cls.weight.grad.clone()
    composed()
    lb = torch_margin_loss(emb, cls.weight, labels, margin, scale, kind, DS_MARGIN_SIN2_FLOOR).item()
    rel = lambda p, q: float((p - q).abs().max() / q.abs().max())                   # noqa: E731
    agree = {"loss_abs_diff": abs(la - lb), "embedding_grad_rel_diff": rel(ga, emb.grad), "weight_grad_rel_diff": rel(gwa, cls.weight.grad)}

    out = {"M": m, "K": 512, "n_cls": n_cls, "kind": kind, "margin": margin, "scale": scale}
    for name, fn in (("margin_loss", ours), ("torch_composed", composed), ("classifier_loss", plain), ("margin_loss_repack", ours_repack)):
        out[name + "_ms"] = round(timed(fn, repeats), 4)
        out[name + "_stream_ms"] = round(timed(fn, repeats, inner=10), 4)
    out["margin_over_torch"] = round(out["margin_loss_ms"] / out["torch_composed_ms"], 3)
    out["margin_over_torch_stream"] = round(out["margin_loss_stream_ms"] / out["torch_composed_stream_ms"], 3)
    out["margin_over_plain"] = round(out["margin_loss_ms"] / out["classifier_loss_ms"], 3)
    out["margin_over_plain_stream"] = round(out["margin_loss_stream_ms"] / out["classifier_loss_stream_ms"], 3)
    out["agreement_with_torch"] = {k: float(f"{v:.3g}") for k, v in agree.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--kind", default="aam", choices=["aam", "am"])
    ap.add_argument("--margin", type=float, default=0.2)
    ap.add_argument("--scale", type=float, default=30.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("margin_head_bench needs an MI355X")
    for n_cls in (1211, 5994):
        print(json.dumps(case(768, n_cls, args.kind, args.margin, args.scale, args.repeats)), flush=True)


if __name__ == "__main__":
    main()
