#!/usr/bin/env python3
"""Measure Mixup / CutMix in the augmentation kernel (csrc/kernels/augment.hip) and the pair-target loss
(csrc/kernels/loss.hip) beside the plain forms they extend.

Reads no dataset: every input comes from a seeded generator. Two measurements on one GPU, HIP events, medians of
``--rounds`` interleaved rounds after ``--warmup`` rounds, all in one process:

1. the augmentation at N = ``--batch``, uint8 256^2 -> bf16 224^2 with ``AugmentParams("rrc")`` boxes: the plain
   kernel, the select form with CutMix boxes (``MixParams`` at ``cutmix_alpha`` 1) and the blend form with Mixup
   weights (``mixup_alpha`` 0.2), each beside its byte count from the shapes (source bytes inside the crop boxes --
   the partner's too where it is sampled -- plus output bytes);
2. the loss at (``--batch``, ``--classes``) bf16, forward + backward: ``cross_entropy_mix`` against
   ``cross_entropy_with_metrics`` at the same label smoothing, beside the logit bytes both move.

The measuring runs in one child process under a time limit (``--timeout`` seconds); the parent never opens the
GPU. Prints one JSON line.

usage: python scripts/mix_bench.py [--batch 1280] [--classes 1000] [--rounds 20] [--warmup 5] [--timeout 300]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=1280)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--smoothing", type=float, default=0.1)
    ap.add_argument("--timeout", type=int, default=300, help="seconds the measuring process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args(argv)


def _interleaved(fns: dict, rounds: int, warmup: int) -> dict:
    """name -> list of HIP-event milliseconds, one per round; every round runs each function once, in order."""
    import torch

    times = {k: [] for k in fns}
    for r in range(warmup + rounds):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                times[name].append(e0.elapsed_time(e1))
    return times


def measure(a) -> dict:
    import torch

    from distributed_learning_amd.ops import _ext, cross_entropy_mix, cross_entropy_with_metrics
    from distributed_learning_amd.ops.augment import (IMAGENET_MEAN, IMAGENET_STD, AugmentParams, MixParams, augment,
                                                      augment_mix)

    _ext.require()
    dev = torch.device("cuda:0")
    n, src_hw, out_hw = a.batch, (256, 256), (224, 224)
    g = torch.Generator().manual_seed(1234)
    src = torch.randint(0, 256, (n, *src_hw, 3), generator=g, dtype=torch.uint8).to(dev)
    params = AugmentParams("rrc", src_hw, out_hw, seed=1234, stream=0)
    _, _, h, w, _ = params.boxes(0, n)
    geom, flip = (t.to(dev) for t in params.params(0, n))
    cut = MixParams(out_hw, 0.0, 1.0, seed=1234).params(0, n)
    mix = MixParams(out_hw, 0.2, 0.0, seed=1234).params(0, n)
    assert cut[4] is False and mix[4] is True
    cut_d, mix_d = [t.to(dev) for t in cut[:3]], [t.to(dev) for t in mix[:3]]
    bf16 = torch.bfloat16

    aug = _interleaved({
        "plain": lambda: augment(src, geom, flip, IMAGENET_MEAN, IMAGENET_STD, out_hw, bf16),
        "select_cutmix": lambda: augment_mix(src, geom, flip, *cut_d, IMAGENET_MEAN, IMAGENET_STD, out_hw, bf16, 0, False),
        "blend_cutmix": lambda: augment_mix(src, geom, flip, *cut_d, IMAGENET_MEAN, IMAGENET_STD, out_hw, bf16, 0, True),
        "blend_mixup": lambda: augment_mix(src, geom, flip, *mix_d, IMAGENET_MEAN, IMAGENET_STD, out_hw, bf16, 0, True),
    }, a.rounds, a.warmup)
    med = statistics.median
    # bytes from the shapes: the crop boxes' source pixels and the output; the forms that sample the partner
    # everywhere read its box too; the select form reads, per sample, the part of each box its pixels come from
    own = (h * w).double() * 3
    partner_box = own[cut[0].long()]
    y0, x0, y1, x1 = cut[2].double().unbind(1)
    frac = (y1 - y0) * (x1 - x0) / float(out_hw[0] * out_hw[1])
    write_b = n * out_hw[0] * out_hw[1] * 3 * 2
    read = {"plain": float(own.sum()), "select_cutmix": float((own * (1 - frac) + partner_box * frac).sum()),
            "blend_cutmix": float((own + partner_box).sum()), "blend_mixup": float((own + own[mix[0].long()]).sum())}
    out = {"batch": n, "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "cutmix_box": cut[2][0].tolist(), "mixup_lam": round(float(mix[1][0]), 4), "augment_write_MB": round(write_b / 1e6, 1)}
    for k, ts in aug.items():
        out[f"augment_{k}_ms"] = round(med(ts), 4)
        out[f"augment_{k}_ms_min_max"] = [round(min(ts), 4), round(max(ts), 4)]
        out[f"augment_{k}_read_MB"] = round(read[k] / 1e6, 1)
        out[f"augment_{k}_TBs"] = round((read[k] + write_b) / med(ts) / 1e9, 3)
    out["select_over_plain"] = round(med(aug["select_cutmix"]) / med(aug["plain"]), 3)
    out["blend_over_plain"] = round(med(aug["blend_mixup"]) / med(aug["plain"]), 3)
    del src

    # 2. the loss, forward + backward
    B, C = a.batch, a.classes
    x = (torch.randn(B, C, generator=g) * 3).to(dev, bf16).requires_grad_(True)
    ta, tb = (torch.randint(0, C, (B,), generator=g).to(dev) for _ in range(2))
    lam = mix[3].to(dev) if B == n else torch.full((B,), 0.3, device=dev)

    def plain_loss():
        x.grad = None
        cross_entropy_with_metrics(x, ta, a.smoothing)[0].backward()

    def mix_loss():
        x.grad = None
        cross_entropy_mix(x, ta, tb, lam, a.smoothing).backward()

    def two_calls():  # what the pair-target kernels replace: two losses and two backward passes over the logits
        x.grad = None
        (0.3 * cross_entropy_with_metrics(x, ta, a.smoothing)[0]
         + 0.7 * cross_entropy_with_metrics(x, tb, a.smoothing)[0]).backward()

    loss = _interleaved({"smoothed": plain_loss, "mix": mix_loss, "two_smoothed": two_calls}, a.rounds, a.warmup)
    logits_b = B * C * 2
    out.update({"loss_shape": [B, C], "loss_logit_MB_fwd_plus_bwd": round(3 * logits_b / 1e6, 2)})  # read, read, write
    for k, ts in loss.items():
        out[f"loss_{k}_fwd_bwd_ms"] = round(med(ts), 4)
        out[f"loss_{k}_fwd_bwd_ms_min_max"] = [round(min(ts), 4), round(max(ts), 4)]
    out["mix_over_smoothed"] = round(med(loss["mix"]) / med(loss["smoothed"]), 3)
    out["mix_over_two_smoothed"] = round(med(loss["mix"]) / med(loss["two_smoothed"]), 3)
    return out


def main(argv=None) -> int:
    a = _args(argv)
    if a.child:
        print(json.dumps(measure(a)), flush=True)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", *(argv if argv is not None else sys.argv[1:])]
    try:
        return subprocess.run(cmd, timeout=a.timeout).returncode
    except subprocess.TimeoutExpired:
        print(f"mix_bench: the measuring process ran past {a.timeout} s and was ended", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
