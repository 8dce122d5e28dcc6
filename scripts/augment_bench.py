#!/usr/bin/env python3
"""Measure the device-side augmentation (csrc/kernels/augment.hip) and the ``data2dev`` phase it replaces.

Reads no dataset: the host batches come from a seeded generator. Two measurements at N = ``--batch`` on one GPU:

1. the kernel alone, uint8 256^2 -> bf16 224^2 with random-resized-crop parameters: HIP events, median of
   ``--iters`` after ``--warmup`` launches, beside its byte count (source bytes inside the crop boxes + output
   bytes) and the time those bytes take at ``--copy-tbs`` (the copy rate the BatchNorm passes run at,
   profiles/r3/resnet50_bs1024_bytes_per_kernel.md);
2. the ``data2dev`` phase both ways, in this one process, interleaved ``--rounds`` times, medians of the
   synchronised wall time: the old way (fp32 [N, 3, 224, 224] host tensor -> ``.to(device)`` -> bf16 cast ->
   ``contiguous(channels_last)``) and the new one (uint8 [N, 256, 256, 3] host tensor -> ``.to(device)`` ->
   ``augment``), each also split into its copy and its device part.

The measuring runs in one child process under a time limit (``--timeout`` seconds); the parent never opens the
GPU. Prints one JSON line.

usage: python scripts/augment_bench.py [--batch 1280] [--iters 20] [--warmup 5] [--rounds 3] [--timeout 300]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=1280)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--copy-tbs", type=float, default=4.9, help="TB/s of a device copy (the BN passes' rate)")
    ap.add_argument("--timeout", type=int, default=300, help="seconds the measuring process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args(argv)


def measure(a) -> dict:
    import torch

    from distributed_learning_amd.ops import _ext
    from distributed_learning_amd.ops.augment import IMAGENET_MEAN, IMAGENET_STD, AugmentParams, augment

    _ext.require()
    dev = torch.device("cuda:0")
    n, src_hw, out_hw = a.batch, (256, 256), (224, 224)
    g = torch.Generator().manual_seed(1234)
    host_u8 = torch.randint(0, 256, (n, *src_hw, 3), generator=g, dtype=torch.uint8)
    host_f32 = torch.rand((n, 3, *out_hw), generator=g)
    params = AugmentParams("rrc", src_hw, out_hw, seed=1234, stream=0)
    y0, x0, h, w, _ = params.boxes(0, n)
    geom, flip = params.params(0, n)
    geom_d, flip_d = geom.to(dev), flip.to(dev)

    def run_augment(x):
        return augment(x, geom_d, flip_d, IMAGENET_MEAN, IMAGENET_STD, out_hw, torch.bfloat16)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    # 1. the kernel alone
    src = host_u8.to(dev)
    for _ in range(a.warmup):
        run_augment(src)
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run_augment(src)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    kernel_ms = statistics.median(ts)
    read_b = int((h * w).sum()) * 3
    write_b = n * out_hw[0] * out_hw[1] * 3 * 2
    floor_ms = (read_b + write_b) / (a.copy_tbs * 1e12) * 1e3
    del src

    # 2. data2dev both ways, interleaved
    def old_way():
        x = host_f32.to(dev, non_blocking=True)
        x = x.to(torch.bfloat16)
        return x.contiguous(memory_format=torch.channels_last)

    def new_way():
        return run_augment(host_u8.to(dev, non_blocking=True))

    old_ms, new_ms, old_parts, new_parts = [], [], [], []
    wall(old_way), wall(new_way)  # first touch of the allocator's blocks
    for _ in range(a.rounds):
        old_ms.append(wall(old_way)[0])
        new_ms.append(wall(new_way)[0])
        t_copy, x = wall(lambda: host_f32.to(dev))
        t_dev, _ = wall(lambda: x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last))
        old_parts.append((t_copy, t_dev))
        t_copy, x = wall(lambda: host_u8.to(dev))
        t_dev, _ = wall(lambda: run_augment(x))
        new_parts.append((t_copy, t_dev))
        del x
    med = statistics.median
    return {
        "batch": n, "device": torch.cuda.get_device_name(0),
        "kernel_ms": round(kernel_ms, 4), "kernel_ms_min": round(min(ts), 4), "kernel_ms_max": round(max(ts), 4),
        "kernel_read_MB": round(read_b / 1e6, 1), "kernel_write_MB": round(write_b / 1e6, 1),
        "kernel_TBs": round((read_b + write_b) / kernel_ms / 1e9, 3),
        "copy_rate_TBs": a.copy_tbs, "bytes_at_copy_rate_ms": round(floor_ms, 4),
        "fraction_of_copy_rate": round(floor_ms / kernel_ms, 3),
        "data2dev_old_ms": round(med(old_ms), 2), "data2dev_new_ms": round(med(new_ms), 2),
        "data2dev_old_all_ms": [round(t, 2) for t in old_ms], "data2dev_new_all_ms": [round(t, 2) for t in new_ms],
        "old_h2d_ms": round(med(p[0] for p in old_parts), 2), "old_cast_layout_ms": round(med(p[1] for p in old_parts), 3),
        "new_h2d_ms": round(med(p[0] for p in new_parts), 2), "new_augment_ms": round(med(p[1] for p in new_parts), 3),
        "old_h2d_MB": round(host_f32.numel() * 4 / 1e6, 1), "new_h2d_MB": round(host_u8.numel() / 1e6, 1),
        "speedup": round(med(old_ms) / med(new_ms), 2),
    }


def main(argv=None) -> int:
    a = _args(argv)
    if a.child:
        print(json.dumps(measure(a)), flush=True)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", *(argv if argv is not None else sys.argv[1:])]
    try:
        return subprocess.run(cmd, timeout=a.timeout).returncode
    except subprocess.TimeoutExpired:
        print(f"augment_bench: the measuring process ran past {a.timeout} s and was ended", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
