#!/usr/bin/env python3
"""Measure the resident-store input path (``--resident 1``) against the host path it replaces.

Reads no dataset: everything is seeded noise. Two modes, each in one child process under a time limit
(``--timeout`` seconds); the parent never opens the GPU. Each prints one JSON line.

default -- the kernel and the phase, N = ``--batch``, uint8 256^2 -> bf16 224^2, random-resized-crop boxes as in
scripts/augment_bench.py, interleaved ``--rounds`` times:

  (a) the host path's ``data2dev``: pageable H2D copy of uint8 [N, 256, 256, 3] plus the plain kernel
      (synchronised wall time);
  (b) the indexed kernel reading a random index out of a noise-filled device store of ``--rows`` images
      (HIP events, median of ``--iters`` launches per round);
  (c) the plain kernel on the same N images gathered contiguously (HIP events likewise).

``--cli`` -- the training command line itself: writes a noise-filled staged directory of ``--images`` images with
numpy (no PIL), then runs ``resnet50`` at batch ``--batch`` over it with ``--staged_dir`` alone and with
``--resident 1``, ``--sync_timers 1`` so that every phase column is that phase's own time, and reports the
``get_data`` and ``data2dev`` columns of ``*_times.csv`` (``*_device_times.csv`` times the device phases forward
to optimizer_step only and has no such columns).

usage: python scripts/resident_bench.py [--batch 1280] [--rows 20000] [--iters 10] [--rounds 3] [--timeout 420]
       python scripts/resident_bench.py --cli [--images 5120] [--batches 8] [--dir DIR] [--timeout 900]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=1280)
    ap.add_argument("--rows", type=int, default=20000, help="images in the device store (3.9 GB at 20000)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cli", action="store_true", help="measure the training command line instead of the kernel")
    ap.add_argument("--images", type=int, default=5120, help="--cli: images in the staged directory")
    ap.add_argument("--batches", type=int, default=8, help="--cli: training batches per run")
    ap.add_argument("--dir", default=None, help="--cli: where the staged files and results go (default: a temp dir)")
    ap.add_argument("--timeout", type=int, default=None, help="seconds the measuring process may take")
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
    host_u8 = torch.randint(0, 256, (n, *src_hw, 3), generator=g, dtype=torch.uint8)  # pageable
    params = AugmentParams("rrc", src_hw, out_hw, seed=1234, stream=0)
    geom, flip = params.params(0, n)
    geom_d, flip_d = geom.to(dev), flip.to(dev)
    gd = torch.Generator(device=dev).manual_seed(99)
    store = torch.empty((a.rows, *src_hw, 3), dtype=torch.uint8, device=dev)
    for lo in range(0, a.rows, 1024):  # noise, filled in chunks
        hi = min(lo + 1024, a.rows)
        store[lo:hi] = torch.randint(0, 256, (hi - lo, *src_hw, 3), generator=gd, dtype=torch.uint8, device=dev)
    index = torch.randint(0, a.rows, (n,), generator=g).to(torch.int32)
    index_d = index.to(dev)
    gathered = store[index_d.long()].contiguous()

    def plain(x):
        return augment(x, geom_d, flip_d, IMAGENET_MEAN, IMAGENET_STD, out_hw, torch.bfloat16)

    def indexed():
        return augment(store, geom_d, flip_d, IMAGENET_MEAN, IMAGENET_STD, out_hw, torch.bfloat16, index=index_d)

    assert torch.equal(indexed().view(torch.int16), plain(gathered).view(torch.int16)), "indexed != gathered"

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def events(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    host_path = lambda: plain(host_u8.to(dev, non_blocking=True))  # noqa: E731
    wall(host_path)  # first touch of the allocator's blocks
    ra, rb, rc, rh = [], [], [], []
    for _ in range(a.rounds):
        ra.append(wall(host_path))
        rh.append(wall(lambda: host_u8.to(dev)))
        rb.append(events(indexed))
        rc.append(events(lambda: plain(gathered)))
    med, r3 = statistics.median, lambda v: [round(t, 4) for t in v]  # noqa: E731
    return {
        "batch": n, "store_rows": a.rows, "store_GB": round(store.numel() / 1e9, 2),
        "device": torch.cuda.get_device_name(0),
        "a_host_h2d_plus_plain_ms": round(med(ra), 3), "a_rounds_ms": r3(ra),
        "a_h2d_alone_ms": round(med(rh), 3), "a_h2d_alone_rounds_ms": r3(rh),
        "h2d_MB": round(host_u8.numel() / 1e6, 1), "h2d_GBs": round(host_u8.numel() / med(rh) / 1e6, 1),
        "b_indexed_kernel_ms": round(med(rb), 4), "b_rounds_ms": r3(rb),
        "c_plain_kernel_gathered_ms": round(med(rc), 4), "c_rounds_ms": r3(rc),
        "b_minus_c_ms": round(med(rb) - med(rc), 4),
        "spread_ms": round(max(max(rb) - min(rb), max(rc) - min(rc)), 4),
        "phase_speedup_a_over_b": round(med(ra) / med(rb), 1),
    }


def write_staged(directory: str, count: int, classes: int = 1000, seed: int = 7) -> None:
    """A noise-filled staged training split, written the way distributed_learning_amd.stage writes a decoded one."""
    import numpy as np

    os.makedirs(directory, exist_ok=True)
    rng = np.random.default_rng(seed)
    images = np.lib.format.open_memmap(os.path.join(directory, "train_images.npy"), mode="w+", dtype=np.uint8,
                                       shape=(count, 256, 256, 3))
    for lo in range(0, count, 256):
        hi = min(lo + 256, count)
        images[lo:hi] = rng.integers(0, 256, (hi - lo, 256, 256, 3), dtype=np.uint8)
    images.flush()
    del images
    np.save(os.path.join(directory, "train_labels.npy"), rng.integers(0, classes, count).astype(np.int64))
    meta = {"count": count, "stage": 256, "classes": [f"c{i:04d}" for i in range(classes)], "split": "train",
            "names_sha256": "0" * 64}
    with open(os.path.join(directory, "train_meta.json"), "w") as f:
        json.dump(meta, f)


def _columns(path: str) -> dict:
    with open(path) as f:
        rows = [line.rstrip("\n").split(", ") for line in f]
    head = rows[0]
    out = {}
    for name in ("get_data", "data2dev", "batch"):
        col = head.index(name)
        out[name] = [round(float(r[col]), 3) for r in rows[1:]]
    return out


def measure_cli(a) -> dict:
    base = a.dir or tempfile.mkdtemp(prefix="resident_bench_")
    staged = os.path.join(base, "staged")
    write_staged(staged, a.images)
    result = {"images": a.images, "batch": a.batch, "batches": a.batches, "model": "resnet50"}
    per_run = max(60, ((a.timeout or 900) - 120) // 2)
    for name, extra in (("staged_dir", []), ("resident", ["--resident", "1"])):
        out = os.path.join(base, name)
        os.makedirs(out, exist_ok=True)
        cmd = [sys.executable, "-m", "distributed_learning_amd.main", "1", "0", "1", "1", "127.0.0.1", "lo", "resnet50",
               staged, "1", "--experiment", "main_single", "--limit_batches", str(a.batches), "--epoch_count", "100",
               "--batch_size", str(a.batch), "--augment", "standard", "--staged_dir", staged, "--sync_timers", "1",
               "--results_root", out, "--job_id", "t", *extra]
        t0 = time.time()
        r = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), cwd=out, capture_output=True, text=True,
                           timeout=per_run)
        if r.returncode != 0:
            raise RuntimeError(f"{name} run failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
        cols = _columns(os.path.join(out, "main_single_1_t", "single_0_0_times.csv"))
        result[name] = {
            "run_s": round(time.time() - t0, 1),
            "get_data_ms": cols["get_data"], "data2dev_ms": cols["data2dev"], "batch_ms": cols["batch"],
            # the first batch pays the loader's start, kernel loading and the allocator's first touch
            "get_data_median_after_first_ms": round(statistics.median(cols["get_data"][1:]), 3),
            "data2dev_median_after_first_ms": round(statistics.median(cols["data2dev"][1:]), 3),
            "batch_median_after_first_ms": round(statistics.median(cols["batch"][1:]), 3),
        }
    return result


def main(argv=None) -> int:
    a = _args(argv)
    if a.child:
        print(json.dumps(measure_cli(a) if a.cli else measure(a)), flush=True)
        return 0
    limit = a.timeout or (900 if a.cli else 420)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", *(argv if argv is not None else sys.argv[1:])]
    try:
        return subprocess.run(cmd, timeout=limit).returncode
    except subprocess.TimeoutExpired:
        print(f"resident_bench: the measuring process ran past {limit} s and was ended", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
