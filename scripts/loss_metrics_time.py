"""Forward + backward time of the two cross-entropy kernel pairs (csrc/kernels/loss.hip), and with --model
the cost of one evaluate() batch against one training forward of ResNet-50.

At (1280, 1000) bf16 and (128, 1000) fp32, in one process: the existing pair (cross_entropy), the new pair
at eps = 0 and at eps = 0.1 (cross_entropy_with_metrics). Warm-up first, then the three variants interleaved
round by round, each round timed with HIP events around `--inner` forward + backward calls; prints one JSON
line per shape with the median per call, then the device and its clocks. The times include the autograd
dispatch of one forward and backward, the same for every variant.

    python scripts/loss_metrics_time.py [--reps 30] [--warmup 10] [--inner 20] [--model] [--batch 256]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_learning_amd.ops import _ext, cross_entropy, cross_entropy_with_metrics  # noqa: E402


def _clocks():
    try:
        out = subprocess.run(["rocm-smi", "-d", "0", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        return [ln.split(":", 1)[1].strip() if ln.startswith("GPU") else ln.strip()
                for ln in out.splitlines() if "sclk" in ln or "mclk" in ln]
    except (OSError, subprocess.SubprocessError):
        return []


def _timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def _graph_timed(fn, inner, reps):
    """The same calls replayed from a HIP graph: device time without the host's share of issuing them."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(inner):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    return [_timed(graph.replay, 1) / inner for _ in range(reps)]


def loss_times(dev, B, C, dtype, reps, warmup, inner):
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(B, C, generator=g) * 3).to(dev, dtype).requires_grad_(True)
    y = torch.randint(0, C, (B,), generator=g).to(dev)

    def run(loss_fn):
        def fn():
            x.grad = None
            loss_fn().backward()
        return fn

    variants = {"existing": run(lambda: cross_entropy(x, y)),
                "new_eps0": run(lambda: cross_entropy_with_metrics(x, y, 0.0, 5)[0]),
                "new_eps0.1": run(lambda: cross_entropy_with_metrics(x, y, 0.1, 5)[0])}
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(reps):  # interleaved: every variant sees the same drift of clocks and neighbours
        for k, fn in variants.items():
            ms[k].append(_timed(fn, inner))
    row = {"shape": [B, C], "dtype": str(dtype).split(".")[-1], "reps": reps, "inner": inner, "warmup": warmup}
    for k, v in ms.items():
        row[k + "_median_us"] = round(statistics.median(v) * 1e3, 2)
        row[k + "_min_us"] = round(min(v) * 1e3, 2)
    for k, fn in variants.items():
        row[k + "_graph_median_us"] = round(statistics.median(_graph_timed(fn, inner, reps)) * 1e3, 2)
    return row


def model_times(dev, batch, reps, warmup):
    """One evaluate() batch (eval-mode forward + loss and counts, no_grad) against one training-mode forward
    (+ loss) of ResNet-50 on the native bf16 path, interleaved."""
    from distributed_learning_amd.data import SyntheticBatches
    from distributed_learning_amd.models import resnet50
    from distributed_learning_amd.ops import nn as dnn
    from distributed_learning_amd.train import evaluate

    torch.manual_seed(0)
    model = resnet50().to(dev).to(memory_format=torch.channels_last)
    dnn.bf16_weights(model)
    dnn.set_backend("native")
    dnn.set_native_conv(True)
    model.train()
    kw = dict(dtype=torch.bfloat16, channels_last=True, regenerate=False)
    val = SyntheticBatches(batch, (3, 224, 224), 1000, dev, seed=2, **kw)
    x, y = SyntheticBatches(batch, (3, 224, 224), 1000, dev, seed=1, **kw).next()

    def train_fwd():
        return cross_entropy(model(x), y)

    def eval_batch():
        return evaluate(model, val, dev, "bf16", 1)

    for _ in range(warmup):
        train_fwd()
        eval_batch()
    torch.cuda.synchronize()
    ms = {"train_forward": [], "evaluate_batch": []}
    for _ in range(reps):
        ms["train_forward"].append(_timed(train_fwd, 1))
        ms["evaluate_batch"].append(_timed(eval_batch, 1))
    row = {"model": "resnet50", "batch": batch, "reps": reps, "warmup": warmup}
    for k, v in ms.items():
        row[k + "_median_ms"] = round(statistics.median(v), 3)
        row[k + "_min_ms"] = round(min(v), 3)
    row["evaluate_over_train_forward"] = round(row["evaluate_batch_median_ms"] / row["train_forward_median_ms"], 3)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--model", action="store_true", help="also time an evaluate() batch against a training forward")
    ap.add_argument("--batch", type=int, default=256)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20 (medians of fewer are noise)")
    _ext.require()
    dev = torch.device("cuda:0")
    for B, C, dtype in ((1280, 1000, torch.bfloat16), (128, 1000, torch.float32)):
        print(json.dumps(loss_times(dev, B, C, dtype, a.reps, a.warmup, a.inner)), flush=True)
    if a.model:
        print(json.dumps(model_times(dev, a.batch, a.reps, a.warmup)), flush=True)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "clocks": _clocks()}), flush=True)


if __name__ == "__main__":
    main()
