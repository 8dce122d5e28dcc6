"""Step time of FusedSGD and FusedLARS on ResNet-50's parameter shapes (bf16 gradients, fp32 masters).

Each optimizer: 5 warm-up steps, then 20 steps timed one by one with HIP events; prints one JSON line per
optimizer with the median and the launch count of a step, then the device and its clocks. The gradients
are fixed random tensors: only the optimizer runs between the events.

    python scripts/optim_step_time.py [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_learning_amd.models import resnet50  # noqa: E402
from distributed_learning_amd.ops import _ext  # noqa: E402
from distributed_learning_amd.ops import nn as dnn  # noqa: E402
from distributed_learning_amd.ops.optim import FusedLARS, FusedSGD  # noqa: E402


def _model(dev):
    torch.manual_seed(0)
    m = resnet50().to(dev).to(memory_format=torch.channels_last)
    dnn.bf16_weights(m)
    g = torch.Generator().manual_seed(1)
    for p in m.parameters():
        p.grad = torch.empty_like(p).copy_((torch.randn(p.shape, generator=g) * 1e-2).to(dev))
    return m


def _launches(opt):
    """(kernel launches of one step, device microseconds per step by kernel name), counted by the profiler
    over 5 steps -- not derived from the optimizer's partitioning rules."""
    from torch.profiler import ProfilerActivity, profile

    n = 5
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(n):
            opt.step()
        torch.cuda.synchronize()
    count, per = 0, {}
    for e in prof.events():
        if e.device_type != torch.autograd.DeviceType.CUDA or "#" in e.name:  # "#": the step's own range mark
            continue
        count += 1
        name = e.name.split("(")[0].split("<")[0].split("::")[-1]
        per[name] = per.get(name, 0.0) + float(getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0))
    return count / n, {k: round(v / n, 2) for k, v in sorted(per.items())}


def _time(opt, steps, warmup):
    for _ in range(warmup):
        opt.step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        opt.step()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def _time_graphed(opt, steps):
    """The same step replayed from a HIP graph: device time without the host's share of issuing it."""
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    graph.replay()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def _clocks():
    try:
        out = subprocess.run(["rocm-smi", "-d", "0", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        return [ln.split(":", 1)[1].strip() if ln.startswith("GPU") else ln.strip()
                for ln in out.splitlines() if "sclk" in ln or "mclk" in ln]
    except (OSError, subprocess.SubprocessError):
        return []


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    _ext.require()
    dev = torch.device("cuda:0")
    rows = []
    for name in ("FusedSGD", "FusedLARS"):
        m = _model(dev)
        params = list(m.parameters())
        if name == "FusedSGD":
            opt = FusedSGD(params, lr=0.01, momentum=0.9, weight_decay=1e-4, master_weights=True)
        else:
            opt = FusedLARS(params, lr=0.01, momentum=0.9, weight_decay=1e-4, max_grad_norm=1.0, master_weights=True)
        ms = _time(opt, a.steps, a.warmup)
        launches, kernel_us = _launches(opt)
        gms = _time_graphed(opt, a.steps)
        n = sum(p.numel() for p in params)
        rows.append({"optimizer": name, "tensors": len(params), "params": n, "median_ms": round(statistics.median(ms), 4),
                     "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                     "graph_replay_median_ms": round(statistics.median(gms), 4),
                     "launches_per_step": launches, "kernel_us_per_step": kernel_us,
                     "steps": a.steps, "warmup": a.warmup})
        print(json.dumps(rows[-1]), flush=True)
    print(json.dumps({"lars_over_sgd": round(rows[1]["median_ms"] / rows[0]["median_ms"], 3),
                      "lars_over_sgd_graph": round(rows[1]["graph_replay_median_ms"] / rows[0]["graph_replay_median_ms"], 3),
                      "device": torch.cuda.get_device_name(0), "clocks": _clocks()}), flush=True)


if __name__ == "__main__":
    main()
