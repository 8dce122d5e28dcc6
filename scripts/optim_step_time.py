"""Step time of FusedSGD, FusedLARS, FusedLAMB and FusedAdamW on ResNet-50's parameter shapes (bf16 gradients,
fp32 masters), and of torch.optim.AdamW(fused=True) on fp32 copies of the same tensors where this torch has it.

Each optimizer: 5 warm-up steps, then 20 steps timed one by one with HIP events; prints one JSON line per
optimizer with the median and the launch count of a step, the device time of every kernel and the rate it
reaches against the bytes it has to move (``_BYTES``), then the device and its clocks. The gradients are fixed
random tensors: only the optimizer runs between the events.

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
from distributed_learning_amd.ops.optim import FusedAdamW, FusedLAMB, FusedLARS, FusedSGD  # noqa: E402


# Bytes per parameter element a kernel has to move, (bf16 gradient + bf16 shadow, fp32 gradient and no shadow):
# fp32 p, m, v (and momentum) at 4 B each way, the gradient read once, the shadow written once.
_BYTES = {
    "sgd_list_kernel": (20, 20),           # r p g m, w p m shadow
    "lars_list_kernel": (20, 20),
    "sqsum_list_kernel": (6, 8),           # r p g (LARS); the clipping pass of LAMB / AdamW reads g only
    "lamb_moments_list_kernel": (22, 24),  # r p g m v, w m v
    "lamb_apply_list_kernel": (18, 16),    # r p m v, w p shadow
    "adamw_list_kernel": (28, 28),         # r p g m v, w p m v shadow
}


def _rates(kernel_us, params, grad_only_sqsum):
    """GB/s of every kernel of ``_BYTES`` over its launches of one step (all gradient dtypes together)."""
    n16 = sum(p.numel() for p in params if p.grad.dtype == torch.bfloat16)
    n32 = sum(p.numel() for p in params if p.grad.dtype == torch.float32)
    out = {}
    for name, us in kernel_us.items():
        if name in _BYTES and us > 0:
            b16, b32 = (2, 4) if name == "sqsum_list_kernel" and grad_only_sqsum else _BYTES[name]
            out[name] = round((b16 * n16 + b32 * n32) / us * 1e-3, 1)
    return out


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
    rows = {}
    makers = {
        "FusedSGD": lambda ps: FusedSGD(ps, lr=0.01, momentum=0.9, weight_decay=1e-4, master_weights=True),
        "FusedLARS": lambda ps: FusedLARS(ps, lr=0.01, momentum=0.9, weight_decay=1e-4, max_grad_norm=1.0,
                                          master_weights=True),
        "FusedLAMB": lambda ps: FusedLAMB(ps, lr=0.002, weight_decay=1e-2, master_weights=True),
        "FusedLAMB+clip": lambda ps: FusedLAMB(ps, lr=0.002, weight_decay=1e-2, max_grad_norm=1.0,
                                               master_weights=True),
        "FusedAdamW": lambda ps: FusedAdamW(ps, lr=0.001, weight_decay=1e-2, master_weights=True),
        "FusedAdamW+clip": lambda ps: FusedAdamW(ps, lr=0.001, weight_decay=1e-2, max_grad_norm=1.0,
                                                 master_weights=True),
    }
    stock = "torch.optim.AdamW(fused=True) fp32"
    try:
        # capturable: its step counts live on the device, so that its step can be replayed from a graph too
        torch.optim.AdamW([torch.zeros(1, device=dev, requires_grad=True)], fused=True, capturable=True)
        makers[stock] = lambda ps: torch.optim.AdamW(ps, lr=0.001, weight_decay=1e-2, fused=True, capturable=True)
    except (RuntimeError, TypeError, ValueError) as e:
        print(json.dumps({"optimizer": stock, "unavailable": str(e)[:200]}), flush=True)
    for name, make in makers.items():
        m = _model(dev)
        params = list(m.parameters())
        if name == stock:  # the stock alternative has no masters: fp32 tensors and fp32 gradients
            grads = [p.grad.float() for p in params]
            params = [p.detach().float().requires_grad_() for p in params]
            for p, g in zip(params, grads):
                p.grad = g
        opt = make(params)
        ms = _time(opt, a.steps, a.warmup)
        launches, kernel_us = _launches(opt)
        gms = _time_graphed(opt, a.steps)
        n = sum(p.numel() for p in params)
        rows[name] = {"optimizer": name, "tensors": len(params), "params": n,
                      "median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
                      "max_ms": round(max(ms), 4), "graph_replay_median_ms": round(statistics.median(gms), 4),
                      "launches_per_step": launches, "kernel_us_per_step": kernel_us,
                      "kernel_gbps": _rates(kernel_us, params, name.startswith(("FusedLAMB", "FusedAdamW"))),
                      "steps": a.steps, "warmup": a.warmup}
        print(json.dumps(rows[name]), flush=True)
        del opt, m, params
    sgd = rows["FusedSGD"]
    print(json.dumps({**{f"{k}_over_sgd": round(r["median_ms"] / sgd["median_ms"], 3) for k, r in rows.items() if r is not sgd},
                      **{f"{k}_over_sgd_graph": round(r["graph_replay_median_ms"] / sgd["graph_replay_median_ms"], 3)
                         for k, r in rows.items() if r is not sgd},
                      "device": torch.cuda.get_device_name(0), "clocks": _clocks()}), flush=True)


if __name__ == "__main__":
    main()
