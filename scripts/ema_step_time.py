"""Step time of FusedSGD / FusedLARS with and without the weight EMA on ResNet-50's parameter list (bf16 weights,
fp32 masters, fixed random gradients: only the optimizer runs between the events). One variant per process:

    python scripts/ema_step_time.py ROOT OPT VARIANT      OPT: sgd | lars      VARIANT: off | fused | lerp

ROOT is the tree whose package is measured (put first on sys.path; "." for this one, a built checkout of another
commit to compare against it). off: ema_decay=0; fused: the EMA inside the update kernels; lerp: ema_decay=0 plus
torch._foreach_lerp_ over the masters after the step, the unfused alternative. 30 warm-up steps, then 300 steps timed
one by one with HIP events (median, 10th and 90th percentile) and once more as one window (per-step time with the
launch gaps). Prints one JSON line."""
import json
import os
import sys

root, optname, variant = os.path.abspath(sys.argv[1]), sys.argv[2], sys.argv[3]
sys.path.insert(0, root)

import torch  # noqa: E402

from distributed_learning_amd.models import create_network  # noqa: E402
from distributed_learning_amd.ops import _ext  # noqa: E402
from distributed_learning_amd.ops import nn as dnn  # noqa: E402
from distributed_learning_amd.ops.optim import FusedLARS, FusedSGD  # noqa: E402

assert torch.cuda.is_available()
_ext.require()
dev = torch.device("cuda:0")
torch.manual_seed(0)
model = create_network("resnet50").to(dev).to(memory_format=torch.channels_last)
dnn.bf16_weights(model)
ps = list(model.parameters())
g = torch.Generator(device=dev).manual_seed(1)
for p in ps:
    p.grad = torch.empty_like(p).copy_(torch.randn(p.shape, generator=g, device=dev) * 1e-3)
kw = dict(ema_decay=0.9999) if variant == "fused" else {}
if optname == "sgd":
    opt = FusedSGD(ps, lr=0.01, momentum=0.9, weight_decay=1e-4, master_weights=True, **kw)
else:
    opt = FusedLARS(ps, lr=0.1, momentum=0.9, weight_decay=1e-4, master_weights=True, **kw)
opt.step()
masters = [opt.state[p]["master"] if "master" in opt.state[p] else p.detach() for p in ps]
emas = [m.clone() for m in masters] if variant == "lerp" else None


def step():
    opt.step()
    if emas is not None:
        torch._foreach_lerp_(emas, masters, 1e-4)


for _ in range(30):
    step()
torch.cuda.synchronize()
N = 300
ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(N)]
for a, b in ev:
    a.record()
    step()
    b.record()
torch.cuda.synchronize()
ts = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
# one window of the same N steps: wall per step including launch gaps
a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
a.record()
for _ in range(N):
    step()
b.record()
torch.cuda.synchronize()
print(json.dumps(dict(opt=optname, variant=variant, tensors=len(ps), params=sum(p.numel() for p in ps),
                      median_us=round(ts[N // 2], 1), p10_us=round(ts[N // 10], 1), p90_us=round(ts[9 * N // 10], 1),
                      window_us_per_step=round(a.elapsed_time(b) * 1e3 / N, 1))), flush=True)
