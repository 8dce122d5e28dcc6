"""Whole models in eval() mode on the native path, and train.evaluate() around training steps (gpu).

ResNet-50 eval-mode parity uses the bound of tests/test_gpu_model_parity.py (the reason is written there):
the native logits' relative L2 error against fp32 torch must stay within max(3 x the error of torch's own
bf16 autocast on the same input, 2e-2).
"""
import copy

import pytest
import torch

from test_gpu_model_parity import DEV, _batch, _models, _rel

pytestmark = pytest.mark.gpu


def test_resnet50_eval_mode_matches_fp32_torch(cuda):
    from distributed_learning_amd.ops import nn as dnn

    nat, ref = _models("resnet50")
    x, _ = _batch(16)
    xn = x.to(DEV, torch.bfloat16).contiguous(memory_format=torch.channels_last)
    dnn.set_backend("native")
    dnn.set_native_conv(True)
    try:
        nat.train()
        with torch.no_grad():  # three training-mode forwards: running statistics away from (0, 1)
            for seed in (21, 22, 23):
                nat(_batch(16, seed)[0].to(DEV, torch.bfloat16).contiguous(memory_format=torch.channels_last))
        assert float(nat.bn1.running_mean.abs().max()) > 0 and float((nat.layer4[2].bn3.running_var - 1).abs().max()) > 0
        ref.load_state_dict(nat.state_dict())  # the fp32 twin: same weights, same running statistics
        assert all(p.dtype == torch.float32 for p in ref.parameters())
        before = {k: v.clone() for k, v in nat.state_dict().items()}
        nat.eval()
        with torch.no_grad():
            out_n = nat(xn).float()
        for k, v in nat.state_dict().items():
            assert torch.equal(v, before[k]), k  # eval mode writes no running statistic
    finally:
        dnn.set_backend("torch")
        dnn.set_native_conv(False)
    auto = copy.deepcopy(ref)
    ref.eval()
    auto.eval()
    xr = x.to(DEV).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        out_r = ref(xr).float()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out_a = auto(xr).float()
    torch.cuda.synchronize()
    e_n, e_a = _rel(out_n, out_r), _rel(out_a, out_r)
    print(f"eval-mode logits rel. L2 error vs fp32 torch: native {e_n:.3g}, torch autocast {e_a:.3g}")
    assert e_n <= max(3 * e_a, 2e-2), (e_n, e_a)


class _Run:
    """The ResNet-18 configuration tests/test_gpu_lars.py steps: bf16 weights with fp32 masters in FusedLARS,
    channels_last, 8 x 32 x 32 synthetic batches."""

    def __init__(self, cuda):
        from distributed_learning_amd.data import SyntheticBatches
        from distributed_learning_amd.models import create_network
        from distributed_learning_amd.ops import nn as dnn
        from distributed_learning_amd.ops.optim import FusedLARS

        torch.manual_seed(0)
        self.model = create_network("resnet18_cifar").to(cuda).to(memory_format=torch.channels_last)
        dnn.bf16_weights(self.model)
        self.model.train()
        self.opt = FusedLARS(self.model.parameters(), lr=0.5, momentum=0.9, weight_decay=1e-4, max_grad_norm=1.0,
                             master_weights=True)
        kw = dict(dtype=torch.bfloat16, channels_last=True)
        self.train = SyntheticBatches(8, (3, 32, 32), 10, cuda, seed=1, **kw)
        self.val = SyntheticBatches(8, (3, 32, 32), 10, cuda, seed=2, **kw)
        self.cuda = cuda

    def step(self):
        from distributed_learning_amd.ops import cross_entropy

        x, y = self.train.next()
        self.opt.zero_grad(set_to_none=True)
        cross_entropy(self.model(x), y, 0.1).backward()
        self.opt.step()

    def evaluate(self):
        from distributed_learning_amd.train import evaluate

        return evaluate(self.model, self.val, self.cuda, "bf16", 2, topk=5)

    def state(self):
        out = {f"model.{k}": v.clone() for k, v in self.model.state_dict().items()}
        for i, p in enumerate(self.model.parameters()):
            for k, v in self.opt.state[p].items():
                if torch.is_tensor(v):
                    out[f"opt.{i}.{k}"] = v.clone()
        return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_evaluate_around_training_steps(cuda):
    from distributed_learning_amd.data import SyntheticBatches
    from distributed_learning_amd.ops import cross_entropy_with_metrics
    from distributed_learning_amd.ops import nn as dnn

    det = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    dnn.set_backend("native")
    dnn.set_native_conv(True)
    try:
        a, b = _Run(cuda), _Run(cuda)
        a.step()
        b.step()
        _same(a.state(), b.state())  # the step itself repeats bit for bit, or the comparison below says nothing
        before = a.state()
        assert any(k.endswith(".master") for k in before) and any("running_mean" in k for k in before)
        rng = torch.cuda.get_rng_state(cuda).clone(), torch.get_rng_state().clone()
        got = a.evaluate()
        _same(a.state(), before)  # parameters, fp32 masters, momentum and running statistics: not a bit moved
        assert torch.equal(torch.cuda.get_rng_state(cuda), rng[0]) and torch.equal(torch.get_rng_state(), rng[1])
        assert a.model.training and a.train.step == 1 and got == a.evaluate()
        # by hand
        val = SyntheticBatches(8, (3, 32, 32), 10, cuda, seed=2, dtype=torch.bfloat16, channels_last=True)
        total = torch.zeros(4, dtype=torch.float64)
        a.model.eval()
        with torch.no_grad():
            for _ in range(2):
                x, y = val.next()
                total += cross_entropy_with_metrics(a.model(x), y, 0.0, 5)[1].double().cpu()
        a.model.train()
        assert got["samples"] == 16 == int(total[1]) and got["k"] == 5
        assert got["loss"] == pytest.approx(float(total[0] / total[1]), rel=1e-6)
        assert got["top1"] == float(total[2] / total[1]) and got["topk"] == float(total[3] / total[1])
        # two steps with an evaluation between them == two steps
        a.step()
        b.step()
        _same(a.state(), b.state())
    finally:
        dnn.set_native_conv(False)
        dnn.set_backend("torch")
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = det
