"""FusedSGD on the GPU (csrc/kernels/multi_tensor.hip: sgd_list_kernel / sgd_body, and the host code of
sgd_step_list in csrc/ops_bindings.cpp) against a float64 oracle of torch.optim.SGD plus ``grad_scale``.

This is the optimizer of bench.py, smoke() and the default CLI: bf16 parameters and gradients, fp32 masters
and momentum, the bf16 parameter rewritten as a shadow of its master in the same pass, by-value tensor lists
of at most 32 tensors per launch, one list per (gradient dtype, first step) partition.

Bound: RTOL / ATOL of tests/test_lars.py (1e-5 / 1e-6) for masters, fp32 parameters and momentum buffers
against the oracle rounded to fp32, after every step; bf16 shadows equal ``master.to(bfloat16)`` bitwise. The
plain-torch form of the formula (FusedSGD._reference_step, what a CPU run of these same functions executes)
meets the bound on these inputs with the worst error under half of it.

Shapes: 1 and 17 elements (scalar tail of one block), 4096 (exactly one chunk), 3 * 4096 + 5 (full chunks
and a tail), 123457 (31 chunks), a channels_last conv weight, a dense view one element past an aligned
address (scalar path at full chunk size), and lists of 33 and 70 tensors against 32 per launch."""
import pytest
import torch

import list_shapes
from test_lars import ATOL, RTOL

pytestmark = pytest.mark.gpu

SIZES = [1, 17, 4096, 4096 * 3 + 5, 123457]
ROWS = [
    dict(momentum=0.5),  # the reference's optimizer
    dict(momentum=0.9, nesterov=True, weight_decay=1e-4),
    dict(momentum=0.9, dampening=0.2, grad_scale=0.5),
    dict(momentum=0.0, weight_decay=0.01),  # the kMomentum = false instantiations
]
DTYPES = [torch.float32, torch.bfloat16]


def sgd_oracle_step(P, M, grads, hp):
    """One torch.optim.SGD step with ``grad_scale`` in float64, in place. ``P``: float64 tensors (parameter
    or master); ``M``: float64 momentum or None where a tensor has had no gradient yet; ``grads``: a tensor
    (any dtype, upcast exactly) or None per parameter; ``hp``: a dict per parameter with lr, momentum,
    dampening, weight_decay, nesterov, grad_scale."""
    for i, (p, g, h) in enumerate(zip(P, grads, hp)):
        if g is None:
            continue
        d = g.detach().double().cpu().reshape(p.shape) * h["grad_scale"]
        if h["weight_decay"] != 0:
            d = d + h["weight_decay"] * p
        if h["momentum"] != 0:
            if M[i] is None:
                M[i] = d.clone()  # the first step: no dampening
            else:
                M[i] = h["momentum"] * M[i] + (1 - h["dampening"]) * d
            d = d + h["momentum"] * M[i] if h["nesterov"] else M[i]
        p.sub_(h["lr"] * d)


def _tensors(dev, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    ts = [torch.randn(n, generator=g).to(dev, dtype) for n in SIZES]
    ts.append(torch.randn(64, 3, 7, 7, generator=g).to(dev, dtype).contiguous(memory_format=torch.channels_last))
    ts.append(torch.randn(4097, generator=g).to(dev, dtype)[1:])  # 4 / 2 bytes past an aligned address, dense
    assert ts[-1].data_ptr() % 16 != 0 and ts[-1].numel() == 4096
    return ts


def _cycle(dev, dtype, count, gen):
    return [torch.randn((5, 4096, 5000)[t % 3], generator=gen).to(dev, dtype) for t in range(count)]


def _like(p, values):
    """values (CPU fp32) as a tensor of p's device, dtype and strides."""
    out = torch.empty_like(p)
    out.copy_(values.to(p.device))
    return out


def _grads(params, gen, mult=lambda t: 1.0):
    return [_like(p, torch.randn(p.shape, generator=gen) * mult(t)) for t, p in enumerate(params)]


def _close(got, ref64):
    torch.testing.assert_close(got.detach().float().cpu(), ref64.float().reshape(got.shape), rtol=RTOL, atol=ATOL)


class Pair:
    """A FusedSGD on the given parameters and the oracle's float64 state of the same parameters."""

    def __init__(self, params, groups=None, master_weights=False, **kw):
        from distributed_learning_amd.ops.optim import FusedSGD

        self.params = [p.requires_grad_() for p in params]
        groups = groups or [(range(len(params)), {})]
        self.opt = FusedSGD([dict(params=[self.params[i] for i in idx], **g) for idx, g in groups],
                            master_weights=master_weights, **kw)
        self.hp = [None] * len(params)
        for (idx, _), g in zip(groups, self.opt.param_groups):
            for i in idx:
                self.hp[i] = {k: g[k] for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov", "grad_scale")}
        self.P = [p.detach().double().cpu().clone() for p in self.params]
        self.M = [None] * len(params)

    def step(self, grads):
        for p, g in zip(self.params, grads):
            p.grad = g
        self.opt.step()
        sgd_oracle_step(self.P, self.M, grads, self.hp)

    def target(self, p):
        return self.opt.state[p]["master"] if "master" in self.opt.state[p] else p

    def check(self):
        for p, ref, mref in zip(self.params, self.P, self.M):
            st = self.opt.state[p]
            _close(self.target(p), ref)
            assert ("momentum_buffer" in st) == (mref is not None)
            if mref is not None:
                assert st["momentum_buffer"].dtype == torch.float32
                _close(st["momentum_buffer"], mref)
            if "master" in st:
                assert p.dtype == torch.bfloat16 and st["master"].dtype == torch.float32
                assert torch.equal(p.detach(), st["master"].to(torch.bfloat16))  # the shadow, bitwise

    def snapshot(self):
        out = []
        for p in self.params:
            st = self.opt.state[p]
            out.append([p.detach().clone()] + [st[k].clone() for k in ("master", "momentum_buffer") if k in st])
        return out


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("row", range(len(ROWS)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_match_oracle(cuda, dtype, row):
    """fp32 parameters with fp32 gradients / bf16 parameters and gradients with fp32 masters."""
    kw = ROWS[row]
    pair = Pair(_tensors(cuda, dtype), lr=0.1, master_weights=dtype != torch.float32, **kw)
    gen = torch.Generator().manual_seed(1 + row)
    for _ in range(3):
        pair.step(_grads(pair.params, gen))
        pair.check()
    for p in pair.params:
        st = pair.opt.state[p]
        assert ("master" in st) == (dtype != torch.float32)
        assert ("momentum_buffer" in st) == (kw["momentum"] != 0)


def test_mixed_model_steps_both_partitions(cuda):
    """bf16 tensors with masters and fp32 1-D tensors (BatchNorm-like) in one optimizer and one step()."""
    gen = torch.Generator().manual_seed(3)
    ps = _tensors(cuda, torch.bfloat16, 4)
    ps += [torch.randn(n, generator=gen).to(cuda) for n in (64, 300, 4096 + 4)]
    ps = ps[:3] + ps[-2:] + ps[3:-2]  # interleaved: the partition, not the order, decides the launch
    pair = Pair(ps, lr=0.1, momentum=0.9, weight_decay=1e-4, master_weights=True)
    for _ in range(3):
        before = [pair.target(p).detach().clone() for p in pair.params]
        pair.step(_grads(pair.params, gen))
        pair.check()
        assert not any(torch.equal(pair.target(p).detach(), b) for p, b in zip(pair.params, before))
    assert {("master" in pair.opt.state[p]) for p in pair.params} == {True, False}


@pytest.mark.parametrize("count", [33, 70, "edges"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_list_boundary(cuda, dtype, count):
    """33 and 70 tensors against 32 per launch; "edges": the list of tests/list_shapes.py."""
    gen = torch.Generator().manual_seed(list_shapes.COUNT if count == "edges" else count)
    ps = list_shapes.edge_list(cuda, dtype, gen) if count == "edges" else _cycle(cuda, dtype, count, gen)
    pair = Pair(ps, lr=0.05, momentum=0.9, weight_decay=1e-4, master_weights=dtype != torch.float32)
    for _ in range(3):
        # scaled by the slot, so every slot matters: randn * (t + 1) / 64. (Unit-variance gradients times t + 1
        # make momentum values of several hundred, whose fp32 rounding alone exceeds ATOL on the elements
        # that cancel to near zero -- the torch form of the formula misses the bound there too.)
        pair.step(_grads(pair.params, gen, mult=lambda t: (t + 1.0) / 64))
        pair.check()


@pytest.mark.parametrize("dtype", DTYPES)
def test_first_step_partition(cuda, dtype):
    """Tensors whose first gradient arrives at step 1 take the first-step form (m = d, no dampening) there,
    in the same step() in which the others take the running form; without a gradient nothing changes."""
    count = 35
    gen = torch.Generator().manual_seed(5)
    pair = Pair(_cycle(cuda, dtype, count, gen), lr=0.05, momentum=0.9, dampening=0.2,
                master_weights=dtype != torch.float32)
    late = {1, count // 2, count - 1}
    start = [p.detach().clone() for p in pair.params]
    for s in range(3):
        grads = _grads(pair.params, gen)
        if s == 0:
            grads = [None if t in late else g for t, g in enumerate(grads)]
        pair.step(grads)
        pair.check()
        if s == 0:
            for t in late:
                assert torch.equal(pair.params[t].detach(), start[t])
                assert len(pair.opt.state[pair.params[t]]) == 0
    # the oracle's two forms differ by the dampening, far outside the bound: the check above can tell them apart
    assert all(pair.M[t] is not None for t in range(count))


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_element_parameter_is_skipped(cuda, dtype):
    gen = torch.Generator().manual_seed(6)
    ps = _cycle(cuda, dtype, 3, gen)
    ps.insert(1, torch.empty(0, device=cuda, dtype=dtype))
    ps.insert(0, torch.empty(0, 4, device=cuda, dtype=dtype))
    pair = Pair(ps, lr=0.1, momentum=0.9, master_weights=dtype != torch.float32)
    for _ in range(2):
        before = [p.detach().clone() for p in pair.params]
        pair.step(_grads(pair.params, gen))
        pair.check()
        assert [torch.equal(p.detach(), b) for p, b in zip(pair.params, before)] == [True, False, True, False, False]


def test_bf16_without_masters_takes_the_torch_formula(cuda):
    """One step: the momentum is fp32 and meets the bound; the parameter is the fp32 result rounded to bf16,
    so it is within one bf16 ulp (2^-7 relative) of the oracle's rounded result -- the bound
    tests/test_gpu_lars.py uses for the same situation. (An in-place ``p.add_(d)`` on the bf16 parameter
    misses it on the GPU: the fp32 update is rounded to bf16 before the add, which loses the weight-decay term
    where p - lr * g cancels; the formula therefore updates an fp32 copy and rounds once.)"""
    gen = torch.Generator().manual_seed(7)
    pair = Pair(_tensors(cuda, torch.bfloat16, 8), lr=0.1, momentum=0.9, weight_decay=1e-4)
    pair.step(_grads(pair.params, gen))
    for p, ref, mref in zip(pair.params, pair.P, pair.M):
        st = pair.opt.state[p]
        assert "master" not in st and p.dtype == torch.bfloat16
        _close(st["momentum_buffer"], mref)
        torch.testing.assert_close(p.detach().float().cpu(), ref.to(torch.bfloat16).float().reshape(p.shape),
                                   rtol=2.0 ** -7, atol=ATOL)


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_param_groups(cuda, dtype):
    ps = _tensors(cuda, dtype, 9)
    pair = Pair(ps, [(range(0, 3), dict(lr=0.2, weight_decay=1e-3)), (range(3, len(ps)), dict(lr=0.05))],
                lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True, master_weights=dtype != torch.float32)
    assert pair.hp[0]["lr"] == 0.2 and pair.hp[0]["weight_decay"] == 1e-3
    assert pair.hp[-1]["lr"] == 0.05 and pair.hp[-1]["weight_decay"] == 1e-4
    gen = torch.Generator().manual_seed(10)
    for _ in range(3):
        pair.step(_grads(pair.params, gen))
        pair.check()


def _faulty_model(cuda, dtype):
    """40 tensors, one good step taken (so masters and momentum buffers exist), and a next set of gradients in
    which number 35's strides differ from its parameter's: contiguous against a channels_last 4-D weight."""
    gen = torch.Generator().manual_seed(11)
    ps = _cycle(cuda, dtype, 40, gen)
    ps[35] = torch.randn(8, 4, 3, 3, generator=gen).to(cuda, dtype).contiguous(memory_format=torch.channels_last)
    pair = Pair(ps, lr=0.1, momentum=0.9, master_weights=dtype != torch.float32)
    pair.step(_grads(pair.params, gen))
    pair.check()
    grads = _grads(pair.params, gen)
    grads[35] = grads[35].contiguous()
    assert grads[35].stride() != pair.params[35].stride() and grads[35].is_cuda
    return pair, grads


@pytest.mark.parametrize("dtype", DTYPES)
def test_bad_tensor_late_in_the_list_updates_nothing(cuda, dtype):
    """A list is checked as a whole before its first launch: a bad 36th tensor must not leave the first 32
    parameters updated."""
    pair, grads = _faulty_model(cuda, dtype)
    before = pair.snapshot()
    for p, g in zip(pair.params, grads):
        p.grad = g
    with pytest.raises(RuntimeError, match="grad 35 must match"):
        pair.opt.step()
    torch.cuda.synchronize(cuda)
    after = pair.snapshot()
    assert all(len(b) == (3 if dtype == torch.bfloat16 else 2) for b in before)
    assert [_same(a, b) for a, b in zip(after, before)] == [True] * 40
    # the binding itself, and the list is usable again once the gradient is fixed
    from distributed_learning_amd.ops import _ext

    fp = [pair.target(p).detach() for p in pair.params]
    bufs = [pair.opt.state[p]["momentum_buffer"] for p in pair.params]
    shadows = [p.detach() for p in pair.params] if dtype == torch.bfloat16 else []
    with pytest.raises(RuntimeError, match="grad 35 must match"):
        _ext.require().sgd_step_list(fp, grads, bufs, shadows, 0.1, 0.9, 0.0, 0.0, False, 1.0, False)
    torch.cuda.synchronize(cuda)
    assert [_same(a, b) for a, b in zip(pair.snapshot(), before)] == [True] * 40
    grads[35] = _like(pair.params[35], grads[35].float().cpu())
    pair.step(grads)
    pair.check()
