"""FusedLARS and multi_tensor_l2norm on the GPU (csrc/kernels/multi_tensor.hip: square sums, finalize,
update) against the float64 oracle of tests/test_lars.py.

Bound: rtol 1e-5, atol 1e-6 against the oracle rounded to fp32 -- the FusedSGD bound of
tests/test_gpu_kernels.py; a chunked tree sum of depth well under 100 additions stays below
100 * 2^-24 = 6e-6 relative. bf16 shadows equal master.to(bfloat16) bitwise.

Shapes: the smallest at which each path can go wrong -- 1 and 17 elements (scalar tail of a single block),
4096 (exactly one full chunk), 3 * 4096 + 5 (full chunks plus a tail), 123457 (31 partials of one tensor),
a channels_last conv weight, a view that starts 4 / 2 bytes past an aligned address (scalar path at full
chunk size), and lists longer than one by-value launch (33 and 70 tensors against 32 per launch)."""
import math

import pytest
import torch

import list_shapes
from test_lars import ATOL, RTOL, hyper, lars_oracle_step

pytestmark = pytest.mark.gpu

SIZES = [1, 17, 4096, 4096 * 3 + 5, 123457]


def _tensors(dev, dtype, seed=0, scale=1.0):
    """The norm / update shape list: 2-D so that LARS adapts them, plus the layouts named above."""
    g = torch.Generator().manual_seed(seed)
    ts = [(torch.randn(1, n, generator=g) * scale).to(dev, dtype) for n in SIZES]
    ts.append((torch.randn(64, 3, 7, 7, generator=g) * scale).to(dev, dtype).contiguous(memory_format=torch.channels_last))
    ts.append((torch.randn(1, 4097, generator=g) * scale).to(dev, dtype)[:, 1:])  # misaligned, dense
    return ts


def _close(got, ref64):
    torch.testing.assert_close(got.detach().float().cpu(), ref64.float().reshape(got.shape), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_l2norm_matches_float64(cuda, dtype):
    from distributed_learning_amd import ops

    ts = _tensors(cuda, dtype) + [torch.zeros(5000, device=cuda, dtype=dtype)]
    assert ts[-2].data_ptr() % 16 != 0 and ts[-2].numel() == 4096
    for scale in (1.0, 0.25):
        per, total = ops.multi_tensor_l2norm(ts, scale)
        assert per.dtype == torch.float32 and per.shape == (len(ts),) and total.shape == (1,)
        ref = torch.stack([t.double().cpu().norm() for t in ts])
        _close(per, ref * scale)
        _close(total, (ref.norm() * scale).reshape(1))
        assert float(per[-1]) == 0.0
    # mixed dtypes in one list, and bitwise reproducible
    mixed = _tensors(cuda, torch.float32, 1) + _tensors(cuda, torch.bfloat16, 2)
    a = ops.multi_tensor_l2norm(mixed)
    b = ops.multi_tensor_l2norm(mixed)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _close(a[0], torch.stack([t.double().cpu().norm() for t in mixed]))
    # the list of tests/list_shapes.py: three launches, the zero-element tensor keeps its slot (and its row)
    edges = list_shapes.edge_list(cuda, list_shapes.mixed_dtypes(), torch.Generator().manual_seed(3), two_d=True)
    per, total = ops.multi_tensor_l2norm(edges)
    ref = torch.stack([t.double().cpu().norm() for t in edges])
    _close(per, ref)
    _close(total, ref.norm().reshape(1))
    assert float(per[list_shapes.EMPTY]) == 0.0


class Pair:
    """A FusedLARS on GPU parameters and the oracle's float64 state of the same parameters."""

    def __init__(self, params, groups, **kw):
        from distributed_learning_amd.ops.optim import FusedLARS

        self.params = [p.requires_grad_() for p in params]
        self.opt = FusedLARS([dict(params=[self.params[i] for i in idx], **g) for idx, g in groups], **kw)
        self.P = [p.detach().double().cpu().clone() for p in self.params]
        self.M = [torch.zeros_like(p) for p in self.P]
        self.kw = kw

    def step(self, grads):
        for p, g in zip(self.params, grads):
            p.grad = g
        self.opt.step()
        return lars_oracle_step(self.P, self.M, grads, hyper(self.opt), self.kw.get("grad_scale", 1.0),
                                self.kw.get("max_grad_norm", 0.0))

    def target(self, p):
        return self.opt.state[p]["master"] if "master" in self.opt.state[p] else p

    def check(self, only=None):
        for i, (p, ref, mref) in enumerate(zip(self.params, self.P, self.M)):
            if only is not None and i not in only:
                continue
            _close(self.target(p), ref)
            _close(self.opt.state[p]["momentum_buffer"], mref)
            if "master" in self.opt.state[p]:
                assert torch.equal(p.detach(), self.opt.state[p]["master"].to(torch.bfloat16))


def _like(p, values):
    """values (CPU fp32) as a tensor of p's device, dtype and strides."""
    out = torch.empty_like(p)
    out.copy_(values.to(p.device))
    return out


def _grads(params, gen, mult=lambda t: 1.0):
    """One gradient per parameter: mult(t) * randn, in the parameter's dtype and layout."""
    return [_like(p, torch.randn(p.shape, generator=gen) * mult(t)) for t, p in enumerate(params)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_update_matches_oracle(cuda, dtype):
    """fp32 gradients on fp32 parameters / bf16 gradients on bf16 parameters with fp32 masters; two groups."""
    ps = _tensors(cuda, dtype) + [torch.randn(300, generator=torch.Generator().manual_seed(9)).to(cuda, dtype)]
    n = len(ps)
    pair = Pair(ps, [(range(0, 4), dict(lr=0.4, weight_decay=1e-4)), (range(4, n), dict(lr=0.1, weight_decay=1e-3))],
                lr=0.1, momentum=0.9, grad_scale=0.5, master_weights=dtype != torch.float32)
    gen = torch.Generator().manual_seed(1)
    for _ in range(3):
        G, _, trusts = pair.step(_grads(pair.params, gen))
        assert trusts[-1] == 1.0 and trusts[0] != 1.0
        _close(pair.opt.last_grad_norm, torch.tensor([G]))
        pair.check()
    assert pair.opt.last_launches == 3  # one square-sum launch, the finalize, one update launch


@pytest.mark.parametrize("count", [33, 70, "edges"])
def test_list_boundary_and_subset(cuda, count):
    """33 and 70 fp32 tensors against 32 per launch; "edges": the list of tests/list_shapes.py, fp32 tensors and
    then bf16 ones with masters (FusedLARS itself leaves the zero-element tensor out, and it has no trust)."""
    edges = count == "edges"
    count = list_shapes.COUNT if edges else count
    g = torch.Generator().manual_seed(count)
    if edges:
        ps = list_shapes.edge_list(cuda, list_shapes.mixed_dtypes(), g, two_d=True)
    else:
        ps = [torch.randn(1, (5, 4096, 5000)[t % 3], generator=g).to(cuda) for t in range(count)]
    half = count // 2
    only = set(range(count)) - {list_shapes.EMPTY} if edges else None  # FusedLARS keeps no state for it
    pair = Pair(ps, [(range(0, half), dict(lr=0.4, weight_decay=1e-4)), (range(half, count), dict(lr=0.1, weight_decay=1e-3))],
                lr=0.1, momentum=0.9, eta=0.02, grad_scale=0.5, master_weights=edges)
    _, gnorms, trusts = pair.step(_grads(pair.params, g, mult=lambda t: t + 1.0))
    assert len({round(math.log(t), 3) for t in trusts}) > count // 2  # every slot matters
    pair.check(only)
    # square-sum and update launches: one per 32 tensors; "edges": 20 fp32 tensors, then 19 bf16 ones
    assert pair.opt.last_launches == 2 * (2 if edges else math.ceil(count / 32)) + 1
    # the same optimizer, three tensors with gradients and the rest without: nothing stale may be read
    subset = {1, half, count - 1}
    grads = [g_ if t in subset else None for t, g_ in enumerate(_grads(pair.params, g, mult=lambda t: 3.0 * (t + 1)))]
    before = [p.detach().clone() for p in pair.params]
    G, _, _ = pair.step(grads)
    _close(pair.opt.last_grad_norm, torch.tensor([G]))
    pair.check(only)
    for t, (p, b) in enumerate(zip(pair.params, before)):
        assert torch.equal(p.detach(), b) == (t not in subset)
    assert pair.opt.last_launches == (5 if edges else 3)  # "edges": the subset has both dtypes
    pair.step(_grads(pair.params, g, mult=lambda t: t + 1.0))  # and back to the whole list
    pair.check(only)
    if edges:
        _direct_update_keeps_the_empty_slot(cuda, g)


def _direct_update_keeps_the_empty_slot(cuda, g):
    """lars_step_list called as FusedLARS calls it, but with the zero-element tensor left in: its slot takes a table
    row and no block in the square-sum and in the update launches, and every other tensor steps as the oracle does."""
    from distributed_learning_amd.ops import _ext

    C = _ext.require()
    n = list_shapes.COUNT
    ps = list_shapes.edge_list(cuda, torch.float32, g, two_d=True)  # fp32 masters; gradients fp32, then bf16
    grads = [_like(p, torch.randn(p.shape, generator=g) * (t + 1.0)).to(dt)
             for t, (p, dt) in enumerate(zip(ps, list_shapes.mixed_dtypes()))]
    moms = [torch.zeros_like(p) for p in ps]
    hp = [dict(lr=0.2, momentum=0.9, weight_decay=1e-4, eta=0.02, eps=0.0, adapt=True)] * n
    plan = C.LarsPlan([p.numel() for p in ps], [0] * n, [True] * n, [1e-4] * n, [0.02] * n, [0.0] * n, [0.9] * n,
                      torch.full((1,), 0.2, device=cuda), ps[0])
    P, M = [p.double().cpu().clone() for p in ps], [torch.zeros_like(p).double().cpu() for p in ps]
    for _ in range(2):
        C.lars_step_list(plan, ps, grads, moms, [], 0.5, 1.0)
        G, _, _ = lars_oracle_step(P, M, grads, hp, 0.5, 1.0)
        _close(plan.grad_norm(), torch.tensor([G]))
        for p, m, ref, mref in zip(ps, moms, P, M):
            _close(p, ref)
            _close(m, mref)
    assert plan.last_launches() == 2 * 2 + 1 and ps[list_shapes.EMPTY].numel() == 0


def test_plan_cache_is_bounded(cuda):
    """Every distinct set of tensors with gradients gets a plan (table + workspace); only a few are kept."""
    g = torch.Generator().manual_seed(3)
    ps = [torch.randn(1, 5000, generator=g).to(cuda) for _ in range(8)]
    pair = Pair(ps, [(range(8), {})], lr=0.3, momentum=0.9, weight_decay=1e-4)
    pair.step(_grads(pair.params, g))  # every tensor once, so each has its momentum buffer
    for drop in list(range(8)) + [0, 1]:  # evicted sets come back and are rebuilt
        grads = [None if t == drop else x for t, x in enumerate(_grads(pair.params, g, mult=lambda t: t + 1.0))]
        pair.step(grads)
        pair.check()
        assert len(pair.opt._tables) <= pair.opt._MAX_PLANS
    assert len(pair.opt._tables) == pair.opt._MAX_PLANS


def test_degenerate_norms_and_scale_invariance(cuda):
    g = torch.Generator().manual_seed(4)
    ps = [torch.randn(1, 5000, generator=g).to(cuda), torch.zeros(1, 5000, device=cuda), torch.randn(3, 7, generator=g).to(cuda)]
    pair = Pair(ps, [(range(3), {})], lr=0.3, momentum=0.9, weight_decay=1e-4)
    grads = _grads(pair.params, g)
    grads[0].zero_()  # zero gradient on tensor 0, zero weight on tensor 1
    _, _, trusts = pair.step(grads)
    assert trusts[0] == 1.0 and trusts[1] == 1.0 and trusts[2] != 1.0
    pair.check()
    assert all(torch.isfinite(p).all() for p in pair.params)
    # eps = 0, wd = 0: scaling every gradient by 2^10 leaves the step unchanged
    outs = []
    for mult in (1.0, 1024.0):
        gen = torch.Generator().manual_seed(5)
        qs = [t.clone() for t in _tensors(cuda, torch.float32, 6)]
        pr = Pair(qs, [(range(len(qs)), {})], lr=0.3, momentum=0.9)
        for _ in range(2):
            pr.step([x * mult for x in _grads(pr.params, gen)])
        outs.append([p.detach().clone() for p in pr.params])
    for a, b in zip(*outs):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=0)


def test_clipping(cuda):
    def make(max_grad_norm):
        qs = [t.clone() for t in _tensors(cuda, torch.float32, 7)[:4]] + [torch.ones(50, device=cuda)]
        return Pair(qs, [(range(len(qs)), {})], lr=0.3, momentum=0.9, weight_decay=1e-4, grad_scale=0.5,
                    max_grad_norm=max_grad_norm)

    pairs = {m: make(m) for m in (1.0, 0.0, 1e9)}
    for m, pair in pairs.items():
        gen = torch.Generator().manual_seed(8)
        for _ in range(2):
            grads = _grads(pair.params, gen, mult=lambda t: 0.8)  # 16,457 elements: G = 0.5 * 0.8 * 128 = 51
            G, _, _ = pair.step(grads)
            assert 40 < G < 60
            _close(pair.opt.last_grad_norm, torch.tensor([G]))
            pair.check()
    for a, b, c in zip(pairs[0.0].params, pairs[1e9].params, pairs[1.0].params):
        assert torch.equal(a.detach(), b.detach())  # a clip that never binds changes no bit
        assert not torch.equal(a.detach(), c.detach())


def test_deterministic(cuda):
    outs = []
    for _ in range(2):
        gen = torch.Generator().manual_seed(11)
        pair = Pair(_tensors(cuda, torch.bfloat16, 10), [(range(7), {})], lr=0.3, momentum=0.9, weight_decay=1e-4,
                    max_grad_norm=1.0, master_weights=True)
        for _ in range(3):
            pair.step(_grads(pair.params, gen))
        outs.append([pair.opt.state[p][k].clone() for p in pair.params for k in ("master", "momentum_buffer")])
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def test_masters_and_fallback_without_masters(cuda):
    gen = torch.Generator().manual_seed(12)
    ps = _tensors(cuda, torch.bfloat16, 13) + [torch.randn(300, generator=gen).to(cuda)]  # + an fp32 tensor
    pair = Pair(ps, [(range(len(ps)), {})], lr=0.3, momentum=0.9, weight_decay=1e-4, master_weights=True)
    for _ in range(2):
        pair.step(_grads(pair.params, gen))
        pair.check()  # master vs the oracle, and the shadow bitwise master.bfloat16()
    assert "master" in pair.opt.state[pair.params[0]] and "master" not in pair.opt.state[pair.params[-1]]
    assert pair.opt.last_launches == 5  # fp32 and bf16 gradients: two launches per pass
    # bf16 parameters without masters: the torch formula. One step: the momentum is fp32 and meets the bound;
    # the parameter is the fp32 result rounded to bf16, so it is within one bf16 ulp (2^-7 relative) of the
    # oracle's rounded result
    pair = Pair(_tensors(cuda, torch.bfloat16, 13), [(range(7), {})], lr=0.3, momentum=0.9, weight_decay=1e-4)
    pair.step(_grads(pair.params, gen))
    assert pair.opt.last_launches == 0
    for p, ref, mref in zip(pair.params, pair.P, pair.M):
        _close(pair.opt.state[p]["momentum_buffer"], mref)
        torch.testing.assert_close(p.detach().float().cpu(), ref.to(torch.bfloat16).float().reshape(p.shape),
                                   rtol=2.0 ** -7, atol=ATOL)


def test_graph_capture_follows_schedule(cuda):
    """A captured step replays with new gradients and new learning rates and equals eager bit for bit."""
    from distributed_learning_amd.ops.optim import FusedLARS, poly_warmup_lr

    def make():
        ps = [t.requires_grad_() for t in _tensors(cuda, torch.bfloat16, 20)[:4] + _tensors(cuda, torch.float32, 21)[2:5]]
        opt = FusedLARS([dict(params=ps[:3], lr=0.5), dict(params=ps[3:], lr=0.5, weight_decay=1e-3)], lr=0.5,
                        momentum=0.9, weight_decay=1e-4, max_grad_norm=1.0, master_weights=True)
        for p in ps:
            p.grad = torch.zeros_like(p)  # static gradient buffers
        return ps, opt

    gen = torch.Generator().manual_seed(22)
    (pe, oe), (pg, og) = make(), make()
    feeds = [[torch.randn(p.shape, generator=gen) for p in pe] for _ in range(5)]

    def feed(ps, opt, s):
        for p, v in zip(ps, feeds[s]):
            p.grad.copy_(v.to(cuda))
        opt.set_lr(poly_warmup_lr(s + 1, 0.5, 3, 10), group=0)
        opt.set_lr(2 * poly_warmup_lr(s + 1, 0.5, 3, 10), group=1)

    for s in range(5):
        feed(pe, oe, s)
        oe.step()
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        for s in range(2):
            feed(pg, og, s)
            og.step()
    torch.cuda.current_stream(cuda).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # a host synchronisation inside the step would fail the capture
        og.step()
    for s in range(2, 5):
        feed(pg, og, s)
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(pe, pg):
        assert torch.equal(a.detach(), b.detach())
        for k in ("master", "momentum_buffer"):
            if k in oe.state[a]:
                assert torch.equal(oe.state[a][k], og.state[b][k])
    assert torch.equal(oe.last_grad_norm, og.last_grad_norm)
    # and the replays did train (the fp32 master: a bf16 shadow may round a small update away)
    assert not torch.equal(og.state[pg[2]]["master"], _tensors(cuda, torch.bfloat16, 20)[2].float())


def test_resnet18_cifar_step_matches_fallback(cuda):
    """One model-level step on the bf16 native path: the kernels against the torch formula (run on CPU copies
    of the same parameters and gradients)."""
    from distributed_learning_amd.models import create_network
    from distributed_learning_amd.ops import nn as dnn
    from distributed_learning_amd.ops.loss import cross_entropy
    from distributed_learning_amd.ops.optim import FusedLARS

    torch.manual_seed(0)
    model = create_network("resnet18_cifar").to(cuda).to(memory_format=torch.channels_last)
    dnn.bf16_weights(model)
    dnn.set_backend("native")
    dnn.set_native_conv(True)
    try:
        g = torch.Generator().manual_seed(1)
        x = torch.rand(8, 3, 32, 32, generator=g).to(cuda, torch.bfloat16).contiguous(memory_format=torch.channels_last)
        y = torch.randint(0, 10, (8,), generator=g).to(cuda)
        cross_entropy(model(x), y).backward()
    finally:
        dnn.set_native_conv(False)
        dnn.set_backend("torch")
    ps = [p for p in model.parameters() if p.grad is not None]
    assert len(ps) > 60 and {p.grad.dtype for p in ps} == {torch.float32, torch.bfloat16}
    cpu = [p.detach().cpu().clone().requires_grad_() for p in ps]
    for c, p in zip(cpu, ps):
        c.grad = p.grad.detach().cpu().clone()
    kw = dict(lr=0.5, momentum=0.9, weight_decay=1e-4, max_grad_norm=1.0, master_weights=True)
    nat, ref = FusedLARS(ps, **kw), FusedLARS(cpu, **kw)
    nat.step()
    ref.step()
    assert nat.last_launches > 0 and ref.last_launches == 0
    torch.testing.assert_close(nat.last_grad_norm.cpu(), ref.last_grad_norm, rtol=RTOL, atol=ATOL)
    for p, c in zip(ps, cpu):
        a, b = nat.state[p], ref.state[c]
        torch.testing.assert_close(a["momentum_buffer"].cpu(), b["momentum_buffer"], rtol=RTOL, atol=ATOL)
        if p.dtype == torch.bfloat16:
            torch.testing.assert_close(a["master"].cpu(), b["master"], rtol=RTOL, atol=ATOL)
            assert torch.equal(p.detach(), a["master"].to(torch.bfloat16))
        else:
            torch.testing.assert_close(p.detach().cpu(), c.detach(), rtol=RTOL, atol=ATOL)
