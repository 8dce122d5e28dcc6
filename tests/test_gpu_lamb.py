"""FusedLAMB and FusedAdamW on the GPU (csrc/kernels/multi_tensor.hip: lamb_moments_list_kernel,
adam_finalize_kernel, lamb_apply_list_kernel, adamw_list_kernel and their EMA forms; AdamPlan in
csrc/ops_bindings.cpp) against the float64 oracle of tests/lamb_oracle.py.

Bound: rtol 1e-5, atol 1e-6 against the oracle rounded to fp32 -- the bound of tests/test_lamb.py, which shows
there that an fp32 evaluation of the formula meets it and that every injected fault misses it. bf16 shadows equal
master.to(bfloat16) bitwise. Bias corrections: relative error <= 1e-6 against float64.

Shapes: those of tests/test_gpu_lars.py -- 1 and 17 elements (scalar tail of a single block), 4096 (exactly one
full chunk), 3 * 4096 + 5 (full chunks plus a tail), 123457 (31 partials of one tensor), a channels_last conv
weight, a view one element past an aligned address (scalar path at full chunk size), lists of 33 and 70 tensors
against 32 per launch, and the list of tests/list_shapes.py with its dtype change."""
import math

import pytest
import torch

import list_shapes
from ema_oracle import check_step, omd32
from lamb_oracle import hyper, lamb_oracle_step
from test_gpu_lars import _grads, _tensors
from test_lamb import BETAS, KS
from test_lars import ATOL, RTOL

pytestmark = pytest.mark.gpu

NAMES = ["lamb", "adamw"]
KW = dict(lr=2e-2, betas=(0.9, 0.999), eps=1e-6, weight_decay=1e-2)
STATE = ("exp_avg", "exp_avg_sq", "step")


def _cls(name):
    from distributed_learning_amd.ops import optim

    return {"lamb": optim.FusedLAMB, "adamw": optim.FusedAdamW}[name]


def _launches(name, lists, clip):
    """The table of the class docstring: launches of one step over ``lists`` by-value lists."""
    if name == "lamb":
        return 3 * lists + 2 if clip else 2 * lists + 1
    return 2 * lists + 1 if clip else lists + 1


def _close(got, ref64):
    torch.testing.assert_close(got.detach().float().cpu(), ref64.float().reshape(got.shape), rtol=RTOL, atol=ATOL)


class Pair:
    """A FusedLAMB / FusedAdamW on GPU parameters and the oracle's float64 state of the same parameters."""

    def __init__(self, name, params, groups, **kw):
        self.name = name
        self.params = [p.requires_grad_() for p in params]
        self.kw = {**KW, **kw}
        self.opt = _cls(name)([dict(params=[self.params[i] for i in idx], **g) for idx, g in groups], **self.kw)
        self.P = [p.detach().double().cpu().clone() for p in self.params]
        self.M, self.V = [torch.zeros_like(p) for p in self.P], [torch.zeros_like(p) for p in self.P]
        self.K = [0] * len(self.P)

    def step(self, grads):
        for p, g in zip(self.params, grads):
            p.grad = g
        self.opt.step()
        return lamb_oracle_step(self.P, self.M, self.V, self.K, grads, hyper(self.opt), self.name == "lamb",
                                self.kw.get("grad_scale", 1.0), self.kw.get("max_grad_norm", 0.0))

    def target(self, p):
        return self.opt.state[p]["master"] if "master" in self.opt.state[p] else p

    def check(self, only=None):
        for i, p in enumerate(self.params):
            if (only is not None and i not in only) or self.K[i] == 0:
                continue
            st = self.opt.state[p]
            _close(self.target(p), self.P[i])
            _close(st["exp_avg"], self.M[i])
            _close(st["exp_avg_sq"], self.V[i])
            assert st["step"].dtype == torch.int32 and st["step"].device == p.device and int(st["step"]) == self.K[i]
            if "master" in st:
                assert torch.equal(p.detach(), st["master"].to(torch.bfloat16))

    def snapshot(self):
        return [[p.detach().clone()] + [v.clone() for _, v in sorted(self.opt.state[p].items())] for p in self.params]


@pytest.mark.parametrize("max_grad_norm", [0.0, 1.0])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", NAMES)
def test_update_matches_oracle(cuda, name, dtype, max_grad_norm):
    """fp32 gradients on fp32 parameters / bf16 gradients on bf16 parameters with fp32 masters; two groups."""
    ps = _tensors(cuda, dtype) + [torch.randn(300, generator=torch.Generator().manual_seed(9)).to(cuda, dtype)]
    n = len(ps)
    assert ps[-2].data_ptr() % 16 != 0 and ps[-2].numel() == 4096
    pair = Pair(name, ps, [(range(0, 4), {}), (range(4, n), dict(lr=1e-2, weight_decay=3e-2))], grad_scale=0.5,
                max_grad_norm=max_grad_norm, master_weights=dtype != torch.float32)
    gen = torch.Generator().manual_seed(1)
    for _ in range(3):
        G, trusts, _ = pair.step(_grads(pair.params, gen))
        assert trusts[-1] == 1.0 and (trusts[0] != 1.0) == (name == "lamb")
        if max_grad_norm > 0:
            assert G > 10 * max_grad_norm  # the clip binds
            _close(pair.opt.last_grad_norm, torch.tensor([G]))
        else:
            assert pair.opt.last_grad_norm is None
        pair.check()
        assert pair.opt.last_launches == _launches(name, 1, max_grad_norm > 0)
    if name == "lamb":  # the norms the trust ratios were formed from, rows in parameter order (one grad dtype)
        assert all(a is b for a, b in zip(pair.opt.last_params, pair.params))
        norms = pair.opt.last_plan.norms().cpu()
        assert norms.shape == (n, 2) and bool((norms > 0).all())


@pytest.mark.parametrize("count", [33, 70, "edges"])
@pytest.mark.parametrize("name", NAMES)
def test_list_boundary_and_subset(cuda, name, count):
    """33 and 70 fp32 tensors against 32 per launch; "edges": the list of tests/list_shapes.py, fp32 tensors and
    then bf16 ones with masters (the optimizer leaves the zero-element tensor out). Then a step in which only
    three tensors have gradients: the state of the others, counts included, keeps every bit."""
    edges = count == "edges"
    count = list_shapes.COUNT if edges else count
    g = torch.Generator().manual_seed(count)
    if edges:
        ps = list_shapes.edge_list(cuda, list_shapes.mixed_dtypes(), g, two_d=True)
    else:
        ps = [torch.randn(1, (5, 4096, 5000)[t % 3], generator=g).to(cuda) for t in range(count)]
    half = count // 2
    only = set(range(count)) - {list_shapes.EMPTY} if edges else None
    pair = Pair(name, ps, [(range(0, half), {}), (range(half, count), dict(lr=1e-2, weight_decay=3e-2))],
                grad_scale=0.5, master_weights=edges)
    lists = 2 if edges else math.ceil(count / 32)  # "edges": 20 fp32 tensors, then 19 bf16 ones
    _, trusts, _ = pair.step(_grads(pair.params, g, mult=lambda t: t + 1.0))
    if name == "lamb":
        assert len({round(math.log(t), 3) for t in trusts if t is not None}) > count // 2  # every slot matters
    pair.check(only)
    assert pair.opt.last_launches == _launches(name, lists, False)
    subset = {1, half, count - 1}
    grads = [g_ if t in subset else None for t, g_ in enumerate(_grads(pair.params, g, mult=lambda t: 3.0 * (t + 1)))]
    before = pair.snapshot()
    pair.step(grads)
    pair.check(only)
    for t, (b, a) in enumerate(zip(before, pair.snapshot())):
        same = len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
        assert same == (t not in subset), t
    assert pair.opt.last_launches == _launches(name, 2 if edges else 1, False)  # "edges": the subset has both dtypes
    pair.step(_grads(pair.params, g, mult=lambda t: t + 1.0))  # and back to the whole list
    pair.check(only)
    assert pair.K[1] == 3 and pair.K[2] == 2


def test_plan_cache_is_bounded(cuda):
    """Every distinct set of tensors with gradients gets a plan (table + workspaces); only a few are kept."""
    g = torch.Generator().manual_seed(3)
    ps = [torch.randn(1, 5000, generator=g).to(cuda) for _ in range(8)]
    pair = Pair("lamb", ps, [(range(8), {})])
    pair.step(_grads(pair.params, g))
    for drop in list(range(8)) + [0, 1]:  # evicted sets come back and are rebuilt
        grads = [None if t == drop else x for t, x in enumerate(_grads(pair.params, g, mult=lambda t: t + 1.0))]
        pair.step(grads)
        pair.check()
        assert len(pair.opt._tables) <= pair.opt._MAX_PLANS
    assert len(pair.opt._tables) == pair.opt._MAX_PLANS


@pytest.mark.parametrize("name", NAMES)
def test_clipping(cuda, name):
    def make(max_grad_norm):
        qs = [t.clone() for t in _tensors(cuda, torch.float32, 7)[:4]] + [torch.ones(50, device=cuda)]
        return Pair(name, qs, [(range(len(qs)), {})], grad_scale=0.5, max_grad_norm=max_grad_norm)

    pairs = {m: make(m) for m in (1.0, 0.0, 1e9)}
    for m, pair in pairs.items():
        gen = torch.Generator().manual_seed(8)
        for _ in range(2):
            grads = _grads(pair.params, gen, mult=lambda t: 0.8)  # 16,457 elements: G = 0.5 * 0.8 * 128 = 51
            G, _, _ = pair.step(grads)
            assert 40 < G < 60
            if m > 0:
                _close(pair.opt.last_grad_norm, torch.tensor([G]))
            pair.check()
    moved = []
    for a, b, c in zip(pairs[0.0].snapshot(), pairs[1e9].snapshot(), pairs[1.0].snapshot()):
        assert all(torch.equal(x, y) for x, y in zip(a, b))  # a clip that never binds changes no bit
        assert not torch.equal(a[1], c[1]) and not torch.equal(a[2], c[2])  # a binding one scales what enters m and v
        moved.append(not torch.equal(a[0], c[0]))
    # ... and moves the parameters, except where the step is invariant under a scaling of the gradient up to eps
    # (LAMB's one-element tensor steps by lr * |p| whatever the size of u)
    assert all(moved[1:]) and (moved[0] or name == "lamb")


@pytest.mark.parametrize("name", NAMES)
def test_deterministic(cuda, name):
    outs = []
    for _ in range(2):
        gen = torch.Generator().manual_seed(11)
        pair = Pair(name, _tensors(cuda, torch.bfloat16, 10), [(range(7), {})], max_grad_norm=1.0, master_weights=True)
        for _ in range(3):
            pair.step(_grads(pair.params, gen))
        outs.append([pair.opt.state[p][k].clone() for p in pair.params for k in ("master",) + STATE])
    assert all(torch.equal(a, b) for a, b in zip(*outs))


@pytest.mark.parametrize("name", NAMES)
def test_masters_and_fallback_without_masters(cuda, name):
    gen = torch.Generator().manual_seed(12)
    ps = _tensors(cuda, torch.bfloat16, 13) + [torch.randn(300, generator=gen).to(cuda)]  # + an fp32 tensor
    pair = Pair(name, ps, [(range(len(ps)), {})], master_weights=True)
    for _ in range(2):
        pair.step(_grads(pair.params, gen))
        pair.check()  # master vs the oracle, and the shadow bitwise master.bfloat16()
    assert "master" in pair.opt.state[pair.params[0]] and "master" not in pair.opt.state[pair.params[-1]]
    assert pair.opt.last_launches == _launches(name, 2, False)  # fp32 and bf16 gradients: two launches per pass
    # bf16 parameters without masters: the torch formula. One step: the moments are fp32 and meet the bound; the
    # parameter is the fp32 result rounded to bf16, within one bf16 ulp (2^-7 relative) of the oracle's rounded one
    pair = Pair(name, _tensors(cuda, torch.bfloat16, 13), [(range(7), {})])
    pair.step(_grads(pair.params, gen))
    assert pair.opt.last_launches == 0 and pair.opt.last_plan is None
    for p, ref, mref, vref in zip(pair.params, pair.P, pair.M, pair.V):
        _close(pair.opt.state[p]["exp_avg"], mref)
        _close(pair.opt.state[p]["exp_avg_sq"], vref)
        assert int(pair.opt.state[p]["step"]) == 1
        torch.testing.assert_close(p.detach().float().cpu(), ref.to(torch.bfloat16).float().reshape(p.shape),
                                   rtol=2.0 ** -7, atol=ATOL)


@pytest.mark.parametrize("decay", [1 - 2.0 ** -3, 0.999])
@pytest.mark.parametrize("name", NAMES)
def test_ema_rides_in_the_update_launches(cuda, name, decay):
    """The average is fmaf(omd, p_new - e, e) of the fp32 value just stored (bit for bit against the fp32 replay
    where omd is a power of two, within the rounding bound of tests/ema_oracle.py otherwise), the update keeps
    every bit, and no launch is added."""
    def make(**kw):
        ps = [p.requires_grad_() for p in _tensors(cuda, torch.bfloat16, 30) + _tensors(cuda, torch.float32, 31)[:3]]
        return ps, _cls(name)(ps, max_grad_norm=1.0, master_weights=True, **KW, **kw)

    def snap(opt, ps):
        out = []
        for p in ps:
            st = opt.state[p]
            out.append(((st["master"] if "master" in st else p.detach()).float().clone(),
                        st["ema"].clone() if "ema" in st else None))
        return out

    (pa, on), (pb, off) = make(ema_decay=decay), make()
    gen = torch.Generator().manual_seed(32)
    for s in range(3):
        grads = _grads(pa, gen)
        if s == 1:
            grads[2] = None
        for p, q, g in zip(pa, pb, grads):
            p.grad, q.grad = g, (None if g is None else g.clone())
        before = snap(on, pa)
        on.step()
        off.step()
        assert check_step(before, snap(on, pa), [g is not None for g in grads], omd32(decay), decay != 0.999) == set()
        for p, q in zip(pa, pb):
            assert torch.equal(p.detach(), q.detach())
            assert set(on.state[p]) - {"ema"} == set(off.state[q])
            assert all(torch.equal(on.state[p][k], off.state[q][k]) for k in off.state[q])
        assert on.last_launches == off.last_launches == _launches(name, 2, True)


@pytest.mark.parametrize("name", NAMES)
def test_bias_corrections_from_the_device(cuda, name):
    """The counters set to k - 1, one zero-gradient step: the (bc1, bc2) the finalize stored are within 1e-6
    (relative) of float64, over the grid of tests/test_lamb.py plus k = 2^24 - 1, and the counters read k."""
    ks = list(KS) + [2 ** 24 - 1]
    cases = [(b1, b2, k) for b1, b2 in ((BETAS[0], BETAS[1]), (BETAS[1], BETAS[2])) for k in ks]
    ps = [torch.randn(1, 8, generator=torch.Generator().manual_seed(t)).to(cuda).requires_grad_() for t in range(len(cases))]
    opt = _cls(name)([dict(params=[p], betas=(b1, b2)) for p, (b1, b2, _) in zip(ps, cases)], lr=1e-3)
    for p in ps:
        p.grad = torch.zeros_like(p)
    opt.step()  # creates the state (k = 1)
    for p, (_, _, k) in zip(ps, cases):
        opt.state[p]["step"].fill_(k - 1)
    opt.step()
    assert all(a is b for a, b in zip(opt.last_params, ps)) and opt.last_launches == _launches(name, 1, False)
    bc = opt.last_plan.bias_corrections().double().cpu()
    for t, (b1, b2, k) in enumerate(cases):
        assert int(opt.state[ps[t]]["step"]) == k
        for got, beta in zip(bc[t], (b1, b2)):
            exact = -math.expm1(k * math.log(beta))
            assert abs(float(got) - exact) <= 1e-6 * exact, (beta, k, float(got), exact)


@pytest.mark.parametrize("name", NAMES)
def test_graph_capture_advances_its_own_counts(cuda, name):
    """A captured step replays with new gradients and new learning rates, advances its own bias corrections, and
    equals eager bit for bit. One linear stream: no parallel branches in the capture."""
    from distributed_learning_amd.ops.optim import poly_warmup_lr

    def make():
        ps = [t.requires_grad_() for t in _tensors(cuda, torch.bfloat16, 20)[:4] + _tensors(cuda, torch.float32, 21)[2:5]]
        opt = _cls(name)([dict(params=ps[:3]), dict(params=ps[3:], weight_decay=3e-2)], max_grad_norm=1.0,
                         master_weights=True, **KW)
        for p in ps:
            p.grad = torch.zeros_like(p)  # static gradient buffers
        return ps, opt

    gen = torch.Generator().manual_seed(22)
    (pe, oe), (pg, og) = make(), make()
    feeds = [[torch.randn(p.shape, generator=gen) for p in pe] for _ in range(5)]

    def feed(ps, opt, s):
        for p, v in zip(ps, feeds[s]):
            p.grad.copy_(v.to(cuda))
        opt.set_lr(poly_warmup_lr(s + 1, 2e-2, 3, 10), group=0)
        opt.set_lr(2 * poly_warmup_lr(s + 1, 2e-2, 3, 10), group=1)

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
        for k in ("master",) + STATE:
            if k in oe.state[a]:
                assert torch.equal(oe.state[a][k], og.state[b][k]), k
        assert int(og.state[b]["step"]) == 5
    assert torch.equal(oe.last_grad_norm, og.last_grad_norm)
    # and the replays did train (the fp32 master: a bf16 shadow may round a small update away)
    assert not torch.equal(og.state[pg[2]]["master"], _tensors(cuda, torch.bfloat16, 20)[2].float())


@pytest.mark.parametrize("bad", ["moment_dtype", "numel", "step_dtype", "cpu"])
@pytest.mark.parametrize("name", NAMES)
def test_host_checks_leave_everything_untouched(cuda, name, bad):
    """A bad tensor in the second by-value list: the call raises before its first launch."""
    from distributed_learning_amd.ops import _ext

    C = _ext.require()
    n, slot = 34, 33
    g = torch.Generator().manual_seed(40)
    ps = [torch.randn(1, 5000, generator=g).to(cuda) for _ in range(n)]
    grads = [torch.randn(1, 5000, generator=g).to(cuda) for _ in range(n)]
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    steps = [torch.zeros(1, dtype=torch.int32, device=cuda) for _ in range(n)]
    lr = torch.full((1,), 1e-2, device=cuda)

    def plan(st):
        return C.AdamPlan(name == "lamb", [p.numel() for p in ps], [0] * n, [True] * n, [1e-2] * n, [0.9] * n,
                          [0.999] * n, [1e-6] * n, st, lr, ps[0])

    run = C.lamb_step_list if name == "lamb" else C.adamw_step_list
    pl = plan(steps)
    run(pl, ps, grads, ms, vs, [], steps, 0.5, 1.0)  # the good call works
    orig = ps + ms + vs + steps
    keep = [t.clone() for t in orig]
    if bad == "moment_dtype":
        vs[slot] = vs[slot].double()
    elif bad == "numel":
        ps[slot], grads[slot] = ps[slot][:, :4999].contiguous(), grads[slot][:, :4999].contiguous()
        ms[slot], vs[slot] = ms[slot][:, :4999].contiguous(), vs[slot][:, :4999].contiguous()
    elif bad == "cpu":
        ms[slot] = ms[slot].cpu()
    if bad == "step_dtype":
        steps[slot] = steps[slot].long()
        with pytest.raises(RuntimeError, match="int32"):
            plan(steps)  # a plan cannot be built on it
    with pytest.raises(RuntimeError):
        run(pl, ps, grads, ms, vs, [], steps, 0.5, 1.0)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(keep, orig))


@pytest.mark.parametrize("name", NAMES)
def test_resnet18_cifar_step_matches_fallback(cuda, name):
    """One model-level step on the bf16 native path: the kernels against the torch formula (run on CPU copies
    of the same parameters and gradients)."""
    from distributed_learning_amd.models import create_network
    from distributed_learning_amd.ops import nn as dnn
    from distributed_learning_amd.ops.loss import cross_entropy

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
    kw = dict(lr=2e-3, weight_decay=1e-2, max_grad_norm=1.0, master_weights=True)
    nat, ref = _cls(name)(ps, **kw), _cls(name)(cpu, **kw)
    nat.step()
    ref.step()
    assert nat.last_launches > 0 and ref.last_launches == 0
    torch.testing.assert_close(nat.last_grad_norm.cpu(), ref.last_grad_norm, rtol=RTOL, atol=ATOL)
    for p, c in zip(ps, cpu):
        a, b = nat.state[p], ref.state[c]
        for k in ("exp_avg", "exp_avg_sq"):
            torch.testing.assert_close(a[k].cpu(), b[k], rtol=RTOL, atol=ATOL)
        assert int(a["step"]) == int(b["step"]) == 1
        if p.dtype == torch.bfloat16:
            torch.testing.assert_close(a["master"].cpu(), b["master"], rtol=RTOL, atol=ATOL)
            assert torch.equal(p.detach(), a["master"].to(torch.bfloat16))
        else:
            torch.testing.assert_close(p.detach().cpu(), c.detach(), rtol=RTOL, atol=ATOL)
