"""The weight EMA on the GPU (csrc/kernels/multi_tensor.hip: the kEma forms of the SGD and LARS list update
kernels, ema_update_list_kernel, ema_swap_list_kernel; their host code in csrc/ops_bindings.cpp) against the
criteria of tests/ema_oracle.py:

* the update itself is untouched, bit for bit, by the EMA riding in its launch;
* e equals the fp32 replay of ``e_old + omd * (p_new - e_old)`` bit for bit where omd is a power of two, and is
  within ``2^-23 * (|ref64| + omd * |p_new - e_old|)`` of the float64 replay for any decay -- both taken from
  the kernel's own p_new and e_old;
* after 4 steps e is within RTOL / ATOL of tests/test_lars.py of an independent float64 oracle (the SGD / LARS
  oracles of tests/test_gpu_sgd.py and tests/test_lars.py, extended by the EMA formula).

Shapes: those of tests/test_gpu_sgd.py (scalar tail, one chunk, chunks plus a tail, 31 chunks, channels_last, a
dense view one element past an aligned address) and lists of 33 and 70 tensors against 32 per launch."""
import os
import subprocess
import sys

import pytest
import torch

import dist_util
import list_shapes
from ema_oracle import EXACT_DECAYS, GENERAL_DECAYS, bound_violations, check_step, ema_oracle_step, omd32, replay32
from test_gpu_lars import _tensors as lars_tensors
from test_gpu_sgd import ROWS, _cycle, _grads, _like, _tensors, sgd_oracle_step
from test_lars import ATOL, RTOL, hyper, lars_oracle_step

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECAYS = EXACT_DECAYS + GENERAL_DECAYS
DTYPES = [torch.float32, torch.bfloat16]


def _target(opt, p):
    return opt.state[p]["master"] if "master" in opt.state[p] else p.detach()


def _snapshot(opt, ps):
    """(fp32 target, EMA or None) per parameter; before its first step a bf16 parameter's master is its fp32 copy."""
    return [(_target(opt, p).float().clone(), opt.state[p]["ema"].clone() if "ema" in opt.state[p] else None)
            for p in ps]


def _assert_same_update(on, off, ps_on, ps_off):
    """Parameters, masters, momentum buffers and bf16 shadows of the optimizer with EMA equal those without."""
    for p, q in zip(ps_on, ps_off):
        assert torch.equal(p.detach(), q.detach())
        a, b = on.state[p], off.state[q]
        assert set(a) - {"ema"} == set(b)
        for k in b:
            assert torch.equal(a[k], b[k]), k


def _step_pair(on, off, ps_on, ps_off, grads, omd, exact):
    for p, q, g in zip(ps_on, ps_off, grads):
        p.grad = g
        q.grad = None if g is None else g.clone()
    before = _snapshot(on, ps_on)
    on.step()
    off.step()
    after = _snapshot(on, ps_on)
    _assert_same_update(on, off, ps_on, ps_off)
    assert check_step(before, after, [g is not None for g in grads], omd, exact) == set()
    return before, after


def _close(got, ref64):
    torch.testing.assert_close(got.detach().float().cpu(), ref64.float().reshape(got.shape), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("row", range(len(ROWS)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_sgd_rows(cuda, dtype, row):
    from distributed_learning_amd.ops.optim import FusedSGD

    kw = dict(lr=0.1, master_weights=dtype != torch.float32, **ROWS[row])
    for decay in DECAYS:
        omd, exact = omd32(decay), decay in EXACT_DECAYS
        ps_on = [p.requires_grad_() for p in _tensors(cuda, dtype)]
        ps_off = [p.requires_grad_() for p in _tensors(cuda, dtype)]
        assert ps_on[-1].data_ptr() % 16 != 0
        on, off = FusedSGD(ps_on, ema_decay=decay, **kw), FusedSGD(ps_off, **kw)
        hp = [{k: on.param_groups[0][k] for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov",
                                                    "grad_scale")}] * len(ps_on)
        P = [p.detach().double().cpu().clone() for p in ps_on]
        M, E = [None] * len(P), [None] * len(P)
        gen = torch.Generator().manual_seed(1 + row)
        for step in range(4):
            grads = _grads(ps_on, gen)
            before, after = _step_pair(on, off, ps_on, ps_off, grads, omd, exact)
            if step == 0:  # e = p0 + omd * (p1 - p0): the EMA starts from the weights before the update
                for (p0, e0), (p1, e1) in zip(before, after):
                    assert e0 is None and e1.dtype == torch.float32 and e1.stride() == p1.stride()
                    if exact:
                        assert torch.equal(e1, p0 + omd * (p1 - p0))
                    else:
                        assert bound_violations(e1, p0, p1, omd) == 0
            P_old = [p.clone() for p in P]
            sgd_oracle_step(P, M, grads, hp)
            ema_oracle_step(E, P_old, P, grads, omd)
        for p, e64 in zip(ps_on, E):
            _close(on.state[p]["ema"], e64)


@pytest.mark.parametrize("max_grad_norm", [0.0, 1.0])
@pytest.mark.parametrize("dtype", DTYPES)
def test_lars(cuda, dtype, max_grad_norm):
    from distributed_learning_amd.ops.optim import FusedLARS

    kw = dict(lr=0.3, momentum=0.9, weight_decay=1e-4, grad_scale=0.5, max_grad_norm=max_grad_norm,
              master_weights=dtype != torch.float32)
    for decay in DECAYS:
        omd, exact = omd32(decay), decay in EXACT_DECAYS
        extra = torch.randn(300, generator=torch.Generator().manual_seed(9))  # a 1-D tensor: excluded from LARS
        ps_on = [p.requires_grad_() for p in lars_tensors(cuda, dtype) + [extra.to(cuda, dtype)]]
        ps_off = [p.requires_grad_() for p in lars_tensors(cuda, dtype) + [extra.to(cuda, dtype)]]
        on, off = FusedLARS(ps_on, ema_decay=decay, **kw), FusedLARS(ps_off, **kw)
        P = [p.detach().double().cpu().clone() for p in ps_on]
        M, E = [torch.zeros_like(p) for p in P], [None] * len(P)
        gen = torch.Generator().manual_seed(2)
        for step in range(4):
            grads = _grads(ps_on, gen)
            _step_pair(on, off, ps_on, ps_off, grads, omd, exact)
            assert on.last_launches == off.last_launches  # the EMA costs no launch
            P_old = [p.clone() for p in P]
            lars_oracle_step(P, M, grads, hyper(on), 0.5, max_grad_norm)
            ema_oracle_step(E, P_old, P, grads, omd)
        for p, e64 in zip(ps_on, E):
            _close(on.state[p]["ema"], e64)


@pytest.mark.parametrize("count", [33, 70, "edges"])
@pytest.mark.parametrize("name", ["sgd", "lars"])
def test_list_boundary_and_subset_without_gradient(cuda, name, count):
    """33 and 70 tensors against 32 per launch; "edges": the list of tests/list_shapes.py, whose zero-element tensor
    FusedSGD hands to the binding and FusedLARS leaves out (so there it never has a gradient, nor an EMA)."""
    from distributed_learning_amd.ops.optim import FusedLARS, FusedSGD

    edges = count == "edges"
    count = list_shapes.COUNT if edges else count
    never = {list_shapes.EMPTY} if edges and name == "lars" else set()
    cls, kw = {"sgd": (FusedSGD, dict(lr=0.05, momentum=0.9, weight_decay=1e-4)),
               "lars": (FusedLARS, dict(lr=0.3, weight_decay=1e-4))}[name]
    decay = EXACT_DECAYS[1]
    omd = omd32(decay)
    tensors = lambda gen: list_shapes.edge_list(cuda, torch.bfloat16, gen) if edges else _cycle(cuda, torch.bfloat16, count, gen)
    make = lambda: [p.requires_grad_() for p in tensors(torch.Generator().manual_seed(count))]
    ps_on, ps_off = make(), make()
    on, off = cls(ps_on, master_weights=True, ema_decay=decay, **kw), cls(ps_off, master_weights=True, **kw)
    gen = torch.Generator().manual_seed(3)
    idle = {1, count // 2, 31, 32, count - 1}
    for step in range(3):
        grads = _grads(ps_on, gen, mult=lambda t: (t + 1.0) / 64)
        grads = [None if t in never or (step == 1 and t in idle) else g for t, g in enumerate(grads)]
        before, after = _step_pair(on, off, ps_on, ps_off, grads, omd, True)
        if step == 1:  # said once more, outside check_step: not a bit of an idle tensor's EMA moves
            assert all(torch.equal(before[t][1], after[t][1]) for t in idle)
            # ("edges": but for the empty tensor and the one-element ones, whose single omd * (p_new - e) may
            # round to no change)
            moving = [t for t in range(count) if t not in idle and (ps_on[t].numel() > 1 or not edges)]
            assert [t for t in moving if torch.equal(before[t][1], after[t][1])] == []


def test_misaligned_ema_takes_the_scalar_path_to_the_same_values(cuda):
    """Direct binding calls: the same update with an aligned EMA and with an EMA view one element past an aligned
    address, which fails the 16-byte test and sends full chunks down the scalar path."""
    from distributed_learning_amd.ops import _ext

    C = _ext.require()
    gen = torch.Generator().manual_seed(4)
    n = 4096 * 2
    omd = torch.full((1,), 2.0 ** -3, device=cuda)
    outs = []
    for misaligned in (False, True):
        g = torch.Generator().manual_seed(5)
        p = torch.randn(n, generator=g).to(cuda)
        grad = torch.randn(n, generator=g).to(cuda, torch.bfloat16)
        m = torch.randn(n, generator=g).to(cuda)
        shadow = p.to(torch.bfloat16)
        store = torch.zeros(n + 1, device=cuda)
        e = store[1:] if misaligned else store[:n]
        assert (e.data_ptr() % 16 != 0) == misaligned
        e.copy_(torch.randn(n, generator=g))
        e_old, store_head = e.clone(), store.clone()
        C.sgd_ema_step_list([p], [grad], [m], [shadow], [e], omd, 0.1, 0.9, 0.0, 1e-4, False, 1.0, False)
        assert torch.equal(e, replay32(e_old, p, 2.0 ** -3)) and torch.equal(shadow, p.to(torch.bfloat16))
        if misaligned:
            assert store[0] == store_head[0]  # the element in front of the view
        else:
            assert store[n] == store_head[n]
        outs.append((p, m, shadow, e.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    # the same for the list kernels that only touch averages
    x = torch.randn(n, generator=gen).to(cuda)
    store = torch.randn(n + 1, generator=gen).to(cuda)
    e, aligned = store[1:], store[1:].clone()
    C.ema_update_list([e], [x], omd)
    C.ema_update_list([aligned], [x], omd)
    assert torch.equal(e, aligned)
    sh_a, sh_b, xa, xb = x.to(torch.bfloat16), x.to(torch.bfloat16), x.clone(), x.clone()
    C.ema_swap_list([xa], [e], [sh_a])
    C.ema_swap_list([xb], [aligned], [sh_b])
    assert torch.equal(xa, xb) and torch.equal(e, aligned) and torch.equal(sh_a, sh_b) and torch.equal(e, x)


@pytest.mark.parametrize("name", ["sgd", "lars"])
def test_graph_capture_follows_the_decay_schedule(cuda, name):
    """A captured step replays with new gradients and new decays and equals eager bit for bit."""
    from distributed_learning_amd.ops.optim import FusedLARS, FusedSGD, ema_decay_at

    def make():
        ps = [t.requires_grad_() for t in _tensors(cuda, torch.bfloat16, 20)[:4] + _tensors(cuda, torch.float32, 21)[2:5]]
        if name == "sgd":
            opt = FusedSGD(ps, lr=0.1, momentum=0.9, weight_decay=1e-4, master_weights=True, ema_decay=0.999)
        else:
            opt = FusedLARS(ps, lr=0.5, momentum=0.9, weight_decay=1e-4, max_grad_norm=1.0, master_weights=True,
                            ema_decay=0.999)
        for p in ps:
            p.grad = torch.zeros_like(p)  # static gradient buffers
        return ps, opt

    gen = torch.Generator().manual_seed(22)
    (pe, oe), (pg, og) = make(), make()
    feeds = [[torch.randn(p.shape, generator=gen) for p in pe] for _ in range(5)]

    def feed(ps, opt, s):
        for p, v in zip(ps, feeds[s]):
            p.grad.copy_(v.to(cuda))
        opt.set_ema_decay(ema_decay_at(s, 0.999, True))

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
        assert set(oe.state[a]) == set(og.state[b]) and "ema" in oe.state[a]
        for k in oe.state[a]:
            assert torch.equal(oe.state[a][k], og.state[b][k]), k
    # the decays did differ: a constant-decay run ends elsewhere
    pc, oc = make()
    for s in range(5):
        feed(pc, oc, s)
        oc.set_ema_decay(0.999)
        oc.step()
    assert not torch.equal(oc.state[pc[2]]["ema"], og.state[pg[2]]["ema"])
    assert torch.equal(oc.state[pc[2]]["master"], og.state[pg[2]]["master"])


def test_ema_update_list(cuda):
    """Buffer-sized tensors, 40 of them (two launches): the replay criteria for every decay. Then the same on the
    list of tests/list_shapes.py, and that list's exchange by ema_swap_list, bit for bit, and back."""
    from distributed_learning_amd.ops import _ext

    C = _ext.require()
    gen = torch.Generator().manual_seed(6)
    sizes = [(1, 64, 2048)[t % 3] for t in range(40)]
    for make in (lambda: [torch.randn(n, generator=gen).to(cuda) for n in sizes],
                 lambda: list_shapes.edge_list(cuda, torch.float32, gen)):
        for decay in DECAYS:
            omd = omd32(decay)
            omd_dev = torch.full((1,), 1.0 - decay, dtype=torch.float32, device=cuda)
            assert float(omd_dev) == omd
            emas = make()
            for _ in range(2):
                xs = make()
                old = [e.clone() for e in emas]
                keep = [x.clone() for x in xs]
                C.ema_update_list(emas, xs, omd_dev)
                assert all(torch.equal(a, b) for a, b in zip(xs, keep))  # the sources are read only
                for e, o, x in zip(emas, old, xs):
                    if decay in EXACT_DECAYS:
                        assert torch.equal(e, replay32(o, x, omd))
                    assert bound_violations(e, o, x, omd) == 0
    C.ema_update_list([], [], omd_dev)  # an empty list is no launch
    # the exchange, on inputs of its own: the list of list_shapes.py, a bf16 shadow for every other tensor
    xs, emas = list_shapes.edge_list(cuda, torch.float32, gen), list_shapes.edge_list(cuda, torch.float32, gen)
    assert len(xs) == list_shapes.COUNT and xs[list_shapes.EMPTY].numel() == 0
    x0, e0 = [x.clone() for x in xs], [e.clone() for e in emas]
    shadows = [torch.empty_like(x, dtype=torch.bfloat16) if t % 2 else None for t, x in enumerate(xs)]
    C.ema_swap_list(xs, emas, shadows)
    assert all(torch.equal(x, e) for x, e in zip(xs, e0)) and all(torch.equal(e, x) for e, x in zip(emas, x0))
    assert all(s is None or torch.equal(s, x.to(torch.bfloat16)) for s, x in zip(shadows, xs))
    C.ema_swap_list(xs, emas, shadows)
    assert all(torch.equal(x, b) for x, b in zip(xs, x0)) and all(torch.equal(e, b) for e, b in zip(emas, e0))


def _bn_conv_model(cuda):
    from distributed_learning_amd.ops import nn as dnn

    torch.manual_seed(7)
    model = torch.nn.Sequential(torch.nn.Conv2d(8, 16, 3, padding=1, bias=False), torch.nn.BatchNorm2d(16),
                                torch.nn.ReLU(), torch.nn.Flatten(), torch.nn.Linear(16 * 4 * 4, 5)).to(cuda)
    dnn.bf16_weights(model)
    return model


def _all_tensors(model, opt, ema):
    out = [p.detach().clone() for p in model.parameters()] + [b.clone() for b in model.buffers()]
    for p in model.parameters():
        out += [opt.state[p][k].clone() for k in sorted(opt.state[p]) if torch.is_tensor(opt.state[p][k])]
    return out + [ema.buffers[k].clone() for k in sorted(ema.buffers)]


@pytest.mark.parametrize("name", ["sgd", "lars"])
def test_swap_and_applied(cuda, name):
    from distributed_learning_amd.ops.optim import FusedLARS, FusedSGD, ModelEMA

    model = _bn_conv_model(cuda)
    assert {p.dtype for p in model.parameters()} == {torch.bfloat16, torch.float32}
    cls, kw = {"sgd": (FusedSGD, dict(lr=0.1, momentum=0.9)), "lars": (FusedLARS, dict(lr=0.3, weight_decay=1e-4))}[name]
    opt = cls(model.parameters(), master_weights=True, ema_decay=0.9, **kw)
    ema = ModelEMA(model, opt, 1 - 2.0 ** -3, warmup=True)
    assert sorted(ema.buffers) == ["1.running_mean", "1.running_var"]
    gen = torch.Generator().manual_seed(8)
    bn = model[1]
    for s in range(3):
        for p in model.parameters():
            p.grad = _like(p, torch.randn(p.shape, generator=gen))
        with torch.no_grad():  # what a training forward does to the statistics
            bn.running_mean.add_(torch.randn(16, generator=gen).to(cuda))
            bn.running_var.mul_(1.25)
            bn.num_batches_tracked.add_(1)
        old = {k: v.clone() for k, v in ema.buffers.items()}
        ema.step(s)
        omd = omd32(min(1 - 2.0 ** -3, (1 + s) / (10 + s)))
        for k, b in (("1.running_mean", bn.running_mean), ("1.running_var", bn.running_var)):
            assert bound_violations(ema.buffers[k], old[k], b, omd) == 0
            assert not torch.equal(ema.buffers[k], old[k])
    before = _all_tensors(model, opt, ema)
    emas = [opt.state[p]["ema"].clone() for p in model.parameters()]
    live = [_target(opt, p).clone() for p in model.parameters()]
    buf_emas = {k: v.clone() for k, v in ema.buffers.items()}

    def check_inside():
        for p, e, w in zip(model.parameters(), emas, live):
            st = opt.state[p]
            if p.dtype == torch.bfloat16:
                assert torch.equal(p.detach(), e.to(torch.bfloat16)) and torch.equal(st["master"], e)
            else:
                assert torch.equal(p.detach(), e)
            assert torch.equal(st["ema"], w) and not torch.equal(e, w)  # the exchange: nothing is lost
        assert torch.equal(bn.running_mean, buf_emas["1.running_mean"])
        assert torch.equal(bn.running_var, buf_emas["1.running_var"])
        assert int(bn.num_batches_tracked) == 3

    with ema.applied():
        check_inside()
    assert all(torch.equal(a, b) for a, b in zip(before, _all_tensors(model, opt, ema)))
    with pytest.raises(ZeroDivisionError):
        with ema.applied():
            check_inside()
            1 / 0
    assert all(torch.equal(a, b) for a, b in zip(before, _all_tensors(model, opt, ema)))
    exported = ema.model_state_dict()
    assert torch.equal(exported["0.weight"], emas[0].to(torch.bfloat16))
    assert torch.equal(exported["1.running_var"], buf_emas["1.running_var"])
    assert all(torch.equal(a, b) for a, b in zip(before, _all_tensors(model, opt, ema)))


def _refusal_lists(cuda, count=34, n=5000):
    gen = torch.Generator().manual_seed(9)
    mk = lambda dt=torch.float32: [torch.randn(n, generator=gen).to(cuda, dt) for _ in range(count)]
    return dict(p=mk(), g=mk(torch.bfloat16), m=mk(), s=mk(torch.bfloat16), e=mk())


BAD = ["dtype", "cpu", "numel", "strided", "omd2", "length"]
REFUSALS = [(op, bad) for op in ("sgd", "lars", "update", "swap") for bad in BAD
            if (op, bad) != ("swap", "omd2")]  # ema_swap_list takes no decay


@pytest.mark.parametrize("op,bad", REFUSALS)
def test_binding_refusals_leave_everything_untouched(cuda, op, bad):
    """The bad slot is number 33 of 34, in the second launch: every launch is built and checked before the first
    one is issued."""
    from distributed_learning_amd.ops import _ext

    C = _ext.require()
    L = _refusal_lists(cuda)
    n = L["p"][0].numel()
    omd = torch.full((1,), 0.125, device=cuda)
    slot = 33
    if bad == "dtype":
        L["e"][slot] = L["e"][slot].double()
    elif bad == "cpu":
        L["e"][slot] = L["e"][slot].cpu()
    elif bad == "numel":
        L["e"][slot] = torch.zeros(n + 1, device=cuda)
    elif bad == "strided":
        L["e"][slot] = torch.zeros(2 * n, device=cuda)[::2]
        assert L["e"][slot].numel() == n and not L["e"][slot].is_contiguous()
    elif bad == "omd2":
        omd = torch.full((2,), 0.125, device=cuda)
    elif bad == "length":
        L["e"] = L["e"][:-1]
    before = {k: [t.clone() for t in v] for k, v in L.items()}
    with pytest.raises(RuntimeError):
        if op == "sgd":
            C.sgd_ema_step_list(L["p"], L["g"], L["m"], L["s"], L["e"], omd, 0.1, 0.9, 0.0, 0.0, False, 1.0, False)
        elif op == "lars":
            T = len(L["p"])
            lr_dev = torch.full((1,), 0.1, device=cuda)
            plan = C.LarsPlan([n] * T, [0] * T, [True] * T, [1e-4] * T, [1e-3] * T, [0.0] * T, [0.9] * T, lr_dev,
                              L["p"][0])
            C.lars_ema_step_list(plan, L["p"], L["g"], L["m"], L["s"], L["e"], omd, 1.0, 0.0)
        elif op == "update":
            C.ema_update_list(L["e"], L["p"], omd)
        else:
            C.ema_swap_list(L["p"], L["e"], L["s"])
    torch.cuda.synchronize(cuda)
    for k, v in L.items():
        assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(v, before[k])), k


def _resnet_run(cuda, eval_after=None, steps=3):
    """ResNet-18 on CIFAR-shaped synthetic data at batch 8 on the bf16 native path with FusedLARS and ModelEMA.
    Returns the model, the optimizer, the EMA, each step's gradients and the evaluation results."""
    from distributed_learning_amd.models import create_network
    from distributed_learning_amd.ops import nn as dnn
    from distributed_learning_amd.ops.loss import cross_entropy
    from distributed_learning_amd.ops.optim import FusedLARS, ModelEMA
    from distributed_learning_amd.train import evaluate

    torch.manual_seed(0)
    model = create_network("resnet18_cifar").to(cuda).to(memory_format=torch.channels_last)
    dnn.bf16_weights(model)
    opt = FusedLARS(model.parameters(), lr=0.5, momentum=0.9, weight_decay=1e-4, max_grad_norm=1.0,
                    master_weights=True, ema_decay=0.5)
    ema = ModelEMA(model, opt, 0.5)
    g = torch.Generator().manual_seed(1)
    held_out = [(torch.rand(8, 3, 32, 32, generator=g).to(cuda, torch.bfloat16), torch.randint(0, 10, (8,), generator=g))]
    grads, results = [], {}
    dnn.set_backend("native")
    dnn.set_native_conv(True)
    try:
        model.train()
        for s in range(steps):
            x = torch.rand(8, 3, 32, 32, generator=g).to(cuda, torch.bfloat16).contiguous(memory_format=torch.channels_last)
            y = torch.randint(0, 10, (8,), generator=g).to(cuda)
            opt.zero_grad(set_to_none=True)
            cross_entropy(model(x), y).backward()
            grads.append([p.grad.detach().cpu().clone() for p in model.parameters()])
            ema.step(s)
            if eval_after == s + 1:
                results["live"] = evaluate(model, held_out, cuda, "bf16")
                with ema.applied():
                    results["ema"] = evaluate(model, held_out, cuda, "bf16")
    finally:
        dnn.set_native_conv(False)
        dnn.set_backend("torch")
    return model, opt, ema, grads, results


def test_resnet18_cifar_ema_end_to_end(cuda):
    from distributed_learning_amd.models import create_network
    from distributed_learning_amd.ops.optim import FusedLARS

    model, opt, ema, grads, _ = _resnet_run(cuda)
    m2, o2, e2, _, res = _resnet_run(cuda, eval_after=2)
    # evaluating from the averages sees another model, and leaves the run alone, bit for bit
    assert res["live"]["samples"] == res["ema"]["samples"] == 8 and res["live"]["loss"] != res["ema"]["loss"]
    for p, q in zip(model.parameters(), m2.parameters()):
        assert torch.equal(p.detach(), q.detach())
        for k in ("ema", "momentum_buffer"):
            assert torch.equal(opt.state[p][k], o2.state[q][k])
    for (k, b), (_, c) in zip(model.named_buffers(), m2.named_buffers()):
        assert torch.equal(b, c), k
    assert all(torch.equal(ema.buffers[k], e2.buffers[k]) for k in ema.buffers)
    # the native EMAs against the torch formula on CPU copies fed the same gradients
    torch.manual_seed(0)
    ref_model = create_network("resnet18_cifar").to(memory_format=torch.channels_last)
    cpu = [p.detach().to(torch.bfloat16 if q.dtype == torch.bfloat16 else torch.float32).requires_grad_()
           for p, q in zip(ref_model.parameters(), model.parameters())]
    ref = FusedLARS(cpu, lr=0.5, momentum=0.9, weight_decay=1e-4, max_grad_norm=1.0, master_weights=True, ema_decay=0.5)
    for gs in grads:
        for c, g in zip(cpu, gs):
            c.grad = g.clone()
        ref.step()
    assert opt.last_launches > 0 and ref.last_launches == 0
    for p, c in zip(model.parameters(), cpu):
        assert opt.state[p]["ema"].dtype == torch.float32
        torch.testing.assert_close(opt.state[p]["ema"].cpu(), ref.state[c]["ema"], rtol=RTOL, atol=ATOL)


@pytest.mark.slow
def test_cli_writes_alternating_eval_lines(cuda, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "distributed_learning_amd.main", "1", "0", "1", "1", "127.0.0.1", "lo",
           "resnet18_cifar", "/nonexistent", "1", "--experiment", "experiment_single", "--ema_decay", "0.9",
           "--eval_batches", "1", "--eval_every", "1", "--limit_batches", "2", "--random_input", "1", "--batch_size", "8",
           "--master_port", str(dist_util.free_port()), "--results_root", str(tmp_path), "--job_id", "t"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = next(tmp_path.glob("*/single_0_0_eval.txt")).read_text().splitlines()
    assert [ln.split()[2] for ln in lines] == ["eval", "eval_ema", "eval", "eval_ema"]
    assert [ln.split()[5] for ln in lines] == ["1:", "1:", "2:", "2:"]
    assert lines[0].split()[7] != lines[1].split()[7]  # another model, another loss
