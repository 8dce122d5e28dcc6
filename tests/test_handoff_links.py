"""The hand-off protocol between the fused BN autograd nodes and the 1x1 conv nodes (ops/conv.py DualBNLink,
StemBNLink, ResidualLink use in _Conv1x1Fork; ops/bn_act.py _BNAct) under autograd graphs other than the one
training step: run on the CPU through the real autograd Functions and link classes, with a torch stand-in for the
extension calls (tests/ext_standin.py).

Graph: ``out = relu(bn(conv3(conv1(x))) + x)`` at 2x16x4x4 -> 2x8x4x4 -> 2x16x4x4, conv1 forking the identity.
Reference: the same graph in float64 from the same (bf16-representable) values.

Bound: per gradient, 4x the relative L2 error of stock torch running the same graph in bf16 (measured in the
same test against the same float64 reference; at this size 5e-3 to 2e-2, mostly ReLU decisions that flip where the
bf16 pre-activation rounds across zero). The hand-off path rounds at other points than stock bf16, hence the
margin; the defects these graphs target are O(1): a gradient counted twice, a stale identity gradient added."""
import copy

import pytest
import torch
import torch.nn as nn

from distributed_learning_amd.models.resnet import resnet50
from distributed_learning_amd.ops import _ext, bn_act
from distributed_learning_amd.ops import conv as nconv

from ext_standin import StandIn, pack_bits, unpack_bits

CL = torch.channels_last
MARGIN = 4.0


@pytest.fixture
def standin(monkeypatch):
    C = StandIn()
    monkeypatch.setattr(_ext, "require", lambda: C)
    monkeypatch.setattr(bn_act, "supported", lambda x, bn, r: True)
    return C


def test_standin_bit_masks_match_the_conv_helper():
    t = torch.rand(2, 16, 3, 5).contiguous(memory_format=CL) > 0.5
    m = pack_bits(t.permute(0, 2, 3, 1))
    assert torch.equal(nconv._unpack_bits(m, t.float()), t.float())
    assert torch.equal(unpack_bits(m, (2, 3, 5, 16)), t.permute(0, 2, 3, 1).float())


def _build(dtype):
    torch.manual_seed(0)
    c1 = nn.Conv2d(16, 8, 1, bias=False).to(memory_format=CL)
    c3 = nn.Conv2d(8, 16, 1, bias=False).to(memory_format=CL)
    bn = nn.BatchNorm2d(16)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.2, 0.2)
    x = torch.randn(2, 16, 4, 4).bfloat16().contiguous(memory_format=CL)
    for c in (c1, c3):
        c.weight.data = c.weight.data.bfloat16().to(dtype)
    if dtype == torch.float64:
        bn = bn.double()
    wl = torch.linspace(-1, 1, x.numel()).view(2, 4, 4, 16).permute(0, 3, 1, 2)  # loss weights, block output
    wa = torch.linspace(1, -1, x.numel() // 2).view(2, 4, 4, 8).permute(0, 3, 1, 2)  # aux loss, conv1 output
    return c1, c3, bn, x.to(dtype), wl.to(dtype), wa.to(dtype)


def _freeze(cond, c1, c3, bn, x):
    x.requires_grad_(cond != "input_nograd")
    for p in (c1.weight, c3.weight):
        p.requires_grad_(cond != "conv_frozen")
    for p in (bn.weight, bn.bias):
        p.requires_grad_(cond != "bn_frozen")


def _grads(x, c1, c3, bn, k=1.0):
    return {n: None if t.grad is None else t.grad.double() * k
            for n, t in (("x", x), ("conv1.weight", c1.weight), ("conv3.weight", c3.weight), ("bn.weight", bn.weight),
                         ("bn.bias", bn.bias))}


def _native(cond):
    c1, c3, bn, x, wl, wa = _build(torch.bfloat16)
    _freeze(cond, c1, c3, bn, x)
    y1, _, ident, _ = nconv.conv1x1_fork(x, c1)
    y3, _ = nconv.conv1x1(y1, c3)
    assert getattr(y3, "_dla_dual", None) is not None  # the BN hand-off link is in play
    out = bn_act.fused_bn_act(y3, bn, True, ident, None)
    loss = (out.float() * wl).sum()
    if cond == "twice":
        loss.backward(retain_graph=True)
        loss.backward()
    elif cond in ("pruned_then_full", "pruned_then_aux"):
        (g,) = torch.autograd.grad(loss, [bn.weight], retain_graph=True)
        assert g is not None and all(t.grad is None for t in (x, c1.weight, c3.weight, bn.weight, bn.bias))
        (loss if cond == "pruned_then_full" else (y1.float() * wa).sum()).backward()
    else:
        loss.backward()
    return _grads(x, c1, c3, bn)


def _reference(cond, dtype=torch.float64):
    """The same graph on stock torch ops: float64 (the reference), or bf16 (the noise the bound is taken from)."""
    c1, c3, bn, x, wl, wa = _build(dtype)
    _freeze(cond, c1, c3, bn, x)
    y1 = c1(x)
    out = torch.relu(bn(c3(y1)) + x)
    ((y1 * wa).sum() if cond == "pruned_then_aux" else (out * wl).sum()).backward()
    return _grads(x, c1, c3, bn, 2.0 if cond == "twice" else 1.0)


@pytest.mark.parametrize("cond", ["plain", "twice", "conv_frozen", "bn_frozen", "input_nograd", "pruned_then_full",
                                  "pruned_then_aux"])
def test_graph_condition_matches_float64(standin, cond):
    got, ref, stock = _native(cond), _reference(cond), _reference(cond, torch.bfloat16)
    report = {}
    for n in ref:
        assert (got[n] is None) == (ref[n] is None), (cond, n)
        if ref[n] is not None:
            nr = ref[n].norm()
            report[n] = (float((got[n] - ref[n]).norm() / nr), float((stock[n] - ref[n]).norm() / nr),
                         float(got[n].norm() / nr))
    print(cond, {n: "rel %.3g stock-bf16 %.3g norm ratio %.4g" % v for n, v in report.items()})
    assert cond == "pruned_then_aux" or "bn_act_bwd" in standin.calls
    for n, (rel, noise, ratio) in report.items():
        assert rel <= MARGIN * noise, \
            f"{cond}: {n} relative L2 {rel:.3g} vs float64 (stock bf16 {noise:.3g}, norm ratio {ratio:.4g})"


def test_plain_graph_materialises_the_parked_gradient_once(standin):
    """The plain step parks in the BN backward and takes in the conv backward: one BN reduction, one
    materialising BN apply (the stand-in's one-pass kernel answers "not served")."""
    _native("plain")
    assert standin.calls.count("bn_act_bwd") == 2 and standin.calls.count("conv1x1_dual") == 1


def test_eval_mode_bn_with_gradients_takes_the_stock_path(standin):
    c1, c3, bn, x, wl, _ = _build(torch.bfloat16)
    bn.eval()
    x.requires_grad_(True)
    out = bn_act.fused_bn_act(x, bn, True, None, None)
    assert "bn_act_fwd" not in standin.calls
    out.float().mul(wl).sum().backward()  # the fused node would raise here
    r = _build(torch.float64)
    xr = r[3].requires_grad_(True)
    torch.relu(r[2].eval()(xr)).mul(r[4]).sum().backward()
    assert float((x.grad.double() - xr.grad).norm() / xr.grad.norm()) <= 2 ** -7  # two bf16 roundings, elementwise
    with torch.no_grad():  # inference stays on the fused kernel
        bn_act.fused_bn_act(x, bn, True, None, None)
    assert standin.calls == ["bn_act_fwd"]


# ---- the link objects themselves -------------------------------------------------------------------------------

class _InBackward(torch.autograd.Function):
    """Runs ``fn`` inside a backward pass of its own."""

    @staticmethod
    def forward(ctx, x, fn):
        ctx.fn = fn
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        ctx.fn()
        return g, None


def _in_backward_pass(fn):
    out = []
    _InBackward.apply(torch.zeros(1, requires_grad=True), lambda: out.append(fn())).sum().backward()
    return out[0]


def _fields(link):
    names = [s for klass in type(link).__mro__ for s in getattr(klass, "__slots__", ())]
    return {s: getattr(link, s) for s in names if s != "claimed"}


def _park(link):
    y = torch.ones(2, 8, 2, 2, dtype=torch.bfloat16)
    if isinstance(link, nconv.StemBNLink):
        return link.park(y, torch.zeros(1), y, torch.zeros(1), torch.ones(8), (3, 2, 1))
    return link.park(y, y, torch.zeros(1), torch.zeros(1, dtype=torch.uint8), torch.ones(8))


@pytest.mark.parametrize("kind", [nconv.DualBNLink, nconv.StemBNLink])
def test_take_clears_every_field(kind):
    link = kind()
    assert link.claim()
    ph = _park(link)
    assert ph.shape == (2, 8, 2, 2) and not ph.any() and link.parked() and not link.can_park(ph)
    unused = ("mask", "mode") if kind is nconv.StemBNLink else ()  # the pooled op parks positions, not a mask
    assert all((v is None) == (n in unused) for n, v in _fields(link).items()), _fields(link)
    taken = link.take()
    assert taken[0] is ph and len(taken) == 7 and all(v is not None for v in taken)
    assert all(v is None for v in _fields(link).values()), _fields(link)
    assert link.claimed and not link.parked()


@pytest.mark.parametrize("kind", [nconv.DualBNLink, nconv.StemBNLink])
def test_a_park_nobody_took_does_not_survive_into_a_later_pass(kind):
    link = kind()
    y = torch.ones(2, 8, 2, 2, dtype=torch.bfloat16)
    _in_backward_pass(lambda: _park(link))
    assert link.ph is not None  # left behind: its consumer did not run
    assert _in_backward_pass(lambda: (link.parked(), link.can_park(y))) == (False, True)
    assert all(v is None for v in _fields(link).values()), _fields(link)
    # parked and taken within one pass: served
    assert _in_backward_pass(lambda: (_park(link) is not None, link.parked(), link.take()[0] is not None)) == \
        (True, True, True)


def test_residual_link_serves_the_pass_that_handed_over_only():
    rl = bn_act.ResidualLink()
    dy, mask = torch.ones(3), torch.zeros(1, dtype=torch.uint8)
    assert rl.take() == (None, None)
    got = _in_backward_pass(lambda: (rl.hand(dy, mask), rl.take())[1])
    assert got[0] is dy and got[1] is mask and rl.dy is None and rl.mask is None
    _in_backward_pass(lambda: rl.hand(dy, mask))
    assert rl.dy is dy  # left behind by a pass that pruned the fork
    assert _in_backward_pass(rl.take) == (None, None)
    assert rl.dy is None and rl.mask is None and rl.task is None


def test_a_torch_without_the_pass_id_raises_at_the_first_handoff_only(monkeypatch):
    """Nothing can be confined to its pass then: an error where something is first parked or handed over, not a
    silent fallback; links that carry nothing (inference, the stock paths) keep working."""
    monkeypatch.setattr(bn_act, "_current_graph_task_id", None)
    link, rl = nconv.DualBNLink(), bn_act.ResidualLink()
    y = torch.ones(2, 8, 2, 2, dtype=torch.bfloat16)
    assert link.claim() and not link.parked() and link.can_park(y) and rl.take() == (None, None)
    with pytest.raises(RuntimeError, match="_current_graph_task_id"):
        _park(link)
    with pytest.raises(RuntimeError, match="_current_graph_task_id"):
        rl.hand(torch.ones(3), None)
    with pytest.raises(RuntimeError, match="_current_graph_task_id"):
        _park(nconv.StemBNLink())


def test_claim_serves_one_bn_only():
    link = nconv.DualBNLink()
    assert link.claim() and not link.claim() and not link.claim()
    link.take()
    assert link.claimed and not link.claim()  # a take does not reopen it


def test_observed_conv_output_refuses_the_park():
    link = nconv.DualBNLink()
    y = (torch.ones(2, 8, 2, 2, requires_grad=True) * 2)
    assert link.can_park(y)
    y.register_hook(lambda g: g)
    assert not link.can_park(y)
    z = (torch.ones(2, 8, 2, 2, requires_grad=True) * 2)
    z.retain_grad()
    assert not link.can_park(z)


# ---- forward observers of a deferred block output (models/resnet.py) -------------------------------------------

def _watched(model):
    return [(li, bi) for li, layer in enumerate((model.layer1, model.layer2, model.layer3, model.layer4), 1)
            for bi, b in enumerate(layer) if any(b.output_watch)]


def test_output_watch_names_the_other_observers_of_a_block_output():
    m = resnet50(num_classes=10)
    assert _watched(m) == [] and m.layer4[2].output_watch == ()
    for register, expect in ((m.layer1.register_forward_hook, [(1, 2)]),
                             (m.layer2.register_forward_pre_hook, [(1, 2)]),
                             (m.layer2[0].register_forward_pre_hook, [(1, 2)]),
                             (m.layer3[4].register_forward_pre_hook, [(3, 3)]),
                             (m.layer3[4].register_forward_hook, [])):  # the block's own hook: its own guard
        h = register(lambda *a: None)
        assert _watched(m) == expect, expect
        h.remove()
        assert _watched(m) == []
    m2 = copy.deepcopy(m)  # the copy watches its own modules' tables, not the original's
    h = m.layer1.register_forward_hook(lambda *a: None)
    assert _watched(m2) == [] and _watched(m) == [(1, 2)]
    h.remove()
    m2.layer1.register_forward_hook(lambda *a: None)
    assert _watched(m2) == [(1, 2)] and _watched(m) == []
