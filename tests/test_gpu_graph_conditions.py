"""The fused hand-offs between autograd nodes under graphs other than the one training step (gpu): frozen
parameters, an input that needs a gradient, a pruned ``autograd.grad`` before the full backward, two backwards on
one graph, forward and gradient observers, eval-mode BN with gradients, a training-mode forward under no_grad, and
the two fp32 conv shapes ``conv_f32.supported`` used to accept without a working backward.

Harnesses (each built from one seed on the native backend, on stock torch in bf16, and on stock torch in float64
from the same bf16-rounded values):

* tail: ``conv1x1_fork(x, c1)`` -> ``conv1x1(h, c3, want_stats)`` -> ``fused_bn_act(y3, bn, True, ident, st)``,
  256 -> 64 and 64 -> 256 channels, at M = 16 x 64 x 64 = 65536 rows (the smallest the one-pass kernel with the BN
  apply serves, and with it the smallest at which a BN hand-off link exists) and at 2 x 8 x 8 (no such link: the
  separate kernels under the same conditions, and the residual hand-off to the fork); and the same with a
  downsample conv + BN as the shortcut (``fused_bn_add_bn_act``: _BNDualAct parks into both convs' links) at
  M = 65536;
* stem: ``conv_bn_act_maxpool`` with the 7x7 / s2 conv at 2 x 3 x 32 x 32 (the quad form);
* model: resnet50 at 4 x 3 x 64 x 64 and resnet18 at 2 x 3 x 64 x 64 with bf16 weights.

Against float64 (tail, stem): every gradient by relative L2; the bound is 4x the error of the stock bf16 run of
the same graph, measured in the same test, which itself must stay below 0.025. What keeps the stock error that
low is the loss ``0.5 * sum(w * out^2)`` (w = linspace(-1, 1)): its gradient ``w * out`` vanishes where the final
ReLU switches, so an element whose bf16 pre-activation rounds across zero costs nothing. A loss linear in ``out``
measures 0.03 at both tail sizes -- ReLU decisions that differ between bf16 and float64 are O(1) errors on a
fraction f of the elements, sqrt(f) in L2. The stem's max-pool has the same effect at near-tied window maxima,
which no loss weighting removes (0.024 with normal data), so the stem runs on data whose conv outputs are exact in
bf16: image values in {-1, 0, 1}, weights in {-1, 0, 1} / 8 (|y| < 32 in steps of 1/8). Measured on MI355X, largest
over all conditions and tensors: stock bf16 4.9e-3 (M = 65536), 6.2e-3 (2 x 8 x 8), 8.8e-3 (stem); native 3.8e-3,
4.3e-3, 3.8e-3, never above the stock error of the same tensor.

The model harness is compared with a native run without hand-offs, not against float64: through 50 layers the
switched ReLU decisions make the stock bf16 gradients themselves differ from float64 by 0.33 (resnet18) and 1.31
(resnet50) in the median at these shapes (largest 0.49 and 1.63; only fc.bias is below 0.025; stock fp32 reaches
1.3e-2), whatever the loss, so no bound of the kind above exists there (profiles/graph_conditions/README.md). Two
native runs have bitwise equal forwards, so every ReLU and pool decision is the same: each condition's gradients
must equal, tensor by tensor, those of the same condition with nothing handed between autograd nodes
(_same_values). Further model checks: gradients are None exactly where the float64 run's are; ``autograd.grad``
leaves ``.grad`` alone; a pruned pass followed by the full backward gives bitwise the plain step's gradients; two
backwards give bitwise twice one; frozen parameters leave the other gradients bitwise as they are; observers see
bitwise what they see with the deferral off."""
import contextlib

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

CL = torch.channels_last
MARGIN, NOISE_MAX = 4.0, 0.025


@pytest.fixture(autouse=True)
def _restore_process_state():
    """What tests/conftest.py does not put back: the stem hand-off switch, the fp32 conv switch, the knob cache,
    torch's deterministic flags and the global module hooks."""
    from distributed_learning_amd import knobs
    from distributed_learning_amd.ops import conv as nconv
    from distributed_learning_amd.ops import nn as dnn

    mod = nn.modules.module
    tables = (mod._global_forward_hooks, mod._global_forward_pre_hooks)
    saved = (nconv.STEM_BN, dnn._NATIVE_F32, dict(knobs._CACHE), torch.are_deterministic_algorithms_enabled(),
             torch.is_deterministic_algorithms_warn_only_enabled(), torch.utils.deterministic.fill_uninitialized_memory,
             [dict(t) for t in tables])
    yield
    nconv.STEM_BN, dnn._NATIVE_F32 = saved[0], saved[1]
    knobs._CACHE.clear()
    knobs._CACHE.update(saved[2])
    torch.use_deterministic_algorithms(saved[3], warn_only=saved[4])
    torch.utils.deterministic.fill_uninitialized_memory = saved[5]
    for t, old in zip(tables, saved[6]):
        t.clear()
        t.update(old)


@pytest.fixture(scope="module")
def refs():
    """Stock bf16 and float64 results, computed once per (harness, size, graph) and shared."""
    cache = {}
    yield cache
    cache.clear()


@pytest.fixture(scope="module", autouse=True)
def _free_shared_values():
    yield
    _VALUES.clear()


@contextlib.contextmanager
def _backend(native: bool):
    from distributed_learning_amd.ops import nn as dnn

    if native:
        dnn.set_backend("native")
        dnn.set_native_conv(True)
    try:
        yield
    finally:
        dnn.set_native_conv(False)
        dnn.set_backend("torch")


def _counters():
    from distributed_learning_amd.ops import bn_act
    from distributed_learning_amd.ops import conv as nconv

    return {**dict(nconv.CALLS), **bn_act.CALLS}


def _used(before):
    after = _counters()
    return {k: after[k] - before.get(k, 0) for k in after if after[k] != before.get(k, 0)}


def _dbl(t):
    return None if t is None else t.detach().double().clone()


def _compare(tag, got, stock, ref):
    """None exactly where the reference is; else relative L2 within MARGIN x the stock bf16 run's."""
    rows = []
    for n, r in ref.items():
        assert (got[n] is None) == (r is None), f"{tag}: {n} is {'None' if got[n] is None else 'set'}, " \
                                                 f"the float64 reference's is {'None' if r is None else 'set'}"
        if r is not None:
            nr = float(r.norm())
            assert nr > 0, (tag, n)
            rows.append((n, float((got[n] - r).norm()) / nr, float((stock[n] - r).norm()) / nr,
                         float(got[n].norm()) / nr))
    print(f"{tag}: " + "; ".join(f"{n} native {e:.2e} stock-bf16 {s:.2e} norm ratio {q:.4f}" for n, e, s, q in rows))
    for n, e, s, q in rows:
        assert s < NOISE_MAX, f"{tag}: {n}: stock bf16 vs float64 {s:.3g} (must stay below {NOISE_MAX})"
        assert e <= MARGIN * s, f"{tag}: {n}: native vs float64 {e:.3g} > {MARGIN} x stock bf16 {s:.3g} " \
                                f"(norm ratio {q:.4f})"


def _run_condition(cond, loss, aux, loss2, pruned_inputs, params):
    """The backward passes of one graph condition (the same calls on the native and the stock graphs)."""
    if pruned_inputs is not None:
        before = [p.grad for p in params]
        got = torch.autograd.grad(loss, pruned_inputs, retain_graph=True)
        assert all(g is not None for g in got)
        assert all(p.grad is b for p, b in zip(params, before)), "autograd.grad touched a .grad"
        (aux if cond == "pruned_then_aux" else loss).backward()
    elif cond == "twice":
        loss.backward(retain_graph=True)
        loss.backward()
    elif cond == "two_losses":
        loss.backward(retain_graph=True)
        loss2.backward()
    else:
        loss.backward()


# ---- tail ------------------------------------------------------------------------------------------------------

SIZES = {"M65536": (16, 64, 64), "M128": (2, 8, 8)}
_VALUES = {}


def _tail_values(cuda, size):
    if size not in _VALUES:
        n, H, W = SIZES[size]
        g = torch.Generator(device=cuda).manual_seed(n * H)

        def rn(*s):
            return torch.randn(*s, generator=g, device=cuda)

        def ru(*s):
            return torch.rand(*s, generator=g, device=cuda)

        _VALUES[size] = dict(
            x=rn(n, 256, H, W).bfloat16().contiguous(memory_format=CL),
            h=rn(n, 64, H, W).bfloat16().contiguous(memory_format=CL),
            w1=(rn(64, 256, 1, 1) * 256 ** -0.5).bfloat16(), w3=(rn(256, 64, 1, 1) * 64 ** -0.5).bfloat16(),
            gamma=ru(256) + 0.5, beta=ru(256) * 0.4 - 0.2, rmean=ru(256) * 0.2 - 0.1, rvar=ru(256) + 0.5,
            wl=torch.linspace(-1, 1, n * 256 * H * W, device=cuda, dtype=torch.float64).view(n, 256, H, W),
            wa=torch.linspace(1, -1, n * 64 * H * W, device=cuda, dtype=torch.float64).view(n, 64, H, W))
    return _VALUES[size]


def _tail(cuda, size, mode, cond):
    """mode: native | stock (torch ops, bf16) | f64 (torch ops, float64). Returns (gradients, counters, output)."""
    from distributed_learning_amd.ops import bn_act
    from distributed_learning_amd.ops import conv as nconv

    v = _tail_values(cuda, size)
    dt = torch.float64 if mode == "f64" else torch.bfloat16
    pdt = torch.float64 if mode == "f64" else torch.float32
    c1 = nn.Conv2d(256, 64, 1, bias=False, device=cuda, dtype=dt).to(memory_format=CL)
    c3 = nn.Conv2d(64, 256, 1, bias=False, device=cuda, dtype=dt).to(memory_format=CL)
    bn = nn.BatchNorm2d(256, device=cuda, dtype=pdt)
    with torch.no_grad():
        c1.weight.copy_(v["w1"])
        c3.weight.copy_(v["w3"])
        bn.weight.copy_(v["gamma"])
        bn.bias.copy_(v["beta"])
        bn.running_mean.copy_(v["rmean"])
        bn.running_var.copy_(v["rvar"])
    x = v["x"].to(dt).clone().requires_grad_(True)
    h = v["h"].to(dt).clone().requires_grad_(cond != "input_nograd")
    for p in (c1.weight, c3.weight):
        p.requires_grad_(cond != "conv_frozen")
    for p in (bn.weight, bn.bias):
        p.requires_grad_(cond != "bn_frozen")
    if cond == "bn_eval":
        bn.eval()
    acc = torch.float64 if mode == "f64" else torch.float32
    before = _counters()
    with _backend(mode == "native"):
        if mode == "native":
            y1, _, ident, _ = nconv.conv1x1_fork(x, c1)
            y3, st = nconv.conv1x1(h, c3, want_stats=bn.training)
            out = bn_act.fused_bn_act(y3, bn, True, ident, st)
        else:
            y1, ident = c1(x), x.view_as(x)
            out = torch.relu(bn(c3(h)) + ident)
        if cond == "retain_ident":
            ident.retain_grad()
        sq = out.to(acc).square()
        loss = 0.5 * (sq * v["wl"].to(acc)).sum()
        aux = (y1.to(acc) * v["wa"].to(acc)).sum()
        loss2 = 0.5 * (sq * v["wl"].flip(1).to(acc)).sum() + aux
        params = (c1.weight, c3.weight, bn.weight, bn.bias)
        pruned = {"pruned_bn": [bn.weight], "pruned_conv": [c3.weight], "pruned_then_aux": [bn.weight]}.get(cond)
        _run_condition(cond, loss, aux, loss2, pruned, params)
        torch.cuda.synchronize()
    grads = {"x": _dbl(x.grad), "h": _dbl(h.grad), "conv1.weight": _dbl(c1.weight.grad),
             "conv3.weight": _dbl(c3.weight.grad), "bn.weight": _dbl(bn.weight.grad), "bn.bias": _dbl(bn.bias.grad)}
    if cond == "retain_ident":
        grads["ident"] = _dbl(ident.grad)
    return grads, _used(before), out


# the graph the stock runs execute for a condition: a pruned pass first changes nothing, so those share "plain"
_SAME_AS_PLAIN = ("pruned_bn", "pruned_conv")


def _tail_refs(cuda, refs, size, cond):
    key = ("tail", size, "plain" if cond in _SAME_AS_PLAIN else cond)
    if key not in refs:
        refs[key] = (_tail(cuda, size, "stock", key[2])[0], _tail(cuda, size, "f64", key[2])[0])
    return refs[key]


TAIL_CONDS = ["plain", "conv_frozen", "bn_frozen", "input_nograd", "pruned_bn", "pruned_conv", "pruned_then_aux",
              "twice", "two_losses", "retain_ident"]


@pytest.mark.parametrize("cond", TAIL_CONDS)
@pytest.mark.parametrize("size", list(SIZES))
def test_tail_condition_matches_float64(cuda, refs, size, cond):
    got, used, _ = _tail(cuda, size, "native", cond)
    stock, ref = _tail_refs(cuda, refs, size, cond)
    _compare(f"tail {size} {cond}", got, stock, ref)
    if cond == "plain":  # the hand-off under test was engaged where the size allows it
        assert used.get("1x1_dual_bn", 0) == (1 if size == "M65536" else 0), used
        assert used.get("1x1_fork", 0) == 1 and used.get("1x1", 0) == 1, used


@pytest.mark.parametrize("size", list(SIZES))
def test_tail_two_backwards_are_bitwise_twice_one(cuda, size):
    once, used1, _ = _tail(cuda, size, "native", "plain")
    twice, used2, _ = _tail(cuda, size, "native", "twice")
    assert used2.get("1x1_dual_bn", 0) == 2 * used1.get("1x1_dual_bn", 0), (used1, used2)
    for n, g in once.items():
        assert (g is None) == (twice[n] is None), n
        if g is not None:
            assert torch.equal(twice[n], 2 * g), n


def test_tail_eval_mode_bn_with_gradients(cuda, refs):
    """Frozen-BN fine-tuning: the eval-mode BN takes the stock path (the fused node has no eval backward)."""
    got, used, out = _tail(cuda, "M128", "native", "bn_eval")
    assert "BNAct" not in type(out.grad_fn).__name__, type(out.grad_fn).__name__
    assert used.get("1x1", 0) == 1 and used.get("1x1_fork", 0) == 1, used  # the convs stay native
    stock, ref = _tail_refs(cuda, refs, "M128", "bn_eval")
    _compare("tail M128 bn_eval", got, stock, ref)


# ---- tail with a downsample shortcut: _BNDualAct and its pair of BN hand-off links -------------------------------

def _tail_down(cuda, mode, cond):
    """``relu(bn(conv3(h)) + bn_d(conv_d(x)))`` with x forked by conv1, 64 -> 256 channels on both branches at
    M = 65536 (ResNet-50 layer1[0]): both 1x1 convs carry a link, the dual BN parks into both."""
    from distributed_learning_amd.ops import bn_act
    from distributed_learning_amd.ops import conv as nconv

    if "down" not in _VALUES:
        n, H, W = SIZES["M65536"]
        g = torch.Generator(device=cuda).manual_seed(11)
        rn = lambda *s: torch.randn(*s, generator=g, device=cuda)  # noqa: E731
        ru = lambda *s: torch.rand(*s, generator=g, device=cuda)  # noqa: E731
        _VALUES["down"] = dict(
            x=rn(n, 64, H, W).bfloat16().contiguous(memory_format=CL),
            h=rn(n, 64, H, W).bfloat16().contiguous(memory_format=CL),
            w1=(rn(64, 64, 1, 1) / 8).bfloat16(), w3=(rn(256, 64, 1, 1) / 8).bfloat16(),
            wd=(rn(256, 64, 1, 1) / 8).bfloat16(), gamma=ru(256) + 0.5, beta=ru(256) * 0.4 - 0.2,
            gamma_d=ru(256) + 0.5, beta_d=ru(256) * 0.4 - 0.2,
            wl=torch.linspace(-1, 1, n * 256 * H * W, device=cuda, dtype=torch.float64).view(n, 256, H, W))
    v = _VALUES["down"]
    f64 = mode == "f64"
    dt, pdt = (torch.float64, torch.float64) if f64 else (torch.bfloat16, torch.float32)
    c1 = nn.Conv2d(64, 64, 1, bias=False, device=cuda, dtype=dt).to(memory_format=CL)
    c3 = nn.Conv2d(64, 256, 1, bias=False, device=cuda, dtype=dt).to(memory_format=CL)
    cd = nn.Conv2d(64, 256, 1, bias=False, device=cuda, dtype=dt).to(memory_format=CL)
    bn, bnd = nn.BatchNorm2d(256, device=cuda, dtype=pdt), nn.BatchNorm2d(256, device=cuda, dtype=pdt)
    with torch.no_grad():
        for m, k in ((c1, "w1"), (c3, "w3"), (cd, "wd"), (bn, "gamma"), (bnd, "gamma_d")):
            m.weight.copy_(v[k])
        bn.bias.copy_(v["beta"])
        bnd.bias.copy_(v["beta_d"])
    x = v["x"].to(dt).clone().requires_grad_(True)
    h = v["h"].to(dt).clone().requires_grad_(True)
    before = _counters()
    with _backend(mode == "native"):
        if mode == "native":
            _, _, ident, _ = nconv.conv1x1_fork(x, c1)
            y3, st = nconv.conv1x1(h, c3, want_stats=True)
            yd, std = nconv.conv1x1(ident, cd, want_stats=True)
            out = bn_act.fused_bn_add_bn_act(y3, bn, yd, bnd, True, st, std)
        else:
            out = torch.relu(bn(c3(h)) + bnd(cd(x)))
        acc = torch.float64 if f64 else torch.float32
        loss = 0.5 * (out.to(acc).square() * v["wl"].to(acc)).sum()
        params = (c1.weight, c3.weight, cd.weight, bn.weight, bn.bias, bnd.weight, bnd.bias)
        pruned = {"pruned_bn": [bn.weight], "pruned_down_bn": [bnd.weight], "pruned_conv": [c3.weight]}.get(cond)
        _run_condition(cond, loss, None, None, pruned, params)
        torch.cuda.synchronize()
    grads = {"x": _dbl(x.grad), "h": _dbl(h.grad)}
    grads.update((k, _dbl(p.grad)) for k, p in zip(("conv1.weight", "conv3.weight", "down.weight", "bn.weight",
                                                    "bn.bias", "down_bn.weight", "down_bn.bias"), params))
    return grads, _used(before)


@pytest.mark.parametrize("cond", ["plain", "pruned_bn", "pruned_down_bn", "pruned_conv", "twice"])
def test_tail_with_downsample_matches_float64(cuda, refs, cond):
    got, used = _tail_down(cuda, "native", cond)
    key = ("down", "twice" if cond == "twice" else "plain")
    if key not in refs:
        refs[key] = (_tail_down(cuda, "stock", key[1])[0], _tail_down(cuda, "f64", key[1])[0])
    _compare(f"tail+downsample {cond}", got, *refs[key])
    if cond == "plain":  # the dual BN handed both applies to the convs' one-pass kernels
        assert used.get("1x1_dual_bn", 0) == 2, used


# ---- stem ------------------------------------------------------------------------------------------------------

def _stem(cuda, mode, cond):
    from distributed_learning_amd.ops import nn as dnn

    if "stem" not in _VALUES:
        g = torch.Generator(device=cuda).manual_seed(3)
        _VALUES["stem"] = dict(
            x=torch.randint(-1, 2, (2, 3, 32, 32), generator=g, device=cuda).bfloat16().contiguous(memory_format=CL),
            w=(torch.randint(-1, 2, (64, 3, 7, 7), generator=g, device=cuda) / 8).bfloat16(),
            gamma=torch.rand(64, generator=g, device=cuda) + 0.5, beta=torch.rand(64, generator=g, device=cuda) - 0.5,
            wl=torch.linspace(-1, 1, 2 * 64 * 8 * 8, device=cuda, dtype=torch.float64).view(2, 64, 8, 8))
    v = _VALUES["stem"]
    dt = torch.float64 if mode == "f64" else torch.bfloat16
    conv = nn.Conv2d(3, 64, 7, 2, 3, bias=False, device=cuda, dtype=dt).to(memory_format=CL)
    bn = nn.BatchNorm2d(64, device=cuda, dtype=torch.float64 if mode == "f64" else torch.float32)
    pool = nn.MaxPool2d(3, 2, 1)
    with torch.no_grad():
        conv.weight.copy_(v["w"])
        bn.weight.copy_(v["gamma"])
        bn.bias.copy_(v["beta"])
    x = v["x"].to(dt).clone().requires_grad_(cond == "image_grad")
    acc = torch.float64 if mode == "f64" else torch.float32
    before = _counters()
    with _backend(mode == "native"):
        out = dnn.conv_bn_act_maxpool(x, conv, bn, pool)
        assert out.shape == (2, 64, 8, 8)
        loss = 0.5 * (out.to(acc).square() * v["wl"].to(acc)).sum()
        params = (conv.weight, bn.weight, bn.bias)
        _run_condition(cond, loss, None, None, {"pruned_bn": [bn.weight], "pruned_conv": [conv.weight]}.get(cond),
                       params)
        torch.cuda.synchronize()
    grads = {"image": _dbl(x.grad), "conv.weight": _dbl(conv.weight.grad), "bn.weight": _dbl(bn.weight.grad),
             "bn.bias": _dbl(bn.bias.grad)}
    return grads, _used(before)


@pytest.mark.parametrize("cond", ["plain", "pruned_bn", "pruned_conv", "twice", "image_grad"])
def test_stem_condition_matches_float64(cuda, refs, cond):
    got, used = _stem(cuda, "native", cond)
    key = ("stem", "plain" if cond in _SAME_AS_PLAIN else cond)
    if key not in refs:
        refs[key] = (_stem(cuda, "stock", key[1])[0], _stem(cuda, "f64", key[1])[0])
    _compare(f"stem {cond}", got, *refs[key])
    if cond == "plain":
        assert used.get("stem", 0) == 1 and used.get("stem_bn", 0) == 1, used
    if cond == "image_grad":  # the native stem conv has no input gradient: the stock conv runs, the image gets one
        assert used.get("stem", 0) == 0 and got["image"] is not None, used


# ---- model -----------------------------------------------------------------------------------------------------

def _model(cuda, name, mode, cond="plain", observer=None, defer=True, fill=False, bitwise=False, handoffs=True):
    """One forward (+ the condition's backward passes) of resnet50 at 4x3x64x64 / resnet18 at 2x3x64x64.
    ``handoffs=False``: no link between autograd nodes carries anything (stem and 1x1 BN hand-offs, the residual
    hand-off to the fork and the deferred apply all off). Returns a dict: logits, gradients by name, what the
    observers saw, buffers, counters."""
    from distributed_learning_amd import knobs
    from distributed_learning_amd.models import resnet as R
    from distributed_learning_amd.ops import _ext, bn_act
    from distributed_learning_amd.ops import conv as nconv
    from distributed_learning_amd.ops import nn as dnn

    defer = defer and handoffs
    switches = (nconv.STEM_BN, nconv.DUAL_BN, nconv.RESIDUAL_HANDOFF)
    nconv.STEM_BN, nconv.DUAL_BN, nconv.RESIDUAL_HANDOFF = (s and handoffs for s in switches)

    C = _ext.require()
    torch.manual_seed(0)
    model = getattr(R, name)(num_classes=10).to(cuda).to(memory_format=CL)
    dnn.bf16_weights(model)
    n = 4 if name == "resnet50" else 2
    x = torch.randn(n, 3, 64, 64, device=cuda).bfloat16().contiguous(memory_format=CL)
    if mode == "f64":
        model, x = model.double(), x.double()
    x.requires_grad_(cond == "image_grad")
    body = [p for k, p in model.named_parameters() if not k.startswith("fc.")]
    convs = [m.weight for m in model.modules() if isinstance(m, nn.Conv2d)]
    bns = [p for m in model.modules() if isinstance(m, nn.BatchNorm2d) for p in (m.weight, m.bias)]
    early = [p for k, p in model.named_parameters() if k.split(".")[0] in ("conv1", "bn1", "layer1")]
    for p in {"conv_frozen": convs, "bn_frozen": bns, "early_frozen": early, "fc_only": body}.get(cond, ()):
        p.requires_grad_(False)
    if cond == "bn_eval":
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eval()
    blk = model.layer1[1] if name == "resnet50" else model.layer2[1]  # a block with an identity shortcut
    pruned = {"pruned_bn": [blk.bn3.weight if name == "resnet50" else blk.bn2.weight],
              "pruned_stem_bn": [model.bn1.weight],
              "pruned_conv": [blk.conv3.weight if name == "resnet50" else blk.conv2.weight],
              "pruned_fc": [model.fc.weight]}.get(cond)
    seen, handles = [], []

    def record(t):
        seen.append(t.detach().float().clone())

    if observer == "layer1_hook":
        handles.append(model.layer1.register_forward_hook(lambda m, i, o: record(o)))
    elif observer == "next_block_pre_hook":
        handles.append(model.layer2[0].register_forward_pre_hook(lambda m, i: record(i[0])))
    elif observer == "global_pre_hook":
        handles.append(nn.modules.module.register_module_forward_pre_hook(
            lambda m, i: record(i[0]) if isinstance(m, R.Bottleneck) else None))
    elif observer == "global_hook":
        handles.append(nn.modules.module.register_module_forward_hook(
            lambda m, i, o: record(o) if isinstance(m, R.Bottleneck) else None))
    elif observer in ("block_noop_hook", "block_grad_hook"):  # a gradient observer installed from a forward hook
        def watch(m, i, o):
            if observer == "block_grad_hook":
                o.retain_grad()
                o.register_hook(record)
                seen.append(o)
        handles.append(model.layer1[1].register_forward_hook(watch))
    knobs._CACHE["DEFER_APPLY"] = "1" if defer else "0"
    knobs._CACHE["DEFER_MID"] = "0"
    if bitwise:  # the same statistics tiles with and without the deferral (as tests/test_gpu_gemm_apply.py)
        C.set_tile256_min_k_stats(1 << 30)
    if fill:  # every allocation NaN-filled: a tensor read before it is written shows
        torch.use_deterministic_algorithms(True, warn_only=True)
        torch.utils.deterministic.fill_uninitialized_memory = True
    before = _counters()
    try:
        with _backend(mode == "native"), torch.set_grad_enabled(cond != "no_grad"):
            out = model(x)
            bn_act.flush_bn_counters()
            pending = bn_act.pending_of(out)
            if cond != "no_grad":
                o = out.double() if mode == "f64" else out.float()
                w = torch.linspace(-1, 1, o.numel(), device=cuda, dtype=o.dtype).view(o.shape)
                loss, loss2 = (o * w).sum(), (o * w.flip(1)).square().sum()
                _run_condition(cond, loss, None, loss2, pruned, list(model.parameters()))
            torch.cuda.synchronize()
    finally:
        for hd in handles:
            hd.remove()
        C.set_tile256_min_k_stats(-1)
        torch.use_deterministic_algorithms(False)
        nconv.STEM_BN, nconv.DUAL_BN, nconv.RESIDUAL_HANDOFF = switches
    grads = {k: _dbl(p.grad) for k, p in model.named_parameters()}
    grads["image"] = _dbl(x.grad)
    if observer == "block_grad_hook":
        grads["observed.hook"], grads["observed.retained"] = _dbl(seen[1]), _dbl(seen[0].grad)
        seen = []
    return dict(logits=out.detach().float().clone(), grads=grads, seen=seen, pending=pending,
                buffers={k: b.detach().clone() for k, b in model.named_buffers()}, used=_used(before))


def _none_pattern_and_finite(tag, got, ref):
    for k, r in ref.items():
        assert (got[k] is None) == (r is None), f"{tag}: {k} is {'None' if got[k] is None else 'set'}, the " \
                                                 f"float64 reference's is {'None' if r is None else 'set'}"
        if r is not None:
            assert torch.isfinite(got[k]).all() and float(got[k].abs().max()) > 0, f"{tag}: {k}"


def _bitwise(tag, a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert (a[k] is None) == (b[k] is None), f"{tag}: {k}"
        assert a[k] is None or torch.equal(a[k], b[k]), f"{tag}: {k} differs"


@pytest.mark.parametrize("name", ["resnet50", "resnet18"])
def test_model_plain_step_engages_the_handoffs(cuda, refs, name):
    r = refs[("model", name, "plain")] = _model(cuda, name, "native")
    assert r["used"].get("stem_bn", 0) == 1, r["used"]
    if name == "resnet50":
        assert r["used"].get("deferred", 0) == 15 and r["used"].get("1x1_apply", 0) > 0, r["used"]
    _none_pattern_and_finite(name, r["grads"], _model(cuda, name, "f64")["grads"])


STEM_WGRAD_BOUND = (1e-5 * 2 ** -8) ** 0.5  # 2.0e-4, see _same_values


def _same_values(tag, got, ref, passes=1):
    """Gradients of two native runs whose forwards are bitwise equal, so that every ReLU and max-pool decision is
    the same: bitwise equal wherever the same kernels ran on the same values. The exception is conv1.weight. Its
    gradient sums the same bf16 dY values in fp32 in an order that is not fixed: the stem weight gradient with the
    BN apply fused against the unfused one, and, where the image needs a gradient, the stock conv's weight
    gradient from run to run. The fp32 sums differ by at most d = 1e-5 relative (the kernel-level bound of
    tests/test_gpu_stem_bn_fused.py); rounding them to the bf16 weight gradient turns that into a different bf16
    value for a fraction d / u of the elements (u = 2^-8, the bf16 spacing) at a cost of u each: relative L2
    sqrt(d * u) = 2.0e-4 per backward pass, sqrt(passes) times that where passes accumulate."""
    assert got.keys() == ref.keys()
    worst = (0.0, "")
    for k, r in ref.items():
        assert (got[k] is None) == (r is None), f"{tag}: {k} is {'None' if got[k] is None else 'set'}, the " \
                                                 f"run without hand-offs has {'None' if r is None else 'a value'}"
        if r is not None:
            assert torch.isfinite(r).all() and float(r.norm()) > 0, f"{tag}: {k}"
            worst = max(worst, (float((got[k] - r).norm() / r.norm()), k))
    print(f"{tag}: largest relative L2 difference {worst[0]:.3g} ({worst[1]})")
    for k, r in ref.items():
        if r is not None and k == "conv1.weight":
            rel = float((got[k] - r).norm() / r.norm())
            assert rel <= STEM_WGRAD_BOUND * passes ** 0.5, f"{tag}: {k} differs by {rel:.3g}"
        elif r is not None:
            assert torch.equal(got[k], r), f"{tag}: {k} differs by {float((got[k] - r).norm() / r.norm()):.3g}"


@pytest.mark.parametrize("cond", ["plain", "conv_frozen", "bn_frozen", "early_frozen", "fc_only", "image_grad",
                                  "two_losses", "twice", "bn_eval"])
@pytest.mark.parametrize("name", ["resnet50", "resnet18"])
def test_model_condition_gives_the_gradients_of_the_run_without_handoffs(cuda, name, cond):
    """Every gradient of every condition against the same condition with nothing handed between autograd nodes;
    a gradient is None exactly where the float64 run of the condition on stock torch has none."""
    on = _model(cuda, name, "native", cond, bitwise=True)
    off = _model(cuda, name, "native", cond, bitwise=True, handoffs=False)
    assert not any(off["used"].get(k, 0) for k in ("stem_bn", "1x1_dual_bn", "deferred", "1x1_apply")), off["used"]
    assert torch.equal(on["logits"], off["logits"])
    _same_values(f"{name} {cond}", on["grads"], off["grads"], 2 if cond in ("two_losses", "twice") else 1)
    _none_pattern_and_finite(f"{name} {cond}", on["grads"], _model(cuda, name, "f64", cond)["grads"])
    if cond == "image_grad":
        assert on["used"].get("stem", 0) == 0, on["used"]
    if cond == "bn_eval":
        assert on["used"].get("deferred", 0) == 0, on["used"]


@pytest.mark.parametrize("cond", ["conv_frozen", "bn_frozen", "early_frozen", "fc_only"])
@pytest.mark.parametrize("name", ["resnet50", "resnet18"])
def test_model_frozen_parameters_leave_the_other_gradients_as_they_are(cuda, refs, name, cond):
    """Freezing parameters only omits work: what is still computed is bitwise the plain step's (conv1.weight as
    in _same_values)."""
    got, plain = _model(cuda, name, "native", cond)["grads"], _plain(cuda, refs, name)["grads"]
    kept = {k: v for k, v in got.items() if v is not None}
    assert kept and len(kept) < sum(v is not None for v in plain.values())
    _same_values(f"{name} {cond} vs plain", kept, {k: plain[k] for k in kept})


def _plain(cuda, refs, name):
    key = ("model", name, "plain")
    if key not in refs:
        refs[key] = _model(cuda, name, "native")
    return refs[key]


@pytest.mark.parametrize("cond", ["pruned_bn", "pruned_stem_bn", "pruned_conv", "pruned_fc"])
@pytest.mark.parametrize("name", ["resnet50", "resnet18"])
def test_model_pruned_pass_then_full_backward_is_bitwise_the_plain_step(cuda, refs, name, cond):
    """The full backward after a pruned pass runs the plain step's kernels on the plain step's inputs: whatever
    the pruned pass left in a link must not reach it."""
    got = _model(cuda, name, "native", cond)
    _bitwise(f"{name} {cond}", got["grads"], _plain(cuda, refs, name)["grads"])


@pytest.mark.parametrize("name", ["resnet50", "resnet18"])
def test_model_two_backwards_are_bitwise_twice_one(cuda, refs, name):
    once, twice = _plain(cuda, refs, name)["grads"], _model(cuda, name, "native", "twice")["grads"]
    _bitwise(f"{name} twice", twice, {k: None if g is None else 2 * g for k, g in once.items()})


# observer -> (tensors it sees, block outputs still deferred of 15). The pre-hook on layer2[0] stops layer1[2]
# (whose output it is handed) and, by the block's guard on its own hooks, layer2[0] itself.
OBSERVERS = {"layer1_hook": (1, 14), "next_block_pre_hook": (1, 13), "global_pre_hook": (16, 0),
             "global_hook": (16, 0)}


@pytest.mark.parametrize("observer", list(OBSERVERS))
def test_forward_observers_see_written_block_outputs(cuda, observer):
    """Whoever is handed a block output inside ResNet.forward sees what the step without the deferral gives it
    (bitwise, every allocation NaN-filled), and only the blocks it can see stop deferring."""
    on = _model(cuda, "resnet50", "native", observer=observer, defer=True, fill=True, bitwise=True)
    off = _model(cuda, "resnet50", "native", observer=observer, defer=False, fill=True, bitwise=True)
    count, deferred = OBSERVERS[observer]
    assert len(on["seen"]) == len(off["seen"]) == count
    assert on["used"].get("deferred", 0) == deferred and off["used"].get("deferred", 0) == 0, (on["used"], off["used"])
    for i, (a, b) in enumerate(zip(on["seen"], off["seen"])):
        assert torch.isfinite(b).all() and torch.equal(a, b), f"{observer}: observed tensor {i} differs"
    assert torch.equal(on["logits"], off["logits"])
    _bitwise(observer, on["grads"], off["grads"])


def test_gradient_observer_installed_by_a_forward_hook(cuda):
    """A forward hook on a bottleneck that puts retain_grad() and a tensor hook on the block output: both see the
    gradient the run without hand-offs shows them (the sum of the next block's conv1 data gradient and its identity
    gradient, there delivered to the fork as a tensor instead of a (gradient, mask) pair), and observing changes no
    parameter gradient."""
    seen = _model(cuda, "resnet50", "native", observer="block_grad_hook", bitwise=True)
    base = _model(cuda, "resnet50", "native", observer="block_noop_hook", bitwise=True)
    off = _model(cuda, "resnet50", "native", observer="block_grad_hook", bitwise=True, handoffs=False)
    g = seen["grads"]
    assert g["observed.hook"] is not None and torch.equal(g["observed.hook"], g["observed.retained"])
    assert torch.isfinite(g["observed.hook"]).all() and float(g["observed.hook"].abs().max()) > 0
    _bitwise("gradient observer", {k: v for k, v in g.items() if not k.startswith("observed.")}, base["grads"])
    _same_values("gradient observer vs no hand-offs", g, off["grads"])


def test_training_forward_under_no_grad(cuda):
    """Outputs and running statistics bitwise those of the grad-enabled forward; nothing left pending."""
    a = _model(cuda, "resnet50", "native", "no_grad", bitwise=True)
    b = _model(cuda, "resnet50", "native", bitwise=True)
    assert a["pending"] is None and b["pending"] is None
    assert a["used"].get("deferred", 0) == 0 and b["used"].get("deferred", 0) > 0
    assert torch.equal(a["logits"], b["logits"])
    _bitwise("buffers", a["buffers"], b["buffers"])
    assert int(a["buffers"]["bn1.num_batches_tracked"]) == 1
    assert all(v is None for v in a["grads"].values())


# ---- fp32 convs the native path must hand to the stock one ------------------------------------------------------

@pytest.mark.parametrize("cin,cout,pad", [(3, 16, 1), (8, 8, 3)])
def test_conv_f32_unserved_shapes_take_the_stock_path(cuda, cin, cout, pad):
    """3 input channels with an input gradient (its data gradient would have 3 output channels) and a padding
    above kernel - 1 (a negative data-gradient padding): forward and backward complete and match float64 to fp32
    summation error (1e-5, the bound of tests/test_gpu_conv_f32.py)."""
    from distributed_learning_amd.ops import conv_f32
    from distributed_learning_amd.ops import nn as dnn

    g = torch.Generator().manual_seed(cin + pad)
    conv = nn.Conv2d(cin, cout, 3, padding=pad, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (cin * 9) ** -0.5)
    conv = conv.to(cuda).to(memory_format=CL)
    x = torch.randn(2, cin, 8, 8, generator=g).to(cuda).contiguous(memory_format=CL).requires_grad_(True)
    assert not conv_f32.supported(x, conv)
    dnn.set_native_conv_f32(True)
    with _backend(True):
        y = dnn._conv(x, conv)
        dy = torch.randn(y.shape, generator=g).to(cuda)
        y.backward(dy)
        torch.cuda.synchronize()
    xd = x.detach().double().requires_grad_(True)
    wd = conv.weight.detach().double().requires_grad_(True)
    yd = torch.nn.functional.conv2d(xd, wd, None, 1, pad)
    yd.backward(dy.double())
    for n, a, b in (("y", y, yd), ("dx", x.grad, xd.grad), ("dw", conv.weight.grad, wd.grad)):
        rel = float((a.detach().double() - b.detach()).norm() / b.detach().norm())
        assert rel < 1e-5, f"{n}: {rel:.3g}"
