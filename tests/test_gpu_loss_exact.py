"""The three cross-entropy kernel pairs of csrc/kernels/loss.hip against the interval and replay oracle of
tests/loss_oracle.py (criteria and their derivation there; tests/test_loss_oracle.py checks the oracle on the CPU).

Inputs (``loss_oracle.case_names()``), each for the plain pair and for the metrics and mix pairs at eps 0 and 0.1,
in fp32 and bf16, with gout cycling through 1, -0.375 and 1024:
  sweep       16 rows at every class count where the row walk changes: one 16-byte vector, one in every lane, one
              lane with a second, a full first trip of 256 vectors, one vector in the second trip, a third trip;
              C = 1, 63, 64, 65, 1001 (2049) off the 16-byte pitch (64 is on it); C = 2056 one element off alignment.
              Targets at column 0, C - 1, every position of the last vector, inside a second-trip vector; rows 12 and
              13 ignored (-100, >= C), for mix also row 14 by its second target alone.
  rows        B = 1, 4, 5, 255, 256, 257, 513, 1283 at C = 40 and 1283 x 520 (past the plain backward's 2048 x 256
              grid-stride span): the batch kernel's second to sixth trip. Ignored: the first row of a 4-row block,
              the last row of one, a whole block.
  ignored     every row ignored: the mean is NaN, the gradient +0.0.
  structured  ascending (every visit a new maximum), descending, constant, one +80 among -20s, all near -1e4, a
              spread above 104, -inf but for a few columns (whole lanes and vectors of -inf; for mix a -inf logit at
              a weight-0 target), integers in [-16, 16]; once on the 16-byte path with a second trip, once at C = 1001.
  nan         a NaN target logit: rank +inf.
Mix rows cycle lam through 0, 1, 0.5 and random values; every fifth row has ta == tb.

The bindings are called directly (they return the per-row workspace); the public functions are held to the
bindings bit for bit under ``(loss * s).backward()``.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import loss_oracle as lo

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
WORST = {}


def _ext():
    from distributed_learning_amd.ops import _ext as e

    return e.require()


def _logits(c, cuda):
    x = torch.tensor(c.x).to(DT[c.dt])  # a copy: the shared inputs are read-only
    if not c.off:
        return x.to(cuda)
    view = torch.empty(c.B * c.C + c.off, device=cuda, dtype=DT[c.dt])[c.off:].view(c.B, c.C)
    view.copy_(x)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


def run_bindings(c, cuda):
    """One forward and one backward through the bindings; the outputs as loss_oracle.criteria reads them."""
    C = _ext()
    x = _logits(c, cuda)
    ta = torch.tensor(c.ta).to(cuda)
    gout = torch.tensor([c.gout], device=cuda)
    B = c.B
    if c.pair == "plain":
        loss, ws = C.xent_fwd(x, ta)
        grad = C.xent_bwd(x, ta, ws, loss, gout)
        sums, mean, per = loss, loss[0], 3
    elif c.pair == "metrics":
        sums, ws = C.xent_metrics_fwd(x, ta, c.eps, c.k)
        grad = C.xent_smooth_bwd(x, ta, ws, sums, gout, c.eps)
        mean, per = ws[-1], 4
    else:
        tb, lam = torch.tensor(c.tb).to(cuda), torch.tensor(c.lam).to(cuda)
        sums, ws = C.xent_mix_fwd(x, ta, tb, lam, c.eps)
        grad = C.xent_mix_bwd(x, ta, tb, lam, ws, sums, gout, c.eps)
        mean, per = ws[-1], 3
    assert grad.dtype == x.dtype and grad.shape == x.shape
    w = ws.cpu().numpy()
    return SimpleNamespace(lse=w[:B], row=w[B:2 * B], valid=w[2 * B:3 * B], rank=w[3 * B:4 * B] if per == 4 else None,
                           sums=sums.cpu().numpy(), mean=np.float32(mean.cpu().numpy()),
                           grad=grad.float().cpu().numpy()), x, grad


@pytest.mark.parametrize("name", lo.case_names())
def test_case_meets_every_criterion(cuda, name):
    c = lo.get_case(name)
    out, _, _ = run_bindings(c, cuda)
    fails, ratios = lo.criteria(c, out)
    print(name, " ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    for k, v in ratios.items():
        key = (k, c.dt)
        WORST[key] = max(WORST.get(key, 0.0), v)
    assert not fails, f"{name}: " + "; ".join(fails)
    if c.kind == "ignored":
        assert np.isnan(out.mean) and not out.grad.view(np.uint32).any()


def test_worst_ratios_are_reported(cuda):
    """Prints the worst error-to-bound ratio per quantity and dtype of the cases above (the record's figures)."""
    for (k, dt), v in sorted(WORST.items()):
        print(f"worst {k} {dt}: {v:.4g} of its bound")
    assert all(v <= 1.0 for v in WORST.values())


PUBLIC = ["sweep-16x1028-f32-{}", "sweep-16x2056-bf16-{}", "rows-513x40-f32-{}", "sweep-16x65-bf16-{}"]


@pytest.mark.parametrize("s", [-0.375, 1024.0])
@pytest.mark.parametrize("pair", ["plain-eps0", "metrics-eps0.1", "mix-eps0.1"])
def test_public_functions_scale_the_gradient(cuda, pair, s):
    """(loss * s).backward() through the public functions is the binding's gradient at gout = s, bit for bit, and
    the loss is the binding's mean: s * 1 is exact, so gout arrives as s."""
    from distributed_learning_amd.ops import cross_entropy, cross_entropy_mix, cross_entropy_with_metrics

    for pattern in PUBLIC:
        c = lo.get_case(pattern.format(pair))
        c.gout = s
        out, x, grad = run_bindings(c, cuda)
        xr = x.detach().clone().requires_grad_(True)
        ta = torch.tensor(c.ta).to(cuda)
        if c.pair == "plain":
            loss = cross_entropy(xr, ta)
        elif c.pair == "metrics":
            loss = cross_entropy_with_metrics(xr, ta, c.eps, c.k)[0]
        else:
            loss = cross_entropy_mix(xr, ta, torch.tensor(c.tb).to(cuda), torch.tensor(c.lam).to(cuda), c.eps)
        (loss * s).backward()
        assert float(loss.detach()) == float(out.mean)
        assert torch.equal(xr.grad, grad) and bool(xr.grad.ne(0).any())


# ------------------------------------------------------------------------------------------------- the plain pair's binding
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_plain_loss_takes_a_strided_target(cuda, dtype):
    """Every second label of a longer vector: the loss and gradient of the labels it names, not of the first B."""
    from distributed_learning_amd.ops import cross_entropy

    g = torch.Generator().manual_seed(3)
    x = (torch.randn(37, 50, generator=g) * 3).to(cuda, dtype)
    labels = torch.randint(0, 50, (74,), generator=g).to(cuda)
    labels[4] = -100
    strided = labels[::2]
    assert not strided.is_contiguous() and not torch.equal(strided, labels[:37])
    grads = []
    for t in (strided, strided.contiguous()):
        xr = x.clone().requires_grad_(True)
        loss = cross_entropy(xr, t)
        loss.backward()
        grads.append((loss.detach(), xr.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    ref = torch.nn.functional.cross_entropy(x.double().cpu(), strided.cpu(), ignore_index=-100)
    torch.testing.assert_close(grads[0][0].double().cpu(), ref, rtol=1e-5, atol=1e-5)


def test_plain_binding_checks(cuda):
    C = _ext()
    x = torch.zeros(4, 10, device=cuda)
    y = torch.zeros(4, dtype=torch.long, device=cuda)
    loss, ws = C.xent_fwd(x, y)
    assert loss.shape == (2,) and ws.shape == (12,) and float(loss[1]) == 4.0
    g = torch.ones(1, device=cuda)
    assert C.xent_bwd(x, y, ws, loss, g).shape == x.shape
    y8 = torch.zeros(8, dtype=torch.long, device=cuda)
    for bad in (lambda: C.xent_fwd(x, y[:3]), lambda: C.xent_fwd(x.cpu(), y), lambda: C.xent_fwd(x, y.cpu()),
                lambda: C.xent_fwd(x.half(), y), lambda: C.xent_fwd(x.t(), y), lambda: C.xent_fwd(x, y.int()),
                lambda: C.xent_fwd(x, y8[::2]), lambda: C.xent_fwd(x[:, :0], y), lambda: C.xent_fwd(x[0], y[:1]),
                lambda: C.xent_bwd(x, y8[::2], ws, loss, g), lambda: C.xent_bwd(x.t(), y, ws, loss, g),
                lambda: C.xent_bwd(x, y, ws[:5], loss, g), lambda: C.xent_bwd(x, y, ws, loss[:1], g),
                lambda: C.xent_bwd(x, y, ws.double(), loss, g), lambda: C.xent_bwd(x, y, ws, loss, g.cpu()),
                lambda: C.xent_bwd(x, y, ws, loss, torch.ones(2, device=cuda)),
                lambda: C.xent_bwd(x[:, :0], y, ws, loss, g)):
        with pytest.raises(RuntimeError):
            bad()


def test_empty_batch_launches_no_row_kernel(cuda):
    """B = 0: NaN and a count of 0 from the batch kernel, an empty gradient, and no launch error left behind."""
    C = _ext()
    x = torch.zeros(0, 10, device=cuda)
    y = torch.zeros(0, dtype=torch.long, device=cuda)
    loss, ws = C.xent_fwd(x, y)
    d = C.xent_bwd(x, y, ws, loss, torch.ones(1, device=cuda))
    torch.cuda.synchronize()
    assert torch.isnan(loss[0]) and float(loss[1]) == 0.0 and ws.numel() == 0 and d.shape == (0, 10)
    loss, _ = C.xent_fwd(torch.zeros(2, 10, device=cuda), torch.zeros(2, dtype=torch.long, device=cuda))
    torch.cuda.synchronize()
    assert float(loss[1]) == 2.0
