"""The pair-target (Mixup / CutMix) cross-entropy ``ops.cross_entropy_mix``: the torch fallback on the CPU, and the
cases and oracle shared with tests/test_gpu_loss_mix.py.

Oracle: float64 ``lam * CE_eps(x, ta) + (1 - lam) * CE_eps(x, tb)`` per row from
``F.cross_entropy(reduction="none")``, the mean over the rows whose targets are both valid, and its autograd
gradient. Bounds: ``LOSS_TOL`` and ``GRAD_TOL`` of tests/test_loss_metrics.py, the project's existing ones.

Inputs: ``lam ~ Beta(0.2, 0.2)`` (a seeded Gamma ratio) with an exact 0 and an exact 1 planted, rows with
``ta == tb``, and rows ignored through either target (-100 or >= C).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from test_loss_metrics import GRAD_TOL, LOSS_TOL, make_case

SHAPES = [(3, 10), (4, 8), (5, 1000), (129, 4097), (256, 1000)]


def make_mix_case(B, C, dtype=torch.float32, seed=0, scale=3.0, ignore=True):
    """(logits, target_a, target_b, lam) on the CPU. ``target_a`` carries make_case's ignored rows (1 and 3);
    ``target_b`` ignores row 2 (-100) and row 5 (>= C) of larger batches; rows 0 and 4 have ta == tb; the last
    two rows have lam = 1 and lam = 0."""
    x, ta = make_case(B, C, dtype, seed, scale, ignore)
    g = torch.Generator().manual_seed(seed + 1000)
    tb = torch.randint(0, C, (B,), generator=g)
    gam = torch._standard_gamma(torch.full((B, 2), 0.2, dtype=torch.float64), generator=g)
    lam = (gam[:, 0] / gam.sum(dim=1).clamp_min(1e-300)).to(torch.float32)
    tb[0] = ta[0]
    if B > 4:
        tb[4] = ta[4]
    if ignore and B > 5:
        tb[2], tb[5] = -100, C
    lam[-2], lam[-1] = 1.0, 0.0
    return x, ta, tb, lam


def oracle_loss_grad(x, ta, tb, lam, eps):
    """float64 loss and gradient of the stored logits."""
    C = x.shape[1]
    x64 = x.detach().double().cpu().requires_grad_(True)
    ta, tb, lam64 = ta.cpu(), tb.cpu(), lam.detach().cpu().double()
    valid = (ta >= 0) & (ta < C) & (tb >= 0) & (tb < C)
    ca = F.cross_entropy(x64, torch.where(valid, ta, torch.zeros_like(ta)), reduction="none", label_smoothing=eps)
    cb = F.cross_entropy(x64, torch.where(valid, tb, torch.zeros_like(tb)), reduction="none", label_smoothing=eps)
    row = lam64 * ca + (1.0 - lam64) * cb
    loss = torch.where(valid, row, torch.zeros_like(row)).sum() / valid.sum()
    loss.backward()
    return loss.detach(), x64.grad, int(valid.sum())


def check_against_oracle(x, ta, tb, lam, eps, dtype):
    """Run cross_entropy_mix on the tensors where they live and compare loss and gradient with the oracle."""
    from distributed_learning_amd.ops import cross_entropy_mix

    xr = x.detach().requires_grad_(True)  # the same storage: a test may depend on its alignment
    loss = cross_entropy_mix(xr, ta, tb, lam, eps)
    loss.backward()
    assert loss.dim() == 0 and xr.grad.dtype == x.dtype and xr.grad.shape == x.shape
    ref, gref, n = oracle_loss_grad(x, ta, tb, lam, eps)
    assert 0 < n
    print(f"loss err {abs(float(loss.detach()) - float(ref)):.3g}, worst grad err "
          f"{float((xr.grad.double().cpu() - gref).abs().max()):.3g}, {n} valid rows")
    torch.testing.assert_close(loss.detach().double().cpu(), ref, **LOSS_TOL)
    torch.testing.assert_close(xr.grad.double().cpu(), gref, **GRAD_TOL[dtype])
    return loss.detach(), xr.grad


def check_unit_weights_equal_the_single_target_loss(x, ta, tb, eps):
    """lam == 1 everywhere with tb valid but different from ta: loss and gradient equal
    cross_entropy_with_metrics(x, ta) bit for bit; lam == 0: the same with tb."""
    from distributed_learning_amd.ops import cross_entropy_mix, cross_entropy_with_metrics

    B = x.shape[0]
    assert bool((ta != tb).any())
    for lam_value, t in ((1.0, ta), (0.0, tb)):
        lam = torch.full((B,), lam_value, device=x.device)
        xm, xs = x.detach().clone().requires_grad_(True), x.detach().clone().requires_grad_(True)
        lm = cross_entropy_mix(xm, ta, tb, lam, eps)
        ls = cross_entropy_with_metrics(xs, t, eps)[0]
        lm.backward()
        ls.backward()
        assert torch.equal(lm.detach(), ls.detach()), (lam_value, float(lm), float(ls))
        assert torch.equal(xm.grad, xs.grad), lam_value


def check_minus_inf_at_a_weightless_target(device, dtype=torch.float32):
    """A -inf logit at the class of a target whose weight is exactly 0 adds nothing: the loss stays finite and
    equals the oracle's, which never touches that class."""
    from distributed_learning_amd.ops import cross_entropy_mix

    x, ta, tb, _ = make_mix_case(6, 40, dtype, seed=8, ignore=False)
    tb = (ta + 1) % 40
    lam = torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0, 0.0])
    x = x.clone()
    for i in range(6):
        x[i, (tb if lam[i] == 1 else ta)[i]] = float("-inf")
    for eps in (0.0,):  # with smoothing every class has weight eps / C > 0 and a -inf logit is an infinite loss
        xr = x.to(device).requires_grad_(True)
        loss = cross_entropy_mix(xr, ta.to(device), tb.to(device), lam.to(device), eps)
        loss.backward()
        assert torch.isfinite(loss) and torch.isfinite(xr.grad).all()
        t = torch.where(lam == 1, ta, tb)
        torch.testing.assert_close(loss.detach().double().cpu(), F.cross_entropy(x.double(), t), **LOSS_TOL)


# --- the fallback ----------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,C", SHAPES)
def test_fallback_matches_oracle(B, C, eps):
    x, ta, tb, lam = make_mix_case(B, C)
    check_against_oracle(x, ta, tb, lam, eps, torch.float32)


def test_fallback_float64_and_bf16_inputs():
    x, ta, tb, lam = make_mix_case(64, 100, seed=3)
    loss, _ = check_against_oracle(x.double(), ta, tb, lam, 0.1, torch.float32)
    assert loss.dtype == torch.float64
    xb, ta, tb, lam = make_mix_case(64, 100, torch.bfloat16, seed=4)
    check_against_oracle(xb, ta, tb, lam, 0.1, torch.bfloat16)


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_fallback_unit_weights(eps):
    x, ta, tb, _ = make_mix_case(33, 50, seed=5, ignore=False)
    check_unit_weights_equal_the_single_target_loss(x, ta, (tb + (tb == ta)) % 50, eps)


def test_fallback_minus_inf_at_a_weightless_target():
    check_minus_inf_at_a_weightless_target("cpu")


def test_case_has_every_kind_of_row():
    x, ta, tb, lam = make_mix_case(256, 1000)
    C = 1000
    assert int((ta == tb).sum()) >= 2 and float(lam[-2]) == 1.0 and float(lam[-1]) == 0.0
    assert int(((ta < 0) | (ta >= C)).sum()) == 2 and int(((tb < 0) | (tb >= C)).sum()) == 2
    inner = lam[:-2]
    assert bool(((inner > 0) & (inner < 1)).any()) and 0.3 < float(lam.mean()) < 0.7  # Beta(0.2, 0.2): mean 0.5


def test_equal_targets_add_their_weights():
    """ta == tb: the two hot terms add to the plain smoothed loss, whatever lam is."""
    from distributed_learning_amd.ops import cross_entropy_mix

    x, ta, _, lam = make_mix_case(40, 30, seed=6, ignore=False)
    ref = F.cross_entropy(x.double(), ta, label_smoothing=0.1)
    torch.testing.assert_close(cross_entropy_mix(x, ta, ta, lam, 0.1).double(), ref, **LOSS_TOL)


def test_zero_valid_rows_and_argument_checks():
    from distributed_learning_amd import ops
    from distributed_learning_amd.ops import cross_entropy_mix

    assert ops.cross_entropy_mix is cross_entropy_mix
    x, ta, tb, lam = make_mix_case(4, 10)
    assert math.isnan(float(cross_entropy_mix(x, ta, torch.full((4,), -100), lam, 0.1)))
    assert math.isnan(float(cross_entropy_mix(x, torch.full((4,), 10), tb, lam)))
    ok = torch.zeros(4, dtype=torch.long)
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            cross_entropy_mix(x, ok, ok, lam, bad)
    for args in ((x, ok[:3], ok, lam), (x, ok, ok[:3], lam), (x, ok, ok, lam[:3]), (x[0], ok, ok, lam),
                 (x, ok, ok, lam[:, None])):
        with pytest.raises(ValueError):
            cross_entropy_mix(*args)
