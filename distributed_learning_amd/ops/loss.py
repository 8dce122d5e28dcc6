"""Fused log-softmax + NLL (cross-entropy) with a native forward/backward.

Reference: ``F.log_softmax`` in the model (/root/reference/src/network.py:29,41) followed by
``F.nll_loss`` (/root/reference/src/main.py:76). ``cross_entropy(logits, target)`` computes the same
mean loss in one kernel (csrc/kernels/loss.hip) keeping only the per-row logsumexp for backward.

``cross_entropy_with_metrics`` is the label-smoothed loss together with the batch's top-1 / top-k
counts, from a second kernel pair in the same file that reads every logit once. The counts follow one
fixed rule, on the GPU and in the fallback alike: the target's rank is the number of logits above it
plus the number of equal logits with a smaller class index, and a row is top-k correct iff its rank
is below k. Ignored rows (target outside ``[0, C)``) and rows whose target logit is NaN are never
correct.

``cross_entropy_mix`` is the same smoothed loss against a weighted target pair (Mixup / CutMix), from a third
kernel pair: one forward and one backward pass over the logits instead of two loss calls.
"""
from __future__ import annotations

from typing import Tuple

import torch
import torch.nn.functional as F

from . import _ext


class _XEnt(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        C = _ext.require()
        logits = logits.contiguous()
        loss, ws = C.xent_fwd(logits, target)
        ctx.save_for_backward(logits, target, ws, loss)
        return loss[0]

    @staticmethod
    def backward(ctx, gout):
        logits, target, ws, loss = ctx.saved_tensors
        C = _ext.require()
        return C.xent_bwd(logits, target, ws, loss, gout.reshape(1)), None


class _XEntMetrics(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, eps, k):
        C = _ext.require()
        logits = logits.contiguous()
        target = target.contiguous()
        stats, ws = C.xent_metrics_fwd(logits, target, eps, k)
        ctx.save_for_backward(logits, target, ws, stats)
        ctx.eps = eps
        ctx.mark_non_differentiable(stats)
        return ws[-1], stats  # stats[0] / stats[1], divided by the batch kernel

    @staticmethod
    def backward(ctx, gout, _gstats):
        logits, target, ws, stats = ctx.saved_tensors
        C = _ext.require()
        return C.xent_smooth_bwd(logits, target, ws, stats, gout.reshape(1), ctx.eps), None, None, None


def _check_smoothing(label_smoothing: float) -> float:
    eps = float(label_smoothing)
    if not 0.0 <= eps < 1.0:
        raise ValueError(f"label_smoothing must be in [0, 1), got {label_smoothing}")
    return eps


def _row_loss(x: torch.Tensor, xt: torch.Tensor, valid: torch.Tensor, eps: float) -> torch.Tensor:
    """Row losses ``lse - (1 - eps) * xt - eps * mean(x)`` of both fallbacks, 0 for an invalid row; ``eps == 0``
    leaves the mean out, as the kernels do."""
    row = torch.logsumexp(x, dim=1) - (1.0 - eps) * xt
    if eps > 0:
        row = row - (eps / x.shape[1]) * x.sum(dim=1)
    return torch.where(valid, row, torch.zeros_like(row))


def _metrics_fallback(logits: torch.Tensor, target: torch.Tensor, eps: float, k: int):
    """The kernels' semantics in plain torch (CPU tensors, unsupported dtypes, no extension)."""
    x = logits if logits.dtype == torch.float64 else logits.float()
    C = x.shape[1]
    valid = (target >= 0) & (target < C)
    t = torch.where(valid, target, torch.zeros_like(target))
    xt = x.gather(1, t[:, None]).squeeze(1)
    row = _row_loss(x, xt, valid, eps)
    xd, xtd = x.detach(), xt.detach()[:, None]
    cols = torch.arange(C, device=x.device)[None, :]
    rank = ((xd > xtd) | ((xd == xtd) & (cols < t[:, None]))).sum(dim=1)
    ok = valid & ~torch.isnan(xtd[:, 0])
    total = row.sum()
    stats = torch.stack([total.detach().float(), valid.sum().float(), (ok & (rank < 1)).sum().float(),
                         (ok & (rank < k)).sum().float()])
    return total / stats[1].to(total.dtype), stats


def cross_entropy_with_metrics(logits: torch.Tensor, target: torch.Tensor, label_smoothing: float = 0.0,
                               topk: int = 5) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(loss, stats)`` of ``[B, C]`` logits: the mean label-smoothed cross-entropy over the valid rows
    (differentiable; NaN without one) and the detached float32 ``stats = [sum of row losses, valid rows,
    top-1 correct, top-k correct]`` on the logits' device. ``loss = stats[0] / stats[1]``; the stats are
    sums, so they add across batches and all-reduce across ranks with SUM."""
    eps, k = _check_smoothing(label_smoothing), int(topk)
    if k < 1:
        raise ValueError(f"topk must be >= 1, got {topk}")
    if logits.dim() != 2 or target.dim() != 1 or target.shape[0] != logits.shape[0]:
        raise ValueError(f"expected [B, C] logits and [B] targets, got {tuple(logits.shape)} and {tuple(target.shape)}")
    if logits.is_cuda and logits.dtype in (torch.float32, torch.bfloat16):
        if _ext.available():
            return _XEntMetrics.apply(logits, target, eps, k)
        if _ext.gpu_required():
            _ext.require()
    return _metrics_fallback(logits, target, eps, k)


class _XEntMix(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target_a, target_b, lam, eps):
        C = _ext.require()
        logits, lam = logits.contiguous(), lam.contiguous()
        target_a, target_b = target_a.contiguous(), target_b.contiguous()
        stats, ws = C.xent_mix_fwd(logits, target_a, target_b, lam, eps)
        ctx.save_for_backward(logits, target_a, target_b, lam, ws, stats)
        ctx.eps = eps
        return ws[-1]  # stats[0] / stats[1], divided by the batch kernel

    @staticmethod
    def backward(ctx, gout):
        logits, target_a, target_b, lam, ws, stats = ctx.saved_tensors
        C = _ext.require()
        d = C.xent_mix_bwd(logits, target_a, target_b, lam, ws, stats, gout.reshape(1), ctx.eps)
        return d, None, None, None, None


def _mix_fallback(logits: torch.Tensor, target_a: torch.Tensor, target_b: torch.Tensor, lam: torch.Tensor,
                  eps: float) -> torch.Tensor:
    """The pair-target kernels' semantics in plain torch (CPU tensors, unsupported dtypes, no extension)."""
    x = logits if logits.dtype == torch.float64 else logits.float()
    C = x.shape[1]
    valid = (target_a >= 0) & (target_a < C) & (target_b >= 0) & (target_b < C)
    ta = torch.where(valid, target_a, torch.zeros_like(target_a))
    tb = torch.where(valid, target_b, torch.zeros_like(target_b))
    wa = lam.to(x.dtype)
    wb = 1.0 - wa
    zero = torch.zeros((), dtype=x.dtype, device=x.device)
    # a term whose weight is exactly 0 is left out: a -inf logit there adds nothing
    xt = torch.where(wa != 0, wa * x.gather(1, ta[:, None]).squeeze(1), zero) \
        + torch.where(wb != 0, wb * x.gather(1, tb[:, None]).squeeze(1), zero)
    row = _row_loss(x, xt, valid, eps)
    return row.sum() / valid.sum().to(row.dtype)


def cross_entropy_mix(logits: torch.Tensor, target_a: torch.Tensor, target_b: torch.Tensor, lam: torch.Tensor,
                      label_smoothing: float = 0.0) -> torch.Tensor:
    """Mean label-smoothed cross-entropy of ``[B, C]`` logits against the target pair of Mixup / CutMix: row
    ``i`` is ``lam[i] * CE(x_i, target_a[i]) + (1 - lam[i]) * CE(x_i, target_b[i])`` computed in one pass,
    ``lse - (1 - eps) * (lam x[ta] + (1 - lam) x[tb]) - eps * mean(x)`` (a term whose weight is exactly 0 is
    left out). ``lam`` is fp32 ``[B]`` on the logits' device. A row counts iff both targets are in ``[0, C)``;
    the mean is over those rows (NaN without one). With ``lam == 1`` everywhere this is
    :func:`cross_entropy_with_metrics`' loss for ``target_a``, bit for bit."""
    eps = _check_smoothing(label_smoothing)
    B = logits.shape[0] if logits.dim() == 2 else -1
    if logits.dim() != 2 or any(t.dim() != 1 or t.shape[0] != B for t in (target_a, target_b, lam)):
        raise ValueError(f"expected [B, C] logits and [B] targets and weights, got {tuple(logits.shape)}, "
                         f"{tuple(target_a.shape)}, {tuple(target_b.shape)} and {tuple(lam.shape)}")
    if lam.device != logits.device:
        raise ValueError(f"lam must be on the logits' device {logits.device}, got {lam.device}")
    if logits.is_cuda and logits.dtype in (torch.float32, torch.bfloat16):
        if _ext.available():
            return _XEntMix.apply(logits, target_a, target_b, lam.to(torch.float32), eps)
        if _ext.gpu_required():
            _ext.require()
    return _mix_fallback(logits, target_a, target_b, lam, eps)


def cross_entropy(logits: torch.Tensor, target: torch.Tensor, label_smoothing: float = 0.0) -> torch.Tensor:
    """Mean cross-entropy over rows with ``target >= 0`` (``ignore_index`` < 0); with ``label_smoothing`` > 0
    the smoothed loss of :func:`cross_entropy_with_metrics`."""
    if _check_smoothing(label_smoothing) > 0.0:
        return cross_entropy_with_metrics(logits, target, label_smoothing, topk=1)[0]
    if logits.is_cuda and logits.dim() == 2 and logits.dtype in (torch.float32, torch.bfloat16):
        if _ext.available():
            return _XEnt.apply(logits, target)
        if _ext.gpu_required():
            _ext.require()
    return F.nll_loss(F.log_softmax(logits.float(), dim=1), target, ignore_index=-100 if (target >= 0).all() else -1) \
        if target.min() >= 0 else F.cross_entropy(logits.float(), target.clamp(min=-1), ignore_index=-1)
