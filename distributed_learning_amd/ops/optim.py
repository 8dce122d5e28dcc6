"""FusedSGD: ``torch.optim.SGD`` semantics in ONE multi-tensor HIP launch per step.

Reference: ``optim.SGD(model.parameters(), lr=0.01, momentum=0.5)`` (/root/reference/src/main.py:36)
stepped once per batch (main.py:91) — a for-each over 187 (GoogLeNet) / 161 (ResNet-50) tensors.
On MI355X the update is HBM-bound (fp32: read p, g, m; write p, m = 20 B/param; ResNet-50 ≈ 0.5 GB
≈ 0.1 ms), so the win is launch count: one launch over a device-resident tensor table
(csrc/kernels/multi_tensor.hip) instead of one or several per tensor.

Extras over torch.optim.SGD: ``grad_scale`` (fold 1/N or loss-scale into the update) and an
optional bf16 shadow copy of each parameter written in the same pass.
On CPU (or without the extension) it falls back to the exact ``torch.optim.SGD`` math.

FusedLARS: layer-wise adaptive rate scaling (You et al. 2017) for the large-batch configurations,
with the norms, trust ratios and the global-norm clip computed on the device: a step is a handful
of launches, reads nothing back to the host, and takes its learning rate from device memory so a
captured step follows a schedule (``set_lr``). ``poly_warmup_lr`` is the usual schedule for it.

FusedLAMB / FusedAdamW: the Adam family on the same machinery -- LAMB (You et al. 2019) is LARS's sibling
with two moments and a trust ratio from the norm of the update, AdamW its one-pass case. Their per-tensor
update counts live on the device and are advanced by the step itself, so a captured step moves its own bias
corrections.

All take ``ema_decay``: an exponential moving average of the weights advanced inside the same update
launches (one more fp32 read and write per element, no launch), ``ModelEMA`` to train with it and evaluate
from it, ``ema_decay_at`` for its warmup. Off by default.
"""
from __future__ import annotations

import contextlib
import math
from typing import List, Optional

import torch

from . import _ext


def ema_decay_at(t: int, decay: float, warmup: bool = False) -> float:
    """The EMA decay of update number ``t`` (the number of updates before it): ``decay``, or with ``warmup``
    ``min(decay, (1 + t) / (10 + t))`` so that the first averages follow the weights closely."""
    return min(decay, (1 + t) / (10 + t)) if warmup else decay


class _MasterWeightsOptimizer(torch.optim.Optimizer):
    """What the fused optimizers share: fp32 master copies of low-precision parameters, a
    ``load_state_dict`` that keeps them (and the momentum buffers and weight averages) fp32, and the
    exponential moving average (EMA) of the weights.

    EMA (``ema_decay`` in (0, 1); 0 = off: no state, and the native calls are the plain ones). The first
    time a tensor is stepped ``state[p]["ema"]`` becomes an fp32 clone of its fp32 target (the master, or
    the fp32 parameter) before the update; every step that updates the tensor then advances it by ::

        ema = ema + (1 - decay) * (p_new - ema)

    from the fp32 value just written, never from the bf16 shadow -- on the GPU inside the update launch
    (one fused multiply-add: ``fmaf(1 - decay, p_new - ema, ema)``), elsewhere in torch. A tensor without
    a gradient in a step is not stepped, and its EMA does not move. ``1 - decay`` lives in a device scalar
    the kernels read, so a step captured in a HIP graph follows ``set_ema_decay`` calls made between
    replays. A low-precision parameter without a master is averaged from its rounded value."""

    master_weights = False
    ema_decay = 0.0
    _ema_on = False
    _omd_dev = None   # fp32 [1] on the parameters' device: 1 - decay
    _omd_seen = None

    def _init_ema(self, ema_decay: float) -> None:
        if not 0.0 <= ema_decay < 1.0:
            raise ValueError(f"ema_decay must be in [0, 1), got {ema_decay}")
        self.ema_decay = float(ema_decay)
        self._ema_on = ema_decay > 0

    @property
    def ema_enabled(self) -> bool:
        return self._ema_on

    @staticmethod
    def _omd_value(decay: float) -> float:
        """float32(1 - decay): what the device scalar holds, as a Python float."""
        return float(torch.tensor(1.0 - decay, dtype=torch.float32))

    def set_ema_decay(self, decay: float) -> None:
        """Set the decay of the following steps: the attribute and the device scalar the kernels read
        (``float32(1 - decay)``). A stream-ordered fill, legal between graph replays."""
        if not self._ema_on:
            raise ValueError("set_ema_decay: the optimizer was built with ema_decay=0 (EMA off)")
        if not 0.0 < decay < 1.0:
            raise ValueError(f"ema_decay must be in (0, 1), got {decay}")
        self.ema_decay = float(decay)
        if self._omd_dev is not None:
            self._omd_dev.fill_(1.0 - decay)
            self._omd_seen = self.ema_decay

    def _sync_omd(self, device) -> torch.Tensor:
        """The device scalar, up to date with ``ema_decay``; never filled while a graph is being captured,
        where the fill would be frozen into the graph."""
        if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            if self._omd_dev is None or self._omd_dev.device != device:
                raise RuntimeError("run a step before capturing one (the EMA's device scalar is created there)")
            return self._omd_dev
        if self._omd_dev is None or self._omd_dev.device != device:
            self._omd_dev = torch.zeros(1, dtype=torch.float32, device=device)
            self._omd_seen = None
        if self._omd_seen != self.ema_decay:
            self._omd_dev.fill_(1.0 - self.ema_decay)
            self._omd_seen = self.ema_decay
        return self._omd_dev

    def _ema(self, p, target):
        """The average of ``p``, created from ``target`` (its fp32 master, or ``p``) before the first update."""
        st = self.state[p]
        if "ema" not in st:
            st["ema"] = target.detach().clone() if target.dtype == torch.float32 else target.detach().float()
        return st["ema"]

    def _reference_ema(self, emas, targets) -> None:
        """``e + omd * (p_new - e)`` in fp32 torch, after the update of ``targets``."""
        omd = self._omd_value(self.ema_decay)
        for e, t in zip(emas, targets):
            e.add_((t.detach().float() - e).mul_(omd))

    def load_state_dict(self, state_dict):
        """torch.optim.Optimizer.load_state_dict casts floating-point state to each parameter's dtype
        (through a policy it calls by class name); the fp32 master copies, momentum buffers, Adam moments and
        weight averages of bf16 parameters must stay fp32 for a bit-exact resume, so they are re-installed
        afterwards."""
        keep = {}
        for idx, st in state_dict.get("state", {}).items():
            for k in ("master", "momentum_buffer", "ema", "exp_avg", "exp_avg_sq"):
                if k in st and torch.is_tensor(st[k]) and st[k].dtype == torch.float32:
                    keep[(idx, k)] = st[k]
            # FusedLAMB / FusedAdamW update counts: torch leaves a "step" entry where (and what) the checkpoint
            # made it; the kernels need it int32 on the parameter's device, in memory of its own
            if torch.is_tensor(st.get("step")) and st["step"].dtype == torch.int32:
                keep[(idx, "step")] = st["step"]
        super().load_state_dict(state_dict)
        params = [p for g in self.param_groups for p in g["params"]]
        for (idx, k), v in keep.items():
            p = params[idx]
            self.state[p][k] = v.to(device=p.device, copy=True)
        self._tables = {}

    def _master(self, p):
        if p.dtype == torch.float32 or not self.master_weights:
            return None
        st = self.state[p]
        if "master" not in st:
            st["master"] = torch.empty_like(p, dtype=torch.float32).copy_(p)
        return st["master"]


class FusedSGD(_MasterWeightsOptimizer):
    """SGD(momentum, dampening, nesterov, weight_decay) as one native launch per (grad dtype) group.

    ``master_weights=True``: low-precision (bf16) parameters get an fp32 master copy in the
    optimizer state; the kernel reads the bf16 gradient, updates master + momentum in fp32 and
    writes the rounded bf16 parameter back in the same pass (no separate cast kernels, and no
    autocast weight casts in the forward). fp32 parameters (e.g. BatchNorm) are updated in place.
    """

    def __init__(self, params, lr: float = 0.01, momentum: float = 0.0, dampening: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False, grad_scale: float = 1.0,
                 master_weights: bool = False, ema_decay: float = 0.0):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                        nesterov=nesterov, grad_scale=grad_scale)
        super().__init__(params, defaults)
        self.master_weights = master_weights
        self._init_ema(ema_decay)
        self._tables = {}

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        from . import conv as _conv

        _conv.join_all_devices()  # late weight gradients of a backward that raised before its own join
        for gi, group in enumerate(self.param_groups):
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            mom = group["momentum"]
            # partition by (grad dtype, first-step) so every launch has uniform semantics
            parts = {}
            for p in ps:
                st = self.state[p]
                first = mom != 0 and "momentum_buffer" not in st
                if mom != 0 and first:
                    st["momentum_buffer"] = torch.zeros_like(p, dtype=torch.float32)
                parts.setdefault((p.grad.dtype, first), []).append(p)
            for (gdt, first), plist in parts.items():
                self._step_part(gi, group, plist, first)
        return loss

    def _step_part(self, gi, group, ps, first):
        mom = group["momentum"]
        gs = [p.grad for p in ps]
        masters = [self._master(p) for p in ps]
        bufs = [self.state[p].get("momentum_buffer") for p in ps]
        native = ps[0].is_cuda and _ext.available() and all(
            (m is not None) or p.dtype == torch.float32 for p, m in zip(ps, masters))
        if ps[0].is_cuda and not native and _ext.gpu_required() and not _ext.available():
            _ext.require()
        targets = [m if m is not None else p for p, m in zip(ps, masters)]
        emas = [self._ema(p, t) for p, t in zip(ps, targets)] if self._ema_on else None
        if not native:
            self._reference_step(targets, [g.float() for g in gs], bufs, group, first)
            if emas is not None:
                self._reference_ema(emas, targets)
            for p, m in zip(ps, masters):
                if m is not None:
                    p.copy_(m)
            return
        fp = targets
        shadows = [p for p, m in zip(ps, masters) if m is not None]
        if shadows and len(shadows) != len(ps):  # mixed within a part cannot happen: grads share dtype
            raise RuntimeError("FusedSGD: mixed master/non-master parameters in one launch group")
        # By-value tensor lists in the kernel arguments (<= 32 tensors per launch): no device table,
        # so gradients may live anywhere and move every step (autograd-owned, set_to_none, views).
        hyper = (group["lr"], mom, group["dampening"], group["weight_decay"], group["nesterov"], group["grad_scale"],
                 first)
        if emas is None:
            _ext.require().sgd_step_list(fp, gs, bufs if mom != 0 else [], shadows, *hyper)
        else:
            _ext.require().sgd_ema_step_list(fp, gs, bufs if mom != 0 else [], shadows, emas,
                                             self._sync_omd(ps[0].device), *hyper)

    @staticmethod
    def _reference_step(ps, gs, bufs, group, first):
        lr, mom, damp, wd, nest, gsc = (group["lr"], group["momentum"], group["dampening"], group["weight_decay"],
                                        group["nesterov"], group["grad_scale"])
        for p, g, b in zip(ps, gs, bufs):
            # a low-precision parameter (no master) is updated in fp32 and rounded once: an in-place
            # p.add_(d) may round the fp32 update to p's dtype before it adds (it does on the GPU)
            pf = p if p.dtype == torch.float32 else p.float()
            d = g * gsc if gsc != 1.0 else g
            if wd != 0:
                d = d.add(pf, alpha=wd)
            if mom != 0:
                if first:
                    b.copy_(d)
                else:
                    b.mul_(mom).add_(d, alpha=1 - damp)
                d = d.add(b, alpha=mom) if nest else b
            pf.add_(d, alpha=-lr)
            if pf is not p:
                p.copy_(pf)


def poly_warmup_lr(step: int, base_lr: float, warmup_steps: int, total_steps: int, power: float = 2.0,
                   end_lr: float = 0.0) -> float:
    """Linear from 0 to ``base_lr`` over ``warmup_steps``, then polynomial decay to ``end_lr`` at
    ``total_steps`` (and ``end_lr`` after it). Without a decay phase (``total_steps <= warmup_steps``)
    the rate stays at ``base_lr`` after the warmup; with both 0 it is constant."""
    if step < warmup_steps:
        return base_lr * step / warmup_steps
    if total_steps <= warmup_steps:
        return base_lr
    frac = min(1.0, (step - warmup_steps) / (total_steps - warmup_steps))
    return end_lr + (base_lr - end_lr) * (1.0 - frac) ** power


def multi_tensor_l2norm(tensors, scale: float = 1.0):
    """``(per_tensor[T], total[1])``: ``scale * ||t||_2`` of every tensor of the list and of all of
    them together, fp32. GPU lists (fp32 / bf16, dense) go through the square-sum and finalize
    kernels of the fused LARS; CPU lists through torch.

    The norms are never read back to the host, but every call builds its table of partial ranges on
    the host and uploads it (a synchronous copy) and allocates a fresh workspace that the results
    are views of: a utility for logging and tests, not for the inside of a step or of a graph
    capture. ``FusedLARS`` keeps its table and workspace across steps and has neither cost."""
    tensors = list(tensors)
    if not tensors:
        raise ValueError("multi_tensor_l2norm: empty tensor list")
    if tensors[0].is_cuda and (_ext.available() or _ext.gpu_required()):
        per, total = _ext.require().multi_tensor_l2norm(tensors, float(scale))
        return per, total
    per = torch.stack([torch.linalg.vector_norm(t.detach().float()) for t in tensors])
    return per * scale, (torch.linalg.vector_norm(per) * scale).reshape(1)


class _PlannedOptimizer(_MasterWeightsOptimizer):
    """What FusedLARS and FusedLAMB / FusedAdamW share on top of that: per-group learning rates in a device array
    the kernels read (``set_lr``), so a step captured in a HIP graph follows a schedule, and the bounded cache of
    native plans (device table + workspace per set of participating tensors)."""

    _MAX_PLANS = 4  # cached native plans (sets of participating tensors), least recently used out first

    def _init_plans(self) -> None:
        self.last_grad_norm: Optional[torch.Tensor] = None  # device tensor [1]: G of the last step
        self._tables = {}     # participating tensors + hyper-parameters -> native plan (table, workspace)
        self._captured = []   # plans a HIP graph was captured with, kept alive outside the cache
        self._lr_dev = None   # fp32 [len(param_groups)] on the parameters' device
        self._lr_seen: List[Optional[float]] = []
        self.last_launches = 0

    def set_lr(self, lr: float, group: Optional[int] = None) -> None:
        """Set the learning rate of one param group (all when ``group`` is None): ``param_groups`` and
        the device scalar the kernels read. A stream-ordered fill, legal between graph replays."""
        for gi, g in enumerate(self.param_groups):
            if group is None or gi == group:
                g["lr"] = lr
                if self._lr_dev is not None:
                    self._lr_dev[gi].fill_(lr)
                    self._lr_seen[gi] = lr

    def _sync_lr(self, device) -> None:
        """Bring the device scalars up to date with ``group["lr"]`` (schedulers write there); never while
        a graph is being captured, where the fill would be frozen into the graph."""
        if torch.cuda.is_current_stream_capturing():
            if self._lr_dev is None:
                raise RuntimeError(f"{type(self).__name__}: run a step before capturing one (the device state is "
                                   "created there)")
            return
        if self._lr_dev is None or self._lr_dev.device != device or len(self._lr_seen) != len(self.param_groups):
            self._lr_dev = torch.zeros(len(self.param_groups), dtype=torch.float32, device=device)
            self._lr_seen = [None] * len(self.param_groups)
            self._tables = {}  # plans hold the array
        for gi, g in enumerate(self.param_groups):
            if self._lr_seen[gi] != g["lr"]:
                self._lr_dev[gi].fill_(g["lr"])
                self._lr_seen[gi] = g["lr"]

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._lr_seen = [None] * len(self._lr_seen)

    def _plan(self, key, make):
        """The cached plan of ``key``, built by ``make()`` when missing. A plan holds a device table and a
        workspace: only the few most recent sets are kept (a model whose set of gradient-less parameters varies
        would otherwise grow the cache without bound)."""
        plan = self._tables.get(key)
        if plan is None:
            plan = make()
            while len(self._tables) >= self._MAX_PLANS:
                self._tables.pop(next(iter(self._tables)))
            self._tables[key] = plan
        else:
            self._tables[key] = self._tables.pop(key)  # most recently used last
        if torch.cuda.is_current_stream_capturing() and plan not in self._captured:
            self._captured.append(plan)  # a captured graph replays into this plan's memory: never freed
        return plan

    @staticmethod
    def _adapt(rows):
        return [not (g["exclude_bias_and_norm"] and p.ndim <= 1) for _, g, p in rows]


class FusedLARS(_PlannedOptimizer):
    """Momentum SGD with layer-wise adaptive rate scaling and optional clipping by the global
    gradient norm. Per tensor ``t`` (``s`` = ``grad_scale``, sums over every tensor stepped in this call)::

        G     = s * sqrt(sum_t ||g_t||^2)
        clip  = min(1, max_grad_norm / (G + 1e-6))          (1 when max_grad_norm == 0)
        c     = s * clip
        wn, gn = ||p_t||, c * ||g_t||
        trust = eta * wn / (gn + wd * wn + eps)              (1 when excluded, or wn == 0, or gn == 0)
        m     = momentum * m + lr * trust * (c * g + wd * p)
        p     = p - m

    With ``exclude_bias_and_norm`` tensors of ``ndim <= 1`` (biases, BatchNorm scale and shift) are
    excluded: trust 1 and no weight decay. No Nesterov, no dampening.

    On the GPU a step is square-sum launches, one finalize launch and update launches over by-value
    tensor lists (csrc/kernels/multi_tensor.hip), whatever the number of param groups. The learning
    rate of each group lives in a device array that the finalize reads, so a step captured in a HIP
    graph follows ``set_lr`` calls made between replays. On CPU, or for low-precision parameters
    without masters, the same formula runs in torch (also without a host read).
    """

    def __init__(self, params, lr: float, momentum: float = 0.9, weight_decay: float = 0.0, eta: float = 1e-3,
                 eps: float = 0.0, exclude_bias_and_norm: bool = True, grad_scale: float = 1.0,
                 max_grad_norm: float = 0.0, master_weights: bool = False, ema_decay: float = 0.0):
        if lr < 0 or momentum < 0 or weight_decay < 0 or eta <= 0 or eps < 0 or max_grad_norm < 0:
            raise ValueError("FusedLARS: lr, momentum, weight_decay, eps, max_grad_norm >= 0 and eta > 0 required")
        defaults = dict(lr=lr, momentum=momentum, weight_decay=weight_decay, eta=eta, eps=eps,
                        exclude_bias_and_norm=exclude_bias_and_norm)
        super().__init__(params, defaults)
        self.grad_scale = grad_scale
        self.max_grad_norm = max_grad_norm
        self.master_weights = master_weights
        self._init_ema(ema_decay)
        self._init_plans()

    # -- step --------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        from . import conv as _conv

        _conv.join_all_devices()  # late weight gradients of a backward that raised before its own join
        rows = []  # (group index, group, parameter), bf16 gradients after fp32 ones: fewest launches
        for gi, group in enumerate(self.param_groups):
            rows += [(gi, group, p) for p in group["params"] if p.grad is not None and p.numel() > 0]
        if not rows:
            return loss
        rows.sort(key=lambda r: r[2].grad.dtype != torch.float32)
        ps = [p for _, _, p in rows]
        for p in ps:
            st = self.state[p]
            if "momentum_buffer" not in st:
                st["momentum_buffer"] = torch.zeros_like(p, dtype=torch.float32)
        masters = [self._master(p) for p in ps]
        bufs = [self.state[p]["momentum_buffer"] for p in ps]
        targets = [m if m is not None else p for p, m in zip(ps, masters)]
        emas = [self._ema(p, t) for p, t in zip(ps, targets)] if self._ema_on else None
        dev = ps[0].device
        on_gpu = all(p.is_cuda and p.grad.is_cuda for p in ps)
        native = on_gpu and _ext.available() and all(
            (m is not None or p.dtype == torch.float32) and p.grad.dtype in (torch.float32, torch.bfloat16)
            for p, m in zip(ps, masters))
        if on_gpu and _ext.gpu_required() and not _ext.available():
            _ext.require()
        if not native:
            self._reference_step(rows, masters, bufs, self._adapt(rows))
            if emas is not None:
                self._reference_ema(emas, targets)
            return loss
        self._sync_lr(dev)
        # the plan (device table + workspace) depends on which tensors take part, in which order, and on
        # their groups' hyper-parameters; the native side checks every tensor's size against it
        key = (tuple(id(p) for p in ps),
               tuple((g["weight_decay"], g["eta"], g["eps"], g["momentum"], g["exclude_bias_and_norm"])
                     for g in self.param_groups))
        plan = self._plan(key, lambda: _ext.require().LarsPlan(
            [p.numel() for p in ps], [gi for gi, _, _ in rows], self._adapt(rows),
            [g["weight_decay"] for _, g, _ in rows], [g["eta"] for _, g, _ in rows], [g["eps"] for _, g, _ in rows],
            [g["momentum"] for _, g, _ in rows], self._lr_dev, ps[0]))
        shadows = [p if m is not None else None for p, m in zip(ps, masters)]
        if emas is None:
            _ext.require().lars_step_list(plan, targets, [p.grad for p in ps], bufs, shadows, self.grad_scale,
                                          self.max_grad_norm)
        else:
            _ext.require().lars_ema_step_list(plan, targets, [p.grad for p in ps], bufs, shadows, emas,
                                              self._sync_omd(dev), self.grad_scale, self.max_grad_norm)
        self.last_grad_norm = plan.grad_norm()
        self.last_launches = plan.last_launches()
        return loss

    def _reference_step(self, rows, masters, bufs, adapt):
        """The formula of the class docstring in torch: fp32 arithmetic, no host read."""
        gs = [p.grad.float() for _, _, p in rows]
        gnorms = torch.stack([torch.linalg.vector_norm(g) for g in gs])
        s = self.grad_scale
        G = torch.linalg.vector_norm(gnorms) * s
        if self.max_grad_norm > 0:
            c = torch.clamp(self.max_grad_norm / (G + 1e-6), max=1.0) * s
        else:
            c = torch.full_like(G, s)
        one = torch.ones_like(G)
        for (gi, group, p), g, gr, master, buf, a in zip(rows, gs, gnorms, masters, bufs, adapt):
            target = master if master is not None else p
            pf = target if target.dtype == torch.float32 else target.float()
            lr, mu, wd = group["lr"], group["momentum"], (group["weight_decay"] if a else 0.0)
            trust = one
            if a:
                wn, gn = torch.linalg.vector_norm(pf), c * gr
                trust = torch.where((wn > 0) & (gn > 0), group["eta"] * wn / (gn + wd * wn + group["eps"]), one)
            d = g * c
            if wd != 0:
                d = d.add(pf, alpha=wd)
            buf.mul_(mu).add_(d * (lr * trust))
            pf.sub_(buf)
            if pf is not target:
                target.copy_(pf)
            if master is not None:
                p.copy_(master)
        self.last_grad_norm = G.reshape(1)
        self.last_launches = 0


class FusedLAMB(_PlannedOptimizer):
    """LAMB (You et al. 2019): Adam moments with decoupled weight decay, the step of every tensor scaled by the
    layer-wise trust ratio ``||p|| / ||u||``, and optional clipping by the global gradient norm. Per tensor ``t``
    stepped in this call (``s`` = ``grad_scale``; ``G``, ``clip`` and ``c`` exactly as in ``FusedLARS``)::

        G     = s * sqrt(sum_t ||g_t||^2)
        clip  = min(1, max_grad_norm / (G + 1e-6))          (1 when max_grad_norm == 0)
        c     = s * clip
        k     = step_t + 1                                   (the tensor's own update count)
        bc1   = 1 - beta1^k,  bc2 = 1 - beta2^k              (computed as -expm1(k * ln(beta)))
        gh    = c * g
        m     = beta1 * m + (1 - beta1) * gh
        v     = beta2 * v + (1 - beta2) * gh * gh
        u     = (m / bc1) / (sqrt(v / bc2) + eps) + wd * p
        trust = ||p|| / ||u||                                (1 when excluded, or ||p|| == 0, or ||u|| == 0)
        p     = p - lr * trust * u

    With ``exclude_bias_and_norm`` tensors of ``ndim <= 1`` get trust 1 and no weight decay. ``FusedAdamW`` is the
    same class with trust 1 everywhere. The moments are ``state[p]["exp_avg"]`` and ``state[p]["exp_avg_sq"]``
    (fp32); ``state[p]["step"]`` is a one-element int32 tensor on the parameter's device that the step itself
    advances, so a step captured in a HIP graph moves its own bias corrections on every replay. A parameter
    without a gradient is not stepped: its moments, count and average stay.

    On the GPU a LAMB step is a moments pass (which also sums ``p^2`` and ``u^2`` per block, ``u`` in registers
    only), one finalize launch (norms, trust, bias corrections, counts) and an apply pass that forms ``u`` again
    from ``p, m, v``; AdamW is the finalize and one update pass. Clipping adds a gradient square-sum pass (and for
    LAMB its own finalize) in front. Learning rates come from the device array of ``set_lr``. On CPU, or for
    low-precision parameters without masters, the same formula runs in torch (also without a host read).
    """

    _trust = True

    def __init__(self, params, lr: float, betas=(0.9, 0.999), eps: float = 1e-6, weight_decay: float = 0.0,
                 exclude_bias_and_norm: bool = True, grad_scale: float = 1.0, max_grad_norm: float = 0.0,
                 master_weights: bool = False, ema_decay: float = 0.0):
        name = type(self).__name__
        if eps <= 0:
            raise ValueError(f"{name}: eps > 0 required (with eps = 0 a zero gradient on the first step is 0/0)")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"{name}: betas must be in [0, 1), got {betas}")
        if lr < 0 or weight_decay < 0 or max_grad_norm < 0:
            raise ValueError(f"{name}: lr, weight_decay, max_grad_norm >= 0 required")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                        exclude_bias_and_norm=exclude_bias_and_norm)
        super().__init__(params, defaults)
        self.grad_scale = grad_scale
        self.max_grad_norm = max_grad_norm
        self.master_weights = master_weights
        self._init_ema(ema_decay)
        self._init_plans()
        self.last_plan = None  # the native plan of the last step (None after a torch step): bias_corrections(), norms()
        self.last_params: List[torch.Tensor] = []  # the parameters of the last step, in the plan's row order

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        from . import conv as _conv

        _conv.join_all_devices()  # late weight gradients of a backward that raised before its own join
        rows = []  # (group index, group, parameter), bf16 gradients after fp32 ones: fewest launches
        for gi, group in enumerate(self.param_groups):
            rows += [(gi, group, p) for p in group["params"] if p.grad is not None and p.numel() > 0]
        if not rows:
            return loss
        rows.sort(key=lambda r: r[2].grad.dtype != torch.float32)
        ps = [p for _, _, p in rows]
        for p in ps:
            st = self.state[p]
            if "exp_avg" not in st:
                st["exp_avg"] = torch.zeros_like(p, dtype=torch.float32)
                st["exp_avg_sq"] = torch.zeros_like(p, dtype=torch.float32)
                st["step"] = torch.zeros(1, dtype=torch.int32, device=p.device)
        masters = [self._master(p) for p in ps]
        ms, vs, steps = ([self.state[p][k] for p in ps] for k in ("exp_avg", "exp_avg_sq", "step"))
        targets = [m if m is not None else p for p, m in zip(ps, masters)]
        emas = [self._ema(p, t) for p, t in zip(ps, targets)] if self._ema_on else None
        dev = ps[0].device
        on_gpu = all(p.is_cuda and p.grad.is_cuda for p in ps)
        native = on_gpu and _ext.available() and all(
            (m is not None or p.dtype == torch.float32) and p.grad.dtype in (torch.float32, torch.bfloat16)
            for p, m in zip(ps, masters))
        if on_gpu and _ext.gpu_required() and not _ext.available():
            _ext.require()
        self.last_params = ps
        adapt = self._adapt(rows)
        if not native:
            self._reference_step(rows, masters, ms, vs, steps, adapt)
            if emas is not None:
                self._reference_ema(emas, targets)
            return loss
        self._sync_lr(dev)
        # the plan (device table + workspaces) depends on which tensors take part, in which order, on their
        # count tensors (the table holds their addresses) and on their groups' hyper-parameters
        key = (tuple(id(p) for p in ps), tuple(id(s) for s in steps),
               tuple((g["weight_decay"], g["betas"], g["eps"], g["exclude_bias_and_norm"]) for g in self.param_groups))
        C = _ext.require()
        plan = self._plan(key, lambda: C.AdamPlan(
            self._trust, [p.numel() for p in ps], [gi for gi, _, _ in rows], adapt,
            [g["weight_decay"] if a else 0.0 for (_, g, _), a in zip(rows, adapt)],
            [g["betas"][0] for _, g, _ in rows], [g["betas"][1] for _, g, _ in rows], [g["eps"] for _, g, _ in rows],
            steps, self._lr_dev, ps[0]))
        shadows = [p if m is not None else None for p, m in zip(ps, masters)]
        args = (plan, targets, [p.grad for p in ps], ms, vs, shadows, steps)
        if emas is None:
            (C.lamb_step_list if self._trust else C.adamw_step_list)(*args, self.grad_scale, self.max_grad_norm)
        else:
            (C.lamb_ema_step_list if self._trust else C.adamw_ema_step_list)(
                *args, emas, self._sync_omd(dev), self.grad_scale, self.max_grad_norm)
        self.last_grad_norm = plan.grad_norm() if self.max_grad_norm > 0 else None
        self.last_launches = plan.last_launches()
        self.last_plan = plan
        return loss

    def _reference_step(self, rows, masters, ms, vs, steps, adapt):
        """The formula of the class docstring in torch: fp32 arithmetic, no host read."""
        gs = [p.grad.float() for _, _, p in rows]
        c = self.grad_scale
        self.last_grad_norm = None
        if self.max_grad_norm > 0:
            G = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in gs])) * self.grad_scale
            c = torch.clamp(self.max_grad_norm / (G + 1e-6), max=1.0) * self.grad_scale
            self.last_grad_norm = G.reshape(1)
        for (gi, group, p), g, master, m, v, step, a in zip(rows, gs, masters, ms, vs, steps, adapt):
            target = master if master is not None else p
            pf = target if target.dtype == torch.float32 else target.float()
            lr, (b1, b2), eps, wd = group["lr"], group["betas"], group["eps"], (group["weight_decay"] if a else 0.0)
            step.add_(1)
            k = step.to(torch.float32)
            bc1, bc2 = (-torch.expm1(k * (math.log(b) if b > 0 else -math.inf)) for b in (b1, b2))
            gh = g * c
            m.mul_(b1).add_(gh, alpha=1 - b1)
            v.mul_(b2).addcmul_(gh, gh, value=1 - b2)
            u = (m / bc1) / ((v / bc2).sqrt_() + eps)
            if wd != 0:
                u.add_(pf, alpha=wd)
            if self._trust and a:
                wn, un = torch.linalg.vector_norm(pf), torch.linalg.vector_norm(u)
                trust = torch.where((wn > 0) & (un > 0), wn / un, torch.ones_like(wn))
                pf.sub_(u * (lr * trust))
            else:
                pf.sub_(u, alpha=lr)
            if pf is not target:
                target.copy_(pf)
            if master is not None:
                p.copy_(master)
        self.last_launches = 0
        self.last_plan = None


class FusedAdamW(FusedLAMB):
    """AdamW (Adam with decoupled weight decay): the formula of ``FusedLAMB`` with trust 1 for every tensor, on
    the GPU one finalize launch (bias corrections and update counts) and one update pass, without any norm work
    unless ``max_grad_norm > 0``."""

    _trust = False


class ModelEMA:
    """Training with, and evaluation from, the exponential moving average of a model's weights.

    The parameter averages live in the optimizer (any fused optimizer here built with ``ema_decay > 0``, bare
    or inside a ``DistributedOptimizer``), which advances them inside its update launches; this class adds the
    averages of the model's floating-point buffers (BatchNorm running statistics; integer buffers such as
    ``num_batches_tracked`` are left alone), the decay schedule, and the exchange of weights and averages for
    evaluation. A buffer's average starts from the buffer's value at construction (or at ``reset_buffers()``).
    """

    def __init__(self, model, optimizer, decay: float, warmup: bool = False):
        if not 0.0 < decay < 1.0:
            raise ValueError(f"ModelEMA: decay must be in (0, 1), got {decay}")
        self.model = getattr(model, "module", model)
        self.optimizer = optimizer
        self._opt = getattr(optimizer, "optimizer", optimizer)  # inside a DistributedOptimizer
        if not getattr(self._opt, "ema_enabled", False):
            raise ValueError("ModelEMA: build the optimizer with ema_decay > 0")
        self.decay, self.warmup = float(decay), bool(warmup)
        self.buffers = {}
        self.reset_buffers()

    def _float_buffers(self):
        return [(n, b) for n, b in self.model.named_buffers() if b.is_floating_point()]

    def reset_buffers(self) -> None:
        """Start every buffer average from the buffer's present value."""
        self.buffers = {n: b.detach().float().clone() for n, b in self._float_buffers()}

    @staticmethod
    def _native(tensors) -> bool:
        on_gpu = bool(tensors) and all(t.is_cuda for t in tensors)
        if on_gpu and _ext.gpu_required() and not _ext.available():
            _ext.require()
        return on_gpu and _ext.available() and all(t.dtype == torch.float32 for t in tensors)

    @torch.no_grad()
    def step(self, batch: int):
        """Set the decay of update number ``batch`` (``ema_decay_at``), step the optimizer, then advance the
        buffer averages by the same formula."""
        self._opt.set_ema_decay(ema_decay_at(batch, self.decay, self.warmup))
        out = self.optimizer.step()
        pairs = [(self.buffers[n], b) for n, b in self._float_buffers()]
        if not pairs:
            return out
        emas, bufs = [e for e, _ in pairs], [b.detach() for _, b in pairs]
        if self._native(emas + bufs):
            _ext.require().ema_update_list(emas, bufs, self._opt._sync_omd(bufs[0].device))
        else:
            self._opt._reference_ema(emas, bufs)
        return out

    def _swap_lists(self):
        """(fp32 targets, their averages, bf16 shadows or None) of everything that has an average, and the
        low-precision parameters without a master, whose average is fp32 while they are not."""
        rows, lowp = [], []  # rows: (target, average, shadow)
        for p in self.model.parameters():
            st = self._opt.state.get(p, {})
            if "ema" not in st:
                continue  # never stepped: the average is the weight itself
            if "master" in st:
                rows.append((st["master"], st["ema"], p.detach()))
            elif p.dtype == torch.float32:
                rows.append((p.detach(), st["ema"], None))
            else:
                lowp.append((p.detach(), st["ema"]))
        for n, b in self._float_buffers():
            if b.dtype == torch.float32:
                rows.append((b.detach(), self.buffers[n], None))
            else:
                lowp.append((b.detach(), self.buffers[n]))
        targets, emas, shadows = ([r[i] for r in rows] for i in range(3))
        return targets, emas, shadows, lowp

    @staticmethod
    def _swap(targets, emas, shadows, native: bool) -> None:
        if native:
            _ext.require().ema_swap_list(targets, emas, shadows)
            return
        for t, e, s in zip(targets, emas, shadows):
            keep = t.clone()
            t.copy_(e)
            e.copy_(keep)
            if s is not None:
                s.copy_(t)

    @contextlib.contextmanager
    def applied(self):
        """Inside the context the model computes from the averages: fp32 targets (masters, fp32 parameters,
        buffers) are exchanged in place with their averages and bf16 shadows rewritten from the new masters;
        on exit, also when the body raises, the exchange is undone and every tensor has its bits back."""
        with torch.no_grad():
            targets, emas, shadows, lowp = self._swap_lists()
            native = self._native(targets + emas)
            stash = [t.clone() for t, _ in lowp]
            self._swap(targets, emas, shadows, native)
            for t, e in lowp:
                t.copy_(e)
        try:
            yield self
        finally:
            with torch.no_grad():
                self._swap(targets, emas, shadows, native)
                for (t, _), keep in zip(lowp, stash):
                    t.copy_(keep)

    def state_dict(self) -> dict:
        """The buffer averages (the parameter averages travel in the optimizer's state dict)."""
        return {"buffers": {n: e.clone() for n, e in self.buffers.items()}}

    def load_state_dict(self, state: dict) -> None:
        got = state["buffers"]
        if set(got) != set(self.buffers):
            raise KeyError(f"ModelEMA: buffer names differ: {sorted(set(got) ^ set(self.buffers))}")
        for n, e in self.buffers.items():
            e.copy_(got[n])

    def model_state_dict(self) -> dict:
        """A cloned ``state_dict()`` of the averaged model, for export."""
        with self.applied():
            return {k: v.detach().clone() for k, v in self.model.state_dict().items()}
