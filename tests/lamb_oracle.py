"""The oracle of the FusedLAMB / FusedAdamW tests (tests/test_lamb.py, tests/test_gpu_lamb.py), written from the
formula of the class docstring and sharing no code with the package:

* ``lamb_oracle_step``: one step in float64 with integer update counts and exact ``1 - beta**k``;
* ``lamb_emulate_step``: the same formula in fp32 torch, with a switch per way of getting it wrong (``FAULTS``), so
  that the tests can show that their bound catches each of them on their own inputs.
"""
import math

import torch

FAULTS = (
    "no_bias_correction",     # u from m and v without the 1 - beta^k divisions
    "eps_inside_sqrt",        # sqrt(v / bc2 + eps) instead of sqrt(v / bc2) + eps
    "coupled_weight_decay",   # wd * p added to the gradient instead of to u
    "trust_from_grad",        # trust = ||p|| / ||c g|| instead of ||p|| / ||u||   (LAMB only)
    "v_unscaled",             # v built from g instead of c g
    "wd_on_excluded",         # weight decay on a tensor excluded from it
    "count_gradless",         # the update count of a tensor without a gradient advanced
)


def hyper(opt):
    """The oracle's per-parameter hyper-parameters of a FusedLAMB / FusedAdamW, in param_groups order."""
    out = []
    for g in opt.param_groups:
        for p in g["params"]:
            out.append(dict(lr=g["lr"], beta1=g["betas"][0], beta2=g["betas"][1], eps=g["eps"],
                            weight_decay=g["weight_decay"], adapt=not (g["exclude_bias_and_norm"] and p.ndim <= 1)))
    return out


def _clip(gs, grad_scale, max_grad_norm):
    total = sum(float((g.double() * g.double()).sum()) for g in gs if g is not None)
    G = grad_scale * math.sqrt(total)
    clip = min(1.0, max_grad_norm / (G + 1e-6)) if max_grad_norm > 0 else 1.0
    return G, grad_scale * clip


def lamb_oracle_step(P, M, V, K, grads, hp, trust, grad_scale=1.0, max_grad_norm=0.0):
    """One step in float64, in place. ``P``, ``M``, ``V``: lists of float64 tensors (parameter or master and the two
    moments); ``K``: list of ints, the update counts; ``grads``: one tensor (any dtype) or None per parameter;
    ``hp``: one dict per parameter (``hyper``); ``trust``: LAMB (True) or AdamW (False). Returns (G, trust ratios,
    (bc1, bc2) pairs) with None for the tensors that were not stepped."""
    gs = [None if g is None else g.detach().double().cpu() for g in grads]
    G, c = _clip(gs, grad_scale, max_grad_norm)
    trusts, bcs = [], []
    for i, (p, m, v, g, h) in enumerate(zip(P, M, V, gs, hp)):
        if g is None:
            trusts.append(None)
            bcs.append(None)
            continue
        K[i] += 1
        bc1, bc2 = 1.0 - h["beta1"] ** K[i], 1.0 - h["beta2"] ** K[i]
        gh = c * g.reshape(p.shape)
        m.mul_(h["beta1"]).add_(gh, alpha=1.0 - h["beta1"])
        v.mul_(h["beta2"]).add_(gh * gh, alpha=1.0 - h["beta2"])
        wd = h["weight_decay"] if h["adapt"] else 0.0
        u = (m / bc1) / ((v / bc2).sqrt() + h["eps"]) + wd * p
        t = 1.0
        if trust and h["adapt"]:
            wn, un = math.sqrt(float((p * p).sum())), math.sqrt(float((u * u).sum()))
            if wn > 0 and un > 0:
                t = wn / un
        p.sub_(u, alpha=h["lr"] * t)
        trusts.append(t)
        bcs.append((bc1, bc2))
    return G, trusts, bcs


def lamb_emulate_step(P, M, V, K, grads, hp, trust, grad_scale=1.0, max_grad_norm=0.0, fault=None):
    """The documented formula in fp32 torch, in place on fp32 ``P``, ``M``, ``V`` and the int list ``K``; ``fault``:
    None or one of ``FAULTS``."""
    assert fault is None or fault in FAULTS
    f32 = torch.float32
    gs = [None if g is None else g.detach().to(f32).cpu() for g in grads]
    _, c = _clip(gs, grad_scale, max_grad_norm)
    c = torch.tensor(c, dtype=f32)
    for i, (p, m, v, g, h) in enumerate(zip(P, M, V, gs, hp)):
        if g is None:
            if fault == "count_gradless":
                K[i] += 1
            continue
        K[i] += 1
        k = torch.tensor(float(K[i]), dtype=f32)
        bc1, bc2 = (-torch.expm1(k * torch.tensor(math.log(b), dtype=f32)) for b in (h["beta1"], h["beta2"]))
        if fault == "no_bias_correction":
            bc1 = bc2 = torch.ones((), dtype=f32)
        wd = h["weight_decay"] if (h["adapt"] or fault == "wd_on_excluded") else 0.0
        gh = c * g.reshape(p.shape)
        if fault == "coupled_weight_decay":
            gh = gh + wd * p
        m.mul_(h["beta1"]).add_(gh, alpha=1.0 - h["beta1"])
        gv = g.reshape(p.shape) if fault == "v_unscaled" else gh
        v.mul_(h["beta2"]).add_(gv * gv, alpha=1.0 - h["beta2"])
        if fault == "eps_inside_sqrt":
            u = (m / bc1) / (v / bc2 + h["eps"]).sqrt()
        else:
            u = (m / bc1) / ((v / bc2).sqrt() + h["eps"])
        if fault != "coupled_weight_decay":
            u = u + wd * p
        t = torch.ones((), dtype=f32)
        if trust and h["adapt"]:
            wn = torch.linalg.vector_norm(p)
            un = torch.linalg.vector_norm(gh if fault == "trust_from_grad" else u)
            if wn > 0 and un > 0:
                t = wn / un
        p.sub_(u * (h["lr"] * t))


def worst_ratio(got, ref64, rtol, atol):
    """max |got - ref| / (atol + rtol |ref|) over the elements: <= 1 is what assert_close accepts."""
    got, ref = got.detach().double().cpu().reshape(-1), ref64.float().double().reshape(-1)
    if got.numel() == 0:
        return 0.0
    return float(((got - ref).abs() / (atol + rtol * ref.abs())).max())
