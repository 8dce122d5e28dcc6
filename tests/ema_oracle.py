"""The weight-EMA oracle of tests/test_ema.py and tests/test_gpu_ema.py: a float64 replay, the criteria both
files hold the optimizers to, and an fp32 emulation of the documented formula into which faults can be injected
(tests/test_ema.py shows that the criteria catch them). Written from the formula; shares no code with the package.

Formula, per element of every tensor stepped (omd = float32(1 - decay)):

    first step of a tensor:  e_old = p_old                (fp32 clone of the fp32 target before the update)
    every step:              e = fmaf(omd, p_new - e_old, e_old)

Criteria (bounds from the arithmetic, not measured):

* exact -- omd a power of two: omd * (p_new - e_old) is exact in fp32 (no subnormals at randn scale), so the fused
  and the multiply-then-add form round once, identically: e must equal the fp32 replay bit for bit.
* bound -- any decay: the subtraction rounds once (half an ulp of p_new - e_old, scaled by omd) and the fused add
  once (half an ulp of e), so |e - ref64| <= 2^-23 * (|ref64| + omd * |p_new - e_old|) holds with a factor 2 to
  spare; the unfused torch form adds one rounding of the product, still inside it.
* untouched -- a tensor without a gradient keeps its EMA (or its absence) bit for bit.
"""
import torch

FAULTS = ("decay_for_omd", "from_p_old", "from_shadow", "no_init", "advance_without_grad")
EXACT_DECAYS = (1 - 2.0 ** -3, 1 - 2.0 ** -10)
GENERAL_DECAYS = (0.999, 0.9999)


def omd32(decay: float) -> float:
    """float32(1 - decay) as a Python float: the value the device scalar holds."""
    return float(torch.tensor(1.0 - decay, dtype=torch.float32))


def ema_oracle_step(E, P_old, P_new, grads, omd: float) -> None:
    """float64, in place on the list ``E`` (None = no EMA yet): the step that took ``P_old`` to ``P_new``."""
    for i, g in enumerate(grads):
        if g is None:
            continue
        if E[i] is None:
            E[i] = P_old[i].clone()
        E[i] = E[i] + omd * (P_new[i] - E[i])


def replay32(e_old, p_new, omd: float):
    """The fp32 torch replay: e_old + omd * (p_new - e_old), product and sum rounded separately."""
    return e_old + (p_new - e_old) * omd


def bound_violations(e, e_old, p_new, omd: float) -> int:
    """Elements outside |e - ref64| <= 2^-23 * (|ref64| + omd * |p_new - e_old|)."""
    e64, o64, p64 = e.double(), e_old.double(), p_new.double()
    d = p64 - o64
    ref = o64 + omd * d
    return int(((e64 - ref).abs() > 2.0 ** -23 * (ref.abs() + omd * d.abs())).sum())


def check_step(before, after, stepped, omd: float, exact: bool):
    """The criteria on one step. ``before`` / ``after``: per tensor ``(fp32 target, EMA or None)`` snapshots
    around the step; ``stepped``: whether the tensor had a gradient. Returns the set of criteria that failed:
    "replay" (a tensor that had an EMA), "first" (its first step: e_old is the target before the update),
    "untouched" (no gradient), "missing" (stepped but no EMA afterwards)."""
    failed = set()
    for (p_old, e_old), (p_new, e), s in zip(before, after, stepped):
        if not s:
            same = (e is None and e_old is None) or (e is not None and e_old is not None and torch.equal(e, e_old))
            if not same:
                failed.add("untouched")
            continue
        if e is None:
            failed.add("missing")
            continue
        name = "first" if e_old is None else "replay"
        start = p_old if e_old is None else e_old
        assert e.dtype == torch.float32 and start.dtype == torch.float32 and p_new.dtype == torch.float32
        if exact:
            ok = torch.equal(e, replay32(start, p_new, omd))
        else:
            ok = bound_violations(e, start, p_new, omd) == 0
        if not ok:
            failed.add(name)
    return failed


class Emulation:
    """fp32 emulation of the documented formula on plain SGD (p -= lr * g on fp32 masters with bf16 shadows),
    with one optional fault of ``FAULTS`` injected."""

    def __init__(self, params, decay: float, lr: float = 0.1, fault=None):
        assert fault is None or fault in FAULTS
        self.p = [t.clone().float() for t in params]
        self.e = [None] * len(params)
        self.decay, self.lr, self.fault = decay, lr, fault

    def snapshot(self):
        return [(p.clone(), None if e is None else e.clone()) for p, e in zip(self.p, self.e)]

    def step(self, grads) -> None:
        omd = omd32(1.0 - self.decay) if self.fault == "decay_for_omd" else omd32(self.decay)
        for i, g in enumerate(grads):
            if g is None:
                if self.fault == "advance_without_grad" and self.e[i] is not None:
                    self.e[i] = replay32(self.e[i], self.p[i], omd)
                continue
            p_old = self.p[i]
            p_new = p_old - self.lr * g.float()
            if self.e[i] is None:
                self.e[i] = torch.zeros_like(p_old) if self.fault == "no_init" else p_old.clone()
            src = p_new
            if self.fault == "from_p_old":
                src = p_old
            elif self.fault == "from_shadow":
                src = p_new.to(torch.bfloat16).float()
            self.e[i] = replay32(self.e[i], src, omd)
            self.p[i] = p_new
