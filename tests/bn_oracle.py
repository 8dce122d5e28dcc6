"""Exact-statistics oracle for the fused BatchNorm kernels (test_gpu_bn_exact.py; checked on the CPU by
test_bn_oracle.py). Shares no code with the package and is importable without a GPU.

Data. Rows are M = N*H*W, channels C. x = z + mu_c with integer noise z in [-3, 3] and an integer channel mean
mu_c in [-2, 2]; every channel is nudged by +-1 until sum z = 0, so the channel mean is the integer mu_c. dy,
the residual and a second BN's input are integers of the same kind. Everything is bf16-exact, so the same
tensors serve bf16 and fp32. The per-block sums of the kernels (S = sum (x - K), Q = sum (x - K)^2 with K = row
0, and the unshifted sums of the GEMM-epilogue statistics) are integers below 2^24: exact in fp32 in any order.
Row 0 is drawn within 1 of the mean: the kernels' variance Q/M - (S/M)^2 cancels, and with |S/M| <= 1 its
rounding stays far enough below the invstd bound when M is no power of two. Channel 0 is constant (variance
exactly 0), channel 1 has variance about 1/64 (eps = 1e-5 moves its invstd by about 3e-4) and mean 0, channel 2
has mean 2.

Two regimes. M a power of two ("exact"): 1/M, mean and the biased variance are exact, and the backward sums
sum dy' and sum dy'(x - mean) are integers. Any other M ("ragged"): the same data; only sum dy' and the
forward S, Q stay exact.

Criteria (one ulp = 2^-23 of the magnitude named; see the functions): the per-channel quantities within a few
ulp of float64, every per-element pass equal to a replay from the kernel's own coefficients, dx within
2^-20 |k1| (|dy'| + |m1| + |(x - mean) k2|) of float64 (for bf16: the rounding of some value in that interval).
No element is excluded anywhere.

The module also holds a plain-torch fp32 emulation of each documented formula with a ``fault=`` switch, which
test_bn_oracle.py uses to show that the criteria hold for a correct implementation and catch the listed defects.
"""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

ULP = 2.0 ** -23
EXACT_LIMIT = 1 << 24
PRE_MIN = 2.0 ** -10  # every ReLU pre-activation is farther than this from 0 (float64, asserted)

# bounds in ulp (of the magnitude each check names)
B_MEAN_RAGGED = 2.0
B_INVSTD = 4.0
B_COEF = 4.0      # scale, shift, running mean / var, m1, k2
B_DGAMMA_RAGGED = 8.0
DX_T = 2.0 ** -20
TWO_VALUED_MAX = 0.01


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(int(seed))


def is_pow2(m: int) -> bool:
    return m >= 1 and (m & (m - 1)) == 0


def f32(v: float) -> float:
    """A Python float rounded to fp32 (what a kernel argument of type float holds)."""
    return float(torch.tensor(float(v), dtype=torch.float32))


# ------------------------------------------------------------------------------------------------- data
def _balance(z: torch.Tensor) -> None:
    """Nudge rows 1.. of every channel by +-1 (staying in [-3, 3]) until the channel sums are 0."""
    for _ in range(8):
        s = z.sum(0)
        if not bool(s.any()):
            return
        body = z[1:]
        el = body > -3
        dec = el & (el.cumsum(0) <= s.clamp(min=0))
        eh = body < 3
        inc = eh & (eh.cumsum(0) <= (-s).clamp(min=0))
        z[1:] = body - dec.float() + inc.float()
    raise AssertionError("channel sums could not be balanced")


def channel_data(M: int, C: int, g: torch.Generator):
    """(x [M, C] fp32 integer-valued, mu [C]): see the module docstring."""
    assert M >= 1 and C >= 8 and C % 8 == 0
    mu = torch.randint(-2, 3, (C,), generator=g).float()
    z = torch.randint(-3, 4, (M, C), generator=g).float()
    z[0] = torch.randint(-1, 2, (C,), generator=g).float() if M > 1 else 0.0
    z[:, 0] = 0.0                          # constant channel
    mu[0] = 1.0 if is_pow2(M) else 0.0    # ragged M: unshifted statistics would cancel mu^2 inexactly
    z[:, 1] = 0.0                          # variance about 1/64, mean 0
    mu[1] = 0.0
    if M >= 4:
        k = max(1, round(M / 128))
        idx = torch.randperm(M - 1, generator=g)[:2 * k] + 1
        z[idx[:k], 1], z[idx[k:], 1] = 1.0, -1.0
    mu[2] = 2.0
    _balance(z)
    x = z + mu
    assert torch.equal(x.sum(0), M * mu) and float(x.abs().max()) <= 5
    assert float(((x - x[0]) ** 2).sum(0).max()) < EXACT_LIMIT, "shifted sum of squares leaves the exact range"
    assert float((x * x).sum(0).max()) < EXACT_LIMIT, "unshifted sum of squares leaves the exact range"
    return x, mu


def ints(shape, g: torch.Generator, lo: int = -3, hi: int = 3) -> torch.Tensor:
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


def bn_params(C: int, g: torch.Generator, affine: bool = True):
    """gamma in [0.5, 1.5], beta in [-0.5, 0.5], non-trivial running statistics."""
    p = SimpleNamespace()
    p.gamma = (torch.rand(C, generator=g) + 0.5) if affine else None
    p.beta = (torch.rand(C, generator=g) - 0.5) if affine else None
    p.rm0 = torch.rand(C, generator=g) * 2 - 1
    p.rv0 = torch.rand(C, generator=g) * 1.5 + 0.5
    return p


def stats64(x: torch.Tensor, eps: float):
    """(mean, biased var, invstd) in float64; eps rounded to fp32 first."""
    xd = x.double()
    mean = xd.mean(0)
    var = ((xd - mean) ** 2).mean(0)
    return mean, var, (var + f32(eps)).rsqrt()


def relu_case(x, p, eps, g, res=None, xd=None, pd=None, eps_d=None):
    """Set beta = 0.5 gamma invstd64 (both BNs), so that the sign of every pre-activation
    gamma invstd (x - mean + 0.5) is decided by an integer; with a residual or a second BN redraw the gamma of
    every channel that has a pre-activation within 2^-10 of 0."""
    mean, _, invstd = stats64(x, eps)
    if xd is not None:
        meand, _, invstdd = stats64(xd, eps_d)
        pd.beta = (0.5 * pd.gamma.double() * invstdd).float()
    for _ in range(64):
        p.beta = (0.5 * p.gamma.double() * invstd).float()
        pre = p.gamma.double() * invstd * (x.double() - mean) + p.beta.double()
        if res is not None:
            pre = pre + res.double()
        if xd is not None:
            pre = pre + pd.gamma.double() * invstdd * (xd.double() - meand) + pd.beta.double()
        bad = (pre.abs() <= 4 * PRE_MIN).any(0)
        if not bool(bad.any()):
            return
        p.gamma = torch.where(bad, torch.rand(p.gamma.shape, generator=g) + 0.5, p.gamma)
    raise AssertionError("could not separate the pre-activations from 0")


# -------------------------------------------------------------------------------------- float64 reference
def ref_fwd(x, p, eps, momentum, relu=False, res=None, xd=None, refd=None):
    """Every forward quantity in float64. ``refd``: the second BN's ref_fwd (its pre-activation is added)."""
    M = x.shape[0]
    r = SimpleNamespace(M=M, exact=is_pow2(M))
    r.mean, r.var, r.invstd = stats64(x, eps)
    g = p.gamma.double() if p.gamma is not None else torch.ones_like(r.mean)
    b = p.beta.double() if p.beta is not None else torch.zeros_like(r.mean)
    r.gamma, r.beta = g, b
    r.scale = g * r.invstd
    r.shift_terms = (b, r.mean * g * r.invstd)
    r.shift = b - r.mean * g * r.invstd
    mom = f32(momentum)
    unb = r.var * M / (M - 1) if M > 1 else r.var
    r.rm_terms = ((1 - mom) * p.rm0.double(), mom * r.mean)
    r.rv_terms = ((1 - mom) * p.rv0.double(), mom * unb)
    r.rm, r.rv = sum(r.rm_terms), sum(r.rv_terms)
    r.bn = (x.double() - r.mean) * r.scale + b
    pre = r.bn.clone()
    if res is not None:
        pre = pre + res.double()
    if refd is not None:
        pre = pre + refd.bn
    r.pre = pre
    if relu:
        assert float(pre.abs().min()) > PRE_MIN, "a pre-activation is within 2^-10 of 0"
    r.bits = pre > 0
    r.y = pre.clamp(min=0) if relu else pre
    return r


def ref_bwd(x, dy, rf, bits=None, two_valued_max=TWO_VALUED_MAX):
    """Every backward quantity in float64. ``bits``: the ReLU mask (None: no ReLU). Asserts, on the reference alone,
    that at most ``two_valued_max`` of the bf16 dx elements admit two values."""
    M = x.shape[0]
    b = SimpleNamespace(M=M, exact=rf.exact)
    dyp = dy.double() * bits.double() if bits is not None else dy.double()
    xc = x.double() - rf.mean
    b.dyp = dyp
    b.S = dyp.sum(0)
    b.Q = (dyp * xc).sum(0)
    b.A = (dyp * xc).abs().sum(0)
    b.dgamma = b.Q * rf.invstd
    b.dbeta = b.S
    b.k1 = rf.gamma * rf.invstd
    b.m1 = b.S / M
    b.k2 = rf.invstd * rf.invstd * b.Q / M
    b.dx = b.k1 * (dyp - b.m1 - xc * b.k2)
    b.t = DX_T * b.k1.abs() * (dyp.abs() + b.m1.abs() + (xc * b.k2).abs())
    lo, hi = (b.dx - b.t).float().to(torch.bfloat16), (b.dx + b.t).float().to(torch.bfloat16)
    b.two_valued = int((lo != hi).sum())
    # (with 1 or 2 rows dx is 0 or nearly 0 by construction, and an interval around 0 spans many tiny bf16 values)
    assert M < 64 or b.two_valued <= two_valued_max * b.dx.numel(), \
        f"{b.two_valued} of {b.dx.numel()} dx elements admit two bf16 values (> {two_valued_max:.0%})"
    if rf.exact:
        assert torch.equal(b.Q, b.Q.round()) and float(b.Q.abs().max()) < EXACT_LIMIT
    assert torch.equal(b.S, b.S.round()) and float(b.S.abs().max()) < EXACT_LIMIT
    return b


# ------------------------------------------------------------------------------- replay of per-element passes
def fma64(x: torch.Tensor, sc: torch.Tensor, sh: torch.Tensor) -> torch.Tensor:
    """fl32(x * sc + sh) with one rounding, evaluated in float64: the product of a small integer and an fp32 is
    exact there, and the sum is asserted exact (TwoSum residual 0). Returns fp32."""
    p = x.double() * sc.double()
    h = sh.double().expand_as(p)
    s = p + h
    bb = s - p
    err = (p - (s - bb)) + (h - bb)
    bad = (err != 0) & torch.isfinite(s)  # a non-finite operand gives the same non-finite result either way
    assert not bool(bad.any()), f"{int(bad.sum())} inexact float64 evaluations of the fma"
    return s.float()


def replay_fwd(x, ws, relu, dtype, res=None, xd=None, wsd=None):
    """(y, bits) of the apply pass from the kernel's own scale / shift (ws[2C:4C]):
    bf16_rne(relu(fl32(x sc + sh) [+ res | + fl32(xd sc2 + sh2)]))."""
    C = x.shape[1]
    o = fma64(x, ws[2 * C:3 * C], ws[3 * C:4 * C])
    if xd is not None:
        o = o + fma64(xd, wsd[2 * C:3 * C], wsd[3 * C:4 * C])
    elif res is not None:
        o = o + res.float()
    bits = o > 0
    if relu:
        o = o.clamp(min=0)
    return o.to(dtype), bits


def pack_bits(bits: torch.Tensor) -> torch.Tensor:
    """[M, C] booleans as the kernels' mask bytes: element i (row-major) is bit i % 8 of byte i // 8."""
    b = bits.reshape(-1, 8).to(torch.int32)
    w = (1 << torch.arange(8, dtype=torch.int32, device=bits.device))
    return (b * w).sum(1).to(torch.uint8)


def unpack_bits(mask: torch.Tensor, M: int, C: int) -> torch.Tensor:
    m = mask.to(torch.int32)
    return torch.stack([(m >> j) & 1 for j in range(8)], 1).reshape(-1)[:M * C].reshape(M, C).bool()


def pool_out(n: int, k: int, s: int, p: int, ceil: bool) -> int:
    o = (n + 2 * p - k + (s - 1 if ceil else 0)) // s + 1
    if ceil and (o - 1) * s >= n + p:
        o -= 1
    return o


def _windows(a, k, s, p, ceil):
    """[N, C, OH, OW, k*k] windows of a [N, C, H, W] (float), -inf outside the input."""
    n, c, h, w = a.shape
    oh, ow = pool_out(h, k, s, p, ceil), pool_out(w, k, s, p, ceil)
    ph, pw = (oh - 1) * s + k - h - p, (ow - 1) * s + k - w - p
    ap = F.pad(a.float(), (p, max(pw, 0), p, max(ph, 0)), value=float("-inf"))
    return ap.unfold(2, k, s).unfold(3, k, s)[:, :, :oh, :ow].reshape(n, c, oh, ow, k * k)


def pool_ref(a, k, s, p, ceil=False):
    """(values, positions) of the row-major first maximum of each window, NaN winning (the first NaN): the rule of
    _pool_reference in test_gpu_pool.py. ``a``: the rounded BN+ReLU output, [N, C, H, W]."""
    win = _windows(a, k, s, p, ceil)
    nan = torch.isnan(win)
    idx = torch.where(nan.any(-1), nan.float().argmax(-1), torch.nan_to_num(win, nan=0.0).argmax(-1))
    return torch.gather(win, -1, idx.unsqueeze(-1)).squeeze(-1), idx


def pool_gather(dyp, pos, H, W, k, s, p):
    """The full-resolution gradient the pooled backward gathers: pixel (h, w) receives dyp of every window whose
    recorded position is that pixel. Integer data: exact."""
    n, c, oh, ow = dyp.shape
    hp, wp = max((oh - 1) * s + k, H + p), max((ow - 1) * s + k, W + p)
    buf = torch.zeros(n, c, hp, wp, dtype=torch.float64, device=dyp.device)
    for q in range(k * k):
        ky, kx = divmod(q, k)
        buf[:, :, ky:ky + (oh - 1) * s + 1:s, kx:kx + (ow - 1) * s + 1:s] += dyp.double() * (pos == q)
    return buf[:, :, p:p + H, p:p + W]


def rows(t: torch.Tensor) -> torch.Tensor:
    """[N, C, H, W] -> [N*H*W, C]; 2-D tensors as they are."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) if t.dim() == 4 else t


def nchw(t2: torch.Tensor, N: int, H: int, W: int) -> torch.Tensor:
    """[M, C] rows -> a channels_last [N, C, H, W] tensor."""
    return t2.reshape(N, H, W, t2.shape[1]).permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)


# --------------------------------------------------------------------------------------------- the checks
class Report:
    """Collects the worst error of every quantity (in ulp of its named magnitude) and the failures."""

    def __init__(self, M: int, C: int, rpb: int = 0):
        self.M, self.C, self.rpb = M, C, rpb
        self.worst, self.failures, self.two_valued, self.bf16_dx = {}, [], 0, 0

    def _where(self, bad: torch.Tensor) -> str:
        idx = bad.nonzero().cpu()
        head = [tuple(i.tolist()) for i in idx[:6]]
        msg = f"{idx.shape[0]} of {bad.numel()} differ; first {head}"
        if bad.dim() == 2:
            ch = torch.unique(idx[:, 1])
            msg += f"; channels {ch[:8].tolist()}{' ...' if ch.numel() > 8 else ''} ({ch.numel()} of {bad.shape[1]})"
            if self.rpb:
                rb = torch.unique(idx[:, 0] // self.rpb)
                msg += f"; row blocks of {self.rpb}: {rb[:8].tolist()}{' ...' if rb.numel() > 8 else ''}"
        else:
            msg += f"; channels {[h[0] for h in head]}"
        return msg

    def equal(self, name, got, ref):
        g, r = got.detach().double(), ref.detach().double().to(got.device)
        if tuple(g.shape) != tuple(r.shape):
            self.failures.append(f"{name}: shape {tuple(g.shape)} != {tuple(r.shape)}")
            return
        bad = ~(g == r)  # NaN never equal, signed zero irrelevant
        self.worst.setdefault(name, 0.0)
        if bool(bad.any()):
            self.worst[name] = float("inf")
            self.failures.append(f"{name}: not equal: {self._where(bad)}")

    def within(self, name, got, ref, mag, bound):
        """|got - ref| <= bound ulp of ``mag`` (a magnitude per element, float64)."""
        g, r = got.detach().double(), ref.detach().double().to(got.device)
        mag = mag.detach().double().to(got.device)
        err = (g - r).abs()
        u = torch.where(err == 0, torch.zeros_like(err), err / (mag * ULP))
        u = torch.nan_to_num(u, nan=float("inf"))
        self.worst[name] = max(self.worst.get(name, 0.0), float(u.max()) if u.numel() else 0.0)
        bad = ~(u <= bound)
        if bool(bad.any()):
            self.failures.append(f"{name}: beyond {bound} ulp (worst {float(u.max()):.3g}): {self._where(bad)}")

    def ok(self) -> bool:
        return not self.failures

    def assert_ok(self, what: str = ""):
        assert self.ok(), what + ": " + " | ".join(self.failures)


def _mx(*ts):
    out = ts[0].abs()
    for t in ts[1:]:
        out = torch.maximum(out, t.abs())
    return out


def check_ws_fwd(rep, ws, rf, K, rm=None, rv=None, tag=""):
    """ws[0:4C] and the running statistics against float64. ``K``: the kernel's shift (row 0, or 0 for unshifted
    statistics), whose magnitude is a term of the mean."""
    C = rf.mean.shape[0]
    w = ws.detach().double().cpu()
    if rf.exact:
        rep.equal(tag + "mean", w[:C], rf.mean)
    else:
        rep.within(tag + "mean", w[:C], rf.mean, _mx(rf.mean, K.double(), rf.mean - K.double()).clamp(min=1e-30),
                   B_MEAN_RAGGED)
    rep.within(tag + "invstd", w[C:2 * C], rf.invstd, rf.invstd, B_INVSTD)
    rep.within(tag + "scale", w[2 * C:3 * C], rf.scale, rf.scale, B_COEF)
    rep.within(tag + "shift", w[3 * C:4 * C], rf.shift, _mx(*rf.shift_terms).clamp(min=1e-30), B_COEF)
    if rm is not None:
        rep.within(tag + "running_mean", rm.cpu(), rf.rm, _mx(*rf.rm_terms), B_COEF)
        rep.within(tag + "running_var", rv.cpu(), rf.rv, _mx(*rf.rv_terms), B_COEF)


def check_bwd_coefs(rep, ws, dgamma, dbeta, rf, rb, tag=""):
    """dgamma, dbeta and ws[4C:7C] (k1, m1, k2)."""
    C = rf.mean.shape[0]
    w = ws.detach().double().cpu()
    M = rb.M
    rep.equal(tag + "dbeta", dbeta.cpu(), rb.dbeta)
    if rb.exact:
        rep.equal(tag + "dgamma", dgamma.cpu(), (rb.Q.float() * w[C:2 * C].float()))
        k2mag = rb.k2.abs()
    else:
        rep.within(tag + "dgamma", dgamma.cpu(), rb.dgamma, (rf.invstd * rb.A).clamp(min=1e-30), B_DGAMMA_RAGGED)
        k2mag = rf.invstd * rf.invstd * rb.A / M  # the ragged sum's error is relative to sum |dy'(x - mean)|
    rep.within(tag + "k1", w[4 * C:5 * C], rb.k1, rb.k1, B_COEF)
    rep.within(tag + "m1", w[5 * C:6 * C], rb.m1, rb.m1.abs().clamp(min=1e-30), B_COEF)
    rep.within(tag + "k2", w[6 * C:7 * C], rb.k2, k2mag.clamp(min=1e-30), B_COEF)


def check_dx(rep, dx, rb, name="dx", ref=None, t=None):
    """fp32: within t of float64. bf16: the rounding of some value in [dx64 - t, dx64 + t]."""
    ref = rb.dx if ref is None else ref
    t = rb.t if t is None else t
    g = dx.detach().cpu()
    if g.dtype == torch.bfloat16:
        lo, hi = (ref - t).float().to(torch.bfloat16).double(), (ref + t).float().to(torch.bfloat16).double()
        gd = g.double()
        bad = ~((gd >= lo) & (gd <= hi))
        rep.two_valued += int((lo != hi).sum())
        rep.bf16_dx += gd.numel()
        rep.worst.setdefault(name, 0.0)
        if bool(bad.any()):
            rep.worst[name] = float("inf")
            rep.failures.append(f"{name}: not a rounding of the admissible interval: {rep._where(bad)}")
    else:
        err = (g.double() - ref).abs()
        u = torch.where(err == 0, torch.zeros_like(err), err / t)
        u = torch.nan_to_num(u, nan=float("inf"))
        rep.worst[name + " (t)"] = max(rep.worst.get(name + " (t)", 0.0), float(u.max()))
        bad = ~(u <= 1.0)
        if bool(bad.any()):
            rep.failures.append(f"{name}: beyond t (worst {float(u.max()):.3g} t): {rep._where(bad)}")


# ---------------------------------------------------------------------------- fp32 emulation with faults
FAULTS = ("eps_dropped", "eps_swapped", "momentum_other", "no_bessel", "row_dropped", "row_twice", "m1_dropped",
          "k2_dropped", "truncate", "mask_neighbour", "tap_dropped", "tie_last")


def _t32(v):
    return torch.tensor(float(v), dtype=torch.float32)


def _store(o: torch.Tensor, dtype, fault=None) -> torch.Tensor:
    if dtype == torch.bfloat16 and fault == "truncate":
        return (o.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
    return o.to(dtype)


def _row_weights(M, fault, nrb=4):
    """1 per row; the last row of the first of ``nrb`` row blocks dropped / counted twice."""
    w = torch.ones(M, 1, dtype=torch.float64)
    if fault in ("row_dropped", "row_twice") and M >= 2:
        per = (M + nrb - 1) // nrb
        w[min(per, M) - 1] = 0.0 if fault == "row_dropped" else 2.0
    return w


def emu_stats(x, fault=None, shifted=True):
    """(K, S, Q): the statistics pass (shifted by row 0) or the GEMM epilogue's unshifted sums."""
    K = x[0].float().clone() if shifted else torch.zeros(x.shape[1])
    d = x.double() - K.double()
    w = _row_weights(x.shape[0], fault)
    return K, (d * w).sum(0).float(), (d * d * w).sum(0).float()


def emu_finalize(K, S, Q, M, p, eps, momentum, fault=None, momentum_other=None):
    """bn_stats_finalize_body, operation by operation in fp32. Returns (ws[0:4C], rm, rv)."""
    inv_m = _t32(1.0) / _t32(M)
    dm = S * inv_m
    mean = K + dm
    v0 = Q * inv_m - dm * dm
    var = torch.where(v0 < 0, torch.zeros_like(v0), v0)
    e = _t32(eps)
    if fault == "eps_dropped":
        e = _t32(0.0)
    elif fault == "eps_swapped":
        e = _t32(1e-3 if eps < 5e-4 else 1e-5)
    invstd = torch.rsqrt(var + e)
    g = p.gamma if p.gamma is not None else torch.ones_like(mean)
    b = p.beta if p.beta is not None else torch.zeros_like(mean)
    ws = torch.cat([mean, invstd, g * invstd, b - mean * g * invstd])
    mom = _t32(momentum_other if fault == "momentum_other" else momentum)
    unb = var * _t32(M) / _t32(M - 1) if (M > 1 and fault != "no_bessel") else var
    rm = (_t32(1.0) - mom) * p.rm0 + mom * mean
    rv = (_t32(1.0) - mom) * p.rv0 + mom * unb
    return ws, rm, rv


def emu_apply(x, ws, relu, dtype, res=None, xd=None, wsd=None, fault=None):
    """(y, mask bytes or None): the apply pass. The fma is one rounding of the float64 value (exact for the oracle's
    data; for other data a double rounding may differ from the hardware fma in rare last bits)."""
    C = x.shape[1]

    def fma(a, w):
        return (a.double() * w[2 * C:3 * C].double() + w[3 * C:4 * C].double()).float()

    o = fma(x, ws)
    if xd is not None:
        o = o + fma(xd, wsd)
    elif res is not None:
        o = o + res.float()
    bits = o > 0
    if relu:
        o = o.clamp(min=0)
    mask = None
    if relu and (res is not None or xd is not None):
        if fault == "mask_neighbour":
            bits = torch.roll(bits, 8, dims=1)
        mask = pack_bits(bits)
    return _store(o, dtype, fault), mask


def emu_bwd(x, dy, ws, p, dtype, bits=None, fault=None, want_dx=True):
    """Backward reduce, finalize and apply in fp32. Returns (dx, dres, dgamma, dbeta, ws[4C:7C])."""
    M, C = x.shape
    mean, invstd = ws[:C], ws[C:2 * C]
    dyp = dy.float() * bits.float() if bits is not None else dy.float()
    xc = x.float() - mean
    w = _row_weights(M, fault)
    S = (dyp.double() * w).sum(0).float()
    Q = (dyp.double() * xc.double() * w).sum(0).float()
    g = p.gamma if p.gamma is not None else torch.ones_like(mean)
    inv_m = _t32(1.0) / _t32(M)
    k1, m1, k2 = g * invstd, S * inv_m, invstd * invstd * Q * inv_m
    dx = None
    if want_dx:
        a1 = torch.zeros_like(m1) if fault == "m1_dropped" else m1
        a2 = torch.zeros_like(k2) if fault == "k2_dropped" else k2
        dx = _store(k1 * (dyp - a1 - xc * a2), dtype, fault)
    return dx, _store(dyp, dtype), Q * invstd, S, torch.cat([k1, m1, k2])


def emu_pool_fwd(a, k, s, p, ceil=False, fault=None):
    """(values, positions): a running row-major scan of each window with a strict '>' (first maximum)."""
    win = _windows(a, k, s, p, ceil)
    best = torch.full(win.shape[:-1], float("-inf"))
    pos = torch.zeros(win.shape[:-1], dtype=torch.int64)
    for q in range(k * k):
        if fault == "tap_dropped" and q == k * k - 1:
            continue
        v = win[..., q]
        take = (v >= best) & (v > float("-inf")) if fault == "tie_last" else v > best
        best = torch.where(take, v, best)
        pos = torch.where(take, torch.full_like(pos, q), pos)
    return best, pos


# ------------------------------------------------------------------------------------------ whole cases
def check_apply(rep, y, mask, x, ws, rf, relu, res=None, xd=None, wsd=None, tag=""):
    """y (rows [M, C]) and the mask equal the replay from the kernel's own coefficients, on y's device; the ReLU
    bits of the replay and of the mask equal the float64 reference's (each has one correct value)."""
    dev = y.device
    mv = lambda t: None if t is None else t.to(dev)  # noqa: E731
    yr, bits = replay_fwd(mv(x), ws.to(dev), relu, y.dtype, mv(res), mv(xd), mv(wsd))
    rep.equal(tag + "y", y, yr)
    if relu:
        rep.equal(tag + "relu bits", bits, rf.bits)
    if mask is not None:
        rep.equal(tag + "mask", unpack_bits(mask, *x.shape), rf.bits)


def make_case(M, C, seed, relu=False, use_res=False, dual=False, eps=1e-5, momentum=0.1, eps_d=1e-3,
              momentum_d=0.01, affine=True):
    """Data, parameters and float64 references of one BN(+residual | +BN_d)(+ReLU) forward / backward."""
    g = gen(seed)
    c = SimpleNamespace(M=M, C=C, relu=relu, eps=eps, momentum=momentum, eps_d=eps_d, momentum_d=momentum_d)
    c.x, c.mu = channel_data(M, C, g)
    c.dy = ints((M, C), g)
    c.res = ints((M, C), g) if use_res else None
    c.p = bn_params(C, g, affine or relu)
    c.xd = c.pd = c.rfd = None
    if dual:
        c.xd, _ = channel_data(M, C, g)
        c.pd = bn_params(C, g)
    if relu:
        relu_case(c.x, c.p, eps, g, c.res, c.xd, c.pd, eps_d)
    if dual:
        c.rfd = ref_fwd(c.xd, c.pd, eps_d, momentum_d)
    c.rf = ref_fwd(c.x, c.p, eps, momentum, relu, c.res, c.xd, c.rfd)
    bits = c.rf.bits if relu else None
    c.rb = ref_bwd(c.x, c.dy, c.rf, bits)
    c.rbd = ref_bwd(c.xd, c.dy, c.rfd, bits) if dual else None
    return c
