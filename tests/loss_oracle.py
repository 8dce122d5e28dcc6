"""Interval and replay oracle for the cross-entropy loss kernels of csrc/kernels/loss.hip (test_gpu_loss_exact.py;
checked on the CPU by test_loss_oracle.py). numpy only: it shares no code with the package and is importable
without a GPU.

The three pairs. ``plain``: lse = m + log(sum exp(x - m)) with the true row maximum m, row = lse - x[t], gradient
(exp(x - lse) - [c == t]) g. ``metrics``: the label-smoothed row lse - (1 - eps) x[t] - eps sum(x) / C (the last term
left out at eps == 0), the target's rank #{x_c > x_t} + #{c < t: x_c == x_t}, gradient
(exp(x - lse) - hot [c == t] - uni) g with hot = 1 - eps, uni = eps / C. ``mix``: the same with
x_t = lam x[ta] + (1 - lam) x[tb] (a term of weight exactly 0 left out) and hot split into ha = hot lam at ta,
hb = hot (1 - lam) at tb (added where ta == tb). A row is valid iff its target(s) lie in [0, C); g = gout / (valid
rows); an invalid row has row loss 0, rank +inf and a gradient of +0.0.

What is bitwise (no tolerance)
    valid flag and rank of every row against the float64 tie rule (+inf for an ignored row or a NaN target logit);
    the batch kernel's outputs against ``replay_batch``: a numpy-float32 replay of its fixed order from the kernel's
    own row values (thread i adds rows i, i + 256, ... from 0; xor butterfly 32..1 over 64 lanes; four wave totals
    left to right; one division). Only additions and one division: contraction cannot change them;
    the gradient of every invalid row: +0.0 in every bit.

Forward bound, in units of u = 2^-24 (``forward_bounds``; first order in u)
    The kernels hold s = sum_c exp(x_c - m) as fp32 partial sums per lane, each relative to the lane's running
    maximum and rescaled by exp(m_old - m_new) when the maximum rises, once more to the row maximum at the merge, then
    added over 64 lanes by a 6-level butterfly. fast exp(a) is exp2(a * log2e) on the hardware instruction.
    Term c reaches the total through
      * one subtraction x - m' (relative rounding u of |x - m'|, i.e. u |x - m'| in the exponent),
      * the product with log2e (its rounding and the constant's own: 2u |x - m'| in the exponent),
      * the exp instruction, E ulp = 2 E u relative,
      * R <= L + 1 rescales, L = ceil(C / 64) the most visits of one lane, each one exp of the same kind on
        m_old - m_new and one product rounding: (2E + 1) u + 3u (m_new - m_old) each. The exponent magnitudes
        of one term's chain add up to exactly m - x_c, so together 3u (m - x_c) + (L + 1)(2E + 1) u + 2 E u =: tau_c;
      * A - 1 additions, A = max(ceil(C / 64), N ceil(C / (64 N))) + 6 with N the elements of a 16-byte access
        (the issue counts ceil(C / 64) + 6; a lane of the 16-byte path makes N additions per visit, which is more
        when C is small), each u relative to a partial sum of non-negative terms: A u of s.
    A term below 2^-126 may be flushed: C 2^-126 absolute, against s >= 1. So
      |ds / s| <= A u + sum_c w_c tau_c + C 2^-126,   w_c = exp(x_c - m) / s      (float64, from the data)
      |lse - lse64| <= ds/s + 2 E u |log s| + u |lse|                              (the log, then m + log s)
    and for the row loss, with h = (1 - eps) x_t and mean = sum(x) / C:
      + u (2 |h| + |lse - h|)                   (1 - eps, its product, the subtraction)
      + eps u (A sum|x| / C + 2 |mean|)         (the plain sum, the division, the product with eps)
      + u |row|                                  (the last subtraction)
      + (1 - eps) u (|lam xa| + 2 |(1 - lam) xb| + |x_t|)   (mix only: 1 - lam, two products, one sum)
    A fused multiply-add only removes a rounding. The plain pair makes no rescale: its error is a subset.
    E is not stated by any document shipped with the toolchain this was written on (see
    profiles/loss_oracle/README.md), so E = 1 ulp is an ASSUMPTION and the whole bound carries the factor 4
    (``F_ASSUME``). Nothing here was fitted to a kernel's output.

Gradient interval (``grad_interval``), around the kernel's own lse_k and count
    g = fp32(gout / count) exactly (numpy float32 division; IEEE, as the device's); p = exp(x - lse_k) in float64 with
    relative error rho = F_ASSUME (3u |x - lse_k| + 2 E u) and 2^-126 absolute (flush). p - h, - uni and * g are
    carried as [lo, hi], each step widened by |v| u >= half an ulp of v. h, uni, ha + hb are formed in numpy float32
    exactly as documented. An fp32 output must lie in [lo, hi], a bf16 one in [bf16_rne(lo), bf16_rne(hi)] (rounding
    is monotone). Every entry of every valid row, no absolute floor.
    "A quarter of the bound" for an entry means the interval built with rho / 4: the half-ulp widenings are IEEE
    facts that a correct implementation may use up completely, the slack belongs to the assumed term.

The emulation (``emulate``) follows the documented lane order in numpy float32 with correctly rounded exp / log
(float64 results rounded once) and has a ``fault=`` switch (``FAULTS``).
"""
import functools
import math
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
E_ULP = 1.0      # assumed accuracy of the hardware exp2 / log2 path in ulp; see the module docstring
F_ASSUME = 4.0   # the factor the assumption costs
TINY = 2.0 ** -126
f32 = np.float32
NEG_INF = f32(-np.inf)

FAULTS = ("drop_uni", "hot_one", "uni_c_minus_1", "gout_ignored", "g_over_B", "expsum_skip_last_vec",
          "sum_skip_last_vec", "rank_skip_last_vec", "second_trip_alias", "batch_sum_256", "target_lane_shift",
          "ignored_not_zeroed", "no_rescale_lane", "no_rescale_merge", "smooth_at_eps0", "bf16_truncate",
          "mix_swap_hab", "mix_same_target_not_added", "mix_zero_weight_kept")

VEC_C = {"f32": (4, 256, 260, 1024, 1028, 2052), "bf16": (8, 512, 520, 2048, 2056, 4104)}
SCALAR_C = {"f32": (1, 63, 64, 65, 1001), "bf16": (1, 63, 64, 65, 1001, 2049)}
ROW_COUNTS = (1, 4, 5, 255, 256, 257, 513, 1283)
GOUTS = (1.0, -0.375, 1024.0)


def elems(dt: str) -> int:
    """Elements of one 16-byte access."""
    return 4 if dt == "f32" else 8


# ------------------------------------------------------------------------------------------------- bf16
def bf16_rne(a):
    """float32 values rounded to the nearest bf16 (ties to even), as float32; NaN stays NaN."""
    a = np.ascontiguousarray(a, dtype=f32)
    b = a.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16 << 16).astype(np.uint32).view(f32)
    return np.where(np.isnan(a), a, r).astype(f32)


def bf16_trunc(a):
    a = np.ascontiguousarray(a, dtype=f32)
    return (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(f32)


def store(a, dt):
    return bf16_rne(a) if dt == "bf16" else np.asarray(a, dtype=f32)


# ------------------------------------------------------------------------------------------------- cases
def _seed(name: str) -> int:
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (1 << 31)


@functools.lru_cache(maxsize=None)
def _random_logits(B, C, dt, seed):
    g = np.random.default_rng(seed)
    return store((g.standard_normal((B, C)) * 3.0).astype(f32), dt)


def _plant_ties(x, t):
    """Row i's target logit becomes the row's (i mod 10)-th largest value: ranks on both sides of k, exact ties."""
    x = x.copy()
    B, C = x.shape
    srt = -np.sort(-x, axis=1)
    for i in np.nonzero((t >= 0) & (t < C))[0]:
        x[i, t[i]] = srt[i, i % min(10, C)]
    return x


def _ascending_bf16(C):
    """C consecutive positive bf16 values ending at 32: strictly ascending, exact in bf16 and fp32."""
    bits = (np.arange(0x4200 - C + 1, 0x4200 + 1, dtype=np.uint32) << 16).astype(np.uint32)
    return bits.view(f32).copy()


def _structured(C, dt, seed):
    """The structured rows (module docstring of test_gpu_loss_exact.py); targets beside them."""
    g = np.random.default_rng(seed)
    N = elems(dt)
    far = min(C - 1, 256 * N + N + 1)  # inside the second trip's vector of lane 1 when the row has one
    rows, t = [], []
    asc = _ascending_bf16(C)
    rows.append(asc); t.append(C - 1)                                 # every visit of every lane a new maximum
    rows.append(asc[::-1].copy()); t.append(far)                      # the first visit holds the maximum
    rows.append(np.full(C, 0.5, f32)); t.append(C // 3)
    r = np.full(C, -20.0, f32); r[far] = 80.0
    rows.append(r); t.append(far)
    rows.append(r.copy()); t.append(2)
    rows.append((-9984.0 + 64.0 * g.integers(-2, 3, C)).astype(f32)); t.append(0)
    r = g.choice(np.array([0.0, 3.0, -110.0, -120.0], f32), C).astype(f32); r[far] = 3.0
    rows.append(r); t.append(far)                                      # spread above 104: small terms vanish
    r = np.full(C, -np.inf, f32)
    keep = sorted({0, 5 % C, far, C - 1})
    r[keep] = g.integers(-3, 4, len(keep)).astype(f32)
    rows.append(r); t.append(keep[1])                                  # whole lanes and whole vectors of -inf
    rows.append(r.copy()); t.append(far)
    rows.append(g.integers(-16, 17, C).astype(f32)); t.append(C - 2)   # exact plain sum
    rows.append(g.integers(-16, 17, C).astype(f32)); t.append(-100)
    rows.append(store((g.standard_normal(C) * 3).astype(f32), dt)); t.append(1)
    return np.stack(rows).astype(f32), np.array(t, np.int64), keep


def _sweep_targets(B, C, dt, g):
    N = elems(dt)
    far = 256 * N + N + 1 if C > 256 * N + N + 1 else C // 2
    t = [0, C - 1] + [max(C - N + j, 0) for j in range(N)] + [far]
    t += list(g.integers(0, C, B - len(t)))
    t = np.array(t[:B], np.int64)
    t[12], t[13] = -100, C + 3
    return t


def _ignore_blocks(t, C):
    """Ignored rows: the first row of a 4-row block, the last row of a block, a whole block."""
    t = t.copy()
    for i, v in ((4, -100), (11, C), (16, -1), (17, -100), (18, C + 7), (19, -100)):
        if i < len(t):
            t[i] = v
    return t


def _make(kind, B, C, dt, off=0):
    """(x, t, extra) of one input family; shared by the pairs and both eps."""
    seed = _seed(f"{kind}-{B}-{C}-{dt}")
    g = np.random.default_rng(seed + 1)
    extra = {}
    if kind == "structured":
        x, t, keep = _structured(C, dt, seed)
        extra["keep"] = keep
        return x, t, extra
    x = _random_logits(B, C, dt, seed)
    if kind == "sweep":
        t = _sweep_targets(B, C, dt, g)
    elif kind == "rows":
        t = _ignore_blocks(g.integers(0, C, B).astype(np.int64), C)
    elif kind == "ignored":
        t = np.array([-100, C, -1, C + 5, -100][:B], np.int64)
    elif kind == "nan":
        t = g.integers(0, C, B).astype(np.int64)
    else:
        raise ValueError(kind)
    x = _plant_ties(x, t)
    if kind == "nan":
        x[2, t[2]] = np.nan
    return x, t, extra


@functools.lru_cache(maxsize=None)
def _family(kind, B, C, dt):
    x, t, extra = _make(kind, B, C, dt)
    x.setflags(write=False)
    t.setflags(write=False)
    return x, t, extra


def _families():
    out = []
    for dt in ("f32", "bf16"):
        for C in VEC_C[dt] + SCALAR_C[dt]:
            out.append(("sweep", 16, C, dt, 0))
        out.append(("sweep", 16, 2056, dt, 1))      # an aligned pitch one element off alignment: scalar path
        for B in ROW_COUNTS:
            out.append(("rows", B, 40, dt, 0))
        out.append(("rows", 1283, 520, dt, 0))      # B * C beyond the plain backward's 2048 x 256 grid-stride span
        out.append(("ignored", 5, 40, dt, 0))
        out.append(("structured", 12, 1028 if dt == "f32" else 2056, dt, 0))
        out.append(("structured", 12, 1001, dt, 0))
    return out


def _build_case(name, kind, B, C, dt, off, pair, eps, idx):
    x, t, extra = _family(kind, B, C, dt)
    B = x.shape[0]
    c = SimpleNamespace(name=name, kind=kind, pair=pair, dt=dt, B=B, C=C, off=off, eps=float(eps), k=5,
                        x=x, ta=t, tb=None, lam=None, gout=GOUTS[idx % 3])
    c.vec = off == 0 and (C * (4 if dt == "f32" else 2)) % 16 == 0 and pair != "plain"
    if pair == "mix":
        g = np.random.default_rng(_seed(name))
        tb = g.integers(0, C, B).astype(np.int64)
        lam = g.random(B).astype(f32)
        rows = np.arange(B)
        lam[rows % 4 == 0], lam[rows % 4 == 1], lam[rows % 4 == 2] = 0.0, 1.0, 0.5
        same = rows % 5 == 3
        tb[same] = np.clip(t[same], 0, C - 1)
        if B > 14:
            tb[14] = -1                     # only the second target ignored
        if kind == "structured":            # a -inf logit at a target of weight 0
            keep = extra["keep"]
            tb[7], lam[7] = (keep[1] + 1) % C, 1.0
            tb[8], lam[8] = t[8], 0.0
            ta = t.copy()
            ta[8] = (keep[1] + 1) % C
            if not np.isneginf(x[7, tb[7]]) or not np.isneginf(x[8, ta[8]]):
                raise AssertionError("the weight-0 targets must sit on -inf logits")
            c.ta = ta
        c.tb, c.lam = tb, lam
    return c


@functools.lru_cache(maxsize=None)
def _index():
    table = {}
    for kind, B, C, dt, off in _families():
        for pair, eps in (("plain", 0.0), ("metrics", 0.0), ("metrics", 0.1), ("mix", 0.0), ("mix", 0.1)):
            name = f"{kind}-{B}x{C}{'+1' if off else ''}-{dt}-{pair}-eps{eps:g}"
            table[name] = (kind, B, C, dt, off, pair, eps, len(table))
    for dt in ("f32", "bf16"):
        table[f"nan-8x20-{dt}-metrics-eps0.1"] = ("nan", 8, 20, dt, 0, "metrics", 0.1, len(table))
    return table


def case_names():
    return list(_index())


def get_case(name):
    return _build_case(name, *_index()[name])


# ------------------------------------------------------------------------------------------------- float64 reference
def _valid(c):
    v = (c.ta >= 0) & (c.ta < c.C)
    if c.pair == "mix":
        v &= (c.tb >= 0) & (c.tb < c.C)
    return v


def reference(c):
    """float64 lse, row loss, valid, rank and the pieces the bounds need, from the documented operation."""
    x = c.x.astype(np.float64)
    B, C = x.shape
    rows = np.arange(B)
    eps = float(f32(c.eps))
    valid = _valid(c)
    with np.errstate(all="ignore"):
        m = x.max(axis=1)
        ex = np.where(np.isneginf(x), 0.0, np.exp(x - m[:, None]))
        S = ex.sum(axis=1)
        lse = m + np.log(S)
        ta = np.where(valid, c.ta, 0)
        xa = x[rows, ta]
        if c.pair == "mix":
            tb = np.where(valid, c.tb, 0)
            wa = c.lam.astype(np.float64)
            wb = 1.0 - wa
            pa = np.where(wa != 0, wa * xa, 0.0)
            pb = np.where(wb != 0, wb * x[rows, tb], 0.0)
            xt = pa + pb
        else:
            pa, pb, xt = xa, np.zeros(B), xa
        hot = 1.0 - eps
        mean = x.sum(axis=1) / C
        h = hot * xt
        row = lse - h - (eps * mean if eps > 0 else 0.0)
        row = np.where(valid, row, 0.0)
        rank = None
        if c.pair == "metrics":
            above = (x > xa[:, None]) | ((x == xa[:, None]) & (np.arange(C)[None, :] < ta[:, None]))
            rank = np.where(valid & ~np.isnan(xa), above.sum(axis=1).astype(np.float64), np.inf)
    return SimpleNamespace(x=x, m=m, ex=ex, S=S, lse=lse, row=row, valid=valid, rank=rank, xt=xt, pa=pa, pb=pb, h=h,
                           mean=mean, eps=eps, hot=hot)


def forward_bounds(c, r):
    """(bound on |lse - lse64|, bound on |row - row64|) per row; the derivation is in the module docstring."""
    C, N = c.C, elems(c.dt)
    L = math.ceil(C / 64)
    A = max(L, N * math.ceil(C / (64 * N))) + 6
    with np.errstate(all="ignore"):
        w = r.ex / r.S[:, None]
        dist = np.where(w > 0, r.m[:, None] - r.x, 0.0)
        tau = 3 * U * (w * dist).sum(axis=1) + (L + 1) * (2 * E_ULP + 1) * U + 2 * E_ULP * U
        ds = A * U + tau + C * TINY
        b_lse = ds + 2 * E_ULP * U * np.abs(np.log(r.S)) + U * np.abs(r.lse)
        b_row = b_lse + U * (2 * np.abs(r.h) + np.abs(r.lse - r.h)) + U * np.abs(r.row)
        if r.eps > 0:
            b_row = b_row + r.eps * U * (A * np.abs(r.x).sum(axis=1) / C + 2 * np.abs(r.mean))
        if c.pair == "mix":
            b_row = b_row + r.hot * U * (np.abs(r.pa) + 2 * np.abs(r.pb) + np.abs(r.xt))
    return F_ASSUME * b_lse, F_ASSUME * b_row


def replay_batch(row, valid, rank=None, k=None):
    """numpy-float32 replay of the one-workgroup batch kernel from the kernel's own rows: (sums, mean)."""
    cols = [np.asarray(row, f32), np.asarray(valid, f32)]
    if rank is not None:
        rk = np.asarray(rank, f32)
        cols += [(rk < f32(1)).astype(f32), (rk < f32(k)).astype(f32)]
    B = len(cols[0])
    tot = []
    with np.errstate(all="ignore"):
        for col in cols:
            acc = np.zeros(256, f32)
            for start in range(0, B, 256):
                part = col[start:start + 256]
                acc[:len(part)] = acc[:len(part)] + part
            lanes = acc.reshape(4, 64)
            for off in (32, 16, 8, 4, 2, 1):
                lanes = lanes + lanes[:, np.arange(64) ^ off]
            w = lanes[:, 0]
            tot.append(f32(f32(f32(w[0] + w[1]) + w[2]) + w[3]))
        mean = f32(tot[0] / tot[1]) if tot[1] > 0 else f32(np.nan)
    return np.array(tot, f32), mean


def _hot_terms(c):
    """The fp32 constants of the backward, formed as documented: (h [B, C] float64-exact fp32 values, uni)."""
    B, C = c.B, c.C
    eps = f32(c.eps)
    hot = f32(1) - eps
    uni = f32(eps / f32(C))
    cols = np.arange(C)[None, :]
    if c.pair == "mix":
        wa = c.lam.astype(f32)
        ha = (hot * wa).astype(f32)
        hb = (hot * (f32(1) - wa)).astype(f32)
        h = (np.where(cols == c.ta[:, None], ha[:, None], f32(0)).astype(f32)
             + np.where(cols == c.tb[:, None], hb[:, None], f32(0)).astype(f32)).astype(f32)
    else:
        h = np.where(cols == c.ta[:, None], hot if c.pair == "metrics" else f32(1), f32(0)).astype(f32)
        if c.pair == "plain":
            uni = f32(0)
    return h.astype(np.float64), float(uni)


def _widen(lo, hi):
    return lo - np.abs(lo) * U - 2.0 ** -150, hi + np.abs(hi) * U + 2.0 ** -150


def grad_interval(c, lse_k, count_k, share=1.0):
    """[lo, hi] (float64) of every entry around the kernel's own lse and valid count; ``share`` scales the
    assumed relative error of exp (1: the bound; 0.25: the quarter the emulation must keep)."""
    x = c.x.astype(np.float64)
    with np.errstate(all="ignore"):
        g = float(f32(c.gout) / f32(count_k))
        d = x - np.asarray(lse_k, np.float64)[:, None]
        p = np.exp(d)
        rho = share * F_ASSUME * (3 * U * np.where(p > 0, np.abs(d), 0.0) + 2 * E_ULP * U)
        lo, hi = p * (1 - rho) - TINY * (p > 0), p * (1 + rho) + TINY * (p > 0)
        h, uni = _hot_terms(c)
        lo, hi = _widen(lo - h, hi - h)
        lo, hi = _widen(lo - uni, hi - uni)
        a, b = lo * g, hi * g
        lo, hi = _widen(np.minimum(a, b), np.maximum(a, b))
    return lo, hi, g


# ------------------------------------------------------------------------------------------------- criteria
def _same_bits(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _ratio(got, ref, bound, what, fails):
    """Worst |got - ref| / bound over finite references; a non-finite reference must be met exactly."""
    got = np.asarray(got, np.float64)
    fin = np.isfinite(ref)
    with np.errstate(all="ignore"):
        bad = ~fin & ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
        if bad.any():
            fails.append(f"{what}: row {int(np.nonzero(bad)[0][0])} is {got[bad][0]} where float64 has {ref[bad][0]}")
        q = np.where(fin, np.abs(got - ref) / bound, 0.0)
        q = np.where(np.isnan(q), np.inf, q)
    worst = float(q.max()) if q.size else 0.0
    if worst > 1.0:
        i = int(q.argmax())
        fails.append(f"{what}: row {i} is off by {abs(got[i] - ref[i]):.3g}, {worst:.3g} of its bound {bound[i]:.3g}")
    return worst


def criteria(c, out, share=1.0):
    """Every criterion on one case's outputs. ``out``: lse, row, valid, rank (metrics), sums, mean, grad -- numpy
    float32, the gradient as stored values. Returns (failures, ratios)."""
    fails, ratios = [], {}
    r = reference(c)
    b_lse, b_row = forward_bounds(c, r)
    ratios["lse"] = _ratio(out.lse, r.lse, b_lse * share, "lse", fails)
    ratios["row"] = _ratio(out.row, r.row, b_row * share, "row loss", fails)
    if not np.array_equal(np.asarray(out.valid, f32).view(np.uint32), r.valid.astype(f32).view(np.uint32)):
        fails.append("valid flags differ from the tie-rule reference")
    if c.pair == "metrics":
        if not _same_bits(out.rank, r.rank.astype(f32)).all():
            i = int(np.nonzero(~_same_bits(out.rank, r.rank.astype(f32)))[0][0])
            fails.append(f"rank: row {i} has {out.rank[i]}, the tie rule gives {r.rank[i]}")
    # the batch kernel, replayed from the kernel's own rows
    sums, mean = replay_batch(out.row, out.valid, out.rank if c.pair == "metrics" else None, c.k)
    if c.pair == "plain":
        got, want = np.array([out.sums[-1]], f32), sums[1:2]   # the plain pair keeps the mean and the count only
    else:
        got, want = np.asarray(out.sums, f32), sums
    if not _same_bits(got, want).all():
        fails.append(f"batch sums {got.tolist()} differ from the fixed-order replay {want.tolist()}")
    if not _same_bits(out.mean, mean).all():
        fails.append(f"mean {float(out.mean)!r} differs from the fixed-order replay {float(mean)!r}")
    # gradient
    grad = np.asarray(out.grad, f32)
    inv = ~r.valid
    if inv.any() and grad[inv].view(np.uint32).any():
        fails.append("an invalid row's gradient is not +0.0 in every bit")
    if r.valid.any():
        count = got[-1] if c.pair == "plain" else got[1]
        lo, hi, g = grad_interval(c, out.lse, count, share)
        if c.dt == "bf16":
            lo, hi = bf16_rne(lo.astype(f32)).astype(np.float64), bf16_rne(hi.astype(f32)).astype(np.float64)
        gv = grad.astype(np.float64)
        with np.errstate(all="ignore"):
            nanrow = np.isnan(lo) | np.isnan(hi)
            ok = np.where(nanrow, np.isnan(gv), (gv >= lo) & (gv <= hi))
        ok |= inv[:, None]
        if not ok.all():
            i, j = (int(v[0]) for v in np.nonzero(~ok))
            fails.append(f"gradient: {int((~ok).sum())} entries outside their interval, first [{i}, {j}] = "
                         f"{gv[i, j]!r} not in [{lo[i, j]!r}, {hi[i, j]!r}] (g = {g!r})")
        # share of the assumed allowance used (report only): excess over the rho = 0 interval, over rho p |g|
        if c.dt == "f32":
            lo0, hi0, _ = grad_interval(c, out.lse, count, 0.0)
            lo1, hi1, _ = grad_interval(c, out.lse, count, 1.0)
            with np.errstate(all="ignore"):
                exc = np.maximum(np.maximum(gv - hi0, lo0 - gv), 0.0)
                room = np.maximum(hi1 - hi0, lo0 - lo1)
                q = np.where(r.valid[:, None] & (exc > 0), exc / room, 0.0)
            ratios["grad"] = float(np.nan_to_num(q, nan=0.0, posinf=np.inf).max())
    return fails, ratios


def check(c, out, share=1.0):
    fails, ratios = criteria(c, out, share)
    assert not fails, f"{c.name}: " + "; ".join(fails)
    return ratios


# ------------------------------------------------------------------------------------------------- fp32 emulation
def _exp32(a):
    with np.errstate(all="ignore"):
        return np.exp(np.asarray(a, f32).astype(np.float64)).astype(f32)


def _log32(a):
    with np.errstate(all="ignore"):
        return np.log(np.asarray(a, f32).astype(np.float64)).astype(f32)


def _butterfly(v, op):
    for off in (32, 16, 8, 4, 2, 1):
        v = op(v, v[:, np.arange(64) ^ off])
    return v[:, 0]


def _visits(C, G):
    """Class index of lane l's visit s, element j: [64, steps, G]; -1 where the lane has nothing left."""
    groups = C // G
    steps = max(1, math.ceil(groups / 64))
    v = np.arange(64)[:, None] + 64 * np.arange(steps)[None, :]
    idx = v[:, :, None] * G + np.arange(G)[None, None, :]
    idx[v >= groups] = -1
    return idx


def _emulate_rows(c, fault):
    """lse, plain sum and rank count of every row in the documented lane order (fp32)."""
    x = c.x
    B, C = x.shape
    G = elems(c.dt) if c.vec else 1
    idx = _visits(C, G)
    steps = idx.shape[1]
    rd = idx.copy()
    if fault == "second_trip_alias" and c.vec:   # a trip is four visits; later trips read the first trip's data
        for s in range(4, steps):
            rd[:, s] = np.where(idx[:, s] >= 0, idx[:, s % 4], -1)
    last = np.arange(C) >= C - G if c.vec else np.zeros(C, bool)
    rows = np.arange(B)
    valid = _valid(c)
    t = np.where(valid, c.ta, 0)
    xt = x[rows, t]
    m = np.full((B, 64), NEG_INF, f32)
    s = np.zeros((B, 64), f32)
    tot = np.zeros((B, 64), f32)
    above = np.zeros((B, 64), np.int64)
    online = c.pair != "plain"
    with np.errstate(all="ignore"):
        if not online:  # the row maximum first, then one sum relative to it
            mx = np.full((B, 64), NEG_INF, f32)
            for st in range(steps):
                have = idx[:, st, 0] >= 0
                f = np.where(have[None, :], x[:, np.maximum(idx[:, st, 0], 0)], NEG_INF)
                mx = np.fmax(mx, f)
            M = _butterfly(mx, np.fmax)
        for st in range(steps):
            have = (idx[:, st, 0] >= 0)[None, :]
            f = x[:, np.maximum(rd[:, st, :], 0)]                       # [B, 64, G]
            if online:
                vm = np.fmax.reduce(np.where(have[:, :, None], f, NEG_INF), axis=2)
                mn = np.fmax(m, vm)
                if fault != "no_rescale_lane":
                    s = np.where(have & (m != NEG_INF), (s * _exp32(m - mn)).astype(f32), s)
                m = np.where(have, mn, m)
            for j in range(G):
                fj = f[:, :, j]
                cls = idx[:, st, j]
                if online:
                    e = np.where(fj == NEG_INF, f32(0), _exp32(fj - m))
                else:
                    e = _exp32(fj - M[:, None])
                skip = last[np.maximum(cls, 0)][None, :]
                s = np.where(have & ~(skip & (fault == "expsum_skip_last_vec")), (s + e).astype(f32), s)
                tot = np.where(have & ~(skip & (fault == "sum_skip_last_vec")), (tot + fj).astype(f32), tot)
                hit = (fj > xt[:, None]) | ((fj == xt[:, None]) & (cls[None, :] < t[:, None]))
                above += hit & have & ~(skip & (fault == "rank_skip_last_vec"))
        if online:
            M = _butterfly(m, np.fmax)
            if fault != "no_rescale_merge":
                s = np.where(m != NEG_INF, (s * _exp32(m - M[:, None])).astype(f32), s)
        S = _butterfly(s, lambda a, b: (a + b).astype(f32))
        lse = (M + _log32(S)).astype(f32)
        total = _butterfly(tot, lambda a, b: (a + b).astype(f32))
    return lse, total, above.sum(axis=1), valid, xt


def _emulate_batch(cols, B, fault):
    """The batch kernel, thread by thread: 256 accumulators, trip after trip."""
    out = []
    with np.errstate(all="ignore"):
        for col in cols:
            acc = np.zeros(256, f32)
            for i in range(B):
                if fault == "batch_sum_256" and i >= 256:
                    break
                acc[i % 256] = f32(acc[i % 256] + col[i])
            waves = [_butterfly(acc[w * 64:(w + 1) * 64][None, :].copy(), lambda a, b: (a + b).astype(f32))[0]
                     for w in range(4)]
            out.append(f32(f32(f32(waves[0] + waves[1]) + waves[2]) + waves[3]))
    return out


def emulate(c, fault=None):
    """The three pairs in numpy float32 from the documented formulas; ``fault`` injects one defect."""
    assert fault is None or fault in FAULTS
    x = c.x
    B, C = x.shape
    rows = np.arange(B)
    lse, total, above, valid, xa = _emulate_rows(c, fault)
    eps = f32(c.eps)
    hot = f32(1) if fault == "hot_one" else f32(f32(1) - eps)
    Cdiv = f32(C - 1) if fault == "uni_c_minus_1" and C > 1 else f32(C)
    with np.errstate(all="ignore"):
        if c.pair == "mix":
            wa = c.lam.astype(f32)
            wb = (f32(1) - wa).astype(f32)
            xb = x[rows, np.where(valid, c.tb, 0)]
            if fault == "mix_zero_weight_kept":
                xt = ((wa * xa).astype(f32) + (wb * xb).astype(f32)).astype(f32)
            else:
                xt = (np.where(wa != 0, (wa * xa).astype(f32), f32(0))
                      + np.where(wb != 0, (wb * xb).astype(f32), f32(0))).astype(f32)
        else:
            xt = xa
        if c.pair == "plain":
            row = (lse - xt).astype(f32)
        else:
            smooth = (eps * (total / Cdiv).astype(f32)).astype(f32) if (eps > 0 or fault == "smooth_at_eps0") \
                else np.zeros(B, f32)
            row = ((lse - (hot * xt).astype(f32)).astype(f32) - smooth).astype(f32)
        row = np.where(valid, row, f32(0)).astype(f32)
        vf = valid.astype(f32)
        rank = None
        cols = [row, vf]
        if c.pair == "metrics":
            rank = np.where(valid & ~np.isnan(xa), above.astype(f32), f32(np.inf)).astype(f32)
            cols += [(rank < f32(1)).astype(f32), (rank < f32(c.k)).astype(f32)]
        sums = _emulate_batch(cols, B, fault)
        mean = f32(sums[0] / sums[1]) if sums[1] > 0 else f32(np.nan)
        # backward
        gout = f32(1) if fault == "gout_ignored" else f32(c.gout)
        g = f32(gout / (f32(B) if fault == "g_over_B" else sums[1]))
        uni = f32(0) if (c.pair == "plain" or fault == "drop_uni") else f32(eps / Cdiv)
        cls = np.arange(C)[None, :]
        ta, tb = c.ta[:, None], (c.tb[:, None] if c.pair == "mix" else None)
        if fault == "target_lane_shift":   # the hot term lands one element further inside its 16-byte vector
            G = elems(c.dt)
            shift = lambda t: np.where(t >= 0, t - t % G + np.minimum((t % G + 1) % G, C - 1 - (t - t % G)), t)
            ta = shift(ta)
            tb = shift(tb) if tb is not None else None
        if c.pair == "mix":
            ha = (hot * wa).astype(f32)[:, None]
            hb = (hot * wb).astype(f32)[:, None]
            if fault == "mix_swap_hab":
                ha, hb = hb, ha
            if fault == "mix_same_target_not_added":
                h = np.where(cls == ta, ha, np.where(cls == tb, hb, f32(0))).astype(f32)
            else:
                h = (np.where(cls == ta, ha, f32(0)).astype(f32) + np.where(cls == tb, hb, f32(0)).astype(f32))
        else:
            h = np.where(cls == ta, hot if c.pair == "metrics" else f32(1), f32(0)).astype(f32)
        xin = x
        if fault == "second_trip_alias" and c.vec:
            G = elems(c.dt)
            src = np.arange(C)
            src = (src // G % 256) * G + src % G
            xin = x[:, src]
        p = _exp32((xin - lse[:, None]).astype(f32))
        d = (((p - h).astype(f32) - uni).astype(f32) * g).astype(f32)
        if fault != "ignored_not_zeroed":
            d = np.where(valid[:, None], d, f32(0)).astype(f32)
        grad = bf16_trunc(d) if (fault == "bf16_truncate" and c.dt == "bf16") else store(d, c.dt)
    return SimpleNamespace(lse=lse, row=row, valid=vf, rank=rank, sums=np.array(sums, f32), mean=mean, grad=grad)
