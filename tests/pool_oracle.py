"""Exact oracle for the max-pool and global-average-pool kernels (test_gpu_pool_exact.py; checked on the CPU by
test_pool_oracle.py). Shares no code with the package and is importable without a GPU.

Forward rule. Each window gives the value and the position (ky * k + kx, one byte) of its row-major FIRST maximum.
Padding is -inf. The first NaN of a window wins. A window whose in-range taps are all -inf gives position 0 (which
may be a padding tap). Ceil mode adds trailing windows, but drops one that would start outside the input
(``bn_oracle.pool_out``).

Backward rule. dx is the gather of dy by position: pixel (h, w) receives dy of every window whose recorded position
is that pixel, selected with ``torch.where`` -- never multiplied by a mask, so a NaN / inf dy reaches exactly the
chosen pixel. A pixel no window covers (stride > window) or chose is +0. dy is integer-valued, so the fp32 sum is
exact in any order; the result is rounded once to the output dtype.

Average-pool rule. y = round_dtype(round_f32(S * f32(1 / HW))) with S the exact integer sum, dx =
round_dtype(round_f32(dy * f32(1 / HW))).

Data (``pool_data``). Integers in [0, 3] (3 twice as likely, or more where many windows have one tap, so that maxima
tie in a quarter of ALL windows), about 2 % NaN, 3 % -inf, 0.5 %
+inf (times 9 / k^2 for windows above 3 x 3, so that a window's chance of holding one stays the same); one planted interior k x k block of -inf (image 0), one -inf block under the window of the padded corner
(last image), two NaNs and two +inf planted inside one window. Everything is bf16-exact, so the same tensors serve
bf16 and fp32. ``make_case`` ASSERTS the coverage of every case from the oracle alone (``Coverage``): see there.

The module also holds a plain-torch emulation of the kernels (``emu_fwd`` / ``emu_bwd``) with a ``fault=`` switch;
``check_maxpool`` is the one set of assertions that test_gpu_pool_exact.py applies to the kernels and
test_pool_oracle.py applies to the emulation, with and without each fault.
"""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from bn_oracle import pool_out, pool_ref

NEG = float("-inf")
TIE_SHARE = 0.25
SEEDS = 16  # seeds a case may try per weighting before its coverage assertions count as failed


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(int(seed))


# ------------------------------------------------------------------------------------------- geometry
# (k, s, p, ceil) -> the kernels it must reach: forward K (0 = runtime window) and backward R = ceil(k / s) when that
# is 1..3, else 0 (runtime loops). test_gpu_pool_exact.py asserts this arithmetic.
GEOMETRIES = [
    (3, 2, 1, False), (3, 2, 0, True),                                         # K = 3, R = 2
    (3, 1, 1, False), (3, 1, 0, False),                                        # separable 4 / 7 / off, R = 3
    (2, 2, 0, False), (2, 2, 0, True), (2, 1, 1, False), (2, 2, 1, True),      # K = 2, R = 1 and 2
    (1, 1, 0, False), (1, 2, 0, False), (2, 3, 0, False),                      # stride >= window: uncovered pixels
    (5, 2, 2, False), (4, 3, 1, True),                                         # runtime k, R = 3 and 2
    (5, 1, 2, False), (7, 2, 3, False), (15, 1, 7, False), (15, 4, 0, True),   # the generic R = 0 backward
]
SHAPES = [(1, 5), (13, 1), (9, 7), (4, 4), (5, 6), (15, 3), (8, 11)]
SHAPES_K15 = [(16, 17), (15, 15)]
NC = [(1, 8), (3, 24), (1, 40), (3, 8), (1, 24), (3, 40)]


def fwd_kernel(k: int) -> int:
    return k if k in (2, 3) else 0


def bwd_kernel(k: int, s: int) -> int:
    r = -(-k // s)
    return r if r <= 3 else 0


def cases():
    """Every (N, C, H, W, k, s, p, ceil) of the exact tests with a non-empty output."""
    out = []
    for gi, (k, s, p, ceil) in enumerate(GEOMETRIES):
        for si, (H, W) in enumerate(SHAPES_K15 if k == 15 else SHAPES):
            if pool_out(H, k, s, p, ceil) < 1 or pool_out(W, k, s, p, ceil) < 1:
                continue
            N, C = NC[(gi + si) % len(NC)]
            out.append((N, C, H, W, k, s, p, ceil))
    return out


def windows(a, k, s, p, oh, ow, pad=NEG):
    """[N, C, oh, ow, k*k] windows of a [N, C, H, W] tensor (float32), ``pad`` outside the input."""
    n, c, h, w = a.shape
    ph, pw = max((oh - 1) * s + k - h - p, 0), max((ow - 1) * s + k - w - p, 0)
    ap = F.pad(a.float(), (p, pw, p, ph), value=pad)
    return ap.unfold(2, k, s).unfold(3, k, s)[:, :, :oh, :ow].reshape(n, c, oh, ow, k * k)


def in_range(H, W, k, s, p, oh, ow):
    """[oh, ow, k*k] booleans: the tap lies inside the input."""
    return windows(torch.ones(1, 1, H, W), k, s, p, oh, ow, pad=0.0)[0, 0] > 0


def targets(pos, k, s, p):
    """(h, w) of the input pixel each recorded position names ([N, C, OH, OW] each; may lie in the padding)."""
    oh, ow = pos.shape[2], pos.shape[3]
    r = torch.arange(oh, device=pos.device).view(1, 1, oh, 1) * s - p
    c = torch.arange(ow, device=pos.device).view(1, 1, 1, ow) * s - p
    return r + pos // k, c + pos % k


# ------------------------------------------------------------------------------------------- references
def maxpool_ref(x, k, s, p, ceil=False):
    """(y, pos) by the forward rule; y float32, pos int64, both [N, C, OH, OW]."""
    return pool_ref(x, k, s, p, ceil)


def maxpool_bwd_ref(dy, pos, H, W, k, s, p, dtype=torch.float32):
    """dx [N, C, H, W] by the backward rule, as float64 holding the value rounded once to ``dtype``."""
    n, c, oh, ow = dy.shape
    hp, wp = max((oh - 1) * s + k, H + p), max((ow - 1) * s + k, W + p)
    d = dy.double()
    zero = torch.zeros_like(d)
    buf = torch.zeros(n, c, hp, wp, dtype=torch.float64, device=dy.device)
    for q in range(k * k):
        ky, kx = divmod(q, k)
        buf[:, :, ky:ky + (oh - 1) * s + 1:s, kx:kx + (ow - 1) * s + 1:s] += torch.where(pos == q, d, zero)
    dx = buf[:, :, p:p + H, p:p + W]
    fin = torch.isfinite(dx)
    assert float(dx[fin].abs().max() if bool(fin.any()) else 0) < (1 << 24), "the gathered sum leaves fp32's integers"
    return dx.float().to(dtype).double()


def covered(H, W, k, s, p, oh, ow):
    """[H, W] booleans: some window covers the pixel."""
    m = torch.zeros(max((oh - 1) * s + k, H + p), max((ow - 1) * s + k, W + p), dtype=torch.bool)
    for q in range(k * k):
        ky, kx = divmod(q, k)
        m[ky:ky + (oh - 1) * s + 1:s, kx:kx + (ow - 1) * s + 1:s] = True
    return m[p:p + H, p:p + W]


def f32(v):
    return torch.tensor(float(v), dtype=torch.float32)


def gap_inv(hw: int) -> torch.Tensor:
    """f32(1 / HW) as the launcher forms it: 1.f / (float)HW."""
    return f32(1.0) / f32(hw)


def gap_fwd_ref(x, dtype):
    """[N, C] float64: round_dtype(round_f32(S * f32(1 / HW))). S (an integer below 2^24) times a 24-bit factor is
    exact in float64, so ``.float()`` is the one fp32 rounding of the kernel's multiply."""
    S = x.double().sum((2, 3))
    assert bool((S == S.round()).all()) and float(S.abs().max()) < (1 << 24)
    return (S * gap_inv(x.shape[2] * x.shape[3]).double()).float().to(dtype).double()


def gap_bwd_ref(dy, H, W, dtype):
    """[N, C, H, W] float64: round_dtype(round_f32(dy * f32(1 / HW))) at every pixel."""
    v = (dy.double() * gap_inv(H * W).double()).float().to(dtype).double()
    return v[:, :, None, None].expand(-1, -1, H, W)


# ------------------------------------------------------------------------------------------------- data
class Coverage(SimpleNamespace):
    """What one case's data exercises, measured on the oracle's windows alone. ``taps`` is the largest number of
    in-range taps of any window. The only cases excused from the tie share, the two NaNs and "first is not last" are
    those with k = 1 (``tie_exempt``): a window then holds one value and none of the three can happen. Every other case
    must reach the shares over ALL its windows; the narrow and padded shapes, where up to 44 % of the windows have
    a single in-range tap, get there with a heavier weight on the top value (``WEIGHTS``).

    tie_share   windows whose maximum (a number or +inf: not NaN, not -inf -- an all -inf window never leaves
                position 0 and exercises nothing of the first-maximum rule) stands at two or more in-range
                positions / all windows
    multi_share windows with two or more in-range taps / all windows (an upper bound of tie_share)
    nan2        windows with two or more NaNs
    all_neg     windows whose in-range taps are all -inf
    first_not_last  windows whose first maximum is not their last maximum
    """


def measure(x, k, s, p, ceil) -> Coverage:
    H, W = x.shape[2:]
    oh, ow = pool_out(H, k, s, p, ceil), pool_out(W, k, s, p, ceil)
    win = windows(x, k, s, p, oh, ow)
    ok = in_range(H, W, k, s, p, oh, ow)
    y, pos = maxpool_ref(x, k, s, p, ceil)
    nan = torch.isnan(win)
    at_max = (win == y.unsqueeze(-1)) & ok
    multi = (ok.sum(-1) >= 2).expand(win.shape[:-1])
    tied = (at_max.sum(-1) >= 2) & (y > NEG)
    last = (k * k - 1) - at_max.flip(-1).float().argmax(-1)
    c = Coverage(taps=int(ok.sum(-1).max()), windows=int(multi.numel()), multi=int(multi.sum()))
    c.tie_share = float(tied.sum()) / c.windows
    c.multi_share = c.multi / c.windows
    c.nan2 = int((nan.sum(-1) >= 2).sum())
    c.all_neg = int(((win == NEG) | ~ok).all(-1).sum())
    c.first_not_last = int((at_max.any(-1) & (last != pos)).sum())
    return c


def tie_exempt(k: int) -> bool:
    """k = 1: every window has exactly one tap, so a tie, two NaNs in a window and a first maximum that is not the
    last are impossible (share 0 by construction). No other case is excused."""
    return k == 1


def coverage_ok(c: Coverage, k: int) -> bool:
    if c.all_neg < 1:
        return False
    return tie_exempt(k) or (c.tie_share >= TIE_SHARE and c.nan2 >= 1 and c.first_not_last >= 1)


# weights of the values 0, 1, 2, 3, tried in this order (SEEDS seeds each): the first serves every case whose windows
# nearly all have several taps; the heavier ones serve the 1-pixel-wide and padded 2 x 2 shapes
WEIGHTS = ((0.2, 0.2, 0.2, 0.4), (0.1, 0.1, 0.1, 0.7), (0.05, 0.05, 0.05, 0.85))


def pool_data(N, C, H, W, k, s, p, ceil, seed, weights=WEIGHTS[0]):
    """x [N, C, H, W] float32: see the module docstring."""
    g = gen(seed)
    oh, ow = pool_out(H, k, s, p, ceil), pool_out(W, k, s, p, ceil)
    x = torch.multinomial(torch.tensor(weights), N * C * H * W, True, generator=g).float().reshape(N, C, H, W)
    # shares of the special values for windows of up to 9 taps; a larger window gets them per window, not per element
    # (at 2 % per element a 15 x 15 window holds a NaN 99 % of the time and the first-maximum rule would go untested)
    f = min(1.0, 9.0 / (k * k))
    r = torch.rand(N, C, H, W, generator=g)
    x[r < 0.02 * f] = float("nan")
    x[(r >= 0.02 * f) & (r < 0.05 * f)] = NEG
    x[(r >= 0.05 * f) & (r < 0.055 * f)] = float("inf")
    # (both blocks in the last two channels)
    # an interior window of -inf (image 0): the window in the middle of the output, clipped to the input
    h0, w0 = (oh // 2) * s - p, (ow // 2) * s - p
    x[0, C - 2:, max(h0, 0):h0 + k, max(w0, 0):w0 + k] = NEG
    # the window of the padded corner (last image): its in-range taps
    x[N - 1, C - 2:, 0:k - p, 0:k - p] = NEG
    # two NaNs (channel 1) and two +inf (channel 2) at the first and last in-range tap of one window of image 0: the
    # last of those with the most in-range taps
    okw = in_range(H, W, k, s, p, oh, ow)
    cnt = okw.sum(-1).flatten()
    wi = int((cnt == cnt.max()).nonzero().max())
    ok = okw.reshape(-1, k * k)[wi].nonzero().flatten().tolist()
    if len(ok) >= 2:
        for q, (ch, v) in ((ok[0], (1, float("nan"))), (ok[-1], (1, float("nan"))), (ok[0], (2, float("inf"))),
                           (ok[-1], (2, float("inf")))):
            x[0, ch, (wi // ow) * s - p + q // k, (wi % ow) * s - p + q % k] = v
    return x


def special_dy(dy, pos, H, W, k, s, p):
    """A copy of the integer dy with one NaN, one +inf and one -inf at three windows whose target pixels lie inside
    the input and differ, and which no other of the three reaches. Returns (dy2, [(value, (n, c, h, w))])."""
    th, tw = targets(pos, k, s, p)
    inside = (th >= 0) & (th < H) & (tw >= 0) & (tw < W)
    n, c, oh, ow = pos.shape
    dy2, placed, used = dy.clone(), [], set()
    idx = inside.nonzero().tolist()
    step = max(1, len(idx) // 7)
    # spread over the tensor, windows with more than one in-range tap first: only there can a gradient leak to a
    # pixel the window did not choose
    ntap = in_range(H, W, k, s, p, oh, ow).sum(-1)
    order = list(range(len(idx) // 2, len(idx), step)) + list(range(0, len(idx)))
    order.sort(key=lambda i: int(ntap[idx[i][2], idx[i][3]]) < 2)
    for i in order:
        a, b, u, v = idx[i]
        t = (a, b, int(th[a, b, u, v]), int(tw[a, b, u, v]))
        if t in used:
            continue
        used.add(t)
        val = (float("nan"), float("inf"), NEG)[len(placed)]
        dy2[a, b, u, v] = val
        placed.append((val, t))
        if len(placed) == 3:
            break
    assert len(placed) == 3, "fewer than three windows with distinct in-range targets"
    return dy2, placed


@functools.lru_cache(maxsize=None)
def make_case(N, C, H, W, k, s, p, ceil):
    """Data, references and measured coverage of one max-pool case (cached: both dtypes share it; read-only)."""
    oh, ow = pool_out(H, k, s, p, ceil), pool_out(W, k, s, p, ceil)
    assert oh >= 1 and ow >= 1
    base = 1000 * (k * 16 + s) + 37 * H + W + 7 * N + C + (500 if ceil else 0) + 50 * p
    for wi, seed in ((wi, seed) for wi in range(len(WEIGHTS)) for seed in range(base, base + SEEDS)):
        x = pool_data(N, C, H, W, k, s, p, ceil, seed, WEIGHTS[wi])
        cov = measure(x, k, s, p, ceil)
        if coverage_ok(cov, k):
            break
    c = SimpleNamespace(N=N, C=C, H=H, W=W, k=k, s=s, p=p, ceil=ceil, OH=oh, OW=ow, x=x, cov=cov, seed=seed,
                        weights=wi, tries=wi * SEEDS + seed - base + 1)
    # the coverage every case must have, asserted here so that no test can quietly stop testing
    assert cov.all_neg >= 1, f"{c}: no window is all -inf"
    if not tie_exempt(k):
        assert cov.tie_share >= TIE_SHARE, f"tied maxima in {cov.tie_share:.1%} of all windows"
        assert cov.nan2 >= 1 and cov.first_not_last >= 1, cov
    c.y, c.pos = maxpool_ref(x, k, s, p, ceil)
    assert c.y.shape == (N, C, oh, ow) and int(c.pos.max()) < k * k <= 225
    g = gen(seed + 1)
    lim = 1 if k == 15 else 3  # k = 15, s = 1: up to 225 windows per pixel; |sum| <= 225 < 256 stays bf16-exact
    c.dy = torch.randint(-lim, lim + 1, (N, C, oh, ow), generator=g).float()
    c.dy2, c.placed = special_dy(c.dy, c.pos, H, W, k, s, p)
    c.covered = covered(H, W, k, s, p, oh, ow)
    c.dx, c.dx2 = {}, {}
    for dt in (torch.float32, torch.bfloat16):
        c.dx[dt] = maxpool_bwd_ref(c.dy, c.pos, H, W, k, s, p, dt)
        c.dx2[dt] = maxpool_bwd_ref(c.dy2, c.pos, H, W, k, s, p, dt)
        assert bool(torch.isfinite(c.dx[dt]).all())
        bad = ~torch.isfinite(c.dx2[dt])
        assert int(bad.sum()) == 3, "the three special gradients must reach three pixels"
        for val, (a, b, h, w) in c.placed:
            got = float(c.dx2[dt][a, b, h, w])
            assert got != got if val != val else got == val
        assert torch.equal(c.dx2[dt][~bad], c.dx[dt][~bad]), "a special gradient changed another pixel"
    return c


# ------------------------------------------------------------------------------------------ comparisons
def same(got, ref):
    """Elementwise: equal by value, or both NaN."""
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    return (g == r) | (torch.isnan(g) & torch.isnan(r))


def assert_same(got, ref, what):
    assert tuple(got.shape) == tuple(ref.shape), f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    ok = same(got, ref)
    if not bool(ok.all()):
        idx = (~ok).nonzero()
        head = [(tuple(i.tolist()), float(got.detach().double().cpu()[tuple(i)]), float(ref.double().cpu()[tuple(i)]))
                for i in idx[:6]]
        raise AssertionError(f"{what}: {idx.shape[0]} of {ok.numel()} differ; first (index, got, want) {head}")


def check_maxpool(c, fwd, bwd, dtype, what=""):
    """Every per-case assertion. ``fwd(x, need_pos) -> (y, pos or None)`` and ``bwd(dy, pos) -> dx`` take and return
    [N, C, H, W]-shaped tensors (x, dy float32 holding bf16-exact values; pos uint8); the outputs must have been
    computed into poisoned memory (NaN for y and dx, 0xff for pos)."""
    tag = f"{what} {(c.N, c.C, c.H, c.W)} k{c.k} s{c.s} p{c.p}{' ceil' if c.ceil else ''} {dtype}"
    y, pos = fwd(c.x, True)
    assert_same(y, c.y, f"{tag}: y")
    assert pos is not None and pos.dtype == torch.uint8
    assert_same(pos, c.pos, f"{tag}: pos")
    y0, pos0 = fwd(c.x, False)
    assert pos0 is None, f"{tag}: need_pos=False returned positions"
    assert_same(y0, c.y, f"{tag}: y without positions")
    # the gradients are routed by the ORACLE's positions
    ref_pos = c.pos.to(torch.uint8)
    dx = bwd(c.dy, ref_pos)
    assert_same(dx, c.dx[dtype], f"{tag}: dx")
    unc = ~c.covered.expand(c.N, c.C, c.H, c.W)
    dxc = dx.detach().float().cpu()
    assert bool(((dxc[unc] == 0) & ~torch.signbit(dxc[unc])).all()), f"{tag}: an uncovered pixel is not +0"
    dx2 = bwd(c.dy2, ref_pos)
    assert_same(dx2, c.dx2[dtype], f"{tag}: dx of the NaN / +inf / -inf gradient")
    d2 = dx2.detach().double().cpu()
    assert int((~torch.isfinite(d2)).sum()) == 3, f"{tag}: a non-finite gradient reached other pixels"
    for val, (a, b, h, w) in c.placed:
        got = float(d2[a, b, h, w])
        assert (got != got) if val != val else got == val, f"{tag}: {val} did not reach pixel {(a, b, h, w)}"


# ------------------------------------------------------------------------------- emulation with faults
FAULTS = ("last_max", "last_nan", "nan_not_sticky", "pad_zero", "no_ceil_drop", "credit_ties", "mask_multiply",
          "strip_remainder", "uncovered_unwritten", "wrong_quotient")
STRIP = 4  # strip height of the emulated 3x3/s1 forward


def _out_nodrop(n, k, s, p, ceil):
    return (n + 2 * p - k + (s - 1 if ceil else 0)) // s + 1


def emu_fwd(x, k, s, p, ceil=False, need_pos=True, fault=None):
    """(y float32, pos uint8 or None): the running row-major scan of the kernels (strict '>' keeps the first maximum; a
    NaN wins unless the best is one already), computed "into" NaN / 0xff poison."""
    H, W = x.shape[2:]
    out = _out_nodrop if fault == "no_ceil_drop" else pool_out
    oh, ow = out(H, k, s, p, ceil), out(W, k, s, p, ceil)
    win = windows(x, k, s, p, oh, ow, pad=0.0 if fault == "pad_zero" else NEG)
    best = torch.full(win.shape[:-1], NEG)
    pos = torch.zeros(win.shape[:-1], dtype=torch.int64)
    for q in range(k * k):
        v = win[..., q]
        vn, bn = torch.isnan(v), torch.isnan(best)
        gt = ((v >= best) & (v > NEG)) if fault == "last_max" else (v > best)
        take = gt | (vn if fault == "last_nan" else vn & ~bn)
        if fault == "nan_not_sticky":
            take = take | (bn & ~vn)
        best = torch.where(take, v, best)
        pos = torch.where(take, torch.full_like(pos, q), pos)
    if fault == "strip_remainder" and k == 3 and s == 1 and oh % STRIP:  # the last, partial strip is not stored
        best[:, :, oh - oh % STRIP:] = float("nan")
        pos[:, :, oh - oh % STRIP:] = 255
    if fault == "wrong_quotient":  # the last pixel of row 0 decodes as (row 1, col -1): its result lands elsewhere
        if oh > 1 and ow > 1:
            best[0, :, 1, ow - 2], pos[0, :, 1, ow - 2] = best[0, :, 0, ow - 1], pos[0, :, 0, ow - 1]
        best[0, :, 0, ow - 1], pos[0, :, 0, ow - 1] = float("nan"), 255
    return best, (pos.to(torch.uint8) if need_pos else None)


def emu_bwd(dy, pos, x, k, s, p, ceil=False, fault=None):
    """dx float32 "into" NaN poison: the gather of the kernels."""
    n, c, oh, ow = dy.shape
    H, W = x.shape[2:]
    hp, wp = max((oh - 1) * s + k, H + p), max((ow - 1) * s + k, W + p)
    buf = torch.zeros(n, c, hp, wp)
    d = dy.float()
    if fault == "credit_ties":  # every position that holds the window's maximum
        win = windows(x, k, s, p, oh, ow)
        y = torch.gather(win, -1, pos.long().unsqueeze(-1))
        hit = (win == y) | (torch.isnan(win) & torch.isnan(y))
    for q in range(k * k):
        ky, kx = divmod(q, k)
        sel = hit[..., q] if fault == "credit_ties" else pos == q
        add = d * sel if fault == "mask_multiply" else torch.where(sel, d, torch.zeros_like(d))
        buf[:, :, ky:ky + (oh - 1) * s + 1:s, kx:kx + (ow - 1) * s + 1:s] += add
    dx = buf[:, :, p:p + H, p:p + W].clone()
    if fault == "uncovered_unwritten":
        dx[:, :, ~covered(H, W, k, s, p, oh, ow)] = float("nan")
    return dx


def emu_pair(c, dtype, fault=None):
    """(fwd, bwd) callables of the emulation for ``check_maxpool``."""
    def fwd(x, need_pos):
        y, pos = emu_fwd(x, c.k, c.s, c.p, c.ceil, need_pos, fault)
        return y.to(dtype), pos

    def bwd(dy, pos):
        return emu_bwd(dy.to(dtype), pos, c.x, c.k, c.s, c.p, c.ceil, fault).to(dtype)

    return fwd, bwd


# ------------------------------------------------------------------------- the multiply-shift division
def emu_fdiv(n: int, d: int) -> int:
    """mm::fdiv(n, make_fastdiv(d)) in 32-bit arithmetic: (umulhi(n, m_lo) + n * m_hi) >> 8, m = ceil(2^40 / d)."""
    m = ((1 << 40) + d - 1) // d
    m_lo, m_hi = m & 0xFFFFFFFF, m >> 32
    return ((((n * m_lo) >> 32) + n * m_hi) & 0xFFFFFFFF) >> 8


def emu_decode(t: int, cg: int, cols: int, rows: int, fast: bool):
    """pool.hip's decode(): flat index -> (n, row, col, channel group)."""
    div = emu_fdiv if fast else (lambda a, b: a // b)
    q = div(t, cg)
    r = div(q, cols)
    n = div(r, rows)
    return n, r - n * rows, q - r * cols, t - q * cg
