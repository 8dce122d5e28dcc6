"""Exact integer-data oracle for the fused backward hand-offs (test_gpu_handoff_exact.py): the BN-apply form of the
one-pass 1x1 gradient kernel (gemm_dual.hip kBN), the stem weight gradient with the BN+ReLU+max-pool backward
fused (stem.hip stem_wgrad_bn_kernel) and the fork data-gradient epilogue with its stride-2 second addend
(dla_mfma.h epilogue_bf16).

Built on tests/exact_oracle.py and under the same rules: every operand is a bf16-exact integer, every bound is
asserted on the worst case, references are float64 and compared with ``torch.equal``. The BatchNorm-backward
coefficients of dY = k1 (g - m1 - (y - mean) k2) go into the 7C workspace as small integers, so dY itself is an
integer that bf16 holds exactly and the only roundings left are the ones the kernels document: one for dx and for a
bf16 weight gradient, up to three in the fork epilogue. m1 is never 0, so rows a kernel pads past the end get a
nonzero dY and are harmless only if the other operand really reads zero there. The module shares no code with the
package and needs no GPU; tests/test_handoff_oracle.py checks it on the CPU."""
import torch
import torch.nn.functional as F

import exact_oracle as xo

DUAL_DY_MAX = 18  # 2 * (3 + 1 + 5 * 1): |k1| (|g| + |m1| + |y - mean| |k2|)
STEM_DY_MAX = 36  # 2 * (12 + 1 + 5 * 1): a pixel can be the argmax of 4 pooled windows of |dy| <= 3
FORK_ADDEND_MAX = 8  # the addends of the gemm_nt_bn cases: |dy'| <= 16 + 2 * 8 in the no-rounding regime


def _choice(vals, n, g):
    return torch.tensor(vals, dtype=torch.float32)[torch.randint(0, len(vals), (n,), generator=g)]


# ------------------------------------------------------------------------------------ BN-backward coefficients
def bn_bwd_coeffs(C: int, g: torch.Generator):
    """(ws [7C] fp32, coefficients as float64 [C]): mean in [-2, 2], k1 in {-2, -1, 1, 2}, m1 in {-1, 1}, k2 in
    {-1, 0, 1}; every third channel has mean and k2 both nonzero, so mean k2 != 0 in at least a quarter of them.
    The forward's scale in {-2, -1, 1, 2} and shift n + 0.5 in [-4.5, 4.5] (the stem recomputes its ReLU from them:
    x scale + shift is a half-integer, never 0, and a fused multiply-add gives what a multiply and an add give)."""
    mean, k2 = xo.ints((C,), g, -2, 2), xo.ints((C,), g, -1, 1)
    k1, m1 = _choice([-2., -1., 1., 2.], C, g), _choice([-1., 1.], C, g)
    mean[::3], k2[::3] = _choice([-2., -1., 1., 2.], (C + 2) // 3, g), _choice([-1., 1.], (C + 2) // 3, g)
    sc, sh = _choice([-2., -1., 1., 2.], C, g), xo.ints((C,), g, -5, 4) + 0.5
    assert int((mean * k2 != 0).sum()) * 4 >= C and bool((m1 != 0).all()) and bool((k1 != 0).all())
    ws = torch.zeros(7 * C)
    ws[:C], ws[C:2 * C], ws[2 * C:3 * C], ws[3 * C:4 * C] = mean, 1.0, sc, sh
    ws[4 * C:5 * C], ws[5 * C:6 * C], ws[6 * C:] = k1, m1, k2
    return ws, {k: v.double() for k, v in dict(mean=mean, sc=sc, sh=sh, k1=k1, m1=m1, k2=k2).items()}


def _per_channel(cf, like: torch.Tensor, dim: int):
    shape = [1] * like.dim()
    shape[dim] = -1
    return {k: v.to(like.device).view(shape) for k, v in cf.items()}


def bn_bwd_dy(g: torch.Tensor, y: torch.Tensor, cf, dim: int = -1, dy_max: int = DUAL_DY_MAX) -> torch.Tensor:
    """dY = k1 (g - m1 - (y - mean) k2) in float64 (channels along ``dim``), asserted integral and small enough
    that bf16 holds it exactly."""
    c = _per_channel(cf, g, dim)
    dY = c["k1"] * (g.double() - c["m1"] - (y.double() - c["mean"]) * c["k2"])
    xo.integral(dY, dy_max, "dY")
    assert torch.equal(dY.float().to(torch.bfloat16).double(), dY)
    return dY


# ------------------------------------------------------------------------------------------- conv1x1_dual + BN
def dual_case(M: int, seed: int, ci: int = 64, co: int = 256):
    """CPU operands of conv1x1_dual(dout, x, w, odt, ybn, ws, mask): all in [-3, 3], random mask bytes, and
    dx[M-1, ci-1] a planted tie that rounds up (the last row: on the last, possibly ragged, tile)."""
    xo.check_dense(co, DUAL_DY_MAX, 3)  # dx: reduction over co
    assert M * DUAL_DY_MAX * 3 < xo.EXACT_LIMIT  # dw: reduction over the M rows
    g = xo.gen(seed)
    dout, ybn = xo.ints((M, co), g, -3, 3), xo.ints((M, co), g, -3, 3)
    x, w = xo.ints((M, ci), g, -3, 3), xo.ints((co, ci), g, -3, 3)
    mask = xo.mask_bytes(M * co, g)
    ws, cf = bn_bwd_coeffs(co, g)
    bits_last = xo.mask_bits(mask[(M - 1) * co // 8:], co)
    partner = xo.tie_partner(bn_bwd_dy(bits_last * dout[M - 1], ybn[M - 1], cf).float())
    assert partner is not None
    w[:, ci - 1] = partner
    return dict(dout=dout, ybn=ybn, x=x, w=w, mask=mask, ws=ws, cf=cf)


def dual_ref(dout, ybn, bits, x, w, cf):
    """(dY, dx, dw) in float64 on the operands' device: dx = dY w before its one rounding, dw = dY^T x."""
    dY = bn_bwd_dy(bits.view(dout.shape).double() * dout.double(), ybn, cf)
    dx = xo.integral(dY @ w.double(), xo.DENSE_LIMIT, "dx")
    dw = xo.integral(dY.t() @ x.double(), xo.EXACT_LIMIT, "dw")
    return dY, dx, dw


# -------------------------------------------------------------------------------------------- stem_wgrad_bn
def stem_pos(n: int, C: int, OH: int, OW: int, g: torch.Generator) -> torch.Tensor:
    """Argmax taps ky * 3 + kx of a 3x3 / s2 / p1 pool, drawn uniformly among the taps of each window that lie
    inside the image (tap row 0 of the top windows and tap column 0 of the left ones do not), independent of any
    activation: the backward kernels take the positions as data."""
    lo_h = (torch.arange(OH) == 0).long().view(1, 1, OH, 1)
    lo_w = (torch.arange(OW) == 0).long().view(1, 1, 1, OW)
    ky = lo_h + torch.minimum((torch.rand(n, C, OH, OW, generator=g) * (3 - lo_h)).long(), 2 - lo_h)
    kx = lo_w + torch.minimum((torch.rand(n, C, OH, OW, generator=g) * (3 - lo_w)).long(), 2 - lo_w)
    return (ky * 3 + kx).to(torch.uint8)


def stem_scatter(dyp: torch.Tensor, pos: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """The max-pool backward: every pooled gradient goes to its argmax pixel (2 oh - 1 + ky, 2 ow - 1 + kx)."""
    n, C, OH, OW = dyp.shape
    p = pos.long()
    hh = 2 * torch.arange(OH).view(1, 1, OH, 1) - 1 + p // 3
    ww = 2 * torch.arange(OW).view(1, 1, 1, OW) - 1 + p % 3
    assert int(p.max()) <= 8 and int(hh.min()) >= 0 and int(hh.max()) < H and int(ww.min()) >= 0 and int(ww.max()) < W
    out = torch.zeros(n, C, H * W, dtype=torch.float64)
    out.scatter_add_(2, (hh * W + ww).view(n, C, -1), dyp.double().view(n, C, -1))
    return out.view(n, C, H, W)


def stem_case(n: int, H: int, W: int, seed: int, C: int = 64):
    """CPU operands of stem_wgrad_bn at conv-output size [n, C, H, W] (image [n, 3, 2H, 2W])."""
    assert H % 2 == 0 and W % 2 == 0
    xo.check_dense(n * H * W, STEM_DY_MAX, 3)
    g = xo.gen(seed)
    img, y = xo.ints((n, 3, 2 * H, 2 * W), g, -3, 3), xo.ints((n, C, H, W), g, -3, 3)
    dyp = xo.ints((n, C, H // 2, W // 2), g, -3, 3)
    pos = stem_pos(n, C, H // 2, W // 2, g)
    ws, cf = bn_bwd_coeffs(C, g)
    return dict(img=img, y=y, dyp=dyp, pos=pos, ws=ws, cf=cf)


def stem_dy_ref(dyp, pos, y, cf) -> torch.Tensor:
    """The conv output's gradient [n, C, H, W]: pooled gradients scattered to their argmax pixels, zeroed where the
    recomputed ReLU pre-activation y scale + shift is not positive, then the BN backward apply."""
    c = _per_channel(cf, y, 1)
    pre = y.double() * c["sc"] + c["sh"]
    assert bool((pre != 0).all())
    g = torch.where(pre > 0, stem_scatter(dyp, pos, y.shape[2], y.shape[3]), torch.zeros((), dtype=torch.float64))
    return bn_bwd_dy(g, y, cf, 1, STEM_DY_MAX)


def stem_pack8(dw8: torch.Tensor) -> torch.Tensor:
    """[Cout, 3, 8, 8] (filter index kh + 1, kw + 1 = 2 t + p) -> the folded 4x4 conv's [Cout, 256]: column
    (th * 4 + tw) * 16 + (ph * 2 + pw) * 3 + c, 4 zero padding channels per tap (csrc/kernels/stem.hip)."""
    co = dw8.shape[0]
    t = dw8.reshape(co, 3, 4, 2, 4, 2).permute(0, 2, 4, 3, 5, 1).reshape(co, 16, 12)
    return F.pad(t, (0, 4)).reshape(co, 256)


def stem_wgrad_ref(img: torch.Tensor, dY: torch.Tensor) -> torch.Tensor:
    """The packed [Cout, 256] weight gradient in float64 on the CPU. The folded conv has a 16th tap row and column
    (kh or kw = -1: zero weights in the forward), whose gradient the kernels produce with the rest: the reference is
    the 8x8 / s2 weight gradient over the image padded by (4, 3), and its 7x7 part must equal conv2d_weight of the
    7x7 / s2 / p3 conv."""
    co = dY.shape[1]
    dw8 = torch.nn.grad.conv2d_weight(F.pad(img.double(), (4, 3, 4, 3)), (co, 3, 8, 8), dY.double(), 2, 0)
    dw7 = torch.nn.grad.conv2d_weight(img.double(), (co, 3, 7, 7), dY.double(), 2, 3)
    assert torch.equal(dw8[:, :, 1:, 1:], dw7)
    return xo.integral(stem_pack8(dw8), xo.DENSE_LIMIT, "stem dw")


def stem_finalized_ref(c):
    """What the stem backward computes when it finalizes its OWN coefficients (bn_relu_maxpool_bwd always does:
    m1 = S / M, k2 = invstd^2 Q / M from its reduction, so integers put into the workspace do not survive it, and
    m1 = +-1 is out of its reach: |S| <= 3 M / 4 with pooled gradients in [-3, 3]). With invstd = 1, weight = k1 and a
    power-of-two pixel count M the finalized coefficients are dyadic, every fp32 operation of the apply is exact
    whatever the compiler fuses (each term is a multiple of 1 / M with a numerator below 2^24, asserted), and dY has
    exactly one rounding, to bf16. Returns S, Q (= dbeta, dgamma), m1, k2, the rounded dY and the packed weight
    gradient from it, all float64."""
    n, C, H, W = c["y"].shape
    M = n * H * W
    assert M & (M - 1) == 0, "a power-of-two pixel count"
    cf = _per_channel(c["cf"], c["y"], 1)
    ym = c["y"].double() - cf["mean"]
    pre = c["y"].double() * cf["sc"] + cf["sh"]
    gg = torch.where(pre > 0, stem_scatter(c["dyp"], c["pos"], H, W), torch.zeros((), dtype=torch.float64))
    S, Q = gg.sum((0, 2, 3)), (gg * ym).sum((0, 2, 3))
    m1, k2 = (S / M).view(1, C, 1, 1), (Q / M).view(1, C, 1, 1)
    dY = cf["k1"] * (gg - m1 - ym * k2)
    for t in (gg - m1, ym * k2, dY):
        assert torch.equal((t * M).round(), t * M) and float((t * M).abs().max()) < xo.EXACT_LIMIT
    assert torch.equal(dY.float().double(), dY)
    dYb = dY.float().to(torch.bfloat16).double()
    dw = stem_pack8(torch.nn.grad.conv2d_weight(F.pad(c["img"].double(), (4, 3, 4, 3)), (C, 3, 8, 8), dYb, 2, 0))
    # |m1| < 1, |k2| <= 5 * 3 / 4, so |dY| <= 2 (12 + 1 + 5 * 3.75) < 64: in units of 1 / M the worst-case sum of
    # |dY x| over the M pixels stays below 2^24 and the weight gradient's fp32 sums are exact in any order
    assert float(dYb.abs().max()) < 64 and M * 64 * 3 * M < xo.EXACT_LIMIT
    assert torch.equal((dw * M).round(), dw * M)
    return dict(S=S, Q=Q, m1=S / M, k2=Q / M, dY=dY, dYb=dYb, dw=dw)


def stem_padding_lanes(dwp: torch.Tensor) -> torch.Tensor:
    return dwp.reshape(dwp.shape[0], 16, 16)[:, :, 12:]


# --------------------------------------------------------------------------------- fork data-gradient epilogue
def even_pixels(n: int, H: int, W: int) -> torch.Tensor:
    """[n*H*W] bool: output rows (n, h, w) with h and w both even."""
    ev = (torch.arange(H) % 2 == 0).view(H, 1) & (torch.arange(W) % 2 == 0).view(1, W)
    return ev.view(1, H, W).expand(n, H, W).reshape(-1)


def spread2(E: torch.Tensor, n: int, H: int, W: int) -> torch.Tensor:
    """The compact stride-2 gradient E [n, H/2, W/2, N] as [n*H*W, N] rows: E at the even pixels, 0 elsewhere."""
    out = torch.zeros(n, H, W, E.shape[-1], dtype=torch.float64, device=E.device)
    out[:, ::2, ::2] = E.double()
    return out.view(n * H * W, -1)


def as_addend2(E: torch.Tensor, dev) -> torch.Tensor:
    """E [n, H/2, W/2, N] as the kernels take it: bf16 [n, N, H/2, W/2] in channels_last memory."""
    return E.to(dev, torch.bfloat16).contiguous().permute(0, 3, 1, 2)


def fork_ref(acc, D, bits, E, n, H, W):
    """bf16(bf16(bf16(acc) + (bit ? D : 0)) + E at even pixels): the order is part of the contract. D, bits and E
    may be None; without E the row stays what ``xo.add_rounded`` gives."""
    v = xo.round_bf16(acc)
    if D is not None:
        v = xo.add_rounded(acc, D, bits)
    if E is not None:
        v = xo.round_bf16(v + spread2(E, n, H, W).to(acc.device))
    return v


def fork_single(acc, D, bits, E, n, H, W):
    """The same sum with one rounding at the end."""
    s = acc.clone()
    if D is not None:
        d = D.double().to(acc.device)
        s = s + (d if bits is None else d * bits.to(acc.device).double().view(acc.shape))
    if E is not None:
        s = s + spread2(E, n, H, W).to(acc.device)
    return xo.round_bf16(s)


def order_witness(acc, D, bits, E, n, H, W, amax: int = xo.ADDEND_MAX) -> int:
    """How many elements of the masked three-rounding result differ from the single-rounding sum (CPU tensors).
    When none does, one (D, E) pair at an even pixel whose mask bit is set is moved (in place, within +-amax) until
    one does; 0 only when no element can: |acc| + amax < 256 everywhere, where nothing rounds at all."""
    count = lambda: int((fork_ref(acc, D, bits, E, n, H, W) != fork_single(acc, D, bits, E, n, H, W)).sum())  # noqa: E731
    c = count()
    if c or float(acc.abs().max()) + amax < 256:
        return c
    ok = even_pixels(n, H, W).view(-1, 1) & (bits.view(acc.shape) == 1)
    cand = torch.where(ok, acc.abs(), torch.full_like(acc, -1.0)).flatten().topk(min(32, acc.numel())).indices
    d = torch.arange(-amax, amax + 1, dtype=torch.float64).view(-1, 1)
    e = torch.arange(-amax, amax + 1, dtype=torch.float64).view(1, -1)
    for i in cand.tolist():
        m, c_ = divmod(i, acc.shape[1])
        a = acc[m, c_]
        if not bool(ok[m, c_]):
            continue
        three = xo.round_bf16(xo.round_bf16(xo.round_bf16(a.view(1, 1)) + d) + e)
        hit = (three != xo.round_bf16(a + d + e)).nonzero()
        if hit.numel():
            di, ei = hit[0].tolist()
            w_, h_ = (m % W) // 2, ((m // W) % H) // 2
            D[m, c_], E[m // (H * W), h_, w_, c_] = float(d[di, 0]), float(e[0, ei])
            return count()
    return 0


def bn_partials_ref(dy, x, cf_or_ws, bits, mode):
    """Exact per-channel sums of dy' and dy' (x - mean), float64 [rows, C]: dy' = dy (mode 0), dy where
    scale x + shift > 0 (mode 1), dy where the BN's mask bit is set (mode 2)."""
    mean, sc, sh = cf_or_ws
    g = dy
    if mode == 1:
        g = torch.where(x * sc + sh > 0, dy, torch.zeros_like(dy))
    elif mode == 2:
        g = dy * bits.view(dy.shape).double()
    return torch.stack([g.sum(0), (g * (x - mean)).sum(0)], 1)
