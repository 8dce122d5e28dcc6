"""Exact integer-data oracle for the bf16 / fp32 matrix-core kernels (test_gpu_exact_gemm.py, test_gpu_exact_conv.py).

With integer-valued operands whose worst-case sum of |a * b| stays below 2^24, every product and every partial
sum of a dot product is an integer that fp32 holds exactly, in any order: tile shape, main loop, split-K and the
row groups of a persistent kernel cannot change the result. Each output element then has exactly one correct
value, and a kernel is compared with a float64 reference by ``torch.equal``: no tolerance, no excluded share.
The module shares no code with the package and is importable without a GPU; tests/test_exact_oracle.py checks
it (bounds, order independence, the rounding, the failure report, sensitivity to injected defects) on the CPU.

Three operand regimes, each of which asserts its bound on the worst case (never on the sampled data) and raises
``ValueError`` past it:

dense        both operands integers in [-3, 3]; 9 * K_total < 2^22, two bits under 2^24 (how the bf16 matrix core
             aligns the products of one instruction is not documented). A share of the rows of both operands
             follows one sign pattern (``_align``), so outputs reach the hundreds or thousands and the fp32 -> bf16
             conversion rounds, exact ties included (``count_ties``); from a reduction of 30 up every case also
             holds one planted tie on which round-to-nearest-even and truncation disagree (``tie_partner``).
no-rounding  one operand in [-2, 2], the other with at most 8 nonzeros of +-1 per output row / channel: |y| <= 16,
             no rounding convention matters, and with M_total * 16^2 < 2^24 every BatchNorm-statistics partial
             (sum y, sum y^2) is exact however the rows are grouped into partials.
wide         (fp32 kernels) one operand up to 2^11, the other with at most 3 nonzeros per output element's dot
             product, each up to 2^11: products need about 22 bits, sums stay below 2^24; a reduced-precision
             product path would show.
"""
import torch
import torch.nn.functional as F

DENSE_MAX = 3
DENSE_LIMIT = 1 << 22
NOROUND_A_MAX = 2
NOROUND_NNZ = 8
NOROUND_Y_MAX = NOROUND_A_MAX * NOROUND_NNZ  # 16
EXACT_LIMIT = 1 << 24
WIDE_MAX = 1 << 11
WIDE_NNZ = 3
ADDEND_MAX = 64


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(int(seed))


# ------------------------------------------------------------------------------------------------ bounds
def check_dense(k_total: int, amax: int = DENSE_MAX, bmax: int = DENSE_MAX) -> None:
    """Worst-case sum of |a b| over a reduction of length ``k_total``."""
    if not amax * bmax * int(k_total) < DENSE_LIMIT:
        raise ValueError(f"dense regime: {amax}*{bmax}*{k_total} = {amax * bmax * int(k_total)} >= 2^22")


def check_norounding(m_total: int) -> None:
    """Worst-case sum of y^2 over ``m_total`` rows with |y| <= 16."""
    if not int(m_total) * NOROUND_Y_MAX ** 2 < EXACT_LIMIT:
        raise ValueError(f"no-rounding regime: {m_total} rows * 16^2 >= 2^24, the statistics partials may round")


def check_wide(nnz: int = WIDE_NNZ, amax: int = WIDE_MAX, bmax: int = WIDE_MAX, extra: int = 0) -> None:
    """Worst-case |sum| of ``nnz`` products (plus an addend bounded by ``extra``)."""
    if not nnz * amax * bmax + extra < EXACT_LIMIT:
        raise ValueError(f"wide regime: {nnz}*{amax}*{bmax}+{extra} >= 2^24")


# -------------------------------------------------------------------------------------------- generators
def ints(shape, g: torch.Generator, lo: int, hi: int) -> torch.Tensor:
    """Integers in [lo, hi] as fp32 on the CPU (exact in bf16 up to |v| <= 256)."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


def sparse_signs(rows: int, k: int, g: torch.Generator, nnz: int = NOROUND_NNZ, vmax: int = 1) -> torch.Tensor:
    """[rows, k] with at most ``nnz`` nonzeros per row at random positions; +-1, or random integers of magnitude
    1..vmax. (Positions are drawn with replacement, so a row may hold fewer.)"""
    out = torch.zeros(rows, k)
    n = min(nnz, k)
    pos = torch.randint(0, k, (rows, n), generator=g)
    mag = torch.randint(1, vmax + 1, (rows, n), generator=g).float()
    sign = torch.randint(0, 2, (rows, n), generator=g).float() * 2 - 1
    out.scatter_(1, pos, mag * sign)  # a repeated position keeps one of its values
    assert int((out != 0).sum(1).max()) <= nnz and float(out.abs().max()) <= vmax
    return out


TIE_MIN_K = 30  # shortest reduction that can hold a planted tie: 29 products of at most 9 reach only 261, which
                # rounds down like a truncation; 30 reach 267 = 29 * 9 + 6, half way between 266 and 268 -> 268


def _align(t: torch.Tensor, d: torch.Tensor, g: torch.Generator, share: float) -> torch.Tensor:
    """Give a random ``share`` of the rows of t [rows, K] the signs of the direction d [K]. Zero-mean operands
    alone give |y| ~ 4 sqrt(K), which reaches the first ties (odd integers above 256) only from K in the thousands;
    a row and a column that both follow d give y = sum |a| |w| ~ 2.9 K, so longer reductions round in many
    places, ties included. The values stay integers in [-3, 3]: the worst-case bound is untouched."""
    pick = torch.rand(t.shape[0], generator=g) < share
    return torch.where(pick.unsqueeze(1), t.abs() * d.unsqueeze(0), t)


def _tie_up(t: int) -> bool:
    """A positive integer half way between two bf16 values whose even neighbour is the LARGER one: round-to-nearest
    -even and truncation disagree on it."""
    sh = t.bit_length() - 8
    if sh < 1:
        return False
    ulp = 1 << sh
    return (t % ulp) * 2 == ulp and (t // ulp) % 2 == 1


def tie_partner(u: torch.Tensor, wmax: int = DENSE_MAX):
    """For a fixed integer operand vector u: a vector w, |w| <= wmax, whose dot product with u is a tie that rounds
    up (``_tie_up``), or None when sum wmax |u| cannot reach 257. Every dense case plants one such pair, so that it
    holds at least one tie by construction and not by the luck of a seed."""
    ui = [int(v) for v in u.reshape(-1).tolist()]
    w, total = [0] * len(ui), 0
    for k, v in enumerate(ui):
        if total >= 257:
            break
        if v:
            w[k] = wmax if v > 0 else -wmax
            total += wmax * abs(v)
    if total < 257:
        return None
    for k in [None] + list(range(len(ui))):
        for c in range(-wmax, wmax + 1):
            t = total if k is None else total - w[k] * ui[k] + c * ui[k]
            if _tie_up(t):
                if k is not None:
                    w[k] = c
                return torch.tensor(w, dtype=torch.float32).view(u.shape)
    return None


def _strong(shape, g: torch.Generator) -> torch.Tensor:
    """+-3 everywhere: the operand of a planted tie where the reduction is short."""
    return (torch.randint(0, 2, tuple(shape), generator=g).float() * 2 - 1) * DENSE_MAX


def _partner(u: torch.Tensor, what: str) -> torch.Tensor:
    w = tie_partner(u)
    assert w is not None, f"{what}: no tie can be planted in a reduction of {u.numel()}"
    return w


def dense_gemm(M: int, N: int, K: int, seed: int):
    """(A [M, K], W [N, K]) for y = A W^T in the dense regime (reduction K). From K = 30 up, y[M-1, N-1] is a planted
    tie that rounds up (the last row and column: inside the ragged tiles)."""
    check_dense(K)
    g = gen(seed)
    a, w = ints((M, K), g, -DENSE_MAX, DENSE_MAX), ints((N, K), g, -DENSE_MAX, DENSE_MAX)
    d = torch.randint(0, 2, (K,), generator=g).float() * 2 - 1
    a, w = _align(a, d, g, 0.25), _align(w, d, g, 0.25)
    if K >= TIE_MIN_K:
        if K < 128:
            a[M - 1] = _strong((K,), g)
        w[N - 1] = _partner(a[M - 1], "dense_gemm")
    return a, w


def norounding_gemm(M: int, N: int, K: int, seed: int):
    """(A [M, K] in [-2, 2], W [N, K] with <= 8 nonzeros of +-1 per output channel): |y| <= 16."""
    check_norounding(M)
    g = gen(seed)
    return ints((M, K), g, -NOROUND_A_MAX, NOROUND_A_MAX), sparse_signs(N, K, g)


def gemm_operands(regime: str, M: int, N: int, K: int, seed: int):
    return {"dense": dense_gemm, "norounding": norounding_gemm}[regime](M, N, K, seed)


def dense_conv(N, Cin, H, W, Cout, seed, k: int = 3, stride: int = 1, pad: int = 1):
    """(x [N, Cin, H, W], w [Cout, Cin, k, k]) in the dense regime (reduction k*k*Cin). The last output channel at
    output pixel (1, 1) of the last image (or the nearest that exists) is a planted tie that rounds up."""
    check_dense(k * k * Cin)
    g = gen(seed)
    x, w = ints((N, Cin, H, W), g, -DENSE_MAX, DENSE_MAX), ints((Cout, Cin, k, k), g, -DENSE_MAX, DENSE_MAX)
    d = torch.randint(0, 2, (Cin,), generator=g).float() * 2 - 1  # per input channel: the same for every tap
    xr = _align(x.permute(0, 2, 3, 1).reshape(-1, Cin), d, g, 0.5)  # half of the pixels
    x = xr.view(N, H, W, Cin).permute(0, 3, 1, 2).contiguous()
    wr = _align(w.permute(0, 2, 3, 1).reshape(Cout, -1), d.repeat(k * k), g, 0.25)  # a quarter of the channels
    w = wr.view(Cout, k, k, Cin).permute(0, 3, 1, 2).contiguous()
    oh, ow = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    ph, pw = min(1, oh - 1), min(1, ow - 1)
    taps = [(r, s_) for r in range(k) for s_ in range(k)
            if 0 <= ph * stride + r - pad < H and 0 <= pw * stride + s_ - pad < W]
    if Cin * len(taps) >= TIE_MIN_K:
        u = torch.zeros(Cin, k, k)
        for r, s_ in taps:
            hi, wi = ph * stride + r - pad, pw * stride + s_ - pad
            if Cin * len(taps) < 128:
                x[N - 1, :, hi, wi] = _strong((Cin,), g)
            u[:, r, s_] = x[N - 1, :, hi, wi]
        w[Cout - 1] = _partner(u, "dense_conv")
    return x, w


def dense_conv_dgrad(N, Cin, H, W, Cout, seed, k: int = 3, stride: int = 1, pad: int = 1):
    """(dy [N, Cout, H, W], w [Cout, Cin, k, k]) for a data gradient (reduction at most k*k*Cout; H, W are dy's):
    the forward generator with the channel roles swapped, and a tie planted in dx[N-1, Cin-1] at input pixel (1, 1)
    (or the nearest that dy reaches): dx[h, w] = sum dy[(h + pad - r) / stride, (w + pad - s) / stride] w[r, s] over
    the taps where the division is whole and in range."""
    dy, wt = dense_conv(N, Cout, H, W, Cin, seed, k, 1, pad)
    w = wt.permute(1, 0, 2, 3).contiguous()
    g = gen(seed + 1)
    ph, pw = min(1, (H - 1) * stride), min(1, (W - 1) * stride)
    taps = [(r, s_) for r in range(k) for s_ in range(k)
            if (ph + pad - r) % stride == 0 and 0 <= (ph + pad - r) // stride < H
            and (pw + pad - s_) % stride == 0 and 0 <= (pw + pad - s_) // stride < W]
    if Cout * len(taps) >= TIE_MIN_K:
        u = torch.zeros(Cout, k, k)
        for r, s_ in taps:
            hi, wi = (ph + pad - r) // stride, (pw + pad - s_) // stride
            if Cout * len(taps) < 128:
                dy[N - 1, :, hi, wi] = _strong((Cout,), g)
            u[:, r, s_] = dy[N - 1, :, hi, wi]
        w[:, Cin - 1] = _partner(u, "dense_conv_dgrad")
    return dy, w


def dense_conv_wgrad(N, Cin, H, W, Cout, seed, k: int = 3, stride: int = 1, pad: int = 1):
    """(dy [N, Cout, OH, OW], x [N, Cin, H, W]) for a weight gradient (reduction over the N*OH*OW output pixels,
    whose worst case is checked). dw[Cout-1, Cin-1] at the centre tap, which reads input pixel (oh*stride, ow*stride)
    for every output pixel, is a planted tie that rounds up."""
    oh, ow = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    P = N * oh * ow
    check_dense(P)
    assert k == 2 * pad + 1, "the centre tap is the one that is never out of range"
    g = gen(seed)
    x, dy = ints((N, Cin, H, W), g, -DENSE_MAX, DENSE_MAX), ints((N, Cout, oh, ow), g, -DENSE_MAX, DENSE_MAX)
    if P >= TIE_MIN_K:
        if P < 128:
            dy[:, Cout - 1] = _strong((N, oh, ow), g)
        x[:, Cin - 1, ::stride, ::stride][:, :oh, :ow] = _partner(dy[:, Cout - 1], "dense_conv_wgrad")
    return dy, x


def norounding_conv(N, Cin, H, W, Cout, seed, k: int = 3, stride: int = 1, pad: int = 1):
    """(x in [-2, 2], w with <= 8 nonzeros of +-1 per output channel) with the output pixel count under the
    statistics bound."""
    oh, ow = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    check_norounding(N * oh * ow)
    g = gen(seed)
    x = ints((N, Cin, H, W), g, -NOROUND_A_MAX, NOROUND_A_MAX)
    # the kernels' reduction order is (tap, channel): draw the positions in that layout
    w = sparse_signs(Cout, k * k * Cin, g).view(Cout, k, k, Cin).permute(0, 3, 1, 2).contiguous()
    return x, w


def conv_operands(regime, N, Cin, H, W, Cout, seed, k=3, stride=1, pad=1):
    if regime == "dense":
        return dense_conv(N, Cin, H, W, Cout, seed, k, stride, pad)
    return norounding_conv(N, Cin, H, W, Cout, seed, k, stride, pad)


def wide_conv(N, Cin, H, W, Cout, seed, k: int = 3, extra: int = 0):
    """fp32 operands: x up to 2^11, w with <= 3 nonzeros per output channel, each up to 2^11."""
    check_wide(extra=extra)
    g = gen(seed)
    x = ints((N, Cin, H, W), g, -WIDE_MAX, WIDE_MAX)
    w = sparse_signs(Cout, k * k * Cin, g, WIDE_NNZ, WIDE_MAX).view(Cout, k, k, Cin).permute(0, 3, 1, 2).contiguous()
    return x, w


def wide_sparse_like(shape, seed: int) -> torch.Tensor:
    """An output gradient [N, C, H, W] with at most 3 nonzero pixels per channel (each up to 2^11): every weight
    gradient element is then a sum of at most 3 products."""
    check_wide()
    n, c, h, w = shape
    return sparse_signs(c, n * h * w, gen(seed), WIDE_NNZ, WIDE_MAX).view(c, n, h, w).permute(1, 0, 2, 3).contiguous()


def addend(shape, g: torch.Generator) -> torch.Tensor:
    """A row addend D: integers in [-64, 64]."""
    return ints(shape, g, -ADDEND_MAX, ADDEND_MAX)


def mask_bytes(n_elems: int, g: torch.Generator) -> torch.Tensor:
    """A 1-bit mask as the kernels read it: element i is bit (i % 8) of byte i // 8."""
    return torch.randint(0, 256, ((n_elems + 7) // 8,), generator=g, dtype=torch.uint8)


def mask_bits(mask: torch.Tensor, n_elems: int) -> torch.Tensor:
    """The bits of ``mask_bytes`` as 0/1 int64, element order."""
    m = mask.to(torch.int64)
    return torch.stack([(m >> j) & 1 for j in range(8)], 1).reshape(-1)[:n_elems]


# ------------------------------------------------------------------ device generators (index-edge operands)
# Operands of 10^8 .. 10^9 elements (test_gpu_index_edges.py) are drawn on the device: the CPU generators above
# would take minutes there. Same value ranges, and the same worst-case checks (``check_dense``; for reductions over
# millions of rows ``check_exact_sum`` on a bound taken from the data actually drawn).
def dev_gen(seed: int, device) -> torch.Generator:
    return torch.Generator(device=device).manual_seed(int(seed))


DEV_BLOCK = 1 << 27  # elements drawn at a time: the int8 draw and its masks stay a fraction of the operand


def _dev_fill(shape, g: torch.Generator, dtype, draw) -> torch.Tensor:
    out = torch.empty(tuple(shape), dtype=dtype, device=g.device)
    flat = out.view(-1)
    for i in range(0, flat.numel(), DEV_BLOCK):
        n = min(DEV_BLOCK, flat.numel() - i)
        flat[i:i + n] = draw(n)
    return out


def dev_ints(shape, g: torch.Generator, lo: int, hi: int, dtype=torch.bfloat16) -> torch.Tensor:
    """Integers in [lo, hi] (within int8) on the generator's device."""
    assert -128 <= lo <= hi <= 127
    return _dev_fill(shape, g, dtype,
                     lambda n: torch.randint(lo, hi + 1, (n,), generator=g, device=g.device, dtype=torch.int8))


def dev_dense(shape, g: torch.Generator, k_total: int, dtype=torch.bfloat16) -> torch.Tensor:
    """A dense-regime operand, integers in [-3, 3], for a reduction of length ``k_total`` (checked)."""
    check_dense(k_total)
    return dev_ints(shape, g, -DENSE_MAX, DENSE_MAX, dtype)


def dev_sparse_signs(shape, g: torch.Generator, one_in: int, dtype=torch.bfloat16) -> torch.Tensor:
    """+-1 at about one element in ``one_in``, zero elsewhere, at independent positions."""
    assert 1 <= one_in <= 63

    def draw(n):
        r = torch.randint(0, 2 * one_in, (n,), generator=g, device=g.device, dtype=torch.int8)
        return (r == 0).to(torch.int8) - (r == 1).to(torch.int8)

    return _dev_fill(shape, g, dtype, draw)


def check_exact_sum(bound, what: str = "reduction") -> None:
    """``bound``: an upper bound of the sum of |products| of the longest reduction, taken from the data drawn."""
    if not float(bound) < EXACT_LIMIT:
        raise ValueError(f"{what}: sum of |products| may reach {float(bound):.0f} >= 2^24, fp32 partial sums may round")


# -------------------------------------------------------------------------------------------- references
def integral(ref: torch.Tensor, limit: int = EXACT_LIMIT, what: str = "reference") -> torch.Tensor:
    """The float64 reference must be integer-valued and within the exactly representable range."""
    assert ref.dtype == torch.float64, ref.dtype
    assert bool((ref == ref.round()).all()), f"{what} is not integral"
    assert float(ref.abs().max()) <= limit, f"{what} exceeds {limit}: {float(ref.abs().max())}"
    return ref


def gemm_ref(A: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    """A [M, K] W[N, K]^T in float64 (on whichever device the operands live)."""
    return integral(A.double() @ W.double().t())


def conv_ref(x, w, stride=1, pad=1) -> torch.Tensor:
    return integral(F.conv2d(x.double().cpu(), w.double().cpu(), None, stride, pad))


def conv_dgrad_ref(x_shape, w, dy, stride=1, pad=1) -> torch.Tensor:
    return integral(torch.nn.grad.conv2d_input(tuple(x_shape), w.double().cpu(), dy.double().cpu(), stride, pad))


def conv_wgrad_ref(x, w_shape, dy, stride=1, pad=1) -> torch.Tensor:
    return integral(torch.nn.grad.conv2d_weight(x.double().cpu(), tuple(w_shape), dy.double().cpu(), stride, pad))


TN_BLOCK = 1 << 19


def tn_ref(a: torch.Tensor, b: torch.Tensor, groups: int = 1024) -> torch.Tensor:
    """a[P, M]^T b[P, N] in float64 for a reduction over millions of rows. The rows are split into ``groups`` batch
    entries that are summed afterwards: a plain matmul with an 8 x 8 output would run its whole reduction in one
    workgroup. Integer operands: exact in any grouping."""
    out = torch.zeros(a.shape[1], b.shape[1], dtype=torch.float64, device=a.device)
    for i in range(0, a.shape[0], TN_BLOCK):  # float64 copies of one block at a time
        ab, bb = a[i:i + TN_BLOCK].double(), b[i:i + TN_BLOCK].double()
        P = ab.shape[0]
        g = max(1, min(groups, P // 64))
        main = P // g * g
        out += torch.bmm(ab[:main].reshape(g, -1, ab.shape[1]).transpose(1, 2), bb[:main].reshape(g, -1, bb.shape[1])).sum(0)
        if main < P:
            out += ab[main:].t() @ bb[main:]
    return out


def nonzeros_per_column(t: torch.Tensor, block_rows: int = 0) -> torch.Tensor:
    """Nonzero count of every column of the [rows, C] view of ``t``, in row blocks of 2^24 elements (a whole-tensor
    ``sum`` of the boolean would be carried out in int64: 8 bytes per element of a 10^9-element operand)."""
    r = rows_view(t)
    block_rows = block_rows or max(1, (1 << 24) // r.shape[1])
    n = torch.zeros(r.shape[1], dtype=torch.int64, device=r.device)
    for i in range(0, r.shape[0], block_rows):
        n += (r[i:i + block_rows] != 0).sum(0)
    return n


def conv_ref_dev(x, w, stride=1, pad=1) -> torch.Tensor:
    """``conv_ref`` where the operands live (no copy to the host, no convolution library): float64, tap by tap,
    y[n, :, oh, ow] += x[n, :, oh s + kh - pad, ow s + kw - pad] w[:, :, kh, kw]^T. For slices of large operands."""
    N, Ci, H, W = x.shape
    Co, k = w.shape[0], w.shape[2]
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xb = F.pad(x.permute(0, 2, 3, 1).double(), (0, 0, pad, pad, pad, pad))
    wd = w.double().to(x.device)
    y = torch.zeros(N, OH, OW, Co, dtype=torch.float64, device=x.device)
    for kh in range(k):
        for kw in range(k):
            t = xb[:, kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride, :]
            y += t @ wd[:, :, kh, kw].t()
    return integral(y.permute(0, 3, 1, 2))


def conv_wgrad_ref_dev(dy, x, k, stride, pad, block_pixels=1 << 21) -> torch.Tensor:
    """``conv_wgrad_ref`` where the operands live, for reductions over millions of pixels: float64 [Cout, C, k, k],
    tap by tap over blocks of output rows, dw[co, c, kh, kw] = sum_p dy[p, co] x[c, oh s + kh - pad, ow s + kw - pad].
    Integer operands: every partial sum is exact in float64."""
    N, Co, OH, OW = dy.shape
    Ci, H = x.shape[1], x.shape[2]
    dw = torch.zeros(Co, Ci, k, k, dtype=torch.float64, device=dy.device)
    rows_per = max(1, block_pixels // OW)
    for n in range(N):
        for r0 in range(0, OH, rows_per):
            r1 = min(OH, r0 + rows_per)
            d = dy[n, :, r0:r1, :].permute(1, 2, 0).reshape(-1, Co).double()
            lo, hi = r0 * stride - pad, (r1 - 1) * stride - pad + k  # input rows [lo, hi), may leave the image
            xb = x[n, :, max(lo, 0):min(hi, H), :].permute(1, 2, 0).double()  # [rows, W, C]
            xb = F.pad(xb, (0, 0, pad, pad, max(0, -lo), max(0, hi - H)))
            for kh in range(k):
                for kw in range(k):
                    t = xb[kh:kh + (r1 - r0 - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride, :]
                    dw[:, :, kh, kw] += tn_ref(d, t.reshape(-1, Ci))
    return integral(dw, what="weight gradient reference")


def round_bf16(ref: torch.Tensor) -> torch.Tensor:
    """One round-to-nearest-even to bf16 of an integral float64 tensor below 2^24 (the fp32 step in between is
    exact there), returned as float64."""
    assert ref.dtype == torch.float64 and float(ref.abs().max()) < EXACT_LIMIT
    return ref.float().to(torch.bfloat16).double()


def add_rounded(ref: torch.Tensor, D: torch.Tensor, bits=None) -> torch.Tensor:
    """The tile kernels' addend epilogue, two roundings: bf16(bf16(acc) + (bit ? D : 0))."""
    d = D.double().to(ref.device)
    if bits is not None:
        d = d * bits.to(ref.device).double().view(ref.shape)
    return round_bf16(round_bf16(ref) + d)


def count_ties(ref: torch.Tensor) -> int:
    """How many elements of the integral reference lie exactly half way between two bf16 values (8 significant
    bits): for 2^e <= |v| < 2^(e+1), e >= 8, the spacing is 2^(e-7) and a tie has |v| mod 2^(e-7) == 2^(e-8).
    Odd integers in (256, 512) are the smallest."""
    a = ref.abs().to(torch.int64)
    _, ex = torch.frexp(a.double())  # a = m * 2^ex, m in [0.5, 1): e = ex - 1
    e = (ex.to(torch.int64) - 1).clamp_min(8)
    ulp = torch.ones_like(a) << (e - 7)
    return int(((a >= 256) & ((a % ulp) * 2 == ulp)).sum())


def col_stats(y: torch.Tensor) -> torch.Tensor:
    """[C, 2] exact column sums of y and y^2 for a float64 [rows, C] (or channels-first [N, C, H, W]) tensor."""
    if y.dim() == 4:
        y = y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])
    return torch.stack([y.sum(0), (y * y).sum(0)], 1)


def rows_view(t: torch.Tensor) -> torch.Tensor:
    """[N, C, H, W] as the implicit GEMM's [N*H*W, C]; 2-D tensors as they are."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) if t.dim() == 4 else t


# ------------------------------------------------------------------------------------------ the comparison
def mismatch_report(got: torch.Tensor, ref: torch.Tensor, tile=None, what: str = "", first: int = 6):
    """None when ``got`` equals ``ref`` by value everywhere (signed zero irrelevant, NaN never equal), else a
    one-line report: the count, the first few (index, got, expected), the bounding box and, given
    ``tile=(rows, cols)`` of the [rows, cols] GEMM view, the tile coordinates touched and whether they lie on
    the last (possibly partial) row / column tile."""
    if tuple(got.shape) != tuple(ref.shape):
        return f"{what}: shape {tuple(got.shape)} != expected {tuple(ref.shape)}"
    g, r = got.detach().double(), ref.detach().double().to(got.device)
    if torch.equal(g, r):
        return None
    g, r = g.cpu(), r.cpu()  # the report itself is written on the CPU
    bad = g != r
    idx = bad.nonzero()
    n = idx.shape[0]
    head = ", ".join(f"{tuple(i.tolist())}: got {g[tuple(i.tolist())].item():g} expected {r[tuple(i.tolist())].item():g}"
                     for i in idx[:first])
    lo, hi = idx.min(0).values.tolist(), idx.max(0).values.tolist()
    msg = f"{what}: {n} of {g.numel()} elements differ; first {head}; bounding box {lo}..{hi}"
    if tile is not None:
        b2 = rows_view(bad)
        rows, cols = b2.shape
        tr, tc = int(tile[0]), int(tile[1])
        i2 = b2.nonzero()
        tiles = [tuple(t) for t in torch.unique(torch.stack([i2[:, 0] // tr, i2[:, 1] // tc], 1), dim=0).tolist()]
        last_r, last_c = (rows - 1) // tr, (cols - 1) // tc
        on_r = sum(t[0] == last_r for t in tiles)
        on_c = sum(t[1] == last_c for t in tiles)
        shown = ", ".join(map(str, tiles[:8])) + (" ..." if len(tiles) > 8 else "")
        msg += (f"; {tr}x{tc} tiles touched ({len(tiles)} of {(last_r + 1) * (last_c + 1)}): {shown}; "
                f"{on_r} on the last row tile {last_r} ({rows - last_r * tr} rows), "
                f"{on_c} on the last column tile {last_c} ({cols - last_c * tc} columns)")
    return msg


def assert_exact(got: torch.Tensor, ref: torch.Tensor, tile=None, what: str = "") -> None:
    msg = mismatch_report(got, ref, tile, what)
    if msg is not None:
        raise AssertionError(msg)


def assert_exact_block(got: torch.Tensor, ref: torch.Tensor, what: str = "", row0: int = 0, total_rows=None,
                       tile_rows: int = 128, first: int = 6) -> None:
    """``assert_exact`` for a block of a large operand, compared where it lives (nothing but the few reported
    elements is copied to the host). ``got`` / ``ref``: the same rows [row0, row0 + rows) of the [total_rows, C] GEMM
    view (4-D channels-first tensors are read as their pixel rows). The failure names the element and byte offsets in
    the whole operand, the ``tile_rows``-row tiles touched and how many mismatches lie on the last row tile."""
    g2, r2 = rows_view(got.detach()), rows_view(ref.detach()).to(got.device)
    assert tuple(g2.shape) == tuple(r2.shape), f"{what}: shape {tuple(g2.shape)} != expected {tuple(r2.shape)}"
    if g2.dtype == r2.dtype and torch.equal(g2, r2):
        return
    bad = g2.double() != r2.double()  # NaN never equal, signed zero irrelevant
    if not bool(bad.any()):
        return
    idx = bad.nonzero()
    n, cols, esz = int(idx.shape[0]), int(g2.shape[1]), got.element_size()
    total = int(total_rows) if total_rows is not None else row0 + int(g2.shape[0])
    rows = idx[:, 0] + row0
    lo, hi = int(rows.min()), int(rows.max())
    last_tile = (total - 1) // tile_rows
    on_last = int((rows // tile_rows == last_tile).sum())
    head = []
    for r, c in idx[:first].tolist():
        e = (row0 + r) * cols + c
        head.append(f"row {row0 + r} col {c} (element {e}, byte {e * esz}, row tile {(row0 + r) // tile_rows}): "
                    f"got {float(g2[r, c]):g} expected {float(r2[r, c]):g}")
    raise AssertionError(
        f"{what}: {n} of {g2.numel()} elements of rows [{row0}, {row0 + g2.shape[0]}) differ; first " + "; ".join(head)
        + f"; rows {lo}..{hi} (element offsets {lo * cols}..{(hi + 1) * cols - 1}), {tile_rows}-row tiles "
        f"{lo // tile_rows}..{hi // tile_rows}; {on_last} on the last row tile {last_tile} "
        f"({total - last_tile * tile_rows} rows, from element {last_tile * tile_rows * cols})")
