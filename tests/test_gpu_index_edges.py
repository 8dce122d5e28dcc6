"""The native kernels at the top of their legal index domain (gpu): just under 2^24 pixels, just under 2 GiB per
operand, the largest legal fast-division divisor (65535). Record: profiles/index_edges/README.md.

ops/limits.py, ``check_span`` (csrc/nn_bindings.cpp) and ``kOOB`` (csrc/include/dla_mfma.h) promise that inside
those bounds nothing computes with a wrapped index; the exact-oracle files pin the arithmetic at a few hundred
pixels. Here every case is the smallest tensor that reaches a bound:

A  [1, 8, 255, 65535], Cout 8      largest legal divisor, pixel indices up to 16,711,424
B  [1337, 64, 112, 112], Cout 64   2^24 - 5,888 pixels and 2^31 - 753,664 bytes in one operand (ResNet-50's limit)
C  GEMM A operand [2^24 - 1, 64]   2^31 - 128 bytes: the last row one tile short of kOOB, ragged last row tile
D  conv1x1_dual dy [2^22 - 1, 256] 2^31 - 512 bytes: the one-pass kernel's gate edge
E  stem input [1, 3, 510, 131070]  folded 255 x 65535: fW / fH at 65535 with 16,711,425 output pixels
F  fp32 conv [1, 4, 255, 65535]    fOW / fOH with M just under 2^24, 3x3 and 1x1

Rules (test_gpu_exact_conv.py's, at this size): integer operands from tests/exact_oracle.py drawn on the device,
every comparison exact and on the device, outputs NaN-poisoned first, setters restored by the fixture. Reductions
over ~2^24 rows use sparse +-1 data, and the bound on the sum of |products| is asserted on the data drawn.

Two kinds of reference. (1) float64 (``xo.*_ref``) on slices: the first and last two rows of the first and last
image, both sides of every image boundary among the last 8 images, a band in the middle -- where a wrong quotient
or a wrapped offset lands. (2) Whole-tensor equality with small-geometry calls of the same binding, which
test_gpu_exact_conv.py / test_gpu_exact_gemm.py pin: batch chunks of at most 64 images (B), row bands with halo rows
of the one image (A, E, F; the bands overlap by their halo, so every row is the interior of one band), float64
chunks of 2^20 rows for the GEMMs (C, D: checked everywhere against float64). Weight gradients and statistics equal
the float64 sum of the chunk results, and the weight gradients also a float64 tap-by-tap reference on the device.
Each test asserts the number of output rows no reference covered: 0 in every case.

One step past each limit every binding refuses on the host, nothing launched (uninitialised operands)."""
import pytest
import torch

import exact_oracle as xo

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
CL = torch.channels_last
LIMIT, SPAN = 1 << 24, 1 << 31
CHUNK_ROWS = 1 << 20


@pytest.fixture
def C():
    from distributed_learning_amd.ops import _ext

    C = _ext.require()
    yield C
    C.set_mfma_pipeline(-1)
    C.set_gemm_stream(-1)
    C.set_stem_stream(-1)
    C.set_halo_wgrad(-1)
    C.set_tn256(-1)
    C.set_wgrad_w4(-1)


# ---- operands: built once per case, the previous case's freed first (peak of the file: one case) ----
_CASE = {}
PEAK = {}


def _reset_peak(dev):
    torch.zeros(1, device=dev)  # the allocator has no statistics before its first allocation
    torch.cuda.reset_peak_memory_stats(dev)


def _case(name, build, dev):
    if name not in _CASE:
        _release()
        _reset_peak(dev)
        _CASE[name] = build()
    return _CASE[name]


def _release():
    for name in list(_CASE):
        PEAK[name] = torch.cuda.max_memory_allocated()
        print(f"[index-edges] case {name}: peak allocation {PEAK[name] / 2 ** 30:.2f} GiB")
    _CASE.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", autouse=True)
def _free_at_the_end():
    yield
    if torch.cuda.is_available():
        _release()


def _poison(dev, *shape, dtype=BF):
    t = torch.full(shape, float("nan"), device=dev, dtype=dtype)
    del t


def _nhwc(t):
    """A contiguous [N, H, W, C] block as the channels_last [N, C, H, W] tensor it is."""
    t = t.permute(0, 3, 1, 2)
    assert t.is_contiguous(memory_format=CL) or t.shape[1] == 1 or t.shape[0] == 1
    return t


def _w3(t, dev, dtype=BF):
    return t.to(dev, dtype).contiguous(memory_format=CL)


def _sparse_w(cout, cin, k, seed):
    """<= 8 nonzeros of +-1 per output channel, drawn in the kernels' (tap, channel) order."""
    return xo.sparse_signs(cout, k * k * cin, xo.gen(seed)).view(cout, k, k, cin).permute(0, 3, 1, 2).contiguous()


def _edge_slices(N, H):
    """(image, first output row, rows) of the float64 slices."""
    s = set()
    for n in (0, N - 1):
        s |= {(n, 0, 2), (n, H - 2, 2)}
    for n in range(max(1, N - 8), N):
        s |= {(n - 1, H - 2, 2), (n, 0, 2)}
    s.add((N // 2, H // 2 - 2, 4))
    return sorted(s)


def _bands(H, band, halo=1):
    """(b, e, a, z): output rows [b, e) need input rows [a, z) of a stride-1 window with ``halo`` rows each side."""
    for b in range(0, H, band):
        e = min(H, b + band)
        yield b, e, max(0, b - halo), min(H, e + halo)


def _rows(t):
    return xo.rows_view(t)


def _stats_of(y):
    """[C, 2] float64 column sums of y and y^2 of a device block."""
    return xo.col_stats(_rows(y).double())


def _conv_slice_ref(x, w, n, r0, nr, stride=1):
    """float64 3x3 / pad 1 forward rows [r0, r0 + nr) of image n from the input rows they read."""
    H = x.shape[2]
    if r0 == 0:
        a, skip = 0, 0
    else:
        a, skip = r0 * stride - stride, 1  # one output row above: the slice's own zero padding lands there
    z = min(H, (r0 + nr - 1) * stride + 2)
    ref = xo.conv_ref(x[n:n + 1, :, a:z, :].float(), w.float(), stride, 1)
    return ref[:, :, skip:skip + nr, :]


# =============================================================================================== case A
A_SHAPE = (1, 8, 255, 65535)
A_COUT = 8
BAND = 32


def _build_a(dev):
    N, Ci, H, W = A_SHAPE
    assert N * H * W == 16711425 < LIMIT and W == 65535
    g = xo.dev_gen(11, dev)
    x = _nhwc(xo.dev_sparse_signs((N, H, W, Ci), g, 32))
    return {"x": x, "g": g}


def test_a_conv3x3_fwd_with_statistics(cuda, C):
    a = _case("A", lambda: _build_a(cuda), cuda)
    x = a["x"]
    N, Ci, H, W = A_SHAPE
    w = _sparse_w(A_COUT, Ci, 3, 5)
    wd = _w3(w, cuda)
    _poison(cuda, N * H * W, A_COUT)
    y, st = C.conv3x3_fwd(x, wd, 1, True)
    assert y.shape == (N, A_COUT, H, W) and y.is_contiguous(memory_format=CL)
    # (1) float64 slices
    for n, r0, nr in _edge_slices(N, H):
        xo.assert_exact(y[n:n + 1, :, r0:r0 + nr, :], xo.round_bf16(_conv_slice_ref(x, w, n, r0, nr)), (128, 128),
                        f"conv3x3_fwd A rows [{r0}, {r0 + nr})")
    # (2) row bands of the same binding, and the statistics from the verified output
    covered = torch.zeros(H, dtype=torch.bool)
    ystats = torch.zeros(A_COUT, 2, dtype=F64, device=cuda)
    for b, e, lo, hi in _bands(H, BAND):
        yb, _ = C.conv3x3_fwd(x[:, :, lo:hi, :].clone(memory_format=CL), wd, 1, False)
        xo.assert_exact_block(y[:, :, b:e, :], yb[:, :, b - lo:e - lo, :], f"conv3x3_fwd A rows [{b}, {e})", b * W,
                              H * W)
        covered[b:e] = True
        ystats += _stats_of(y[:, :, b:e, :])
    assert int((~covered).sum()) == 0, "output rows no reference covers"
    assert float((y != 0).float().mean()) > 0.1, "the sparse operands leave the output almost empty"
    xo.check_exact_sum(ystats[:, 1].max(), "statistics sum of y^2 over 16.7M pixels")
    xo.assert_exact(st.double().sum(0), ystats, None, "conv3x3_fwd A statistics")


@pytest.mark.parametrize("with_addend", [False, True])
def test_a_conv3x3_dgrad(cuda, C, with_addend):
    a = _case("A", lambda: _build_a(cuda), cuda)
    N, Ci, H, W = A_SHAPE
    g = xo.dev_gen(12, cuda)
    dy = _nhwc(xo.dev_dense((N, H, W, A_COUT), g, 9 * A_COUT))
    w = xo.ints((A_COUT, Ci, 3, 3), xo.gen(6), -3, 3)
    wd = _w3(w, cuda)
    D = _nhwc(xo.dev_ints((N, H, W, Ci), g, -xo.ADDEND_MAX, xo.ADDEND_MAX)) if with_addend else None
    _poison(cuda, N * H * W, Ci)
    dx = C.conv3x3_dgrad(dy, wd, D)
    assert dx.shape == A_SHAPE and dx.is_contiguous(memory_format=CL)
    for n, r0, nr in _edge_slices(N, H):
        lo, hi = max(0, r0 - 1), min(H, r0 + nr + 1)
        ref = xo.conv_dgrad_ref((1, Ci, hi - lo, W), w, dy[n:n + 1, :, lo:hi, :].float())[:, :, r0 - lo:r0 - lo + nr, :]
        exp = xo.add_rounded(ref, D[n:n + 1, :, r0:r0 + nr, :].float().cpu()) if with_addend else xo.round_bf16(ref)
        xo.assert_exact(dx[n:n + 1, :, r0:r0 + nr, :], exp, (128, 128), f"conv3x3_dgrad A rows [{r0}, {r0 + nr})")
    covered = torch.zeros(H, dtype=torch.bool)
    for b, e, lo, hi in _bands(H, BAND):
        Db = D[:, :, lo:hi, :].clone(memory_format=CL) if with_addend else None
        db = C.conv3x3_dgrad(dy[:, :, lo:hi, :].clone(memory_format=CL), wd, Db)
        xo.assert_exact_block(dx[:, :, b:e, :], db[:, :, b - lo:e - lo, :], f"conv3x3_dgrad A rows [{b}, {e})", b * W,
                              H * W)
        covered[b:e] = True
    assert int((~covered).sum()) == 0, "output rows no reference covers"


def test_a_conv3x3_wgrad(cuda, C):
    """Reduction over all 16.7M pixels (split arithmetic included): dy in [-2, 2], x sparse +-1."""
    a = _case("A", lambda: _build_a(cuda), cuda)
    x = a["x"]
    N, Ci, H, W = A_SHAPE
    dy = _nhwc(xo.dev_ints((N, H, W, A_COUT), xo.dev_gen(13, cuda), -2, 2))
    xo.check_exact_sum(2 * int(xo.nonzeros_per_column(x).max()), "conv3x3_wgrad A: 2 * nonzeros of one input channel")
    _poison(cuda, A_COUT, 9 * Ci, dtype=F32)
    dw = C.conv3x3_wgrad(dy, x, 1, F32)
    assert dw.shape == (A_COUT, Ci, 3, 3)
    xo.assert_exact(dw, xo.conv_wgrad_ref_dev(dy, x, 3, 1, 1), None, "conv3x3_wgrad A against float64")
    # the float64 sum of the same binding over row bands (dy zero on the halo rows: they belong to the neighbours)
    total = torch.zeros(A_COUT, Ci, 3, 3, dtype=F64, device=cuda)
    rows = 0
    for b, e, lo, hi in _bands(H, BAND):
        dyb = dy[:, :, lo:hi, :].clone(memory_format=CL)
        dyb[:, :, :b - lo, :] = 0
        dyb[:, :, e - lo:, :] = 0
        total += C.conv3x3_wgrad(dyb, x[:, :, lo:hi, :].clone(memory_format=CL), 1, F32).double()
        rows += e - b
    assert rows == H
    xo.assert_exact(dw, total, None, "conv3x3_wgrad A against the sum over row bands")


# ---- the halo weight gradient (64 -> 64 channels, W <= 61) on both sides of its gate. It decodes padded positions
# q < N (H + 2) (W + 2): the gate is N (H + 2) < 2^24 (which is q < 2^24 (W + 2), the range of the first division) and
# H + 2 < 65536; past it the implicit-GEMM kernel runs. With fewer than 2^24 pixels q stays below 9 * 2^24 / 3, so
# the top of the first division is reached at H = W = 1.
HALO_GATE = [  # N, H, W, on the halo kernel
    (5592404, 1, 1, True),    # N (H + 2) = 2^24 - 4: padded positions up to 3 * 2^24 - 13 with the divisor 3
    (5592406, 1, 1, False),   # N (H + 2) = 2^24 + 2
    (200, 65533, 1, True),    # H + 2 = 65535, the largest legal second divisor, r up to 13,106,999
    (1, 65534, 61, False),    # H + 2 = 65536
]


@pytest.mark.parametrize("N,H,W,halo", HALO_GATE)
def test_halo_wgrad_on_both_sides_of_its_gate(cuda, C, N, H, W, halo):
    _release()
    _reset_peak(cuda)
    C.set_halo_wgrad(1)
    assert N * H * W < LIMIT and C.halo_wgrad_eligible(64, 64, W, 1)
    assert C.halo_wgrad_serves(N, H, W, 64, 64, 1) == halo
    assert (N * (H + 2) < LIMIT and H + 2 < 65536) == halo
    g = xo.dev_gen(N + H + W, cuda)
    x = _nhwc(xo.dev_sparse_signs((N, H, W, 64), g, 32))
    dy = _nhwc(xo.dev_ints((N, H, W, 64), g, -2, 2))
    xo.check_exact_sum(2 * int(xo.nonzeros_per_column(x).max()), "halo conv3x3_wgrad: 2 * nonzeros of one input channel")
    _poison(cuda, 64, 9 * 64, dtype=F32)
    dw = C.conv3x3_wgrad(dy, x, 1, F32)
    if H == 1 and W == 1:  # one pixel per image: only the centre tap is inside it
        ref = torch.zeros(64, 64, 3, 3, dtype=F64, device=cuda)
        ref[:, :, 1, 1] = xo.tn_ref(_rows(dy), _rows(x))
        ref = xo.integral(ref)
    else:
        ref = xo.conv_wgrad_ref_dev(dy, x, 3, 1, 1)
    assert float(ref.abs().max()) > 100
    xo.assert_exact(dw, ref, None, f"conv3x3_wgrad {'halo' if halo else 'implicit GEMM'} [{N}, 64, {H}, {W}]")
    del x, dy
    PEAK[f"halo {N}x{H}x{W}"] = torch.cuda.max_memory_allocated()


# =============================================================================================== case B
B_SHAPE = (1337, 64, 112, 112)
B_COUT = 64
B_CHUNK = 64


def _build_b(dev):
    N, Ci, H, W = B_SHAPE
    assert N * H * W == LIMIT - 5888 and N * H * W * Ci * 2 == SPAN - 753664
    g = xo.dev_gen(21, dev)
    return {"x": _nhwc(xo.dev_sparse_signs((N, H, W, Ci), g, 32))}


def _b_chunks():
    N = B_SHAPE[0]
    return [(i, min(N, i + B_CHUNK)) for i in range(0, N, B_CHUNK)]


@pytest.mark.parametrize("stride", [1, 2])
def test_b_conv3x3_fwd(cuda, C, stride):
    """Cout 64 keeps the output (2^31 - 753,664 bytes at stride 1) inside the 2 GiB output check, so the statistics
    form runs; one more group of 8 output channels is refused by that check (the other side of it)."""
    x = _case("B", lambda: _build_b(cuda), cuda)["x"]
    N, Ci, H, W = B_SHAPE
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    assert N * H * W * B_COUT * 2 < SPAN <= N * H * W * (B_COUT + 8) * 2
    with pytest.raises(RuntimeError, match="conv3x3: the output reaches the 2 GiB"):
        C.conv3x3_fwd(x, torch.empty(B_COUT + 8, Ci, 3, 3, dtype=BF, device=cuda).contiguous(memory_format=CL), 1, False)
    w = _sparse_w(B_COUT, Ci, 3, 7)
    wd = _w3(w, cuda)
    _poison(cuda, N * OH * OW, B_COUT)
    y, st = C.conv3x3_fwd(x, wd, stride, True)
    assert y.shape == (N, B_COUT, OH, OW) and y.is_contiguous(memory_format=CL)
    for n, r0, nr in _edge_slices(N, OH):
        xo.assert_exact(y[n:n + 1, :, r0:r0 + nr, :], xo.round_bf16(_conv_slice_ref(x, w, n, r0, nr, stride)),
                        (128, 128), f"conv3x3_fwd B stride {stride} image {n} rows [{r0}, {r0 + nr})")
    images = 0
    ystats = torch.zeros(B_COUT, 2, dtype=F64, device=cuda)
    cstats = torch.zeros(B_COUT, 2, dtype=F64, device=cuda)
    for i, j in _b_chunks():
        yc, sc = C.conv3x3_fwd(x[i:j], wd, stride, True)
        xo.assert_exact_block(y[i:j], yc, f"conv3x3_fwd B stride {stride} images [{i}, {j})", i * OH * OW, N * OH * OW)
        ystats += _stats_of(yc)
        cstats += sc.double().sum(0)
        images += j - i
    assert images == N, "images no reference covers"
    xo.check_exact_sum(ystats[:, 1].max(), "statistics sum of y^2")
    xo.assert_exact(st.double().sum(0), ystats, None, f"conv3x3_fwd B stride {stride} statistics against the output's")
    xo.assert_exact(st.double().sum(0), cstats, None, f"conv3x3_fwd B stride {stride} statistics against the chunks'")


def test_b_conv3x3s2_dgrad(cuda, C):
    """dx [1337, 64, 112, 112] is the operand 753,664 bytes under 2 GiB."""
    N, Ci, H, W = B_SHAPE
    _case("B", lambda: _build_b(cuda), cuda)
    g = xo.dev_gen(22, cuda)
    dy = _nhwc(xo.dev_dense((N, H // 2, W // 2, B_COUT), g, 9 * B_COUT))
    w = xo.ints((B_COUT, Ci, 3, 3), xo.gen(8), -3, 3)
    wd = _w3(w, cuda)
    _poison(cuda, N * H * W, Ci)
    dx = C.conv3x3s2_dgrad(dy, wd, H, W)
    assert dx.shape == B_SHAPE and dx.is_contiguous(memory_format=CL)
    for n in sorted({0, N // 2} | set(range(N - 9, N))):  # whole images: every row the slice rule names lies in them
        ref = xo.conv_dgrad_ref((1, Ci, H, W), w, dy[n:n + 1].float(), 2, 1)
        xo.assert_exact(dx[n:n + 1], xo.round_bf16(ref), (128, 128), f"conv3x3s2_dgrad B image {n}")
    images = 0
    for i, j in _b_chunks():
        xo.assert_exact_block(dx[i:j], C.conv3x3s2_dgrad(dy[i:j], wd, H, W), f"conv3x3s2_dgrad B images [{i}, {j})",
                              i * H * W, N * H * W)
        images += j - i
    assert images == N, "images no reference covers"


def test_b_conv3x3_wgrad_stride2(cuda, C):
    x = _case("B", lambda: _build_b(cuda), cuda)["x"]
    N, Ci, H, W = B_SHAPE
    dy = _nhwc(xo.dev_ints((N, H // 2, W // 2, B_COUT), xo.dev_gen(23, cuda), -2, 2))
    xo.check_exact_sum(2 * int(xo.nonzeros_per_column(x).max()), "conv3x3_wgrad B: 2 * nonzeros of one input channel")
    _poison(cuda, B_COUT, 9 * Ci, dtype=F32)
    dw = C.conv3x3_wgrad(dy, x, 2, F32)
    total = torch.zeros(B_COUT, Ci, 3, 3, dtype=F64, device=cuda)
    ref = torch.zeros_like(total)
    for i, j in _b_chunks():
        total += C.conv3x3_wgrad(dy[i:j], x[i:j], 2, F32).double()
        ref += xo.conv_wgrad_ref_dev(dy[i:j], x[i:j], 3, 2, 1)
    xo.assert_exact(dw, ref, None, "conv3x3_wgrad B stride 2 against float64")
    xo.assert_exact(dw, total, None, "conv3x3_wgrad B stride 2 against the sum over batch chunks")


# =============================================================================================== case C
C_M, C_K, C_N = LIMIT - 1, 64, 8


def _build_c(dev):
    assert C_M * C_K * 2 == SPAN - 128 and C_M % 128 == 127  # ragged last row tile, one tile short of kOOB
    g = xo.dev_gen(31, dev)
    return {"A": xo.dev_dense((C_M, C_K), g, C_K), "g": g}


def _row_chunks(M):
    return [(i, min(M, i + CHUNK_ROWS)) for i in range(0, M, CHUNK_ROWS)]


@pytest.mark.parametrize("kmajor", [False, True])
def test_c_gemm_nt(cuda, C, kmajor):
    A = _case("C", lambda: _build_c(cuda), cuda)["A"]
    W = xo.ints((C_N, C_K), xo.gen(9), -3, 3).to(cuda, BF)
    Wk = W.t().contiguous()
    _poison(cuda, C_M, C_N)
    y, _ = C.gemm_nt(A, Wk if kmajor else W, False, None, kmajor)
    assert y.shape == (C_M, C_N)
    rows = 0
    for i, j in _row_chunks(C_M):
        xo.assert_exact_block(y[i:j], xo.round_bf16(xo.gemm_ref(A[i:j], W)), f"gemm_nt C rows [{i}, {j})", i, C_M)
        rows += j - i
    assert rows == C_M, "rows no reference covers"


def test_c_gemm_tn(cuda, C):
    """dy [M, 8]^T x [M, 64] in fp32: the reduction runs over all 2^24 - 1 rows."""
    c = _case("C", lambda: _build_c(cuda), cuda)
    A = c["A"]
    dy = xo.dev_sparse_signs((C_M, C_N), xo.dev_gen(32, cuda), 8)
    xo.check_exact_sum(3 * int(xo.nonzeros_per_column(dy).max()), "gemm_tn C: 3 * nonzeros of one dy column")
    _poison(cuda, C_N, C_K, dtype=F32)
    out = C.gemm_tn(dy, A, F32, 1.0)
    ref = torch.zeros(C_N, C_K, dtype=F64, device=cuda)
    for i, j in _row_chunks(C_M):
        ref += xo.tn_ref(dy[i:j], A[i:j])
    xo.assert_exact(out, xo.integral(ref), None, "gemm_tn C")


def test_c_host_predicates_on_both_sides_of_2_gib(cuda, C):
    """No launch: the gates of the streaming, apply and one-pass kernels at the last legal M and one row later."""
    C.set_gemm_stream(1)
    m = LIMIT - 1  # [m, 64] bf16 spans 2^31 - 128 bytes
    assert C.gemm_stream_rows(m, 64, 64, 64, 64) > 0 and C.gemm_stream_rows(m + 1, 64, 64, 64, 64) == 0
    assert C.gemm_stream_rows(m, 64, 64, 64, 64, True, True) > 0 and C.gemm_stream_rows(m + 1, 64, 64, 64, 64, True, True) == 0
    assert C.gemm_nt_apply_ok(m, 64, 64) and not C.gemm_nt_apply_ok(m + 1, 64, 64)
    assert C.gemm_nt_stream_apply_ok(m, 64, 64) and not C.gemm_nt_stream_apply_ok(m + 1, 64, 64)
    m = (1 << 22) - 1  # dy [m, 256] spans 2^31 - 512 bytes
    assert C.conv1x1_dual_blocks(m, 64, 256) > 0 and C.conv1x1_dual_blocks(m + 1, 64, 256) == 0
    m = (1 << 21) - 1  # Cout 512
    assert C.conv1x1_dual_blocks(m, 128, 512) > 0 and C.conv1x1_dual_blocks(m + 1, 128, 512) == 0


# =============================================================================================== case D
D_M, D_CI, D_CO = (1 << 22) - 1, 64, 256


def test_d_conv1x1_dual(cuda, C):
    """The one-pass 1x1 gradients at their gate's edge (no BN apply): dx = dy w, dw = dy^T x over 2^22 - 1 rows."""
    _release()
    _reset_peak(cuda)
    assert D_M * D_CO * 2 == SPAN - 512 and C.conv1x1_dual_blocks(D_M, D_CI, D_CO) > 0
    g = xo.dev_gen(41, cuda)
    dy = xo.dev_sparse_signs((D_M, D_CO), g, 8)
    x = xo.dev_dense((D_M, D_CI), g, 1)
    xo.check_dense(D_CO, 1, 3)
    xo.check_exact_sum(3 * int(xo.nonzeros_per_column(dy).max()), "conv1x1_dual D: 3 * nonzeros of one dy column")
    w = xo.ints((D_CO, D_CI), xo.gen(10), -3, 3).to(cuda, BF)
    _poison(cuda, D_M, D_CI)
    dx, dw = C.conv1x1_dual(dy, x, w, F32)
    assert dx.shape == (D_M, D_CI) and dw.shape == (D_CO, D_CI) and dw.dtype == F32
    ref_dw = torch.zeros(D_CO, D_CI, dtype=F64, device=cuda)
    rows = 0
    for i, j in _row_chunks(D_M):
        xo.assert_exact_block(dx[i:j], xo.round_bf16(xo.gemm_ref(dy[i:j], w.t())), f"conv1x1_dual D dx rows [{i}, {j})",
                              i, D_M, 64)
        ref_dw += xo.tn_ref(dy[i:j], x[i:j])
        rows += j - i
    assert rows == D_M, "rows no reference covers"
    xo.assert_exact(dw, xo.integral(ref_dw), None, "conv1x1_dual D dw")
    del dy, x, dx
    PEAK["D"] = torch.cuda.max_memory_allocated()
    print(f"[index-edges] case D: peak allocation {PEAK['D'] / 2 ** 30:.2f} GiB")


# =============================================================================================== case E
E_SHAPE = (1, 3, 510, 131070)
E_COUT = 64
E_BAND = 32


def _build_e(dev):
    N, _, H, W = E_SHAPE
    assert N * (H // 2) * (W // 2) == 16711425 < LIMIT and W // 2 == 65535
    x = _nhwc(xo.dev_sparse_signs((N, H, W, 3), xo.dev_gen(51, dev), 32))
    return {"x": x}


def _stem_bands(OH, band):
    """(b, e, b0, e0): output rows [b, e) are the interior of the band of output rows [b0, e0) = input rows
    [2 b0, 2 e0): a 7x7 / s2 / p3 output row reads input rows 2 oh - 3 .. 2 oh + 3, two output rows each side."""
    for b in range(0, OH, band):
        e = min(OH, b + band)
        yield b, e, max(0, b - 2), min(OH, e + 2)


@pytest.mark.parametrize("stream", [0, 1])
def test_e_stem_fwd(cuda, C, stream):
    from distributed_learning_amd.ops.conv import stem_pack_weight

    x = _case("E", lambda: _build_e(cuda), cuda)["x"]
    N, _, H, W = E_SHAPE
    OH, OW = H // 2, W // 2
    wt = _sparse_w(E_COUT, 3, 7, 14)
    wpk = stem_pack_weight(wt.to(cuda, BF))
    C.set_stem_stream(stream)
    _poison(cuda, N * OH * OW, E_COUT)
    y, st, xs = C.stem_fwd(x, wpk, True)
    assert y.shape == (N, E_COUT, OH, OW) and y.is_contiguous(memory_format=CL) and xs.shape == (N, OH, OW, 16)
    # which kernel decoded: the tile kernel writes one statistics row per 128 pixels, the persistent streaming
    # kernel (sfW / sfH) one per row group, 8 per XCD slot and at most 256
    tile_rows = (N * OH * OW + 127) // 128
    assert st.shape[0] == tile_rows if stream == 0 else (0 < st.shape[0] <= 256 and st.shape[0] % 8 == 0), st.shape
    for n, r0, nr in _edge_slices(N, OH):
        b0, e0 = max(0, r0 - 2), min(OH, r0 + nr + 2)
        ref = xo.conv_ref_dev(x[:, :, 2 * b0:2 * e0, :], wt, 2, 3)[:, :, r0 - b0:r0 - b0 + nr, :]
        xo.assert_exact(y[:, :, r0:r0 + nr, :], xo.round_bf16(ref), (128, 64), f"stem_fwd E rows [{r0}, {r0 + nr})")
    covered = torch.zeros(OH, dtype=torch.bool)
    ystats = torch.zeros(E_COUT, 2, dtype=F64, device=cuda)
    for b, e, b0, e0 in _stem_bands(OH, E_BAND):
        yb = C.stem_fwd(x[:, :, 2 * b0:2 * e0, :].clone(memory_format=CL), wpk, True)[0]
        xo.assert_exact_block(y[:, :, b:e, :], yb[:, :, b - b0:e - b0, :], f"stem_fwd E rows [{b}, {e})", b * OW,
                              OH * OW)
        covered[b:e] = True
        ystats += _stats_of(y[:, :, b:e, :])
    assert int((~covered).sum()) == 0, "output rows no reference covers"
    xo.check_exact_sum(ystats[:, 1].max(), "stem statistics sum of y^2")
    xo.assert_exact(st.double().sum(0), ystats, None, f"stem_fwd E statistics, stream {stream}")


def test_e_stem_wgrad(cuda, C):
    from distributed_learning_amd.ops.conv import stem_pack_weight, stem_unpack_grad

    x = _case("E", lambda: _build_e(cuda), cuda)["x"]
    N, _, H, W = E_SHAPE
    OH, OW = H // 2, W // 2
    wpk = stem_pack_weight(_sparse_w(E_COUT, 3, 7, 14).to(cuda, BF))
    dy = _nhwc(xo.dev_ints((N, OH, OW, E_COUT), xo.dev_gen(52, cuda), -2, 2))
    xo.check_exact_sum(2 * int(xo.nonzeros_per_column(x).max()), "stem_wgrad E: 2 * nonzeros of one input channel")
    xs = C.stem_fwd(x, wpk, False)[2]
    _poison(cuda, E_COUT, 256, dtype=F32)
    dwp = C.stem_wgrad(dy, xs, H, W, F32)
    xo.assert_exact(stem_unpack_grad(dwp), xo.conv_wgrad_ref_dev(dy, x, 7, 2, 3), None, "stem_wgrad E against float64")
    total = torch.zeros(E_COUT, 256, dtype=F64, device=cuda)
    rows = 0
    for b, e, b0, e0 in _stem_bands(OH, E_BAND):
        dyb = dy[:, :, b0:e0, :].clone(memory_format=CL)
        dyb[:, :, :b - b0, :] = 0
        dyb[:, :, e - b0:, :] = 0
        xsb = C.stem_fwd(x[:, :, 2 * b0:2 * e0, :].clone(memory_format=CL), wpk, False)[2]
        total += C.stem_wgrad(dyb, xsb, 2 * (e0 - b0), W, F32).double()
        rows += e - b
    assert rows == OH
    xo.assert_exact(dwp, total, None, "stem_wgrad E against the sum over row bands")


# =============================================================================================== case F
F_SHAPE = (1, 4, 255, 65535)
F_COUT = 4


def _build_f(dev):
    N, Ci, H, W = F_SHAPE
    assert N * H * W == 16711425 < LIMIT
    xo.check_wide()
    g = xo.dev_gen(61, dev)
    x = torch.randint(-xo.WIDE_MAX, xo.WIDE_MAX + 1, (N, H, W, Ci), generator=g, device=dev, dtype=torch.int16)
    return {"x": _nhwc(x.float()), "xs": _nhwc(xo.dev_sparse_signs((N, H, W, Ci), g, 32, F32))}


@pytest.mark.parametrize("k", [3, 1])
def test_f_conv_f32_fwd(cuda, C, k):
    """Wide-mantissa operands (11-bit x, <= 3 nonzeros of up to 2^11 per output channel)."""
    x = _case("F", lambda: _build_f(cuda), cuda)["x"]
    N, Ci, H, W = F_SHAPE
    pad = k // 2
    w = xo.sparse_signs(F_COUT, k * k * Ci, xo.gen(15 + k), xo.WIDE_NNZ, xo.WIDE_MAX)
    w = w.view(F_COUT, k, k, Ci).permute(0, 3, 1, 2).contiguous()  # [Cout, C, k, k]
    wd = w.permute(0, 2, 3, 1).contiguous().to(cuda)  # OHWI
    _poison(cuda, N * H * W, F_COUT, dtype=F32)
    y = C.conv_f32_fwd(x, wd, pad, 1)
    assert y.shape == (N, F_COUT, H, W) and y.is_contiguous(memory_format=CL)
    for n, r0, nr in _edge_slices(N, H):
        lo, hi = max(0, r0 - pad), min(H, r0 + nr + pad)
        ref = xo.conv_ref(x[:, :, lo:hi, :], w, 1, pad)[:, :, r0 - lo:r0 - lo + nr, :]
        xo.assert_exact(y[:, :, r0:r0 + nr, :], ref, (128, 128), f"conv_f32_fwd F {k}x{k} rows [{r0}, {r0 + nr})")
    covered = torch.zeros(H, dtype=torch.bool)
    for b, e, lo, hi in _bands(H, BAND, pad):
        yb = C.conv_f32_fwd(x[:, :, lo:hi, :].clone(memory_format=CL), wd, pad, 1)
        xo.assert_exact_block(y[:, :, b:e, :], yb[:, :, b - lo:e - lo, :], f"conv_f32_fwd F {k}x{k} rows [{b}, {e})",
                              b * W, H * W)
        covered[b:e] = True
    assert int((~covered).sum()) == 0, "output rows no reference covers"


@pytest.mark.parametrize("k", [3, 1])
def test_f_conv_f32_wgrad(cuda, C, k):
    xs = _case("F", lambda: _build_f(cuda), cuda)["xs"]
    N, Ci, H, W = F_SHAPE
    pad = k // 2
    dy = _nhwc(xo.dev_ints((N, H, W, F_COUT), xo.dev_gen(62 + k, cuda), -2, 2, F32))
    xo.check_exact_sum(2 * int(xo.nonzeros_per_column(xs).max()), "conv_f32_wgrad F: 2 * nonzeros of one input channel")
    _poison(cuda, F_COUT, k * k * Ci, dtype=F32)
    dw = C.conv_f32_wgrad(dy, xs, k, k, pad, 1)  # [Cout, R, S, C]
    xo.assert_exact(dw.permute(0, 3, 1, 2), xo.conv_wgrad_ref_dev(dy, xs, k, 1, pad), None, f"conv_f32_wgrad F {k}x{k}")
    total = torch.zeros(F_COUT, k, k, Ci, dtype=F64, device=cuda)
    for b, e, lo, hi in _bands(H, BAND, pad):
        dyb = dy[:, :, lo:hi, :].clone(memory_format=CL)
        dyb[:, :, :b - lo, :] = 0
        dyb[:, :, e - lo:, :] = 0
        total += C.conv_f32_wgrad(dyb, xs[:, :, lo:hi, :].clone(memory_format=CL), k, k, pad, 1).double()
    xo.assert_exact(dw, total, None, f"conv_f32_wgrad F {k}x{k} against the sum over row bands")


# ======================================================================================== refusal side
def _e(dev, *shape, dtype=BF):
    """An uninitialised channels_last operand: refused on the host, never read."""
    return torch.empty(shape[0], shape[2], shape[3], shape[1], dtype=dtype, device=dev).permute(0, 3, 1, 2)


# one step past each limit: 2^24 pixels exactly ([2, 8, 2048, 4096]), a divisor of 65536, the counterexample the
# bindings accepted before (W = 66011)
PAST_PIXELS = (2, 8, 2048, 4096)
PAST_DIVISOR = [(1, 8, 1, 65536), (1, 8, 65536, 1), (1, 8, 254, 66011)]


def test_refused_one_step_past_the_limits_conv3x3(cuda, C):
    _release()
    assert PAST_PIXELS[0] * PAST_PIXELS[2] * PAST_PIXELS[3] == LIMIT
    w8 = torch.empty(8, 8, 3, 3, dtype=BF, device=cuda).contiguous(memory_format=CL)
    w64 = torch.empty(64, 64, 3, 3, dtype=BF, device=cuda).contiguous(memory_format=CL)
    ws, part_mode = torch.zeros(7 * 8, device=cuda), 1
    for shape, msg in [(PAST_PIXELS, "too many pixels")] + [(s, "below 65536") for s in PAST_DIVISOR]:
        t = _e(cuda, *shape)
        with pytest.raises(RuntimeError, match=f"conv3x3: .*{msg}"):
            C.conv3x3_fwd(t, w8, 1, True)
        with pytest.raises(RuntimeError, match=f"conv3x3: .*{msg}"):
            C.conv3x3_dgrad(t, w8)
        with pytest.raises(RuntimeError, match=f"conv3x3: .*{msg}"):
            C.conv3x3_dgrad_bn(t, w8, None, t, ws, None, part_mode)
        with pytest.raises(RuntimeError, match=f"conv3x3_wgrad: .*({msg}|too many pixels)"):
            C.conv3x3_wgrad(t, t, 1, F32)
    # the stride-2 data gradient: dx is the checked operand
    for (n, c, h, w_), msg in [((2, 64, 2048, 4096), "too many pixels"), ((1, 64, 2, 65536), "below 65536"),
                               ((1, 64, 65536, 2), "below 65536")]:
        with pytest.raises(RuntimeError, match=f"conv3x3: .*{msg}"):
            C.conv3x3s2_dgrad(_e(cuda, n, 64, h // 2, w_ // 2), w64, h, w_)
    # a span of exactly 2^31 bytes with 2^20 pixels
    x = _e(cuda, 1, 1024, 1024, 1024)
    assert x.numel() * 2 == SPAN
    with pytest.raises(RuntimeError, match="conv3x3 input: 2147483648 bytes reach the 2 GiB"):
        C.conv3x3_fwd(x, torch.empty(8, 1024, 3, 3, dtype=BF, device=cuda).contiguous(memory_format=CL), 1, False)
    # conv3x3_wgrad checks its operands itself (it does not go through check_conv3): x, then dy, of 2^31 bytes
    small = _e(cuda, 1, 8, 1024, 1024)
    with pytest.raises(RuntimeError, match="conv3x3_wgrad x: 2147483648 bytes reach the 2 GiB"):
        C.conv3x3_wgrad(small, x, 1, F32)
    with pytest.raises(RuntimeError, match="conv3x3_wgrad dy: 2147483648 bytes reach the 2 GiB"):
        C.conv3x3_wgrad(x, small, 1, F32)
    del x
    torch.cuda.synchronize()


def _stem_bn_args(dev, h, w):
    """stem_wgrad_bn operands of an [1, 3, h, w] image (folded to even BH, BW), uninitialised apart from ws."""
    bh, bw = (h + 1) // 2, (w + 1) // 2
    dyp = _e(dev, 1, 64, bh // 2, bw // 2)
    pos = torch.empty(1, bh // 2, bw // 2, 64, dtype=torch.uint8, device=dev).permute(0, 3, 1, 2)
    xs = torch.empty(1, bh, bw, 16, dtype=BF, device=dev)
    return dyp, pos, _e(dev, 1, 64, bh, bw), torch.zeros(7 * 64, device=dev), xs, h, w, F32


def test_refused_one_step_past_the_limits_stem_and_fp32(cuda, C):
    wpk = torch.empty(64, 256, dtype=BF, device=cuda)
    # the output's span: 2^23 output pixels of 128 channels are 2^31 bytes
    with pytest.raises(RuntimeError, match="stem_fwd: the output reaches the 2 GiB"):
        C.stem_fwd(_e(cuda, 1, 3, 4096, 8192), torch.empty(128, 256, dtype=BF, device=cuda), True)
    for h, w_ in [(131072, 4), (4, 131072), (508, 132024)]:  # folded 65536 x 2, 2 x 65536, 254 x 66012
        with pytest.raises(RuntimeError, match="stem_wgrad_bn: the folded BH, BW must be below 65536"):
            C.stem_wgrad_bn(*_stem_bn_args(cuda, h, w_))
    # at 2^24 output pixels a dy of 64 channels spans 2^31 bytes: stem_wgrad's span check speaks before its pixel check
    for shape, msg in [((1, 3, 8192, 8192), "too many output pixels|2 GiB"), ((1, 3, 2, 131072), "BH, BW must be below 65536"),
                       ((1, 3, 131071, 2), "BH, BW must be below 65536"), ((1, 3, 508, 132022), "BH, BW must be below")]:
        n, _, h, w_ = shape
        with pytest.raises(RuntimeError, match=f"stem_fwd: .*({msg})"):
            C.stem_fwd(_e(cuda, *shape), wpk, True)
        oh, ow = (h + 1) // 2, (w_ + 1) // 2
        xs = torch.empty(n, oh, ow, 16, dtype=BF, device=cuda)
        with pytest.raises(RuntimeError, match=f"(stem_wgrad|dy): .*({msg})"):
            C.stem_wgrad(_e(cuda, n, 64, oh, ow), xs, h, w_, F32)
        del xs
    w3 = torch.empty(4, 3, 3, 4, device=cuda)
    for shape, msg in [((2, 4, 2048, 4096), "fewer than 2\\^24|M < 2\\^24"), ((1, 4, 1, 65536), "below 65536"),
                       ((1, 4, 65536, 1), "below 65536"), ((1, 4, 254, 66011), "below 65536")]:
        t = _e(cuda, *shape, dtype=F32)
        with pytest.raises(RuntimeError, match=f"conv_f32_fwd: .*({msg})"):
            C.conv_f32_fwd(t, w3, 1, 1)
        with pytest.raises(RuntimeError, match=f"conv_f32_wgrad: .*({msg})"):
            C.conv_f32_wgrad(t, t, 3, 3, 1, 1)
    # the channel count as a divisor: K = C < 2^24 passes conv_f32_supported
    t = _e(cuda, 1, 65536, 2, 2, dtype=F32)
    with pytest.raises(RuntimeError, match="conv_f32_fwd: .*below 65536"):
        C.conv_f32_fwd(t, torch.empty(4, 1, 1, 65536, device=cuda), 0, 1)
    torch.cuda.synchronize()


def test_refused_one_step_past_the_limits_gemm(cuda, C):
    """gemm_nt / gemm_tn operands of exactly 2^31 bytes (check_mat's span check); the stride-2 addend's rows and
    divisors are test_gpu_binding_checks.py::test_addend2_refuses_rows_outside_the_fast_division."""
    A = torch.empty(LIMIT, 64, dtype=BF, device=cuda)
    assert A.numel() * 2 == SPAN
    W = torch.empty(8, 64, dtype=BF, device=cuda)
    with pytest.raises(RuntimeError, match="2 GiB"):
        C.gemm_nt(A, W)
    with pytest.raises(RuntimeError, match="2 GiB"):
        C.gemm_tn(torch.empty(LIMIT, 8, dtype=BF, device=cuda), A, F32, 1.0)
    del A
    torch.cuda.synchronize()
