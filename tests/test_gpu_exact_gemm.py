"""Exact integer-data oracle tests of the bf16 GEMM kernels (gemm.hip, gemm_stream.hip, gemm_direct.hip,
gemm_dual.hip, gemm_apply.hip and the BatchNorm-backward epilogue) against float64 (gpu).

The operands come from tests/exact_oracle.py: integer-valued, with the worst-case sum of |a b| under 2^24 (2^22 in
the dense regime), so fp32 accumulation is exact in any order and every output element has one correct value. All
comparisons are ``assert_exact`` (``torch.equal`` by value): no tolerance and no excluded share. Outputs are
compared after one round-to-nearest-even to bf16 (two where a kernel documents two: the tile kernels' addend is
bf16(bf16(acc) + D); the split-K reduce adds its bias row in fp32 before its one rounding), dense cases must
contain exact rounding ties, and in the no-rounding regime the per-partial BatchNorm statistics must sum to the
exact column sums of y and y^2. Every output block is NaN-poisoned first; process-global setters go back to
their defaults in the fixture teardown."""
import functools

import pytest
import torch

import exact_oracle as xo

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
TILE_RC = {0: (128, 128), 1: (128, 128), 2: (128, 64), 3: (64, 64), 8: (256, 256)}
REGIMES = ["dense", "norounding"]


@pytest.fixture
def C():
    from distributed_learning_amd.ops import _ext

    C = _ext.require()
    yield C
    C.set_mfma_pipeline(-1)
    C.set_gemm_stream(-1)
    C.set_gemm_direct(-1)
    C.set_gemm_persist(-1)
    C.set_gemm256_direct(-1)
    C.set_tile256_min_k_stats(-1)
    C.set_tn256(-1)
    C.set_gemm_apply_max_k(-1)


def _poison(dev, *shape, dtype=BF):
    """The caching allocator hands this block to the next output of the same size: a skipped store leaves NaN."""
    t = torch.full(shape, float("nan"), device=dev, dtype=dtype)
    del t


@functools.lru_cache(maxsize=6)
def _gemm_case(regime, M, N, K):
    """Operands on the device and the float64 reference, computed once per shape and never modified."""
    dev = torch.device("cuda:0")
    a, w = xo.gemm_operands(regime, M, N, K, seed=M + 3 * N + 7 * K)
    A, W = a.to(dev, BF), w.to(dev, BF)
    ref = xo.gemm_ref(A, W)  # float64 on the device: exact on these inputs
    if regime == "dense" and K >= xo.TIE_MIN_K:  # K = 8 cannot round at all: |y| <= 72
        assert xo.count_ties(ref) > 0, "dense inputs without rounding ties"
    if regime == "norounding":
        assert float(ref.abs().max()) <= 16
    return A, W, W.t().contiguous(), ref


def _check_stats(st, ref, what):
    """Per-partial statistics [rows, C, 2] summed over the partial rows == exact column sums of y and y^2."""
    xo.assert_exact(st.double().sum(0), xo.col_stats(ref), None, what + " statistics")


# ------------------------------------------------------------------------------------------- tile kernels
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("tile", [0, 1, 2, 3, 8])
@pytest.mark.parametrize("shape", [(130, 8, 8), (777, 136, 72), (1000, 64, 256), (1300, 520, 640)])
def test_gemm_nt_tiles(cuda, C, regime, tile, shape):
    """Forced tiles and the auto pick; ragged M, ragged N, K no multiple of the k-step, a 256x256 tile partly
    outside in both directions; statistics on and off, both weight layouts."""
    M, N, K = shape
    A, W, Wk, ref = _gemm_case(regime, M, N, K)
    exp = xo.round_bf16(ref)
    for kmajor in (False, True):
        for stats in (True, False):
            _poison(cuda, M, N)
            y, st = C.gemm_nt(A, Wk if kmajor else W, stats, None, kmajor, tile)
            what = f"gemm_nt tile {tile} kmajor {kmajor} stats {stats}"
            xo.assert_exact(y, exp, TILE_RC[tile], what)
            if stats and regime == "norounding":
                _check_stats(st, ref, what)


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 8])
@pytest.mark.parametrize("shape", [(130, 8, 8), (777, 136, 72), (1000, 64, 256), (1300, 520, 640)])
def test_gemm_nt_row_addend(cuda, C, tile, shape):
    """Row addend D (integers in [-64, 64]) with and without the 1-bit mask: two roundings,
    bf16(bf16(acc) + (bit ? D : 0)), in the tile kernels and in the register-stored ones alike."""
    M, N, K = shape
    A, W, Wk, ref = _gemm_case("dense", M, N, K)
    g = xo.gen(M + N)
    D = xo.addend((M, N), g)
    mask = xo.mask_bytes(M * N, g)
    Dd, maskd = D.to(cuda, BF), mask.to(cuda)
    bits = xo.mask_bits(mask, M * N)
    for kmajor in (False, True):
        _poison(cuda, M, N)
        y, _ = C.gemm_nt(A, Wk if kmajor else W, False, Dd, kmajor, tile)
        xo.assert_exact(y, xo.add_rounded(ref, D), TILE_RC[tile], f"gemm_nt + D tile {tile} kmajor {kmajor}")
    _poison(cuda, M, N)
    y, _ = C.gemm_nt(A, Wk, False, Dd, True, tile, maskd)
    xo.assert_exact(y, xo.add_rounded(ref, D, bits), TILE_RC[tile], f"gemm_nt + masked D tile {tile}")


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("pipe", [0, 2, 3, 4, 5, 6])
def test_gemm_nt_main_loops(cuda, C, regime, pipe):
    M, N, K = 1000, 136, 200
    A, W, Wk, ref = _gemm_case(regime, M, N, K)
    exp = xo.round_bf16(ref)
    C.set_mfma_pipeline(pipe)
    _poison(cuda, M, N)
    y, st = C.gemm_nt(A, W, True)
    xo.assert_exact(y, exp, (128, 128), f"gemm_nt pipeline {pipe}")
    if regime == "norounding":
        _check_stats(st, ref, f"gemm_nt pipeline {pipe}")
    _poison(cuda, M, N)
    yk, _ = C.gemm_nt(A, Wk, False, None, True)
    xo.assert_exact(yk, exp, (128, 128), f"gemm_nt k-major pipeline {pipe}")


# ------------------------------------------------------------------------------------------ split-K heads
@pytest.mark.parametrize("M,N,K,kmajor,bias", [(8, 64, 4096, False, True), (300, 136, 1000, True, False),
                                              (128, 1024, 2048, False, True)])
def test_gemm_nt_splitk_heads(cuda, C, M, N, K, kmajor, bias):
    """fp32 slabs summed in a fixed order; the bias row is added in fp32 before the one rounding
    (gemm.hip splitk_reduce_sg_kernel: from_f32(s + addend)), unlike the tile kernels' two."""
    assert C.gemm_nt_splitk_splits(M, N, K) > 1
    A, W, Wk, ref = _gemm_case("dense", M, N, K)
    D = None
    exp = xo.round_bf16(ref)
    if bias:
        b = xo.addend((N,), xo.gen(N))
        D = b.to(cuda, BF).expand(M, N)
        exp = xo.round_bf16(ref + b.double().to(cuda))
    _poison(cuda, M, N)
    y, _ = C.gemm_nt(A, Wk if kmajor else W, False, D, kmajor)
    xo.assert_exact(y, exp, (128, 128), "split-K gemm_nt")


# ------------------------------------------------------------------------------------------------ gemm_tn
@pytest.mark.parametrize("tn256", [0, 1])
@pytest.mark.parametrize("K,Mo,No", [(333, 136, 72), (3333, 512, 256), (16384, 8, 8), (8192, 24, 40)])
def test_gemm_tn(cuda, C, tn256, K, Mo, No):
    """Weight-gradient form A^T B (split-K over rows): fp32 output with scale 0.5 (exact: a power of two),
    bf16 output with scale 1 (one rounding of the summed slabs)."""
    At, Bt, _, ref = _gemm_case("dense", Mo, No, K)  # [Mo, K], [No, K]: reference At Bt^T
    A, B = At.t().contiguous(), Bt.t().contiguous()
    C.set_tn256(tn256)
    _poison(cuda, Mo, No, dtype=torch.float32)
    out = C.gemm_tn(A, B, torch.float32, 0.5)
    xo.assert_exact(out, ref * 0.5, (128, 128), "gemm_tn fp32")
    _poison(cuda, Mo, No)
    outb = C.gemm_tn(A, B, BF, 1.0)
    xo.assert_exact(outb, xo.round_bf16(ref), (128, 128), "gemm_tn bf16")


# -------------------------------------------------------------------------------------- streaming kernel
STREAM = [(9000, 64, 64), (9000, 64, 256), (5001, 256, 128), (20000, 128, 512), (33333, 128, 128)]  # (M, K, N)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("kmajor", [False, True])
@pytest.mark.parametrize("shape", STREAM)
def test_stream(cuda, C, regime, kmajor, shape):
    M, K, N = shape
    A, W, Wk, ref = _gemm_case(regime, M, N, K)
    C.set_gemm_stream(1)
    rows = C.gemm_stream_rows(M, N, K, K, N, kmajor)
    assert rows > 0, "shape not served by the streaming kernel"
    exp = xo.round_bf16(ref)
    _poison(cuda, M, N)
    y, st = C.gemm_nt(A, Wk if kmajor else W, True, None, kmajor)
    xo.assert_exact(y, exp, (128, 128), "streaming gemm_nt with statistics")
    assert st.shape == (rows, N, 2)
    if regime == "norounding":
        _check_stats(st, ref, "streaming gemm_nt")
    _poison(cuda, M, N)
    y, st = C.gemm_nt(A, Wk if kmajor else W, False, None, kmajor)
    assert st is None or st.numel() == 0
    xo.assert_exact(y, exp, (128, 128), "streaming gemm_nt without statistics")


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shape", [s for s in STREAM if s[1] <= 128])
def test_stream_dgrad_addend(cuda, C, shape, masked):
    """The data-gradient form with the identity-gradient addend (served for K <= 128)."""
    M, K, N = shape
    A, W, Wk, ref = _gemm_case("dense", M, N, K)
    g = xo.gen(M + K)
    D = xo.addend((M, N), g)
    mask = xo.mask_bytes(M * N, g) if masked else None
    C.set_gemm_stream(1)
    assert C.gemm_stream_rows(M, N, K, K, N, True, True) > 0, "shape not served by the streaming kernel"
    _poison(cuda, M, N)
    y, _ = C.gemm_nt(A, Wk, False, D.to(cuda, BF), True, 0, mask.to(cuda) if masked else None)
    bits = xo.mask_bits(mask, M * N) if masked else None
    xo.assert_exact(y, xo.add_rounded(ref, D, bits), (128, 128), "streaming dgrad + addend")


@pytest.mark.parametrize("regime", REGIMES)
def test_stream_row_strided_input(cuda, C, regime):
    """A is a channel slice of a wider tensor (lda > K)."""
    M, K, N = 12345, 64, 128
    a, w = xo.gemm_operands(regime, M, N, K, 7)
    wide = xo.ints((M, 3 * K), xo.gen(8), -3, 3)
    wide[:, K:2 * K] = a
    A = wide.to(cuda, BF)[:, K:2 * K]
    W = w.to(cuda, BF)
    ref = xo.gemm_ref(a.to(cuda), W)
    if regime == "dense":
        assert xo.count_ties(ref) > 0, "dense inputs without rounding ties"
    C.set_gemm_stream(1)
    assert C.gemm_stream_rows(M, N, K, A.stride(0), N) > 0, "shape not served by the streaming kernel"
    _poison(cuda, M, N)
    y, st = C.gemm_nt(A, W, True)
    xo.assert_exact(y, xo.round_bf16(ref), (128, 128), "streaming gemm_nt, row-strided A")
    if regime == "norounding":
        _check_stats(st, ref, "streaming gemm_nt, row-strided A")


# ---------------------------------------------------------------------------------- register-stored tiles
DIRECT = [(3000, 64, 256), (5001, 512, 128), (12345, 128, 320), (9000, 1024, 384)]  # (M, K, N)


@pytest.fixture
def direct(C):
    """test_gpu_gemm_direct.py's settings: streaming off, statistics forwards held on the 128x128 tiles."""
    C.set_gemm_stream(0)
    C.set_tile256_min_k_stats(1 << 30)
    C.set_gemm_direct(1)
    return C


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("pipe", [-1, 6])
@pytest.mark.parametrize("shape", DIRECT)
def test_direct_tiles(cuda, direct, regime, pipe, shape):
    C = direct
    M, K, N = shape
    A, W, Wk, ref = _gemm_case(regime, M, N, K)
    exp = xo.round_bf16(ref)
    C.set_mfma_pipeline(pipe)
    for kmajor in (False, True):
        _poison(cuda, M, N)
        y, st = C.gemm_nt(A, Wk if kmajor else W, True, None, kmajor)
        what = f"direct gemm_nt pipe {pipe} kmajor {kmajor}"
        xo.assert_exact(y, exp, (128, 128), what)
        assert st.shape == ((M + 127) // 128, N, 2)
        if regime == "norounding":
            _check_stats(st, ref, what)
    _poison(cuda, M, N)
    y, _ = C.gemm_nt(A, W, False)
    xo.assert_exact(y, exp, (128, 128), f"direct gemm_nt pipe {pipe} without statistics")
    if regime == "dense":
        g = xo.gen(M + K)
        D = xo.addend((M, N), g)
        mask = xo.mask_bytes(M * N, g)
        for m in (None, mask):
            _poison(cuda, M, N)
            y, _ = C.gemm_nt(A, Wk, False, D.to(cuda, BF), True, 0, None if m is None else m.to(cuda))
            bits = None if m is None else xo.mask_bits(m, M * N)
            xo.assert_exact(y, xo.add_rounded(ref, D, bits), (128, 128), f"direct dgrad + addend pipe {pipe}")


@pytest.mark.parametrize("regime", REGIMES)
def test_direct_persistent(cuda, direct, regime):
    """The persistent form (one block per CU walking 97 x 3 = 291 tiles, the last row and column tiles ragged)."""
    C = direct
    M, K, N = 12345, 128, 320
    A, W, Wk, ref = _gemm_case(regime, M, N, K)
    C.set_gemm_persist(1)
    _poison(cuda, M, N)
    y, st = C.gemm_nt(A, W, True)
    xo.assert_exact(y, xo.round_bf16(ref), (128, 128), "persistent direct gemm_nt")
    if regime == "norounding":
        _check_stats(st, ref, "persistent direct gemm_nt")
    _poison(cuda, M, N)
    y, _ = C.gemm_nt(A, Wk, False, None, True)
    xo.assert_exact(y, xo.round_bf16(ref), (128, 128), "persistent direct gemm_nt k-major")


@pytest.mark.parametrize("regime", REGIMES)
def test_direct_256(cuda, C, regime):
    """256x256 statistics forward stored from the registers, 5001 rows (the last row tile holds 137)."""
    M, K, N = 5001, 256, 512
    A, W, _, ref = _gemm_case(regime, M, N, K)
    C.set_gemm256_direct(1)
    _poison(cuda, M, N)
    y, st = C.gemm_nt(A, W, True, None, False, 8)
    xo.assert_exact(y, xo.round_bf16(ref), (256, 256), "256x256 direct gemm_nt")
    assert st.shape == ((M + 255) // 256, N, 2)
    if regime == "norounding":
        _check_stats(st, ref, "256x256 direct gemm_nt")


# ------------------------------------------------------------------------------------------ conv1x1_dual
@pytest.mark.parametrize("odt", [torch.float32, BF])
@pytest.mark.parametrize("M,ci,co", [(65536, 64, 256), (70001, 64, 256), (16384, 128, 512), (40003, 256, 512)])
def test_conv1x1_dual(cuda, C, M, ci, co, odt):
    """One-pass data + weight gradient (plain form): dx = dy w (reduction Cout), dw = dy^T x (reduction M)."""
    assert C.conv1x1_dual_blocks(M, ci, co) > 0, "shape not served by the one-pass kernel"
    xo.check_dense(M)
    dy, wt, w, dx_ref = _gemm_case("dense", M, ci, co)  # dy [M, co], wt [ci, co], w = wt^T [co, ci]
    x = xo.ints((M, ci), xo.gen(M + ci), -3, 3).to(cuda, BF)
    dw_ref = xo.integral(dy.double().t() @ x.double())
    _poison(cuda, M, ci)
    dx, dw = C.conv1x1_dual(dy, x, w, odt)
    assert dw.dtype == odt and dw.shape == (co, ci)
    xo.assert_exact(dx, xo.round_bf16(dx_ref), (128, 64), "conv1x1_dual dx")
    if odt == BF:
        assert xo.count_ties(dw_ref) > 0
    xo.assert_exact(dw, dw_ref if odt == torch.float32 else xo.round_bf16(dw_ref), (128, 64), "conv1x1_dual dw")


# ------------------------------------------------------------------------- deferred BN apply in the GEMM
MASK_FILL = 0xFF  # the mask buffer before the kernel: all 8 pre-activations of a byte positive is rare (checked)
APPLY_NNZ = 2  # no-rounding weights here: out <= 22, so |C| <= 44 and M * 44^2 < 2^24 up to M = 8664


def _ws(K, g, dev):
    """A 7K workspace with integer coefficients: scale in {-2, -1, 1, 2}, shift in [-4, 4]."""
    ws = torch.zeros(7 * K)
    sc = torch.tensor([-2., -1., 1., 2.])[torch.randint(0, 4, (K,), generator=g)]
    sh = xo.ints((K,), g, -4, 4)
    ws[2 * K:3 * K], ws[3 * K:4 * K] = sc, sh
    return ws.to(dev), sc.double(), sh.double()


def _apply_case(regime, M, K, N, dual, seed, dev):
    g = xo.gen(seed)
    y, r = xo.ints((M, K), g, -3, 3), xo.ints((M, K), g, -4, 4)
    ws, sc, sh = _ws(K, g, dev)
    pre = y.double() * sc + sh
    wsd = None
    if dual:
        wsd, scd, shd = _ws(K, g, dev)
        pre = pre + r.double() * scd + shd
    else:
        pre = pre + r.double()
    out = pre.clamp_min(0)
    omax = int(out.max())
    assert omax <= 22 and torch.equal(out.to(BF).double(), out)
    if regime == "dense":
        xo.check_dense(K, 22, 3)
        w = xo.ints((N, K), g, -3, 3)
        w[N - 1] = xo.tie_partner(out[M - 1])  # C[M-1, N-1]: a planted tie that rounds up
    else:
        assert M * (APPLY_NNZ * 22) ** 2 < xo.EXACT_LIMIT
        w = xo.sparse_signs(N, K, g, APPLY_NNZ)
    c_ref = xo.integral(out.to(dev) @ w.double().to(dev).t())
    if regime == "dense":
        assert xo.count_ties(c_ref) > 0, "dense inputs without rounding ties"
    return y.to(dev, BF), r.to(dev, BF), ws, wsd, w.to(dev, BF), pre, out, c_ref


def _mask_ref(pre):
    """The ReLU mask bytes of the pre-activation: element i is bit i % 8 of byte i // 8."""
    b = (pre.reshape(-1) > 0).to(torch.int64)
    b = torch.cat([b, b.new_zeros((-b.numel()) % 8)]).view(-1, 8)
    return (b << torch.arange(8)).sum(1).to(torch.uint8)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("shape", [(777, 256, 64), (3000, 256, 64), (5001, 512, 128)])
def test_gemm_nt_apply(cuda, C, regime, dual, shape):
    """relu(BN(y) + r) (identity) / relu(BN(y) + BN_d(r)) (dual) with integer coefficients: the written block
    output, every mask bit, C and the statistics are exact (no fma-versus-mul+add allowance needed)."""
    M, K, N = shape
    assert C.gemm_nt_apply_ok(M, N, K), "shape not served"
    y, r, ws, wsd, w, pre, out_ref, c_ref = _apply_case(regime, M, K, N, dual, M + K + dual, cuda)
    out = torch.full((M, K), float("nan"), device=cuda, dtype=BF)
    mask = torch.full(((M * K + 7) // 8,), MASK_FILL, device=cuda, dtype=torch.uint8)
    assert int((_mask_ref(pre) == MASK_FILL).sum()) < mask.numel() // 50  # a skipped byte store shows
    _poison(cuda, M, N)
    c, st = C.gemm_nt_apply(y, r, ws, wsd, w, True, out, mask)
    xo.assert_exact(out, out_ref, (128, 128), "gemm_nt_apply block output")
    xo.assert_exact(mask, _mask_ref(pre), None, "gemm_nt_apply mask bytes")
    xo.assert_exact(c, xo.round_bf16(c_ref), (128, 64 if N <= 64 else 128), "gemm_nt_apply C")
    if regime == "norounding":
        _check_stats(st, c_ref, "gemm_nt_apply")


def test_gemm_nt_apply_stride2_subsample(cuda, C):
    n, H, W, K, N = 3, 14, 10, 256, 128
    M = n * H * W
    y, r, ws, wsd, w, pre, out_ref, c_ref = _apply_case("norounding", M, K, N, False, 3, cuda)
    out = torch.full((M, K), float("nan"), device=cuda, dtype=BF)
    mask = torch.full(((M * K + 7) // 8,), MASK_FILL, device=cuda, dtype=torch.uint8)
    xs = torch.full((n, K, H // 2, W // 2), float("nan"), device=cuda, dtype=BF).contiguous(
        memory_format=torch.channels_last)
    _poison(cuda, M, N)
    c, st = C.gemm_nt_apply(y, r, ws, wsd, w, True, out, mask, xs, H, W)
    xo.assert_exact(out, out_ref, (128, 128), "gemm_nt_apply block output")
    xo.assert_exact(xs, out_ref.view(n, H, W, K)[:, ::2, ::2].permute(0, 3, 1, 2), None, "gemm_nt_apply subsample")
    xo.assert_exact(mask, _mask_ref(pre), None, "gemm_nt_apply mask bytes")
    xo.assert_exact(c, xo.round_bf16(c_ref), (128, 128), "gemm_nt_apply C")
    _check_stats(st, c_ref, "gemm_nt_apply")


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("M,K,N", [(8000, 64, 256), (8001, 128, 512), (5003, 128, 128)])
def test_gemm_nt_stream_apply(cuda, C, regime, M, K, N):
    """The streaming kernel with relu(BN(y)) on its operand. (The tile-kernel shapes above are not streamed; these
    are the nearest ones that are, short enough for the statistics bound: 8001 rows * (2 * 10)^2 < 2^24. 5003 rows
    are 40 row tiles, the last of 11 rows, over 16 row groups of 2 or 3 tiles.)"""
    assert C.gemm_nt_stream_apply_ok(M, N, K), "shape not served by the streaming kernel"
    g = xo.gen(M + K)
    y = xo.ints((M, K), g, -3, 3)
    ws, sc, sh = _ws(K, g, cuda)
    out_ref = (y.double() * sc + sh).clamp_min(0)
    assert int(out_ref.max()) <= 10
    if regime == "dense":
        xo.check_dense(K, 10, 3)
        w = xo.ints((N, K), g, -3, 3)
        w[N - 1] = xo.tie_partner(out_ref[M - 1])  # C[M-1, N-1]: a planted tie that rounds up
    else:
        assert M * (APPLY_NNZ * 10) ** 2 < xo.EXACT_LIMIT
        w = xo.sparse_signs(N, K, g, APPLY_NNZ)
    c_ref = xo.integral(out_ref.to(cuda) @ w.double().to(cuda).t())
    if regime == "dense":
        assert xo.count_ties(c_ref) > 0, "dense inputs without rounding ties"
    out = torch.full((M, K), float("nan"), device=cuda, dtype=BF)
    _poison(cuda, M, N)
    c, st = C.gemm_nt_stream_apply(y.to(cuda, BF), ws, w.to(cuda, BF), out)
    xo.assert_exact(out, out_ref, (128, 128), "gemm_nt_stream_apply operand")
    xo.assert_exact(c, xo.round_bf16(c_ref), (128, 128), "gemm_nt_stream_apply C")
    if regime == "norounding":
        _check_stats(st, c_ref, "gemm_nt_stream_apply")


# ----------------------------------------------------------------------- BatchNorm-backward epilogue
def _bn_partials_ref(dy, x, mean, sc, sh, bits, mode):
    """Exact sums of dy' and dy' (x - mean) per channel: dy' = dy (mode 0), dy where scale x + shift > 0 (mode 1),
    dy where the mask bit is set (mode 2). dy, x: float64 [rows, C]."""
    g = dy
    if mode == 1:
        g = torch.where(x * sc + sh > 0, dy, torch.zeros_like(dy))
    elif mode == 2:
        g = dy * bits.view(dy.shape).double()
    return torch.stack([g.sum(0), (g * (x - mean)).sum(0)], 1)


def _bn_ws(N, g):
    ws = torch.zeros(7 * N)
    mean = xo.ints((N,), g, -2, 2)
    sc = torch.tensor([-2., -1., 1., 2.])[torch.randint(0, 4, (N,), generator=g)]
    sh = xo.ints((N,), g, -4, 4)
    ws[:N], ws[2 * N:3 * N], ws[3 * N:4 * N] = mean, sc, sh
    return ws, mean.double(), sc.double(), sh.double()


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_gemm_nt_bn(cuda, C, regime, mode):
    """dy = A W of a fused BN with integer mean, scale and shift in the workspace: dy exact in both regimes, the
    partials sum dy' and sum dy' (x - mean) exact in the no-rounding regime (|dy'| <= 16, |x - mean| <= 5)."""
    M, K, N = 3000, 256, 128
    A, W, Wk, ref = _gemm_case(regime, M, N, K)
    g = xo.gen(mode + 11)
    x = xo.ints((M, N), g, -3, 3)
    ws, mean, sc, sh = _bn_ws(N, g)
    mask = xo.mask_bytes(M * N, g)
    _poison(cuda, M, N)
    dy, part = C.gemm_nt_bn(A, Wk, None, True, x.to(cuda, BF), ws.to(cuda), mask.to(cuda), mode)
    xo.assert_exact(dy, xo.round_bf16(ref), (128, 128), f"gemm_nt_bn mode {mode} dy")
    if regime == "norounding":
        exp = _bn_partials_ref(ref.cpu(), x.double(), mean, sc, sh, xo.mask_bits(mask, M * N), mode)
        xo.assert_exact(part.double().sum(0), exp, None, f"gemm_nt_bn mode {mode} partials")


@pytest.mark.parametrize("regime", REGIMES)
def test_conv3x3_dgrad_bn(cuda, C, regime):
    """3x3 data gradient 128 -> 64 channels at 2 x 14 x 14 with the BN-backward reduction (mode 1) in its
    epilogue."""
    n, cout, cin, H, Wd = 2, 128, 64, 14, 14
    CL = torch.channels_last
    g = xo.gen(5)
    if regime == "dense":
        dy, w = xo.dense_conv_dgrad(n, cin, H, Wd, cout, 5)
    else:
        xo.check_norounding(n * H * Wd)
        dy = xo.ints((n, cout, H, Wd), g, -2, 2)  # <= 8 nonzeros of +-1 per input channel over (tap, Cout)
        w = xo.sparse_signs(cin, 9 * cout, g).view(cin, 3, 3, cout).permute(3, 0, 1, 2).contiguous()
    x = xo.ints((n, cin, H, Wd), g, -3, 3)
    ws, mean, sc, sh = _bn_ws(cin, g)
    ref = xo.conv_dgrad_ref(x.shape, w, dy)
    if regime == "dense":
        assert xo.count_ties(ref) > 0, "dense inputs without rounding ties"
    _poison(cuda, n * H * Wd, cin)
    dx, part = C.conv3x3_dgrad_bn(dy.to(cuda, BF).contiguous(memory_format=CL), w.to(cuda, BF).contiguous(memory_format=CL),
                                  None, x.to(cuda, BF).contiguous(memory_format=CL), ws.to(cuda), None, 1)
    xo.assert_exact(dx, xo.round_bf16(ref), (128, 64), "conv3x3_dgrad_bn dx")
    if regime == "norounding":
        assert float(ref.abs().max()) <= 16
        exp = _bn_partials_ref(xo.rows_view(ref), xo.rows_view(x.double()), mean, sc, sh, None, 1)
        xo.assert_exact(part.double().sum(0), exp, None, "conv3x3_dgrad_bn partials")
