"""Exact integer-data oracle tests of the fused backward hand-offs against float64 (gpu): the BN-apply form of the
one-pass 1x1 gradient kernel (gemm_dual.hip kBN), the stem weight gradient with the BN+ReLU+max-pool backward fused
(stem.hip stem_wgrad_bn_kernel), and the fork data-gradient epilogue with its stride-2 second addend, with and
without the BN-backward partials (dla_mfma.h epilogue_bf16 through gemm_nt / gemm_nt_bn).

Same rules as test_gpu_exact_gemm.py: operands from tests/exact_oracle.py and tests/handoff_oracle.py, every
comparison ``assert_exact`` against float64 (no tolerance, nothing excluded), output blocks NaN-poisoned first. The
BatchNorm-backward coefficients sit in the 7C workspace as integers, so dY = k1 (g - m1 - (y - mean) k2) is exact
in bf16 and the roundings left are the documented ones: one for dx and a bf16 weight gradient, three in the fork
epilogue, bf16(bf16(bf16(acc) + (bit ? D : 0)) + E at even pixels), in that order."""
import functools

import pytest
import torch

import exact_oracle as xo
import handoff_oracle as ho

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
CL = torch.channels_last
TILE_RC = {0: (128, 128), 1: (128, 128), 2: (128, 64), 3: (64, 64), 8: (256, 256)}
REGIMES = ["dense", "norounding"]


@pytest.fixture
def C():
    from distributed_learning_amd.ops import _ext

    return _ext.require()


def _poison(dev, *shape, dtype=BF):
    """The caching allocator hands this block to the next output of the same size: a skipped store leaves NaN."""
    t = torch.full(shape, float("nan"), device=dev, dtype=dtype)
    del t


# ---------------------------------------------------------------------------------- A. conv1x1_dual + BN apply
@functools.lru_cache(maxsize=1)
def _dual_case(M):
    """Operands on the device and the float64 references, computed once per M and never modified."""
    dev = torch.device("cuda:0")
    c = ho.dual_case(M, M)
    d = {k: c[k].to(dev, BF) for k in ("dout", "ybn", "x", "w")}
    d["mask"], d["ws"] = c["mask"].to(dev), c["ws"].to(dev)
    bits = xo.mask_bits(d["mask"], M * 256)  # on the device
    dY, dx, dw = ho.dual_ref(d["dout"], d["ybn"], bits, d["x"], d["w"], c["cf"])
    assert float(dY.abs().max()) <= ho.DUAL_DY_MAX
    assert xo.count_ties(dx) > 0 and float(xo.round_bf16(dx[M - 1, 63]).abs()) > float(dx[M - 1, 63].abs())
    assert xo.count_ties(dw) > 0
    return d, xo.round_bf16(dx), dw


@pytest.mark.parametrize("odt", [torch.float32, BF])
@pytest.mark.parametrize("M", [65473, 65536, 70001])
def test_conv1x1_dual_bn_apply(cuda, C, M, odt):
    """65473: the smallest M the gate serves, one row on the last 32-row tile; 65536: whole tiles; 70001: 17 rows on
    the last tile and row groups of 8 and 9 tiles. dx[M-1, 63] is a planted tie that rounds up."""
    ci, co = 64, 256
    assert C.conv1x1_dual_bn_ok(M, ci, co), "shape not served by the BN-apply form"
    assert not C.conv1x1_dual_bn_ok(65472, ci, co)
    xo.check_dense(co, ho.DUAL_DY_MAX, 3)
    assert M * ho.DUAL_DY_MAX * 3 < xo.EXACT_LIMIT
    d, dx_exp, dw_ref = _dual_case(M)
    mask0, ybn0 = d["mask"].clone(), d["ybn"].clone()
    _poison(cuda, M, ci)
    dx, dw = C.conv1x1_dual(d["dout"], d["x"], d["w"], odt, d["ybn"], d["ws"], d["mask"])
    assert dw.dtype == odt and dw.shape == (co, ci) and dx.shape == (M, ci)
    xo.assert_exact(dx, dx_exp, (32, 64), "conv1x1_dual + BN dx")
    xo.assert_exact(dw, dw_ref if odt == torch.float32 else xo.round_bf16(dw_ref), (128, 64), "conv1x1_dual + BN dw")
    xo.assert_exact(d["mask"], mask0, None, "mask buffer after the call")
    xo.assert_exact(d["ybn"], ybn0, None, "BN input after the call")


# ------------------------------------------------------------------------------------------ B. stem_wgrad_bn
# conv-output sizes (n, H, W), image (2H, 2W): 4 quads (under one 16-quad k-step), 189 quads (no multiple of 16),
# 768 quads (48 k-steps over 48 splits)
STEM = [(1, 4, 4), (3, 18, 14), (2, 32, 48)]


@functools.lru_cache(maxsize=4)
def _stem_case(n, H, W):
    from distributed_learning_amd.ops import _ext

    dev = torch.device("cuda:0")
    c = ho.stem_case(n, H, W, n + H + W)
    pos = c["pos"].long()
    assert set(pos.unique().tolist()) == set(range(9)), "not every tap occurs"
    assert int((pos[:, :, 0] // 3).min()) >= 1 and int((pos[:, :, :, 0] % 3).min()) >= 1  # the border windows
    dY = ho.stem_dy_ref(c["dyp"], c["pos"], c["y"], c["cf"])
    ref = ho.stem_wgrad_ref(c["img"], dY)  # float64 on the CPU
    img = c["img"].to(dev, BF).contiguous(memory_format=CL)
    xs = _ext.require().stem_fwd(img, torch.zeros(64, 256, device=dev, dtype=BF), False)[2]  # the fold
    d = dict(xs=xs, y=c["y"].to(dev, BF).contiguous(memory_format=CL), dyp=c["dyp"].to(dev, BF).contiguous(memory_format=CL),
             pos=c["pos"].to(dev).contiguous(memory_format=CL), ws=c["ws"].to(dev), dY=dY)
    return d, ref


def _check_packed(dwp, ref, what):
    xo.assert_exact(dwp, ref, (64, 64), what)
    pad = ho.stem_padding_lanes(dwp)
    xo.assert_exact(pad, torch.zeros(pad.shape, dtype=torch.float64), None, what + " fold padding")


@pytest.mark.parametrize("shape", STEM)
def test_stem_wgrad_bn(cuda, C, shape):
    """The fused kernel with integer coefficients in the workspace, fp32 and bf16 output, compared in the packed
    [64, 256] layout (the folded conv's 16th tap row and column included, see handoff_oracle.stem_wgrad_ref)."""
    n, H, W = shape
    d, ref = _stem_case(*shape)
    if shape == STEM[0]:
        assert C.stem_wgrad_bn_splits(n, 2 * H, 2 * W) == 1
    if shape == STEM[2]:
        assert C.stem_wgrad_bn_splits(n, 2 * H, 2 * W) >= 3
    ws0 = d["ws"].clone()
    _poison(cuda, 64, 256, dtype=torch.float32)
    got = C.stem_wgrad_bn(d["dyp"], d["pos"], d["y"], d["ws"], d["xs"], 2 * H, 2 * W, torch.float32)
    _check_packed(got, ref, "stem_wgrad_bn fp32")
    if float(ref.abs().max()) < 256:
        assert shape == STEM[0] and xo.count_ties(ref) == 0  # 16 pixels: nothing can round
    else:
        assert xo.count_ties(ref) > 0, "no rounding tie in the bf16 weight gradient"
    _poison(cuda, 64, 256)
    gotb = C.stem_wgrad_bn(d["dyp"], d["pos"], d["y"], d["ws"], d["xs"], 2 * H, 2 * W, BF)
    assert gotb.dtype == BF
    _check_packed(gotb, xo.round_bf16(ref), "stem_wgrad_bn bf16")
    xo.assert_exact(d["ws"], ws0, None, "workspace after the call")


@pytest.mark.parametrize("shape", STEM)
def test_stem_wgrad_from_the_same_dy(cuda, C, shape):
    """The unfused weight gradient on the reference's dY (exact in bf16): the same packed numbers."""
    n, H, W = shape
    d, ref = _stem_case(*shape)
    dY = d["dY"].to(cuda, BF).contiguous(memory_format=CL)
    _poison(cuda, 64, 256, dtype=torch.float32)
    _check_packed(C.stem_wgrad(dY, d["xs"], 2 * H, 2 * W, torch.float32), ref, "stem_wgrad fp32")
    _poison(cuda, 64, 256)
    _check_packed(C.stem_wgrad(dY, d["xs"], 2 * H, 2 * W, BF), xo.round_bf16(ref), "stem_wgrad bf16")


@pytest.mark.parametrize("shape", [(1, 4, 4), (2, 8, 16)])
def test_stem_unfused_pair_and_fused_on_finalized_coefficients(cuda, C, shape):
    """bn_relu_maxpool_bwd(want_dx=True) always finalizes its own coefficients, so the integers of the cases above do
    not survive it. At a power-of-two pixel count (16 and 256; 4 and 64 quads) the finalized coefficients are dyadic
    and the whole backward has one correct value (handoff_oracle.stem_finalized_ref): the unfused pair, and the
    fused kernel on the workspace that the reduce-only call finalized, must both give it, bit for bit."""
    n, H, W = shape
    c = ho.stem_case(n, H, W, n + H + W)
    r = ho.stem_finalized_ref(c)
    if n * H * W == 16:  # multiples of 1 / 16 below 16 fit bf16's 8 bits: this case cannot round
        assert float(r["dY"].abs().max()) < 16
    else:
        assert not torch.equal(r["dYb"], r["dY"]), "the finalized coefficients were expected to make dY round"
    y, dyp, pos, img = (c[k].to(cuda, torch.uint8 if k == "pos" else BF).contiguous(memory_format=CL)
                        for k in ("y", "dyp", "pos", "img"))
    xs = C.stem_fwd(img, torch.zeros(64, 256, device=cuda, dtype=BF), False)[2]
    gamma = c["cf"]["k1"].float().to(cuda)  # k1 = weight * invstd, invstd = 1
    ws_u, ws_f = c["ws"].to(cuda), c["ws"].to(cuda)
    dy_u, dg_u, db_u = C.bn_relu_maxpool_bwd(dyp, pos, y, ws_u, gamma, 3, 2, 1)
    none, dg_f, db_f = C.bn_relu_maxpool_bwd(dyp, pos, y, ws_f, gamma, 3, 2, 1, want_dx=False)
    assert none is None
    xo.assert_exact(ws_f, ws_u.double(), None, "finalized workspace, reduce-only against the full backward")
    xo.assert_exact(ws_u[4 * 64:5 * 64], c["cf"]["k1"], None, "finalized k1")
    xo.assert_exact(ws_u[5 * 64:6 * 64], r["m1"], None, "finalized m1")
    xo.assert_exact(ws_u[6 * 64:], r["k2"], None, "finalized k2")
    for got, exp, what in ((db_u, r["S"], "dbeta"), (dg_u, r["Q"], "dgamma"), (db_f, r["S"], "dbeta (reduce only)"),
                           (dg_f, r["Q"], "dgamma (reduce only)")):
        xo.assert_exact(got, exp, None, what)
    xo.assert_exact(dy_u, r["dYb"], (64, 64), "bn_relu_maxpool_bwd dx")
    _poison(cuda, 64, 256, dtype=torch.float32)
    xo.assert_exact(C.stem_wgrad(dy_u, xs, 2 * H, 2 * W, torch.float32), r["dw"], (64, 64), "unfused pair")
    _poison(cuda, 64, 256, dtype=torch.float32)
    xo.assert_exact(C.stem_wgrad_bn(dyp, pos, y, ws_f, xs, 2 * H, 2 * W, torch.float32), r["dw"], (64, 64),
                    "stem_wgrad_bn on the finalized workspace")


# -------------------------------------------------------------------- C. gemm_nt with the stride-2 addend
FORK = [(1, 2, 2, 8, 8), (3, 14, 10, 136, 72), (5, 6, 26, 64, 256), (13, 10, 10, 520, 640)]  # (n, H, W, N, K)


@functools.lru_cache(maxsize=4)
def _fork_case(regime, n, H, W, N, K, amax=xo.ADDEND_MAX):
    """gemm operands of test_gpu_exact_gemm.py's ``_gemm_case`` (same generator, same seed) with both addends and
    the addend's mask; one (D, E) pair is moved on the CPU if the data hold no element on which the three
    roundings and a single one disagree."""
    dev = torch.device("cuda:0")
    M = n * H * W
    a, w = xo.gemm_operands(regime, M, N, K, seed=M + 3 * N + 7 * K)
    A, Wk = a.to(dev, BF), w.to(dev, BF).t().contiguous()
    ref = xo.gemm_ref(A, w.to(dev, BF))  # float64 on the device
    g = xo.gen(M + N)
    D, E = xo.ints((M, N), g, -amax, amax), xo.ints((n, H // 2, W // 2, N), g, -amax, amax)
    mask = xo.mask_bytes(M * N, g)
    bits = xo.mask_bits(mask, M * N)
    witness = ho.order_witness(ref.cpu(), D, bits, E, n, H, W, amax) if regime == "dense" else 0
    return A, Wk, ref, D, E, mask, bits, witness


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 8])
@pytest.mark.parametrize("shape", FORK)
def test_gemm_nt_addend2(cuda, C, tile, shape):
    """The k-major data-gradient form (what ops/conv.py calls) with addend2 alone, addend + addend2 and
    addend + addend_mask + addend2. W = 26 is no power of two and the 6 x 26 images straddle 64-, 128- and 256-row
    tile edges; odd pixels must equal the result without addend2."""
    n, H, W, N, K = shape
    M = n * H * W
    A, Wk, ref, D, E, mask, bits, witness = _fork_case("dense", *shape)
    if K == 8:  # |acc| <= 72 and two addends of at most 64: nothing reaches 256, so no order can matter
        assert witness == 0 and float(ref.abs().max()) + 2 * xo.ADDEND_MAX < 256
    else:
        assert witness > 0, "no element tells three roundings from one"
    Dd, E4, maskd = D.to(cuda, BF), ho.as_addend2(E, cuda), mask.to(cuda)
    odd = ~ho.even_pixels(n, H, W).to(cuda)
    for what, d_, m_, b_ in (("addend2", None, None, None), ("addend + addend2", Dd, None, None),
                            ("masked addend + addend2", Dd, maskd, bits)):
        exp = ho.fork_ref(ref, None if d_ is None else D, b_, E, n, H, W)
        _poison(cuda, M, N)
        y, _ = C.gemm_nt(A, Wk, False, d_, True, tile, m_, E4, H, W)
        xo.assert_exact(y, exp, TILE_RC[tile], f"gemm_nt + {what} tile {tile}")
        _poison(cuda, M, N)
        y1, _ = C.gemm_nt(A, Wk, False, d_, True, tile, m_)
        xo.assert_exact(y[odd], y1[odd].double(), None, f"gemm_nt + {what} tile {tile}: odd pixels")


# ------------------------------------------------------------------- D. gemm_nt_bn with the full fork epilogue
def _bn_ws(N, g):
    ws = torch.zeros(7 * N)
    mean = xo.ints((N,), g, -2, 2)
    sc = torch.tensor([-2., -1., 1., 2.])[torch.randint(0, 4, (N,), generator=g)]
    sh = xo.ints((N,), g, -4, 4)
    ws[:N], ws[2 * N:3 * N], ws[3 * N:4 * N] = mean, sc, sh
    return ws, (mean.double(), sc.double(), sh.double())


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_gemm_nt_bn_fork_epilogue(cuda, C, regime, mode):
    """addend + addend_mask + addend2 (integers in [-8, 8]) and the BN-backward partials of the FINAL values: dy
    exact in both regimes, sum dy' and sum dy' (x - mean) exact in the no-rounding one (|dy'| <= 32, |x - mean| <= 5)."""
    n, H, W, N, K = 5, 20, 30, 128, 256
    M = n * H * W
    assert M * 32 * 5 < xo.EXACT_LIMIT
    A, Wk, ref, D, E, mask, bits, _ = _fork_case(regime, n, H, W, N, K, ho.FORK_ADDEND_MAX)
    g = xo.gen(mode + 11)
    x = xo.ints((M, N), g, -3, 3)
    ws, coef = _bn_ws(N, g)
    bnmask = xo.mask_bytes(M * N, g)
    exp = ho.fork_ref(ref, D, bits, E, n, H, W)
    if regime == "norounding":
        assert float(exp.abs().max()) <= 32
    _poison(cuda, M, N)
    dy, part = C.gemm_nt_bn(A, Wk, D.to(cuda, BF), True, x.to(cuda, BF), ws.to(cuda), bnmask.to(cuda), mode,
                            mask.to(cuda), ho.as_addend2(E, cuda), H, W)
    xo.assert_exact(dy, exp, (128, 128), f"gemm_nt_bn fork epilogue mode {mode} dy")
    if regime == "norounding":
        pexp = ho.bn_partials_ref(exp.cpu(), x.double(), coef, xo.mask_bits(bnmask, M * N), mode)
        xo.assert_exact(part.double().sum(0), pexp, None, f"gemm_nt_bn fork epilogue mode {mode} partials")


@pytest.mark.parametrize("regime", REGIMES)
def test_conv3x3_dgrad_bn_addend(cuda, C, regime):
    """test_gpu_exact_gemm.py's conv3x3_dgrad_bn case (128 -> 64 channels at 2 x 14 x 14, mode 1) with a non-null
    addend in [-8, 8]: dx = bf16(bf16(acc) + D), the partials from that sum."""
    n, cout, cin, H, Wd = 2, 128, 64, 14, 14
    g = xo.gen(5)
    if regime == "dense":
        dy, w = xo.dense_conv_dgrad(n, cin, H, Wd, cout, 5)
    else:
        xo.check_norounding(n * H * Wd)
        dy = xo.ints((n, cout, H, Wd), g, -2, 2)
        w = xo.sparse_signs(cin, 9 * cout, g).view(cin, 3, 3, cout).permute(3, 0, 1, 2).contiguous()
    x = xo.ints((n, cin, H, Wd), g, -3, 3)
    D = xo.ints((n, cin, H, Wd), g, -ho.FORK_ADDEND_MAX, ho.FORK_ADDEND_MAX)
    ws, coef = _bn_ws(cin, g)
    ref = xo.conv_dgrad_ref(x.shape, w, dy)
    if regime == "dense":
        assert xo.count_ties(ref) > 0, "dense inputs without rounding ties"
    exp = xo.add_rounded(ref, D)
    dev = lambda t: t.to(cuda, BF).contiguous(memory_format=CL)  # noqa: E731
    _poison(cuda, n * H * Wd, cin)
    dx, part = C.conv3x3_dgrad_bn(dev(dy), dev(w), dev(D), dev(x), ws.to(cuda), None, 1)
    xo.assert_exact(dx, exp, (128, 64), "conv3x3_dgrad_bn + addend dx")
    if regime == "norounding":
        assert float(exp.abs().max()) <= 16 + ho.FORK_ADDEND_MAX
        pexp = ho.bn_partials_ref(xo.rows_view(exp), xo.rows_view(x.double()), coef, None, 1)
        xo.assert_exact(part.double().sum(0), pexp, None, "conv3x3_dgrad_bn + addend partials")
