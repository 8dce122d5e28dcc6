"""The hand-off oracle (tests/handoff_oracle.py) is tested before it is trusted (CPU): its generators hold their
asserted bounds and tie counts, its references agree with independently written plain-torch emulations of the three
kernels' formulas, and every defect injected into those emulations (``fault=``) is caught by the exact comparison
on the inputs the GPU tests use, while the criteria of the older tests (max |dx - dx'| <= 2^-7 max |dx'|, relative
L2 < 5e-3, < 1e-5 and < 1e-4) are evaluated on the same outputs and shown to pass the faults they pass."""
import functools

import pytest
import torch
import torch.nn.functional as F

import exact_oracle as xo
import handoff_oracle as ho

BF = torch.bfloat16


def _bf(v32: torch.Tensor, truncate: bool = False) -> torch.Tensor:
    """fp32 -> bf16 -> fp32: round-to-nearest-even, or (the fault) the low 16 bits dropped."""
    if truncate:
        return (v32.float().contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32)
    return v32.float().to(BF).float()


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------ generators
def test_coefficients_hold_their_bounds():
    for seed in range(5):
        for C in (64, 256):
            ws, cf = ho.bn_bwd_coeffs(C, xo.gen(seed))
            assert ws.shape == (7 * C,) and torch.equal(ws[:C].double(), cf["mean"]) and torch.equal(ws[4 * C:5 * C].double(), cf["k1"])
            assert torch.equal(ws[5 * C:6 * C].double(), cf["m1"]) and torch.equal(ws[6 * C:].double(), cf["k2"])
            assert cf["mean"].abs().max() <= 2 and set(cf["k1"].tolist()) <= {-2., -1., 1., 2.}
            assert set(cf["m1"].tolist()) == {-1., 1.} and set(cf["k2"].tolist()) == {-1., 0., 1.}
            assert int((cf["mean"] * cf["k2"] != 0).sum()) * 4 >= C
            assert set(cf["sc"].tolist()) <= {-2., -1., 1., 2.} and cf["sh"].abs().max() <= 4.5
            assert bool(((cf["sh"] - 0.5) == (cf["sh"] - 0.5).round()).all())
            # rows padded past the end: dY = k1 (-m1 + mean k2), nonzero in most channels
            assert int((cf["k1"] * (cf["mean"] * cf["k2"] - cf["m1"]) != 0).sum()) > C // 2


@functools.lru_cache(maxsize=2)
def _dual(M):
    c = ho.dual_case(M, M)
    bits = xo.mask_bits(c["mask"], M * 256).view(M, 256)
    return c, bits, ho.dual_ref(c["dout"], c["ybn"], bits, c["x"], c["w"], c["cf"])


def _rounds_up(v: float) -> bool:
    t = torch.tensor([v], dtype=torch.float64)
    return xo.count_ties(t) == 1 and abs(float(xo.round_bf16(t))) > abs(v)


@pytest.mark.parametrize("M", [4001, 70001])
def test_dual_case_bounds_and_ties(M):
    c, bits, (dY, dx, dw) = _dual(M)
    for k in ("dout", "ybn", "x", "w"):
        assert c[k].abs().max() == 3 and torch.equal(c[k].to(BF).float(), c[k])
    assert float(dY.abs().max()) <= ho.DUAL_DY_MAX and float(dY.abs().max()) >= 12
    assert _rounds_up(float(dx[M - 1, 63])) and xo.count_ties(dx) > 0
    assert float(dw.abs().max()) < M * ho.DUAL_DY_MAX * 3 < xo.EXACT_LIMIT
    if M == 70001:
        assert xo.count_ties(dw) > 0
    with pytest.raises(AssertionError):
        ho.dual_case(1 << 19, 0)  # 2^19 * 54 >= 2^24: the weight gradient could round in fp32


def test_stem_case_bounds_taps_and_borders():
    for n, H, W in ((1, 4, 4), (3, 18, 14), (2, 32, 48)):
        c = ho.stem_case(n, H, W, n + H + W)
        pos = c["pos"].long()
        assert c["pos"].dtype == torch.uint8 and set(pos.unique().tolist()) == set(range(9))  # all nine taps
        assert int((pos[:, :, 0] // 3).min()) >= 1 and int((pos[:, :, :, 0] % 3).min()) >= 1  # border windows stay inside
        assert int((pos[:, :, 1:] // 3).min()) == 0 and int((pos[:, :, :, 1:] % 3).min()) == 0
        g = ho.stem_scatter(c["dyp"], c["pos"], H, W)
        assert torch.equal(g.sum((2, 3)), c["dyp"].double().sum((2, 3))) and float(g.abs().max()) <= 12
        dY = ho.stem_dy_ref(c["dyp"], c["pos"], c["y"], c["cf"])
        assert float(dY.abs().max()) <= ho.STEM_DY_MAX
        # uniform among the valid taps: an interior window's nine taps each near 1/9
        inner = torch.bincount(pos[:, :, 1:, 1:].reshape(-1), minlength=9).double()
        assert float((inner / inner.sum() - 1 / 9).abs().max()) < (0.08 if H == 4 else 0.02)


def test_stem_pack_layout_and_reference():
    idx = torch.arange(64 * 3 * 8 * 8, dtype=torch.float64).view(64, 3, 8, 8)
    pk = ho.stem_pack8(idx)
    assert pk.shape == (64, 256)
    for th, tw, ph, pw, c in ((0, 0, 0, 0, 0), (3, 3, 1, 1, 2), (1, 2, 0, 1, 1), (2, 0, 1, 0, 2)):
        assert torch.equal(pk[:, (th * 4 + tw) * 16 + (ph * 2 + pw) * 3 + c], idx[:, c, 2 * th + ph, 2 * tw + pw])
    assert float(ho.stem_padding_lanes(pk).abs().max()) == 0
    # the folded 4x4 / s1 conv over the space-to-depth image with the packed weight IS the 7x7 / s2 / p3 conv
    g = xo.gen(0)
    img, w7 = xo.ints((2, 3, 12, 8), g, -3, 3).double(), xo.ints((64, 3, 7, 7), g, -3, 3).double()
    ref = F.conv2d(img, w7, None, 2, 3)
    xs = F.pad(img.view(2, 3, 6, 2, 4, 2).permute(0, 3, 5, 1, 2, 4).reshape(2, 12, 6, 4), (0, 0, 0, 0, 0, 4))  # (ph, pw, c)
    wf = ho.stem_pack8(F.pad(w7, (1, 0, 1, 0))).view(64, 4, 4, 16).permute(0, 3, 1, 2)
    assert torch.equal(F.conv2d(F.pad(xs, (2, 1, 2, 1)), wf), ref)


def test_stem_finalized_reference_is_exact_and_rounds():
    """The cases of the unfused pair: dyadic finalized coefficients, a dY that really rounds to bf16, and a weight
    gradient that an fp32 accumulation of the rounded dY reproduces in any order."""
    for n, H, W in ((1, 4, 4), (2, 8, 16)):
        c = ho.stem_case(n, H, W, n + H + W)
        r = ho.stem_finalized_ref(c)
        M = n * H * W
        assert float(r["m1"].abs().max()) <= 0.75 and float(r["m1"].abs().max()) > 0
        assert torch.equal(r["m1"].float().double(), r["m1"]) and torch.equal(r["k2"].float().double(), r["k2"])
        if M == 16:  # multiples of 1 / 16 below 16 fit bf16's 8 bits: this case cannot round
            assert float(r["dY"].abs().max()) < 16 and torch.equal(r["dYb"], r["dY"])
        else:
            assert int((r["dYb"] != r["dY"]).sum()) > 256  # about 1 in 15 here
        cols = torch.nn.functional.unfold(F.pad(c["img"], (4, 3, 4, 3)), 8, stride=2)  # [n, 3 * 64, H * W] fp32
        dy32 = r["dYb"].float().view(n, 64, H * W)
        perm = torch.randperm(H * W, generator=xo.gen(0))
        for order in (slice(None), perm):
            dw = sum(dy32[i][:, order] @ cols[i][:, order].t() for i in range(n)).view(64, 3, 8, 8)
            assert torch.equal(ho.stem_pack8(dw).double(), r["dw"])
    with pytest.raises(AssertionError):
        ho.stem_finalized_ref(ho.stem_case(3, 18, 14, 0))  # 756 pixels: 1 / M is no fp32 number


# --------------------------------------------------------------------------------- conv1x1_dual with BN apply
R_BN = 32  # rows per tile of the BN-apply form


def _dual_emulate(c, bits, M, fault=None):
    """The kernel's structure in plain torch: 32-row tiles whose loads past M read zeros (so padded rows get
    dY = k1 (-m1 + mean k2) != 0), dY rounded to bf16, dx rows stored only below M, dw summed over whole tiles."""
    mp = (M + R_BN - 1) // R_BN * R_BN
    pad = lambda t: F.pad(t.float(), (0, 0, 0, mp - M))  # noqa: E731
    dout, ybn, x, b = pad(c["dout"]), pad(c["ybn"]), pad(c["x"]), pad(bits)
    lo = mp - R_BN
    if fault == "next_row_mask" and M % R_BN:  # last ragged tile: chunk column 31 reads the next row's mask byte
        b[lo:mp - 1, 248:] = b[lo + 1:mp, 248:].clone()
        b[mp - 1, 248:] = 0
    if fault == "pad_rows_x":  # the X tile's rows past M are not zero-filled
        x[M:] = 1.0
    trunc = fault == "truncate"
    cf = {k: v.float() for k, v in c["cf"].items()}
    dY = _bf(cf["k1"] * (b * dout - cf["m1"] - (ybn - cf["mean"]) * cf["k2"]), trunc)
    dx = _bf(dY @ c["w"].float(), trunc)[:M]
    dw = dY.t() @ x  # integers below 2^24: exact in fp32 in any order
    return dx, dw, _bf(dw, trunc)


def _dual_old_criteria(got, clean, dY, w):
    """test_dual_with_bn_apply_matches_separate's three: against the unfused pair (here the clean emulation) and
    fp32 torch."""
    dx, dw = got[0], got[1]
    return {"2^-7 max": float((dx - clean[0]).abs().max()) <= float(clean[0].abs().max()) * 2 ** -7,
            "dx 5e-3": _rel(dx, dY.float() @ w.float()) < 5e-3,
            "dw 1e-5": _rel(dw, clean[1]) < 1e-5}


def _caught(got, exp, tile, what):
    try:
        xo.assert_exact(got, exp, tile, what)
    except AssertionError as e:
        return str(e)
    return None


def test_dual_faults_are_caught_and_what_the_old_criteria_pass():
    M = 70001  # 17 rows on the last 32-row tile
    c, bits, (dY, dx_ref, dw_ref) = _dual(M)
    exp = (xo.round_bf16(dx_ref), dw_ref, xo.round_bf16(dw_ref))
    clean = _dual_emulate(c, bits, M)
    for got, e, what in zip(clean, exp, ("dx", "dw fp32", "dw bf16")):
        xo.assert_exact(got, e, (R_BN, 64), "no defect: " + what)
    assert all(_dual_old_criteria(clean, clean, dY, c["w"]).values())
    old = {}
    for fault in ("next_row_mask", "truncate", "pad_rows_x"):
        got = _dual_emulate(c, bits, M, fault)
        reports = [_caught(g, e, (R_BN, 64), fault) for g, e in zip(got, exp)]
        assert any(reports), f"{fault} not caught"
        old[fault] = _dual_old_criteria(got, clean, dY, c["w"])
        if fault == "next_row_mask":  # dx: the last row tile and nowhere else
            assert f"on the last row tile {M // R_BN} (17 rows)" in reports[0] and "tiles touched (1 of" in reports[0], reports[0]
        if fault == "truncate":  # dY is exact on these data: the defect shows in the two output roundings
            assert reports[0] and reports[2] and not reports[1]
        if fault == "pad_rows_x":  # dx never sees the padded rows; the weight gradient does
            assert not reports[0] and reports[1]
    # truncation: every old criterion passes it (one bf16 ulp per element is the 2^-7 allowance itself)
    assert all(old["truncate"].values()), old["truncate"]
    # a wrong mask byte per row of the last tile (8 of 256 channels of 17 of 70001 rows): both norm criteria of dx
    # pass it; whether the max criterion does depends on the gradient under the flipped bits
    assert old["next_row_mask"]["dx 5e-3"], old["next_row_mask"]
    assert not old["pad_rows_x"]["dw 1e-5"] and old["pad_rows_x"]["dx 5e-3"] and old["pad_rows_x"]["2^-7 max"]


def test_one_wrong_mask_byte_against_the_old_criteria_on_the_old_tests_data():
    """The older test's own kind of data (standard normal gradient, weights of norm 1 / sqrt(Cout), batch
    statistics as coefficients) at the smallest served M, whose last 32-row tile holds one row: that row's last
    mask byte read from the row after it (zeros past the end). Both relative-L2 criteria of dx (the older test's and
    smoke()'s 5e-3) pass it. The max criterion and the fp32 weight gradient's 1e-5 do notice a whole wrong byte
    under a nonzero gradient -- at a row count with a ragged tile, which the older test has one of (100003: 3 rows),
    none with a single row, and with random floats, where a failure names no element."""
    M, co, ci = 65473, 256, 64
    g = xo.gen(1)
    dout, ybn = torch.randn(M, co, generator=g).to(BF).float(), (torch.randn(M, co, generator=g) * 2 + 0.5).to(BF).float()
    x, w = torch.randn(M, ci, generator=g).to(BF).float(), (torch.randn(co, ci, generator=g) * co ** -0.5).to(BF).float()
    bits = xo.mask_bits(xo.mask_bytes(M * co, g), M * co).view(M, co).float()
    gamma = torch.rand(co, generator=g) + 0.5
    mean, invstd = ybn.mean(0), (ybn.var(0, unbiased=False) + 1e-5).rsqrt()

    S, Q = (bits * dout).sum(0), (bits * dout * (ybn - mean)).sum(0)  # the reduction pass reads the mask correctly

    def run(b):
        dY = _bf(gamma * invstd * (b * dout - S / M - (ybn - mean) * invstd * invstd * Q / M))
        return _bf(dY @ w), dY.t() @ x, dY

    clean = run(bits)
    bad_bits = bits.clone()
    bad_bits[M - 1, 248:] = 0
    assert int((bits[M - 1, 248:] * (dout[M - 1, 248:] != 0)).sum()) > 0  # the byte matters
    bad = run(bad_bits)
    assert not torch.equal(bad[0], clean[0])  # an exact comparison sees it
    old = _dual_old_criteria(bad, clean, clean[2], w)
    assert old == {"dx 5e-3": True, "2^-7 max": False, "dw 1e-5": False}, old


# -------------------------------------------------------------------------------- fork data-gradient epilogue
def _fork_emulate(acc, D, bits, E, n, H, W, fault=None, bn=None):
    """epilogue_bf16 with both addends in plain torch: bf16(acc), + masked D, rounded, + E at even pixels, rounded;
    then (bn = (x, mean, sc, sh, bnbits, mode)) the BN-backward partials of the final values."""
    trunc = fault == "truncate"
    M, N = acc.shape
    v = _bf(acc.float(), trunc)
    first = v.clone()
    d = D.float() * (1 if bits is None else bits.view(M, N).float())
    rows = torch.arange(M)
    w_, h_, n_ = rows % W, (rows // W) % H, rows // (H * W)
    ok2 = (w_ % 2 == 0) if fault == "even_w_only" else ((h_ | w_) % 2 == 0)
    e = torch.where(ok2.view(M, 1), E.float()[n_, h_ // 2, w_ // 2], torch.zeros(()))
    for add in ((e, d) if fault == "addend2_first" else (d, e)):
        v = _bf(v + add, trunc)
    part = None
    if bn is not None:
        x, mean, sc, sh, bnbits, mode = bn
        src = (first if fault == "partials_before_addends" else v).double()
        part = ho.bn_partials_ref(src, x.double(), (mean, sc, sh), bnbits, mode)
    return v, part


@functools.lru_cache(maxsize=4)
def _fork_case(n, H, W, N, K, regime="dense", amax=xo.ADDEND_MAX):
    M = n * H * W
    a, w = xo.gemm_operands(regime, M, N, K, seed=M + 3 * N + 7 * K)
    acc = xo.gemm_ref(a, w)
    g = xo.gen(M + N)
    D, E = xo.ints((M, N), g, -amax, amax), xo.ints((n, H // 2, W // 2, N), g, -amax, amax)
    mask = xo.mask_bytes(M * N, g)
    bits = xo.mask_bits(mask, M * N)
    return acc, D, E, bits


FORK_SHAPES = [(1, 2, 2, 8, 8), (3, 14, 10, 136, 72), (5, 6, 26, 64, 256)]


@pytest.mark.parametrize("shape", FORK_SHAPES)
def test_fork_reference_order_matters_and_matches_the_emulation(shape):
    n, H, W, N, K = shape
    acc, D, E, bits = _fork_case(*shape)
    D, E = D.clone(), E.clone()
    diff = ho.order_witness(acc, D, bits, E, n, H, W)
    if K == 8:  # |acc| <= 72 and two addends of at most 64: nothing reaches 256, nothing rounds
        assert diff == 0 and float(acc.abs().max()) + 2 * xo.ADDEND_MAX < 256
    else:
        assert diff > 0
        assert int((ho.fork_ref(acc, D, None, E, n, H, W) != ho.fork_single(acc, D, None, E, n, H, W)).sum()) > 0
    ev = ho.even_pixels(n, H, W)
    assert int(ev.sum()) == n * (H // 2) * (W // 2)
    for d_, b_ in ((None, None), (D, None), (D, bits)):
        exp = ho.fork_ref(acc, d_, b_, E, n, H, W)
        got, _ = _fork_emulate(acc, torch.zeros_like(acc) if d_ is None else d_, b_, E, n, H, W)
        xo.assert_exact(got, exp, (128, 128), "no defect")
        base = ho.fork_ref(acc, d_, b_, None, n, H, W)
        assert torch.equal(exp[~ev], base[~ev])  # odd pixels: the result without addend2


def test_order_witness_plants_one_when_the_data_hold_none():
    n, H, W, N = 1, 2, 2, 8
    acc = torch.zeros(4, 8, dtype=torch.float64)
    acc[0, 3] = 300.0  # the only element that can round, at an even pixel
    D, E = torch.zeros(4, 8), torch.zeros(1, 1, 1, 8)
    bits = torch.ones(32, dtype=torch.int64)
    assert int((ho.fork_ref(acc, D, bits, E, n, H, W) != ho.fork_single(acc, D, bits, E, n, H, W)).sum()) == 0
    assert ho.order_witness(acc, D, bits, E, n, H, W) == 1
    assert D.abs().max() <= 64 and E.abs().max() <= 64 and (D[0, 3] != 0 or E[0, 0, 0, 3] != 0)


def test_fork_faults_are_caught_and_the_model_criterion_passes_the_rounding_ones():
    """The stride-2 addend had no kernel-level test: its only older criterion is the whole-model parity bound
    (2e-2 relative L2), evaluated here on the epilogue's own output."""
    shape = (5, 6, 26, 64, 256)  # W no power of two, H != W
    n, H, W, N, K = shape
    acc, D, E, bits = _fork_case(*shape)
    M = n * H * W
    g = xo.gen(7)
    x = xo.ints((M, N), g, -3, 3)
    mean, sc, sh = xo.ints((N,), g, -2, 2).double(), torch.ones(N, dtype=torch.float64), xo.ints((N,), g, -4, 4).double()
    bnbits = xo.mask_bits(xo.mask_bytes(M * N, g), M * N)
    exp = ho.fork_ref(acc, D, bits, E, n, H, W)
    old = {}
    for mode in (0, 1, 2):
        bn = (x, mean, sc, sh, bnbits, mode)
        pexp = ho.bn_partials_ref(exp, x.double(), (mean, sc, sh), bnbits, mode)
        got, part = _fork_emulate(acc, D, bits, E, n, H, W, None, bn)
        xo.assert_exact(got, exp, (128, 64), "no defect")
        xo.assert_exact(part, pexp, None, "no defect: partials")
        for fault in ("even_w_only", "addend2_first", "partials_before_addends", "truncate"):
            got, part = _fork_emulate(acc, D, bits, E, n, H, W, fault, bn)
            seen = _caught(got, exp, (128, 64), fault), _caught(part, pexp, None, fault + " partials")
            assert any(seen), f"{fault} not caught (mode {mode})"
            if fault == "partials_before_addends":
                assert not seen[0] and seen[1]
            old[fault] = _rel(got, exp) < 2e-2
    assert old["addend2_first"] and old["truncate"], old  # one bf16 ulp here and there: far inside 2e-2
    assert not old["even_w_only"]


# ---------------------------------------------------------------------------------------------- stem_wgrad_bn
def _stem_emulate(c, fault=None):
    """stem_wgrad_bn_kernel's formulation in plain torch: per 2x2 quad of conv-output pixels, the 4 pooled windows
    that cover it are compared with compile-time tap numbers (a gather, where the reference scatters)."""
    dyp, pos, y = c["dyp"].float(), c["pos"].long(), c["y"].float()
    n, C, H, W = y.shape
    OH, OW = H // 2, W // 2
    g = torch.zeros(n, C, H, W)
    dpad, ppad = F.pad(dyp, (0, 1, 0, 1)), F.pad(pos, (0, 1, 0, 1), value=255)  # far windows outside: no tap matches
    for a in (0, 1):
        for b in (0, 1):
            for dh in (0, 1):
                for dw in (0, 1):
                    ky, kx = dh - 2 * a + 1, dw - 2 * b + 1
                    if ky < 0 or kx < 0:
                        continue
                    tap = ky * 3 + kx + (1 if fault == "far_tap_off_by_one" and (a or b) else 0)
                    hit = ppad[:, :, a:a + OH, b:b + OW] == tap
                    g[:, :, dh::2, dw::2] += torch.where(hit, dpad[:, :, a:a + OH, b:b + OW], torch.zeros(()))
    cf = {k: v.float().view(1, C, 1, 1) for k, v in c["cf"].items()}
    gg = torch.where(torch.addcmul(cf["sh"], y, cf["sc"]) > 0, g, torch.zeros(()))
    dY = _bf(cf["k1"] * (gg - cf["m1"] - (y - cf["mean"]) * cf["k2"]))
    dw8 = torch.nn.grad.conv2d_weight(F.pad(c["img"].double(), (4, 3, 4, 3)), (C, 3, 8, 8), dY.double(), 2, 0)
    dwp = ho.stem_pack8(dw8).float()
    return dY, dwp, _bf(dwp, fault == "truncate")


@pytest.mark.parametrize("shape", [(1, 4, 4), (3, 18, 14), (2, 32, 48)])
def test_stem_faults_are_caught(shape):
    n, H, W = shape
    c = ho.stem_case(n, H, W, n + H + W)
    dY_ref = ho.stem_dy_ref(c["dyp"], c["pos"], c["y"], c["cf"])
    ref = ho.stem_wgrad_ref(c["img"], dY_ref)
    dY, dwp, dwb = _stem_emulate(c)
    xo.assert_exact(dY, dY_ref, None, "no defect: dY")
    xo.assert_exact(dwp, ref, None, "no defect: dw")
    xo.assert_exact(dwb, xo.round_bf16(ref), None, "no defect: bf16 dw")
    assert float(ho.stem_padding_lanes(ref).abs().max()) == 0
    _, bad, _ = _stem_emulate(c, "far_tap_off_by_one")
    assert _caught(bad, ref, None, "far tap")
    assert _rel(bad, dwp) > 1e-4  # the older criteria (< 1e-5 against the unfused pair, < 1e-4 against aten) see this one too
    _, _, badb = _stem_emulate(c, "truncate")
    if float(ref.abs().max()) < 256:  # the 4 x 4 case: 16 pixels of |dY| <= 36, |x| <= 3 ... cannot round when small
        assert xo.count_ties(ref) == 0 and torch.equal(badb, dwb)
    else:
        assert _caught(badb, xo.round_bf16(ref), None, "truncated bf16 dw")
        torch.testing.assert_close(badb, dwp, rtol=1e-2, atol=1e-2 * float(dwp.abs().max()))  # the older bf16 criterion passes it
