"""The exact integer-data oracle (tests/exact_oracle.py) is tested before it is trusted (CPU): the generators
hold their bounds and refuse requests past them, an fp32 accumulation of the generated data equals the float64
reference bit for bit in any order, the bf16 rounding agrees with one written out in integer arithmetic, the
comparison names the right tile, and the inputs the GPU tests use make every injected kernel defect visible
while the norm criterion of the older tests lets them pass."""
import pytest
import torch
import torch.nn.functional as F

import exact_oracle as xo


# ----------------------------------------------------------------------------------------------- bounds
def test_generators_hold_their_bounds():
    a, w = xo.dense_gemm(50, 40, 300, 1)
    assert a.abs().max() == 3 and w.abs().max() == 3 and a.min() == -3 and w.max() == 3
    assert torch.equal(a, a.round()) and torch.equal(a.to(torch.bfloat16).float(), a)
    a, w = xo.norounding_gemm(500, 40, 300, 2)
    assert a.abs().max() == 2 and w.abs().max() == 1
    assert int((w != 0).sum(1).max()) <= 8 and int((w != 0).sum(1).min()) >= 1
    assert float(xo.gemm_ref(a, w).abs().max()) <= 16
    x, w = xo.norounding_conv(2, 24, 9, 13, 40, 3)
    assert int((w != 0).flatten(1).sum(1).max()) <= 8 and x.abs().max() == 2
    assert float(xo.conv_ref(x, w).abs().max()) <= 16
    x, w = xo.wide_conv(2, 20, 9, 11, 36, 4)
    assert x.abs().max() <= 2048 and w.abs().max() <= 2048 and int((w != 0).flatten(1).sum(1).max()) <= 3
    assert float(x.abs().max()) > 1024 and float(w.abs().max()) > 1024  # products that need > 20 bits
    assert float(xo.conv_ref(x, w).abs().max()) < 2 ** 24
    dy = xo.wide_sparse_like((2, 36, 9, 11), 5)
    assert int((dy != 0).permute(1, 0, 2, 3).flatten(1).sum(1).max()) <= 3
    d = xo.addend((30, 20), xo.gen(0))
    assert d.abs().max() <= 64 and torch.equal(d.to(torch.bfloat16).float(), d)
    m = xo.mask_bytes(77, xo.gen(0))
    bits = xo.mask_bits(m, 77)
    assert bits.shape == (77,) and int(bits[9]) == (int(m[1]) >> 1) & 1


def test_requests_past_a_bound_raise():
    xo.check_dense(466033)  # 9 * 466033 = 2^22 - 7
    with pytest.raises(ValueError):
        xo.check_dense(466034)
    with pytest.raises(ValueError):
        xo.dense_gemm(4, 4, 1 << 19, 0)
    with pytest.raises(ValueError):
        xo.dense_conv(1, 1 << 16, 1, 1, 1, 0)
    xo.check_norounding(65535)
    with pytest.raises(ValueError):
        xo.check_norounding(65536)
    with pytest.raises(ValueError):
        xo.norounding_gemm(70000, 8, 8, 0)
    with pytest.raises(ValueError):
        xo.norounding_conv(100, 8, 56, 56, 8, 0)
    xo.check_wide()
    with pytest.raises(ValueError):
        xo.check_wide(nnz=4)
    with pytest.raises(ValueError):
        xo.check_wide(extra=1 << 22)
    with pytest.raises(AssertionError):
        xo.integral(torch.tensor([1.5], dtype=torch.float64))


# -------------------------------------------------------------------------------------- order independence
def _slab_sum(a, w, splits):
    K = a.shape[1]
    edges = [K * i // splits for i in range(splits + 1)]
    out = torch.zeros(a.shape[0], w.shape[0])
    for lo, hi in zip(edges[:-1], edges[1:]):
        out = out + a[:, lo:hi] @ w[:, lo:hi].t()  # fp32 slabs summed in fp32
    return out


@pytest.mark.parametrize("regime", ["dense", "norounding"])
def test_fp32_gemm_is_exact_in_any_order(regime):
    a, w = xo.gemm_operands(regime, 97, 56, 4608, 11)
    ref = xo.gemm_ref(a, w)
    assert torch.equal((a @ w.t()).double(), ref)  # natural order
    perm = torch.randperm(4608, generator=xo.gen(3))
    assert torch.equal((a[:, perm] @ w[:, perm].t()).double(), ref)
    for splits in range(2, 8):
        assert torch.equal(_slab_sum(a, w, splits).double(), ref), splits
    # a serial fp32 accumulation, one k at a time (no blocked summation inside the BLAS to rely on)
    acc = torch.zeros(97, 56)
    for k in perm[:512].tolist():
        acc += a[:, k:k + 1] * w[:, k].unsqueeze(0)
    assert torch.equal(acc.double(), xo.gemm_ref(a[:, perm[:512]], w[:, perm[:512]]))


def test_fp32_conv_is_exact_in_any_order():
    x, w = xo.dense_conv(2, 24, 9, 13, 40, 5)
    ref = xo.conv_ref(x, w)
    assert torch.equal(F.conv2d(x, w, None, 1, 1).double(), ref)
    perm = torch.randperm(24, generator=xo.gen(1))
    assert torch.equal(F.conv2d(x[:, perm], w[:, perm], None, 1, 1).double(), ref)
    for splits in range(2, 8):
        edges = [24 * i // splits for i in range(splits + 1)]
        out = sum(F.conv2d(x[:, lo:hi], w[:, lo:hi], None, 1, 1) for lo, hi in zip(edges[:-1], edges[1:]))
        assert torch.equal(out.double(), ref), splits
    # tap by tap
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.zeros_like(ref, dtype=torch.float32)
    for t in torch.randperm(9, generator=xo.gen(2)).tolist():
        r, s = divmod(t, 3)
        out += torch.einsum("nchw,oc->nohw", xp[:, :, r:r + 9, s:s + 13], w[:, :, r, s])
    assert torch.equal(out.double(), ref)
    # wide-mantissa regime, fp32 products of 11-bit operands
    x, w = xo.wide_conv(2, 20, 9, 11, 36, 6)
    assert torch.equal(F.conv2d(x, w, None, 1, 1).double(), xo.conv_ref(x, w))


# --------------------------------------------------------------------------------------------- rounding
def _round_bf16_int(v: torch.Tensor) -> torch.Tensor:
    """Round-to-nearest-even to 8 significant bits in int64 arithmetic."""
    a = v.abs()
    bits = torch.zeros_like(a)
    t = a.clone()
    while bool((t > 0).any()):
        bits += (t > 0).to(torch.int64)
        t >>= 1
    sh = (bits - 8).clamp_min(0)
    ulp = torch.ones_like(a) << sh
    q, rem = a // ulp, a % ulp
    up = (rem * 2 > ulp) | ((rem * 2 == ulp) & (q % 2 == 1))
    return torch.sign(v) * (q + up.to(torch.int64)) * ulp


def test_round_bf16_matches_integer_arithmetic():
    for v, r in ((257, 256), (259, 260), (385, 384), (65793, 66048), (-257, -256), (-259, -260), (511, 512),
                 (255, 255), (1110, 1112), (258, 258)):
        assert xo.round_bf16(torch.tensor([float(v)], dtype=torch.float64)).item() == r, v
    v = torch.cat([torch.arange(-70000, 70000), torch.randint(-(1 << 24) + 1, 1 << 24, (200000,), generator=xo.gen(0))])
    assert torch.equal(xo.round_bf16(v.double()), _round_bf16_int(v).double())
    # the tie count: exactly the values whose two neighbours are equally far
    d = v.double()
    r = xo.round_bf16(d)
    other = torch.where(r > d, r - 2 * (r - d), r + 2 * (d - r))  # the value mirrored across d
    tie = (r != d) & (other.float().to(torch.bfloat16).double() == other) & (other != r)
    assert xo.count_ties(d) == int(tie.sum())
    assert xo.count_ties(torch.tensor([257., 259., 511., 513., 514., 256., 255., 1026., 1028.], dtype=torch.float64)) == 5


def test_dense_reference_has_ties():
    a, w = xo.dense_gemm(777, 136, 4608, 0)
    ref = xo.gemm_ref(a, w)
    assert 256 < float(ref.abs().max()) < 4608 * 9
    assert xo.count_ties(ref) > ref.numel() // 100
    # rounding the two ways differs exactly where it should
    trunc = _truncate_bf16(ref)
    assert int((trunc != xo.round_bf16(ref)).sum()) >= xo.count_ties(ref) // 2


def _rounds_up(v: float) -> bool:
    t = torch.tensor([v], dtype=torch.float64)
    return xo.count_ties(t) == 1 and abs(float(xo.round_bf16(t))) > abs(v)


def test_every_dense_generator_plants_a_tie_that_rounds_up():
    """Not by the luck of a seed: each dense case holds one element, in its last row / channel, on which
    round-to-nearest-even and truncation disagree, from the shortest reduction that allows one."""
    assert xo.tie_partner(torch.full((29,), 3.0)) is None  # 29 * 9 = 261 is the only tie in reach and rounds down
    for K in (30, 31, 64, 72, 200, 4608):
        for seed in range(3):
            a, w = xo.dense_gemm(9, 7, K, seed)
            assert a.abs().max() <= 3 and w.abs().max() <= 3
            assert _rounds_up(float(xo.gemm_ref(a, w)[8, 6])), (K, seed)
    assert xo.count_ties(xo.gemm_ref(*xo.dense_gemm(130, 8, 8, 0))) == 0  # |y| <= 72: nothing can round
    for shape, stride in (((1, 8, 5, 7, 24), 1), ((3, 128, 11, 7, 64), 2), ((1, 64, 1, 1, 64), 1), ((2, 24, 9, 13, 40), 1)):
        n, cin, h, wd, cout = shape
        x, w = xo.dense_conv(n, cin, h, wd, cout, 1, stride=stride)
        y = xo.conv_ref(x, w, stride, 1)
        assert w.abs().max() <= 3 and _rounds_up(float(y[n - 1, cout - 1, min(1, y.shape[2] - 1), min(1, y.shape[3] - 1)]))
        oh, ow = y.shape[2:]
        dy, w2 = xo.dense_conv_dgrad(n, cin, oh, ow, cout, 2, stride=stride)
        if stride == 1 or (h % 2 == 0 and wd % 2 == 0):
            dx = xo.conv_dgrad_ref((n, cin, h, wd), w2, dy, stride, 1)
            assert _rounds_up(float(dx[n - 1, cin - 1, min(1, h - 1), min(1, wd - 1)])), shape
        dy, x = xo.dense_conv_wgrad(n, cin, h, wd, cout, 3, stride=stride)
        if n * oh * ow >= xo.TIE_MIN_K:
            assert x.abs().max() <= 3 and dy.abs().max() <= 3
            assert _rounds_up(float(xo.conv_wgrad_ref(x, (cout, cin, 3, 3), dy, stride, 1)[cout - 1, cin - 1, 1, 1])), shape
    x, w = xo.dense_conv(1, 3, 8, 8, 64, 0, k=7, stride=2, pad=3)  # the stem
    assert _rounds_up(float(xo.conv_ref(x, w, 2, 3)[0, 63, 1, 1]))
    x, w = xo.dense_conv_dgrad(2, 128, 4, 3, 128, 0, stride=2)  # stride-2 data gradient of an 8 x 6 image
    assert _rounds_up(float(xo.conv_dgrad_ref((2, 128, 8, 6), w, x, 2, 1)[1, 127, 1, 1]))


# ------------------------------------------------------------------------------------------ assert_exact
def test_assert_exact_passes_and_names_the_tile():
    a, w = xo.dense_gemm(300, 136, 512, 2)
    ref = xo.round_bf16(xo.gemm_ref(a, w))
    got = ref.to(torch.bfloat16)
    xo.assert_exact(got, ref, (128, 128), "equal")
    xo.assert_exact(torch.tensor([-0.0]), torch.tensor([0.0], dtype=torch.float64))  # signed zero is irrelevant
    bad = got.clone()
    v = bad[299, 130].view(torch.int16)
    v += 1  # one bf16 ulp
    with pytest.raises(AssertionError) as e:
        xo.assert_exact(bad, ref, (128, 128), "one ulp")
    msg = str(e.value)
    assert "one ulp: 1 of 40800 elements differ" in msg and "(299, 130)" in msg
    assert "bounding box [299, 130]..[299, 130]" in msg
    assert "(2, 1)" in msg and "1 on the last row tile 2 (44 rows)" in msg and "1 on the last column tile 1 (8 columns)" in msg
    bad = got.clone()
    bad[5, 3] = float("nan")  # a poisoned element never written
    with pytest.raises(AssertionError) as e:
        xo.assert_exact(bad, ref, (128, 128))
    assert "(0, 0)" in str(e.value) and "0 on the last row tile" in str(e.value)
    with pytest.raises(AssertionError):
        xo.assert_exact(got[:-1], ref)
    # a channels-first conv output is reported in its [N*H*W, C] view
    y = torch.zeros(2, 40, 5, 7)
    y2 = y.clone()
    y2[1, 33, 4, 6] = 1
    with pytest.raises(AssertionError) as e:
        xo.assert_exact(y2, y.double(), (32, 32), "conv")
    assert "(2, 1)" in str(e.value) and "1 on the last row tile 2 (6 rows)" in str(e.value)


# ----------------------------------------------------------------------------- sensitivity of the inputs
def _truncate_bf16(y: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 by dropping the low 16 bits (round toward zero)."""
    bits = y.float().contiguous().view(torch.int32) & ~0xFFFF
    return bits.view(torch.float32).double()


def _blocked_gemm(a, w, bm=128, bn=128, bk=32, drop_last_k_of_last_row_tile=False, skip_vector=None, truncate=False):
    """A plain blocked emulation of a tiled bf16 GEMM: fp32 accumulation over k-chunks per tile, one conversion to
    bf16 in the epilogue, 8-wide vector stores into a NaN-poisoned output; one defect at a time."""
    M, K = a.shape
    N = w.shape[0]
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16)
    chunks = list(range(0, K, bk))
    for r0 in range(0, M, bm):
        last_row_tile = r0 + bm >= M
        for c0 in range(0, N, bn):
            acc = torch.zeros(min(bm, M - r0), min(bn, N - c0))
            for k0 in chunks:
                if drop_last_k_of_last_row_tile and last_row_tile and k0 == chunks[-1]:
                    continue
                acc += a[r0:r0 + bm, k0:k0 + bk] @ w[c0:c0 + bn, k0:k0 + bk].t()
            tile = _truncate_bf16(acc).to(torch.bfloat16) if truncate else acc.to(torch.bfloat16)
            out[r0:r0 + bm, c0:c0 + bn] = tile
    if skip_vector is not None:
        r, c = skip_vector
        out[r, c:c + 8] = 0  # the store never happened: whatever the allocation held (here zeros, not the poison)
    return out


def _old_norm_criterion(out, ref32):
    """The check of the norm-ratio tests (test_gpu_gemm_stream.py and others): passes below 5e-3."""
    o, r = out.double(), ref32.double()
    return float((o - r).norm() / r.norm().clamp_min(1e-30)) < 5e-3


def test_injected_gemm_defects_are_caught_and_the_norm_criterion_passes_them():
    M, N, K = 1025, 136, 4608  # ragged M (one row in the last row tile), ragged N
    a, w = xo.dense_gemm(M, N, K, 0)
    ref = xo.gemm_ref(a, w)
    exp = xo.round_bf16(ref)
    assert xo.count_ties(ref) > 0
    ref32 = a @ w.t()
    clean = _blocked_gemm(a, w)
    xo.assert_exact(clean, exp, (128, 128), "no defect")
    assert _old_norm_criterion(clean, ref32)
    defects = {
        "last k-chunk dropped on the last row tile": dict(drop_last_k_of_last_row_tile=True),
        "one 8-wide vector not stored": dict(skip_vector=(700, 128)),
        "truncation instead of round-to-nearest-even": dict(truncate=True),
    }
    passed_by_norm = {}
    for name, kw in defects.items():
        got = _blocked_gemm(a, w, **kw)
        with pytest.raises(AssertionError) as e:
            xo.assert_exact(got, exp, (128, 128), name)
        passed_by_norm[name] = _old_norm_criterion(got, ref32)
        if "last k-chunk" in name:  # the report points at the last row tile and nowhere else
            assert "0 on the last row tile" not in str(e.value) and "(8, 0), (8, 1)" in str(e.value), str(e.value)
            assert "tiles touched (2 of 18)" in str(e.value), str(e.value)
    assert passed_by_norm["last k-chunk dropped on the last row tile"], "the norm criterion was expected to miss this"
    # (8 zeroed elements of this 139,400-element output move the norm ratio to 7.6e-3: that one the old criterion
    # sees here, and misses from about 320,000 elements up; a truncated epilogue it misses at every size)
    assert passed_by_norm["truncation instead of round-to-nearest-even"]


def test_injected_conv_defect_is_caught_and_the_norm_criterion_passes_it():
    """One tap treated as out of range one column too early at the right image border."""
    n, cin, h, wd, cout = 2, 64, 9, 13, 128
    x, w = xo.dense_conv(n, cin, h, wd, cout, 1)
    ref = xo.conv_ref(x, w)
    exp = xo.round_bf16(ref)
    assert xo.count_ties(ref) > 0
    y32 = F.conv2d(x, w, None, 1, 1)
    xo.assert_exact(y32.to(torch.bfloat16), exp, (128, 128), "no defect")
    bad = y32.clone()
    # output column W-2 of image 0, row 4 loses tap (r=1, s=2), which reads the last real column W-1
    bad[0, :, 4, wd - 2] -= w[:, :, 1, 2] @ x[0, :, 4, wd - 1]
    got = bad.to(torch.bfloat16)
    with pytest.raises(AssertionError) as e:
        xo.assert_exact(got, exp, (128, 128), "tap dropped at the right border")
    assert "bounding box [0, 0, 4, 11]" in str(e.value) or "bounding box [0, 1, 4, 11]" in str(e.value), str(e.value)
    assert float((got.double() - y32.double()).norm() / y32.double().norm()) < 1e-2  # test_gpu_conv3x3.py's bound


# -------------------------------------------------------------- device generators and the block comparison
def test_device_generators_keep_the_regimes_bounds():
    g = xo.dev_gen(3, "cpu")
    t = xo.dev_dense((1000, 64), g, 64)
    assert t.dtype == torch.bfloat16 and float(t.abs().max()) == 3 and bool((t == t.round()).all())
    with pytest.raises(ValueError, match="dense regime"):
        xo.dev_dense((4, 4), g, 1 << 22)
    s = xo.dev_sparse_signs((1 << 16, 8), g, 32)
    assert set(s.unique().tolist()) == {-1.0, 0.0, 1.0}
    share = float((s != 0).float().mean())
    assert 0.8 / 32 < share < 1.25 / 32
    assert torch.equal(xo.dev_ints((64,), xo.dev_gen(5, "cpu"), -2, 2), xo.dev_ints((64,), xo.dev_gen(5, "cpu"), -2, 2))
    xo.check_exact_sum((1 << 24) - 1)
    with pytest.raises(ValueError, match="2\\^24"):
        xo.check_exact_sum(1 << 24)


def test_assert_exact_block_names_offsets_and_the_last_row_tile():
    ref = torch.arange(300 * 8, dtype=torch.float32).view(300, 8).to(torch.bfloat16)
    xo.assert_exact_block(ref.clone(), ref, "same")
    xo.assert_exact_block(ref.clone(), ref.double(), "same value, other dtype")
    z = torch.zeros(4, 8)
    xo.assert_exact_block(-z, z, "signed zero")
    got = ref.clone()
    got[299, 7] = 1.0  # global row 1299 of 1300: the last (ragged, 20-row) tile of 128 rows
    with pytest.raises(AssertionError) as e:
        xo.assert_exact_block(got, ref, "block", row0=1000, total_rows=1300)
    msg = str(e.value)
    assert "row 1299 col 7 (element 10399, byte 20798, row tile 10)" in msg
    assert "1 on the last row tile 10 (20 rows, from element 10240)" in msg
    nan = ref.clone()
    nan[0, 0] = float("nan")
    with pytest.raises(AssertionError, match="1 of 2400 elements"):
        xo.assert_exact_block(nan, nan.clone(), "NaN is never equal")
    img = torch.zeros(2, 8, 3, 5)
    bad = img.clone()
    bad[1, 2, 2, 4] = 1
    with pytest.raises(AssertionError, match=r"row 29 col 2 \(element 234"):
        xo.assert_exact_block(bad, img, "4-D blocks are read as pixel rows")


@pytest.mark.parametrize("k,stride,pad", [(3, 1, 1), (3, 2, 1), (7, 2, 3), (1, 1, 0)])
def test_device_references_are_the_library_references(k, stride, pad):
    """conv_ref_dev / conv_wgrad_ref_dev (float64 tap by tap, for slices and reductions of the index-edge operands)
    against F.conv2d / conv2d_weight in float64; the weight gradient also in blocks of a few rows."""
    g = xo.gen(k + stride)
    x, w = xo.ints((2, 5, 9, 12), g, -3, 3), xo.ints((6, 5, k, k), g, -3, 3)
    ref = xo.conv_ref(x, w, stride, pad)
    assert torch.equal(xo.conv_ref_dev(x, w, stride, pad), ref)
    dy = xo.ints(ref.shape, g, -2, 2)
    wref = xo.conv_wgrad_ref(x, w.shape, dy, stride, pad)
    assert torch.equal(xo.conv_wgrad_ref_dev(dy, x, k, stride, pad), wref)
    assert torch.equal(xo.conv_wgrad_ref_dev(dy, x, k, stride, pad, block_pixels=2 * ref.shape[3]), wref)


def test_grouped_reduction_and_column_counts():
    g = xo.gen(2)
    for P in (1, 63, 64, 1000, 70001):
        a, b = xo.ints((P, 8), g, -3, 3), xo.ints((P, 5), g, -3, 3)
        assert torch.equal(xo.tn_ref(a, b), a.double().t() @ b.double())
    t = xo.ints((3, 8, 5, 7), g, -1, 1).contiguous(memory_format=torch.channels_last)
    assert torch.equal(xo.nonzeros_per_column(t, block_rows=16), (t != 0).sum((0, 2, 3)))
