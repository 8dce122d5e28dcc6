"""Exact integer-data oracle tests of the convolution kernels (conv.hip, conv_halo.hip, conv_halo_wgrad.hip, stem.hip,
conv_f32.hip) against float64 PyTorch convolutions (gpu).

Same rules as test_gpu_exact_gemm.py: operands from tests/exact_oracle.py (fp32 accumulation exact in any order),
``assert_exact`` everywhere, one round-to-nearest-even to bf16 of the reference (two for the data gradient's
addend, bf16(bf16(acc) + D)), exact BatchNorm statistics in the no-rounding regime, exact fp32 weight gradients,
NaN-poisoned outputs, setters restored in the fixture teardown. The fp32 kernels get the wide-mantissa regime
(products of 11-bit operands)."""
import functools
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import exact_oracle as xo

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
CL = torch.channels_last
CONV_TILE = {0: (128, 128), 1: (128, 128), 2: (128, 64), 3: (64, 64), 8: (256, 256), 9: (512, 128)}
REGIMES = ["dense", "norounding"]


@pytest.fixture
def C():
    from distributed_learning_amd.ops import _ext

    C = _ext.require()
    yield C
    C.set_mfma_pipeline(-1)
    C.set_wgrad_w4(-1)
    C.set_halo_wgrad(-1)
    C.set_stem_stream(-1)
    C.set_tn256(-1)


def _poison(dev, *shape, dtype=BF):
    t = torch.full(shape, float("nan"), device=dev, dtype=dtype)
    del t


def _dev(t, dev, dtype=BF):
    return t.to(dev, dtype).contiguous(memory_format=CL)


def _out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


@functools.lru_cache(maxsize=4)
def _fwd_case(regime, N, Cin, H, W, Cout, stride):
    """Forward operands and float64 reference, computed once per shape."""
    x, w = xo.conv_operands(regime, N, Cin, H, W, Cout, seed=N + Cin + H * W + Cout + stride, stride=stride)
    ref = xo.conv_ref(x, w, stride, 1)
    if regime == "dense":
        assert xo.count_ties(ref) > 0, "dense inputs without rounding ties"
    if regime == "norounding":
        assert float(ref.abs().max()) <= 16
    return x, w, ref


def _check_stats(st, ref, what):
    xo.assert_exact(st.double().sum(0), xo.col_stats(ref), None, what + " statistics")


SHAPES = [  # N, Cin, H, W, Cout, stride
    (1, 8, 5, 7, 24, 1), (2, 24, 14, 14, 64, 1), (2, 64, 9, 13, 128, 1), (3, 128, 11, 7, 64, 2),
    (2, 128, 8, 6, 128, 2), (2, 144, 14, 14, 288, 1), (4, 512, 7, 7, 512, 1),
]


# ------------------------------------------------------------------------------------- implicit-GEMM 3x3
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", SHAPES)
def test_conv3x3_fwd(cuda, C, regime, shape):
    N, Cin, H, W, Cout, stride = shape
    x, w, ref = _fwd_case(regime, *shape)
    oh, ow = _out_hw(H, W, stride)
    _poison(cuda, N * oh * ow, Cout)
    y, st = C.conv3x3_fwd(_dev(x, cuda), _dev(w, cuda), stride, True)
    assert y.shape == ref.shape and y.is_contiguous(memory_format=CL)
    xo.assert_exact(y, xo.round_bf16(ref), (128, 128), "conv3x3_fwd")
    if regime == "norounding":
        _check_stats(st, ref, "conv3x3_fwd")
    _poison(cuda, N * oh * ow, Cout)
    y, _ = C.conv3x3_fwd(_dev(x, cuda), _dev(w, cuda), stride, False)
    xo.assert_exact(y, xo.round_bf16(ref), (128, 128), "conv3x3_fwd without statistics")


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[5] == 1 or (s[2] % 2 == 0 and s[3] % 2 == 0)])
def test_conv3x3_dgrad(cuda, C, shape):
    """Stride 1: with and without the addend (two roundings). Stride 2 at even sizes: the parity-class kernel (the
    odd size at stride 2 is a forward and weight-gradient case only)."""
    N, Cin, H, W, Cout, stride = shape
    oh, ow = _out_hw(H, W, stride)
    dy, w = xo.dense_conv_dgrad(N, Cin, oh, ow, Cout, seed=N + Cin + Cout, stride=stride)
    ref = xo.conv_dgrad_ref((N, Cin, H, W), w, dy, stride, 1)
    assert xo.count_ties(ref) > 0, "dense inputs without rounding ties"
    _poison(cuda, N * H * W, Cin)
    if stride == 2:
        dx = C.conv3x3s2_dgrad(_dev(dy, cuda), _dev(w, cuda), H, W)
        assert dx.is_contiguous(memory_format=CL)
        xo.assert_exact(dx, xo.round_bf16(ref), (128, 128), "conv3x3s2_dgrad")
        return
    dx = C.conv3x3_dgrad(_dev(dy, cuda), _dev(w, cuda))
    xo.assert_exact(dx, xo.round_bf16(ref), (128, 128), "conv3x3_dgrad")
    D = xo.addend((N, Cin, H, W), xo.gen(H + W))
    _poison(cuda, N * H * W, Cin)
    dx = C.conv3x3_dgrad(_dev(dy, cuda), _dev(w, cuda), _dev(D, cuda))
    xo.assert_exact(dx, xo.add_rounded(ref, D), (128, 128), "conv3x3_dgrad + addend")


def _wgrad_case(N, Cin, H, W, Cout, stride, seed):
    """(dy, x, reference): the reduction runs over the N * OH * OW output pixels; one planted tie at least."""
    dy, x = xo.dense_conv_wgrad(N, Cin, H, W, Cout, seed, stride=stride)
    ref = xo.conv_wgrad_ref(x, (Cout, Cin, 3, 3), dy, stride, 1)
    oh, ow = _out_hw(H, W, stride)
    if N * oh * ow >= xo.TIE_MIN_K:
        assert xo.count_ties(ref) > 0, "dense inputs without rounding ties"
    else:  # (2, 128, 8, 6, 128, 2): 24 output pixels, |dw| <= 216 -- no bf16 rounding is possible at all
        assert 9 * N * oh * ow < 256
    return dy, x, ref


@pytest.mark.parametrize("shape", SHAPES)
def test_conv3x3_wgrad(cuda, C, shape):
    """fp32 output exact; bf16 output one rounding of the summed slabs."""
    N, Cin, H, W, Cout, stride = shape
    dy, x, ref = _wgrad_case(*shape, seed=sum(shape))
    _poison(cuda, Cout, 9 * Cin, dtype=torch.float32)
    dw = C.conv3x3_wgrad(_dev(dy, cuda), _dev(x, cuda), stride, torch.float32)
    assert dw.shape == ref.shape and dw.is_contiguous(memory_format=CL)
    xo.assert_exact(dw, ref, None, "conv3x3_wgrad fp32")
    _poison(cuda, Cout, 9 * Cin)
    dwb = C.conv3x3_wgrad(_dev(dy, cuda), _dev(x, cuda), stride, BF)
    xo.assert_exact(dwb, xo.round_bf16(ref), None, "conv3x3_wgrad bf16")


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("tile", [1, 2, 3, 8, 9])
def test_conv3x3_forced_tiles(cuda, C, regime, tile):
    shape = (3, 256, 14, 14, 256, 1)  # 588 pixels: every tile height leaves a partial last row tile
    x, w, ref = _fwd_case(regime, *shape)
    _poison(cuda, 588, 256)
    y, st = C.conv3x3_fwd(_dev(x, cuda), _dev(w, cuda), 1, True, tile)
    xo.assert_exact(y, xo.round_bf16(ref), CONV_TILE[tile], f"conv3x3_fwd tile {tile}")
    if regime == "norounding":
        _check_stats(st, ref, f"conv3x3_fwd tile {tile}")
    else:
        dy, w2 = xo.dense_conv_dgrad(3, 256, 14, 14, 256, seed=9)
        dref = xo.conv_dgrad_ref((3, 256, 14, 14), w2, dy)
        assert xo.count_ties(dref) > 0
        _poison(cuda, 588, 256)
        dx = C.conv3x3_dgrad(_dev(dy, cuda), _dev(w2, cuda), None, tile)
        xo.assert_exact(dx, xo.round_bf16(dref), CONV_TILE[tile], f"conv3x3_dgrad tile {tile}")


def test_conv3x3_wgrad_128x256_tiles(cuda, C):
    shape = (3, 128, 13, 13, 128, 1)
    dy, x, ref = _wgrad_case(*shape, seed=4)
    C.set_wgrad_w4(1)
    _poison(cuda, 128, 9 * 128, dtype=torch.float32)
    dw = C.conv3x3_wgrad(_dev(dy, cuda), _dev(x, cuda), 1, torch.float32)
    xo.assert_exact(dw, ref, None, "conv3x3_wgrad 128x256 tiles")


@pytest.mark.parametrize("pipe", [0, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("cin", [24, 64])
def test_conv3x3_main_loops(cuda, C, pipe, cin):
    shape = (2, cin, 9, 13, 128, 1)
    C.set_mfma_pipeline(pipe)
    for regime in REGIMES:
        x, w, ref = _fwd_case(regime, *shape)
        _poison(cuda, 2 * 9 * 13, 128)
        y, st = C.conv3x3_fwd(_dev(x, cuda), _dev(w, cuda), 1, True)
        xo.assert_exact(y, xo.round_bf16(ref), (128, 128), f"conv3x3_fwd pipeline {pipe} {regime}")
        if regime == "norounding":
            _check_stats(st, ref, f"conv3x3_fwd pipeline {pipe}")
    ref2 = xo.conv_ref(x, w, 2, 1)  # the no-rounding operands at stride 2
    y2, _ = C.conv3x3_fwd(_dev(x, cuda), _dev(w, cuda), 2, False)
    xo.assert_exact(y2, ref2, (128, 128), f"conv3x3_fwd stride 2 pipeline {pipe}")
    dy, w2 = xo.dense_conv_dgrad(2, cin, 9, 13, 128, seed=cin)
    dref = xo.conv_dgrad_ref((2, cin, 9, 13), w2, dy)
    assert xo.count_ties(dref) > 0
    dx = C.conv3x3_dgrad(_dev(dy, cuda), _dev(w2, cuda))
    xo.assert_exact(dx, xo.round_bf16(dref), (128, 128), f"conv3x3_dgrad pipeline {pipe}")
    dyw, xw, wref = _wgrad_case(*shape, seed=cin + 1)
    dw = C.conv3x3_wgrad(_dev(dyw, cuda), _dev(xw, cuda), 1, torch.float32)
    xo.assert_exact(dw, wref, None, f"conv3x3_wgrad pipeline {pipe}")


# ------------------------------------------------------------------------------------------ halo kernels
_HALO_SCRIPT = r"""
import sys, torch
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import exact_oracle as xo
from distributed_learning_amd.ops import _ext
C = _ext.require()
CL = torch.channels_last
dev = torch.device("cuda:0")
BF = torch.bfloat16
put = lambda t: t.to(dev, BF).contiguous(memory_format=CL)
bad = []
def check(got, ref, what):
    m = xo.mismatch_report(got, ref, (128, 64), what)
    if m is not None:
        bad.append(m)
        print("MISMATCH " + m)
for N, H, W in [(2, 56, 56), (3, 9, 13), (2, 7, 63), (1, 1, 1)]:
    assert C.halo_conv_eligible(64, 64, W, 1, True) and C.halo_conv_eligible(64, 64, W, 1, False), (N, H, W)
    for regime in ("dense", "norounding"):
        x, w = xo.conv_operands(regime, N, 64, H, W, 64, seed=N + H + W)
        ref = xo.conv_ref(x, w)
        assert regime != "dense" or xo.count_ties(ref) > 0, ("no ties", N, H, W)
        t = torch.full((N * H * W, 64), float("nan"), device=dev, dtype=BF); del t
        y, s = C.conv3x3_fwd(put(x), put(w), 1, True, 0)
        check(y, xo.round_bf16(ref), f"halo fwd {regime} {(N, H, W)}")
        if regime == "norounding":
            check(s.double().sum(0), xo.col_stats(ref), f"halo fwd statistics {(N, H, W)}")
    dy, w = xo.dense_conv_dgrad(N, 64, H, W, 64, seed=H * W)
    ref = xo.conv_dgrad_ref((N, 64, H, W), w, dy)
    assert xo.count_ties(ref) > 0, ("no ties in dx", N, H, W)
    t = torch.full((N * H * W, 64), float("nan"), device=dev, dtype=BF); del t
    check(C.conv3x3_dgrad(put(dy), put(w)), xo.round_bf16(ref), f"halo dgrad {(N, H, W)}")
    D = xo.addend((N, 64, H, W), xo.gen(H))
    check(C.conv3x3_dgrad(put(dy), put(w), put(D)), xo.add_rounded(ref, D), f"halo dgrad + addend {(N, H, W)}")
torch.cuda.synchronize()
print("halo exact ok" if not bad else f"halo exact: {len(bad)} mismatching outputs")
"""


@pytest.mark.parametrize("version", ["1", "2", "3", "1d", "3df"])
def test_conv3x3_halo(cuda, version):
    """64 -> 64 channel halo-tiled kernels, forward (with statistics) and data gradient (with and without addend),
    in a fresh process: DLA_HALO* is read once per process. The child prints one line per mismatch report."""
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, DLA_HALO="2", DLA_HALO_V=version[0], DLA_HALO_DIRECT="1" if "d" in version else "0",
               DLA_HALO_DIRECT_FWD="1" if "f" in version else "0")
    r = subprocess.run([sys.executable, "-c", _HALO_SCRIPT % (os.path.dirname(tests), tests)], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "halo exact ok" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]


@pytest.mark.parametrize("odt", [torch.float32, BF])
@pytest.mark.parametrize("shape", [(3, 17, 23), (1, 7, 9), (2, 56, 56)])
def test_halo_wgrad(cuda, C, shape, odt):
    n, h, w = shape
    dy, x, ref = _wgrad_case(n, 64, h, w, 64, 1, seed=n + h + w)
    C.set_halo_wgrad(1)
    assert C.halo_wgrad_eligible(64, 64, w, 1)
    _poison(cuda, 64, 9 * 64, dtype=odt)
    dw = C.conv3x3_wgrad(_dev(dy, cuda), _dev(x, cuda), 1, odt)
    assert dw.dtype == odt
    xo.assert_exact(dw, ref if odt == torch.float32 else xo.round_bf16(ref), None, "halo conv3x3_wgrad")


# --------------------------------------------------------------------------------------------------- stem
@functools.lru_cache(maxsize=8)
def _stem_case(regime, n, h, w):
    x, wt = xo.conv_operands(regime, n, 3, h, w, 64, seed=n + h + w, k=7, stride=2, pad=3)
    ref = xo.conv_ref(x, wt, 2, 3)
    if regime == "dense":
        assert xo.count_ties(ref) > 0, "dense inputs without rounding ties"
    return x, wt, ref


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("stream", [0, 1])
@pytest.mark.parametrize("shape", [(1, 8, 8), (3, 37, 29), (2, 64, 96)])
def test_stem_fwd(cuda, C, regime, stream, shape):
    from distributed_learning_amd.ops.conv import stem_pack_weight

    x, wt, ref = _stem_case(regime, *shape)
    C.set_stem_stream(stream)
    _poison(cuda, ref.numel() // 64, 64)
    y, st, _ = C.stem_fwd(_dev(x, cuda), stem_pack_weight(wt.to(cuda, BF)), True)
    assert y.shape == ref.shape and y.is_contiguous(memory_format=CL)
    xo.assert_exact(y, xo.round_bf16(ref), (128, 64), f"stem_fwd stream {stream}")
    if regime == "norounding":
        _check_stats(st, ref, f"stem_fwd stream {stream}")


@pytest.mark.parametrize("shape", [(1, 8, 8), (3, 37, 29)])
def test_stem_wgrad(cuda, C, shape):
    from distributed_learning_amd.ops.conv import stem_pack_weight, stem_unpack_grad

    n, h, w = shape
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    xo.check_dense(n * oh * ow)
    g = xo.gen(h + w)
    x, dy = xo.ints((n, 3, h, w), g, -3, 3), xo.ints((n, 64, oh, ow), g, -3, 3)
    wt = xo.ints((64, 3, 7, 7), g, -3, 3)
    ref = xo.conv_wgrad_ref(x, (64, 3, 7, 7), dy, 2, 3)
    xs = C.stem_fwd(_dev(x, cuda), stem_pack_weight(wt.to(cuda, BF)), False)[2]
    _poison(cuda, 64, 256, dtype=torch.float32)
    dwp = C.stem_wgrad(_dev(dy, cuda), xs, h, w, torch.float32)
    xo.assert_exact(stem_unpack_grad(dwp), ref, None, "stem_wgrad")
    pad = dwp.reshape(64, 16, 16)[:, :, 12:]  # the 4 padding channels of the fold carry no gradient
    xo.assert_exact(pad, torch.zeros(pad.shape, dtype=torch.float64), None, "stem_wgrad fold padding")


# ------------------------------------------------------------------------------------------- fp32 kernels
@pytest.mark.parametrize("case", [(3, 20, 9, 11, 36, 3, 1, 1), (4, 192, 28, 28, 64, 1, 0, 1), (4, 3, 64, 64, 64, 7, 3, 2)])
def test_conv_f32(cuda, C, case):
    """Wide-mantissa regime: products of 11-bit operands need 22 bits; at most 3 per sum, so every sum stays under
    2^24 (with the accumulate form's base of up to 2^20 on top)."""
    n, cin, h, w, cout, k, pad, stride = case
    base_max = 1 << 20
    x, wt = xo.wide_conv(n, cin, h, w, cout, seed=sum(case), k=k, extra=base_max)
    ref = xo.conv_ref(x, wt, stride, pad)
    assert float(ref.abs().max()) > 1 << 21  # sums that need more than 21 bits
    dy = xo.wide_sparse_like(ref.shape, seed=cin)
    wref = xo.conv_wgrad_ref(x, wt.shape, dy, stride, pad)
    if cin % 4:  # the stem form: 3 channels -> 4, zero channel and zero weights
        x, wt = F.pad(x, (0, 0, 0, 0, 0, 4 - cin)), F.pad(wt, (0, 0, 0, 0, 0, 4 - cin))
        wref = F.pad(wref, (0, 0, 0, 0, 0, 4 - cin))
    xd = _dev(x, cuda, torch.float32)
    wd = wt.permute(0, 2, 3, 1).contiguous().to(cuda)  # OHWI
    _poison(cuda, *ref.shape, dtype=torch.float32)
    y = C.conv_f32_fwd(xd, wd, pad, stride)
    assert y.is_contiguous(memory_format=CL)
    xo.assert_exact(y, ref, (128, 128), "conv_f32_fwd")
    base = xo.ints(ref.shape, xo.gen(1), -base_max, base_max)
    out = _dev(base, cuda, torch.float32)
    C.conv_f32_fwd(xd, wd, pad, stride, out)
    xo.assert_exact(out, xo.integral(ref + base.double()), (128, 128), "conv_f32_fwd accumulating into out")
    _poison(cuda, cout, k * k * x.shape[1], dtype=torch.float32)
    dw = C.conv_f32_wgrad(_dev(dy, cuda, torch.float32), xd, k, k, pad, stride)  # [Cout, R, S, C]
    xo.assert_exact(dw.permute(0, 3, 1, 2), wref, None, "conv_f32_wgrad")
