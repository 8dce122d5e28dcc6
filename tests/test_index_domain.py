"""The index decodes of the native kernels, emulated on the CPU at the edge of their legal domain (no GPU).

Every kernel that turns a flat index into coordinates does it with ``mm::fdiv`` (csrc/include/dla_mfma.h), which is
``floor(n / d)`` only for n < 2^24 AND d < 2^16. The host checks (csrc/nn_bindings.cpp, ops/limits.py) keep every
launch inside that domain; this file emulates each decode chain of the audit table (profiles/index_edges/README.md)
with ``pool_oracle.emu_fdiv``'s arithmetic, vectorised, and compares it with ``divmod``:

* at the legal corners (the widest legal image, the ResNet-50 batch limit, a prime width just below 2^16);
* at the worst-case dividends q d + d - 1 of every divisor below 2^16;
* and, outside the domain (d = 66011, which the bindings accepted before they bounded the divisor), it must come out
  wrong: the emulation is sensitive to the defect the checks exclude.

The chains (kernel source in brackets):

pixel   p -> (n, h, w)       two divisions, by W then H           [conv.hip, stem.hip, gemm_stream.hip, conv_f32.hip]
k       k -> (tap, c)        one division by C, tap -> (kh, kw) by (tap * 11) >> 5               [conv.hip any-C loaders]
k32     k -> (tap, c) -> (r, s)   divisions by C then S                                          [conv_f32.hip]
quad    q -> (n, j, i)       two divisions, by W/2 then H/2 of the folded image   [stem.hip stem_wgrad_bn, bn_act.hip]
halo    q -> pixel or -1     padded position, divisions by W + 2 (q < 2^30) then H + 2          [conv_halo_wgrad.hip]
"""
import time

import numpy as np
import pytest
import torch

import pool_oracle as po
from distributed_learning_amd.ops import limits

U = np.uint64
LIMIT = 1 << 24


# ------------------------------------------------------------------------------------------- the emulation
def vfdiv(n, d):
    """``pool_oracle.emu_fdiv`` on arrays: (umulhi(n, m_lo) + n * m_hi) mod 2^32 >> 8 with m = ceil(2^40 / d).
    n < 2^31 keeps n * m_lo below 2^63."""
    n, d = np.asarray(n, dtype=U), np.asarray(d, dtype=U)
    assert int(n.max(initial=0)) < (1 << 31) and int(d.min(initial=1)) >= 1
    m = ((U(1) << U(40)) + d - U(1)) // d
    m_lo, m_hi = m & U(0xFFFFFFFF), m >> U(32)
    return ((((n * m_lo) >> U(32)) + n * m_hi) & U(0xFFFFFFFF)) >> U(8)


def test_vectorised_emulation_is_emu_fdiv():
    rng = np.random.default_rng(0)
    n = rng.integers(0, 1 << 30, 4000)
    d = rng.integers(1, 1 << 21, 4000)
    n[:8] = [0, 1, 16766793, 16766793, LIMIT - 1, LIMIT - 1, 1048576, (1 << 30) - 1]
    d[:8] = [1, 1, 66011, 65535, 65535, 1, 1048577, 63]
    got = vfdiv(n, d)
    assert [int(v) for v in got] == [po.emu_fdiv(int(a), int(b)) for a, b in zip(n, d)]
    assert po.emu_fdiv(16766793, 66011) == 254 and 16766793 // 66011 == 253  # the pair test_pool_oracle.py pins


def signed(a):
    return np.asarray(a, dtype=U).astype(np.int64)


def emu_pixel(p, H, W):
    """conv.hip / stem.hip / gemm_stream.hip / conv_f32.hip pixel_of: q = p / W, w = p - q W, n = q / H, h = q - n H."""
    q = vfdiv(p, W)
    w = signed(p) - signed(q) * W
    n = vfdiv(q, H)
    return signed(n), signed(q) - signed(n) * H, w


def ref_pixel(p, H, W):
    p = np.asarray(p, dtype=np.int64)
    q, w = np.divmod(p, W)
    n, h = np.divmod(q, H)
    return n, h, w


def emu_k(k, C):
    """conv.hip ImplicitLoader::at: tap = k / C, c = k - tap C, kh = tap * 11 >> 5, kw = tap - 3 kh (tap <= 8)."""
    tap = signed(vfdiv(k, C))
    kh = (tap * 11) >> 5
    return tap, signed(k) - tap * C, kh, tap - 3 * kh


def emu_k32(k, C, S):
    """conv_f32.hip: tap = k / C, c = k - tap C, r = tap / S, s = tap - r S."""
    tap = vfdiv(k, C)
    r = vfdiv(tap, S)
    return signed(k) - signed(tap) * C, signed(r), signed(tap) - signed(r) * S


def emu_halo(q, N, H, W):
    """conv_halo_wgrad.hip padded_pixel: the pixel index of padded position q, -1 for padding."""
    r = vfdiv(q, W + 2)
    wp = signed(q) - signed(r) * (W + 2)
    n = vfdiv(r, H + 2)
    hp = signed(r) - signed(n) * (H + 2)
    pad = (hp < 1) | (hp > H) | (wp < 1) | (wp > W)
    return np.where(pad, -1, (signed(n) * H + hp - 1) * W + wp - 1)


def ref_halo(q, N, H, W):
    q = np.asarray(q, dtype=np.int64)
    r, wp = np.divmod(q, W + 2)
    n, hp = np.divmod(r, H + 2)
    pad = (hp < 1) | (hp > H) | (wp < 1) | (wp > W)
    return np.where(pad, -1, (n * H + hp - 1) * W + wp - 1)


def edge_indices(N, H, W):
    """Every index of the first two and last two image rows of the first and the last image, the rows on both sides
    of the last 8 image boundaries, and a stride-997 sample of everything in between."""
    P = N * H * W
    rows = {0, 1, N * H - 2, N * H - 1, H - 2, H - 1, H, H + 1}
    for b in range(max(1, N - 8), N):
        rows |= {b * H - 2, b * H - 1, b * H, b * H + 1}
    rows = sorted(r for r in rows if 0 <= r < N * H)
    idx = np.concatenate([np.arange(r * W, (r + 1) * W, dtype=np.int64) for r in rows]
                         + [np.arange(0, P, 997, dtype=np.int64), np.array([P - 1], dtype=np.int64)])
    return np.unique(idx)


# (N, H, W) of the decoded image; for the stem that is the folded image, [340, 3, 224, 224] -> [340, 112, 112]
CORNERS = [
    (1, 255, 65535),     # largest legal divisor, 16,711,425 pixels
    (5, 51, 65535),      # the same N * H = 255 rows as 5 images
    (255, 1, 65535),     # H = 1: every row an image boundary
    (1, 65535, 255),     # the tall form: H the largest divisor
    (1337, 112, 112),    # ResNet-50's batch limit at the stage-1 3x3 and the stem output, 2^24 - 5,888 pixels
    (340, 112, 112),     # the stem's 340 x 224 x 224 batch, folded
    (334, 224, 224),     # the most 224 x 224 images that fit (340 x 224 x 224 pixels exceed 2^24)
    (1, 256, 65521),     # a prime width just below 2^16, 16,773,376 pixels
    (1, 251, 65521),     # with a prime height
]


def test_corners_are_legal_and_near_the_limit():
    assert 340 * 224 * 224 >= LIMIT > 334 * 224 * 224
    for N, H, W in CORNERS:
        limits.pixels_ok(N * H * W, "corner")
        limits.divisors_ok({"H": H, "W": W}, "corner")
    assert max(N * H * W for N, H, W in CORNERS) == 1 * 256 * 65521 == LIMIT - 3840
    assert 1337 * 112 * 112 == LIMIT - 5888
    assert max(W for _, _, W in CORNERS) == 65535 == max(H for _, H, _ in CORNERS)


@pytest.mark.parametrize("N,H,W", CORNERS)
def test_pixel_decode_at_the_legal_corners(N, H, W):
    p = edge_indices(N, H, W)
    assert p[-1] == N * H * W - 1 and len(p) >= min(N * H, 4) * W
    got, ref = emu_pixel(p, H, W), ref_pixel(p, H, W)
    for g, r, name in zip(got, ref, "nhw"):
        bad = np.nonzero(g != r)[0]
        assert bad.size == 0, f"{name} of pixel {p[bad[0]]} in [{N}, {H}, {W}]: {g[bad[0]]} != {r[bad[0]]}"


# folded images [N, BH, BW] (even sides, fewer than 2^24 pixels, BH and BW below 65536)
QUAD_CORNERS = [
    (1337, 112, 112), (340, 112, 112),
    (1, 256, 65534),     # the widest even fold: quad width 32767, 16,776,704 pixels
    (1, 65534, 256),     # the tallest
    (1, 254, 66052),     # NOT legal for the kernels (BW >= 65536): the quad divisor 33026 is, and the dividends are
                         # the largest of any row here (254 * 66052 = 2^24 - 8); the decode alone is checked
    (1, 510, 32896),     # 2^24 - 256 pixels, quad image 255 x 16448
]


@pytest.mark.parametrize("N,BH,BW", QUAD_CORNERS)
def test_quad_decode_at_the_legal_corners(N, BH, BW):
    """stem_wgrad_bn / bn_relu_maxpool_bwd walk 2x2 quads of the folded [N, BH, BW] image: divisors BW / 2, BH / 2."""
    assert N * BH * BW < LIMIT and BH % 2 == 0 and BW % 2 == 0 and BW // 2 < 65536 and BH // 2 < 65536
    QH, QW = BH // 2, BW // 2
    q = edge_indices(N, QH, QW)
    got, ref = emu_pixel(q, QH, QW), ref_pixel(q, QH, QW)
    assert all((g == r).all() for g, r in zip(got, ref))


@pytest.mark.parametrize("C", [8, 24, 64, 65528, 65535])
def test_k_decode_of_the_3x3_loaders(C):
    k = np.arange(0, (9 * C + 63) // 64 * 64, dtype=np.int64)  # the padded reduction of the kBK = 64 main loop
    tap, c, kh, kw = emu_k(k, C)
    assert (tap == k // C).all() and (c == k % C).all()
    real = tap < 9
    assert (kh[real] == tap[real] // 3).all() and (kw[real] == tap[real] % 3).all()


@pytest.mark.parametrize("C,R,S", [(4, 3, 3), (4, 7, 7), (192, 1, 1), (65532, 1, 1), (65532, 16, 16), (4, 1, 65535),
                                   (16, 1023, 1023)])
def test_k_decode_of_the_fp32_conv(C, R, S):
    K = R * S * C
    assert K < LIMIT  # conv_f32_supported
    k = np.unique(np.concatenate([np.arange(0, min(K, 4 * C)), np.arange(max(0, K - 4 * C), K), np.arange(0, K, 997)]))
    c, r, s = emu_k32(k, C, S)
    assert (c == k % C).all() and (r == k // C // S).all() and (s == k // C % S).all()


@pytest.mark.parametrize("N,H,W", [(2, 56, 56), (4370, 61, 61), (255, 65533, 1), (1, 65533, 61)])
def test_halo_wgrad_decode_in_its_gate(N, H, W):
    """conv3x3_wgrad takes the halo kernel when W + 2 <= 63, N (H + 2) (W + 2) < 2^30, N (H + 2) < 2^24 and
    H + 2 < 2^16: the first division has a dividend past 2^24 but below 2^24 (W + 2) with a divisor of at most 63
    (test_small_divisors_past_2_to_24), the second is inside both documented bounds."""
    Q = N * (H + 2) * (W + 2)
    assert W + 2 <= 63 and Q < (1 << 30) and N * (H + 2) < LIMIT and H + 2 < 65536 and N * H * W < LIMIT
    q = edge_indices(N, H + 2, W + 2)
    assert (emu_halo(q, N, H, W) == ref_halo(q, N, H, W)).all()


def test_small_divisors_past_2_to_24():
    """The halo kernel's first division has q < N (H + 2) (W + 2) with N (H + 2) < 2^24, that is q < 2^24 d for
    d = W + 2 <= 63. That is exactly as far as the 32-bit sum (umulhi(n, m_lo) + n m_hi) holds: n m / 2^32 < 2^32.
    The quotient is exact there (n d < 2^40 keeps the overshoot below 1 / d); at n = 2^24 d the sum wraps."""
    d = np.arange(1, 64, dtype=np.int64)
    top = np.minimum(LIMIT * d, 1 << 30)
    for back in range(0, 3):
        n = (top // d - 1 - back) * d + d - 1
        assert (n < top).all() and (signed(vfdiv(n, d)) == n // d).all()
    for dd in (3, 58, 63):
        hi = min(LIMIT * dd, 1 << 30)
        n = np.arange(hi - (1 << 20), hi, dtype=np.int64)
        assert (signed(vfdiv(n, np.full_like(n, dd))) == n // dd).all()
    # one step past: [2^23, 64, 1, 1] has 2^23 pixels and 9 * 2^23 padded positions, more than 3 * 2^24
    assert int(vfdiv(np.array([LIMIT * 3]), np.array([3]))[0]) != LIMIT


# ------------------------------------------------------------------------- every divisor, worst dividends
def test_every_legal_divisor_at_its_worst_dividends(capsys):
    """For each d < 2^16 the quotient is most at risk at n = q d + d - 1 (the fraction closest to the next integer)
    with the largest n: the two largest q with n < 2^24, plus the first multiples of d (the exact quotients)."""
    t0 = time.perf_counter()
    d = np.arange(1, 1 << 16, dtype=np.int64)
    qmax = (LIMIT - d) // d  # largest q with q d + d - 1 < 2^24
    checked = 0
    for back in (0, 1):
        q = np.maximum(qmax - back, 0)
        n = q * d + d - 1
        assert (n < LIMIT).all()
        assert (signed(vfdiv(n, d)) == q).all(), f"worst-case dividend, q = qmax - {back}"
        n = (q + 1) * d  # and the exact multiple next to it
        n = np.where(n < LIMIT, n, q * d)
        assert (signed(vfdiv(n, d)) == n // d).all()
        checked += 2 * d.size
    # all worst-case dividends (every q) of the divisors next to 2^16 and of a spread of others
    for dd in list(range(65500, 65536)) + [2, 3, 7, 112, 224, 255, 4099, 32771, 65521]:
        q = np.arange(0, (LIMIT - dd) // dd + 1, dtype=np.int64)
        n = q * dd + dd - 1
        assert (signed(vfdiv(n, np.full_like(n, dd))) == q).all(), dd
        checked += q.size
    dt = time.perf_counter() - t0
    with capsys.disabled():
        print(f"\n[index-domain] {checked} worst-case dividends over every d < 2^16 in {dt:.2f} s")


# ----------------------------------------------------------------------------- outside the domain: wrong
BAD_D = 66011  # 254 * 66011 - 1 = 16,766,793 < 2^24 divides to 254, not 253


def test_pixel_decode_is_wrong_past_the_divisor_bound():
    """[1, 8, 254, 66011] passed every conv3x3 check before the divisor was bounded: its last pixel decodes to image
    1, row 0, column -1 instead of image 0, row 253, column 66010."""
    N, H, W = 1, 254, BAD_D
    p = np.array([N * H * W - 1])
    assert p[0] < LIMIT
    n, h, w = (int(v[0]) for v in emu_pixel(p, H, W))
    assert (n, h, w) == (1, 0, -1) and tuple(int(v[0]) for v in ref_pixel(p, H, W)) == (0, 253, 66010)
    every = edge_indices(N, H, W)
    bad = emu_pixel(every, H, W)[2] != ref_pixel(every, H, W)[2]
    assert 0 < int(bad.sum()) < 1000  # a handful of pixels: no small-geometry test would ever see it
    # the tall form: the second division with d = 66011 (q = 254 d - 1 rows of 1 pixel)
    n, h, w = (int(v[0]) for v in emu_pixel(np.array([254 * BAD_D - 1]), BAD_D, 1))
    assert (n, h) != (253, BAD_D - 1)


def test_quad_decode_is_wrong_past_the_divisor_bound():
    """The stem backward's quads: a folded image [1, 508, 132022] has 254 x 66011 quads."""
    q = np.array([254 * BAD_D - 1])
    got = tuple(int(v[0]) for v in emu_pixel(q, 254, BAD_D))
    assert got != tuple(int(v[0]) for v in ref_pixel(q, 254, BAD_D)) and got[2] == -1


def test_fp32_k_decode_is_wrong_past_the_divisor_bound():
    """conv_f32: K = R S C < 2^24 alone bounds only the dividend. A 16 x 16 kernel over 66011 channels ... is not a
    multiple of 4; the channel count 66012 needs its own pair, found by search over the worst dividends."""
    found = None
    for C in range(65536, 70000, 4):
        q = np.arange(0, (LIMIT - C) // C + 1, dtype=np.int64)
        n = q * C + C - 1
        bad = np.nonzero(signed(vfdiv(n, np.full_like(n, C))) != q)[0]
        if bad.size:
            found = (C, int(n[bad[0]]))
            break
    assert found is not None
    C, k = found
    assert k < LIMIT
    c, r, s = emu_k32(np.array([k]), C, 16)
    assert int(c[0]) != k % C and int(c[0]) == -1  # channel -1 of the next tap
    with pytest.raises(limits.NativeLimitError):
        limits.divisors_ok({"Cin": C}, "fp32 conv")


def test_3x3_k_decode_is_wrong_past_the_divisor_bound():
    """tap = k / C with k < 9 C: wrong once 9 C^2 reaches about 2^40 (C a multiple of 8 as the loaders need)."""
    found = None
    for C in range(1 << 18, 1 << 21, 8):
        k = np.arange(1, 10, dtype=np.int64) * C - 1
        tap = emu_k(k, C)[0]
        if (tap != k // C).any():
            found = C
            break
    assert found is not None and found < (1 << 30)  # a [1, C, 1, 1] bf16 operand of that C spans far less than 2 GiB


def test_halo_wgrad_decode_is_wrong_past_its_gate():
    """A [1, 64, H, 1] input with H + 2 near 2^23 has fewer than 2^24 pixels, yet the second division (by H + 2)
    sends the last real rows of the image to image 1, row < 1: they would be dropped as padding. The gate of the
    halo kernel now requires H + 2 < 2^16 and N (H + 2) < 2^24."""
    wrong = 0
    for H in range((1 << 23) - 40, (1 << 23) - 2):
        q = np.arange((H + 2 - 200) * 3, (H + 2) * 3, dtype=np.int64)
        wrong += int((emu_halo(q, 1, H, 1) != ref_halo(q, 1, H, 1)).sum())
    assert wrong > 0


# ------------------------------------------------------------------------------------- the Python limit helper
class _Conv:
    def __init__(self, k, stride, pad, cin, cout):
        self.kernel_size, self.stride, self.padding = (k, k), (stride, stride), (pad, pad)
        self.dilation, self.groups, self.bias = (1, 1), 1, None
        self.in_channels, self.out_channels = cin, cout
        self.weight = torch.empty(0, dtype=torch.float32)


class _Meta:
    """What the ``supported*`` predicates read of an activation, without its storage (no GPU here, and a
    [1, 8, 254, 66011] tensor is not something a unit test allocates)."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype, self.is_cuda, self.requires_grad = torch.Size(shape), dtype, True, False

    def dim(self):
        return len(self.shape)

    def numel(self):
        return self.shape.numel()

    def element_size(self):
        return torch.empty(0, dtype=self.dtype).element_size()

    def is_contiguous(self, memory_format=None):
        return True

    def data_ptr(self):
        return 0


def test_divisors_ok():
    assert limits.divisors_ok({"H": 255, "W": 65535}, "conv3x3")
    with pytest.raises(limits.NativeLimitError, match=r"conv3x3: W = 66011 >= 65536"):
        limits.divisors_ok({"H": 254, "W": BAD_D}, "conv3x3")
    with pytest.raises(limits.NativeLimitError, match=r"stem conv: folded W = 65536"):
        limits.divisors_ok({"folded H": 1, "folded W": 65536}, "stem conv")
    assert issubclass(limits.NativeLimitError, RuntimeError)


def test_supported_predicates_refuse_the_open_geometry():
    from distributed_learning_amd.ops import conv, conv_f32

    c3 = _Conv(3, 1, 1, 8, 8)
    assert limits.pixels_ok(254 * BAD_D, "conv3x3")  # the pixel bound alone lets it through
    with pytest.raises(limits.NativeLimitError, match="conv3x3: W = 66011"):
        conv.supported3x3(_Meta((1, 8, 254, BAD_D), torch.bfloat16), c3)
    with pytest.raises(limits.NativeLimitError, match="conv3x3: H = 66011"):
        conv.supported3x3(_Meta((1, 8, BAD_D, 254), torch.bfloat16), c3)
    assert conv.supported3x3(_Meta((1, 8, 255, 65535), torch.bfloat16), c3)
    stem = _Conv(7, 2, 3, 3, 64)
    with pytest.raises(limits.NativeLimitError, match="stem conv: folded W = 65536"):
        conv.supported_stem(_Meta((1, 3, 2, 131072), torch.bfloat16), stem)
    assert conv.supported_stem(_Meta((1, 3, 510, 131070), torch.bfloat16), stem)
    f3 = _Conv(3, 1, 1, 8, 8)
    with pytest.raises(limits.NativeLimitError, match="fp32 conv: W = 66011"):
        conv_f32.supported(_Meta((1, 8, 254, BAD_D), torch.float32), f3)
    assert conv_f32.supported(_Meta((1, 4, 255, 65535), torch.float32), _Conv(3, 1, 1, 4, 4))
