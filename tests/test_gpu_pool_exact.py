"""The max-pool and global-average-pool kernels (csrc/kernels/pool.hip) against the exact oracle of pool_oracle.py
(gpu): raw bindings, bf16 and fp32, every comparison bitwise by value (NaN equal to NaN) -- no tolerance anywhere.

Each case runs the forward with and without positions and the backward with an integer gradient and with one that
holds a NaN, a +inf and a -inf, all into poisoned memory (every byte 0xff: NaN in bf16 and fp32, 0xff as a position),
under pool_oracle.check_maxpool -- the assertions test_pool_oracle.py shows to catch each planted fault. The
geometries name the kernel they must reach (REACHES); the 3x3/s1 forward runs as strips of 4, strips of 7 and the
generic kernel; two fp32 cases sit just under 2^24 work items (multiply-shift index decode at its largest dividends)
and one image is 1048577 pixels wide (a divisor outside that decode's domain: hardware division)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import pool_oracle as po
from bn_oracle import pool_out

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF, F32 = torch.bfloat16, torch.float32
DTYPES = [F32, BF]
CASES = po.cases()


def _id(c):
    return "n{}c{}-{}x{}-k{}s{}p{}{}".format(*c[:7], "c" if c[7] else "")


# (k, s, p, ceil) -> (forward kernel K, backward kernel R); 0 = the runtime-loop instantiation
REACHES = {
    (3, 2, 1, False): (3, 2), (3, 2, 0, True): (3, 2),
    (3, 1, 1, False): (3, 3), (3, 1, 0, False): (3, 3),
    (2, 2, 0, False): (2, 1), (2, 2, 0, True): (2, 1), (2, 1, 1, False): (2, 2), (2, 2, 1, True): (2, 1),
    (1, 1, 0, False): (0, 1), (1, 2, 0, False): (0, 1), (2, 3, 0, False): (2, 1),
    (5, 2, 2, False): (0, 3), (4, 3, 1, True): (0, 2),
    (5, 1, 2, False): (0, 0), (7, 2, 3, False): (0, 0), (15, 1, 7, False): (0, 0), (15, 4, 0, True): (0, 0),
}


@pytest.fixture
def C():
    from distributed_learning_amd.ops import _ext

    C = _ext.require()
    yield C
    C.set_pool3_sep(-1)


def _poison(dev, *nbytes):
    """Fill freed blocks of these sizes with 0xff bytes and return their addresses. Allocating and freeing them leaves
    the caching allocator as it was, so the next allocations of the same sizes in the same order get the same
    blocks; every caller asserts that through ``_landed``, so an output that missed its poison fails the test."""
    ts = [torch.full((n,), 0xFF, dtype=torch.uint8, device=dev) for n in nbytes]
    ptrs = [t.data_ptr() for t in ts]
    del ts
    return ptrs


def _landed(ptrs, *outs):
    assert [o.data_ptr() for o in outs] == ptrs[:len(outs)], "an output was not allocated on its poisoned block"


def _esize(dtype):
    return 2 if dtype == BF else 4


def _pair(C, dev, dtype, c):
    """The kernels as check_maxpool's (fwd, bwd)."""
    def fwd(x, need_pos):
        xd = x.to(dev, dtype).contiguous(memory_format=CL)
        n = c.N * c.C * c.OH * c.OW
        ptrs = _poison(dev, n * _esize(dtype), *([n] if need_pos else []))
        y, pos = C.maxpool_fwd(xd, c.k, c.s, c.p, c.ceil, need_pos)
        _landed(ptrs, y, *([pos] if need_pos else []))
        assert y.dtype == dtype and y.is_contiguous(memory_format=CL)
        assert pos is None or pos.is_contiguous(memory_format=CL)
        return y, pos

    def bwd(dy, pos):
        dyd, posd = dy.to(dev, dtype).contiguous(memory_format=CL), pos.to(dev).contiguous(memory_format=CL)
        ptrs = _poison(dev, c.N * c.C * c.H * c.W * _esize(dtype))
        dx = C.maxpool_bwd(dyd, posd, c.H, c.W, c.k, c.s, c.p)
        _landed(ptrs, dx)
        assert dx.dtype == dtype and dx.is_contiguous(memory_format=CL)
        return dx

    return fwd, bwd


def test_poison_reaches_the_next_allocation(cuda):
    """The idiom every case relies on: a freed block is handed to the next allocation of its size, bytes intact."""
    for n in (8 * 5 * 2, 24 * 9 * 7 * 4, 1 << 22):
        ptrs = _poison(cuda, n, n // 2)
        t, u = torch.empty(n, dtype=torch.uint8, device=cuda), torch.empty(n // 2, dtype=torch.uint8, device=cuda)
        _landed(ptrs, t, u)
        assert bool((t == 0xFF).all()) and bool((u == 0xFF).all()), n


def test_geometries_reach_the_kernels_they_name():
    """launch_maxpool_fwd takes K = k for k in {2, 3}, else the runtime window; launch_maxpool_bwd takes
    R = ceil(k / s) in {1, 2, 3}, else the runtime loops. A dispatch change must revisit this table."""
    assert set(REACHES) == set(po.GEOMETRIES)
    for (k, s, p, ceil), (K, R) in REACHES.items():
        assert K == (k if k in (2, 3) else 0) == po.fwd_kernel(k)
        r = (k + s - 1) // s
        assert R == (r if 1 <= r <= 3 else 0) == po.bwd_kernel(k, s)
    assert {K for K, _ in REACHES.values()} == {0, 2, 3} and {R for _, R in REACHES.values()} == {0, 1, 2, 3}
    assert sum(R == 0 for _, R in REACHES.values()) == 4  # the generic backward
    assert max(k * k - 1 for k, _, _, _ in REACHES) == 224  # the largest position byte


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_maxpool_exact(cuda, C, case, dtype):
    c = po.make_case(*case)
    if (c.k, c.s) == (3, 1):
        C.set_pool3_sep(4)
        assert C.pool3_strip_rows() == 4
    work_f, work_b = c.N * c.OH * c.OW * (c.C // 8), c.N * c.H * c.W * (c.C // 8)
    assert C.pool_fast_index(work_f, c.C // 8, c.OW, c.OH) and C.pool_fast_index(work_b, c.C // 8, c.W, c.H)
    po.check_maxpool(c, *_pair(C, cuda, dtype, c), dtype, "maxpool")


S1_CASES = [c for c in CASES if c[4:6] == (3, 1)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", S1_CASES, ids=[_id(c) for c in S1_CASES])
def test_maxpool3s1_variants_agree(cuda, C, case, dtype):
    """Strips of 4 rows, strips of 7 rows and the generic K = 3 kernel: each passes the oracle, and their y and pos
    are identical byte for byte."""
    c = po.make_case(*case)
    outs = []
    for sep in (4, 7, 0):
        C.set_pool3_sep(sep)
        assert C.pool3_strip_rows() == sep
        fwd, bwd = _pair(C, cuda, dtype, c)
        po.check_maxpool(c, fwd, bwd, dtype, f"maxpool 3x3/s1 strips {sep}")
        y, pos = fwd(c.x, True)
        outs.append((y.view(torch.int16 if dtype == BF else torch.int32).cpu(), pos.cpu()))
    for y, pos in outs[1:]:
        assert torch.equal(y, outs[0][0]) and torch.equal(pos, outs[0][1])
    C.set_pool3_sep(-1)
    assert C.pool3_strip_rows() in (0, 4, 7)


# ------------------------------------------------------------------- index decode at the fast path's edge
# k = 2 windows over [1, 24, *, *] fp32 random data against F.max_pool2d on the device, bitwise: 2364 * 2365 * 3 =
# 16772580 work items, 4636 short of 2^24, divisors 3, 2365 (odd) and 2364 -- the largest dividends the multiply-
# shift decode sees with divisors that are no power of two. About index decode, not about ties.
EDGE_H, EDGE_W = 2364, 2365


def test_forward_just_under_2_24_work_items(cuda, C):
    work = EDGE_H * EDGE_W * 3
    assert (1 << 24) - 8192 < work < (1 << 24) and C.pool_fast_index(work, 3, EDGE_W, EDGE_H)
    x = torch.randn(1, 24, EDGE_H + 1, EDGE_W + 1, device=cuda, generator=torch.Generator(device=cuda).manual_seed(1))
    x = x.contiguous(memory_format=CL)
    yr, ir = F.max_pool2d(x, 2, 1, 0, return_indices=True)  # indices: h * W + w of the input plane
    ptrs = _poison(cuda, work * 8 * 4, work * 8)
    y, pos = C.maxpool_fwd(x, 2, 1, 0, False, True)
    _landed(ptrs, y, pos)
    assert tuple(y.shape) == (1, 24, EDGE_H, EDGE_W)
    assert torch.equal(y, yr)
    ky = ir // (EDGE_W + 1) - torch.arange(EDGE_H, device=cuda).view(1, 1, -1, 1)
    kx = ir % (EDGE_W + 1) - torch.arange(EDGE_W, device=cuda).view(1, 1, 1, -1)
    assert torch.equal(pos, (ky * 2 + kx).to(torch.uint8))


def test_backward_just_under_2_24_work_items(cuda, C):
    work = EDGE_H * EDGE_W * 3
    assert C.pool_fast_index(work, 3, EDGE_W, EDGE_H)
    g = torch.Generator(device=cuda).manual_seed(2)
    x = torch.randn(1, 24, EDGE_H, EDGE_W, device=cuda, generator=g).contiguous(memory_format=CL).requires_grad_(True)
    yr = F.max_pool2d(x, 2, 2, 0)
    y, pos = C.maxpool_fwd(x.detach(), 2, 2, 0, False, True)
    assert torch.equal(y, yr.detach())
    dy = torch.randn(yr.shape, device=cuda, generator=g).contiguous(memory_format=CL)
    yr.backward(dy)
    ptrs = _poison(cuda, work * 8 * 4)
    dx = C.maxpool_bwd(dy, pos, EDGE_H, EDGE_W, 2, 2, 0)
    _landed(ptrs, dx)
    assert torch.equal(dx, x.grad)  # windows do not overlap: nothing is summed


# ------------------------------------------------------------------------- a divisor above 2^16
WIDE = 1048577


def _wide_data(dev):
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randint(0, 4, (1, 8, 2, WIDE), device=dev, generator=g).float()
    r = torch.rand(x.shape, device=dev, generator=g)
    x[r < 0.02] = float("nan")
    x[(r >= 0.02) & (r < 0.05)] = float("-inf")
    return x


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("geom", [(3, 1, 1), (2, 2, 0)], ids=["k3s1p1", "k2s2p0"])
def test_wide_image_runs_the_hardware_division_kernels(cuda, C, geom, dtype):
    """[1, 8, 2, 1048577]: 2^21 work items at most, but the width divisor is outside fdiv's domain (its quotient at
    flat pixel 1048576 is 1, not 0: test_pool_oracle.py). The launchers must decode by hardware division; forward and
    backward against the oracle, evaluated on the device."""
    k, s, p = geom
    H, OH, OW = 2, pool_out(2, k, s, p, False), pool_out(WIDE, k, s, p, False)
    x = _wide_data(cuda)
    yr, posr = po.maxpool_ref(x, k, s, p)
    dy = torch.randint(-3, 4, yr.shape, device=cuda, generator=torch.Generator(device=cuda).manual_seed(6)).float()
    dxr = po.maxpool_bwd_ref(dy, posr, H, WIDE, k, s, p, dtype)
    xd, dyd = x.to(dtype).contiguous(memory_format=CL), dy.to(dtype).contiguous(memory_format=CL)
    posd = posr.to(torch.uint8).contiguous(memory_format=CL)
    assert not C.pool_fast_index(H * WIDE, 1, WIDE, H) and not C.pool_fast_index(OH * OW, 1, OW, OH)
    for sep in ((4, 0) if (k, s) == (3, 1) else (4,)):
        C.set_pool3_sep(sep)
        if (k, s) == (3, 1) and sep:
            assert not C.pool_fast_index(OW, 1, OW, 1)  # one strip
        ptrs = _poison(cuda, 8 * OH * OW * _esize(dtype), 8 * OH * OW)
        y, pos = C.maxpool_fwd(xd, k, s, p, False, True)
        _landed(ptrs, y, pos)
        ok = (y.double() == yr.double()) | (torch.isnan(y) & torch.isnan(yr))
        assert tuple(y.shape) == tuple(yr.shape) and bool(ok.all()), f"strips {sep}: {int((~ok).sum())} values differ"
        assert torch.equal(pos, posd), f"strips {sep}: positions differ"
    ptrs = _poison(cuda, 8 * H * WIDE * _esize(dtype))
    dx = C.maxpool_bwd(dyd, posd, H, WIDE, k, s, p)
    _landed(ptrs, dx)
    assert torch.equal(dx.double(), dxr)


# ------------------------------------------------------------------------------ global average pool
@functools.lru_cache(maxsize=None)
def _gap_case(N, Cn, H, W):
    g = po.gen(1000 * N + Cn + 7 * H + W)
    x = torch.randint(-8, 9, (N, Cn, H, W), generator=g).float()
    dy = torch.randint(-8, 9, (N, Cn), generator=g).float()
    return x, dy


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("hw", [(1, 1), (2, 1), (1, 3), (5, 1), (7, 7), (8, 8)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_global_avg_pool_exact(cuda, C, hw, dtype):
    """Integer data in [-8, 8]: the sum is exact in any order, so y = dtype(f32(S * f32(1 / HW))) and
    dx = dtype(f32(dy * f32(1 / HW))) have one correct value each. 1 wave-slice to 4 per block, C = 520: a partial
    second channel block."""
    H, W = hw
    for N in (1, 3):
        for Cn in (8, 512, 520):
            x, dy = _gap_case(N, Cn, H, W)
            xd = x.to(cuda, dtype).contiguous(memory_format=CL)
            ptrs = _poison(cuda, N * Cn * _esize(dtype))
            y = C.gap_fwd(xd)
            _landed(ptrs, y)
            assert y.dtype == dtype and tuple(y.shape) == (N, Cn) and y.is_contiguous()
            po.assert_same(y, po.gap_fwd_ref(x, dtype), f"gap_fwd {(N, Cn, H, W)} {dtype}")
            dyd = dy.to(cuda, dtype)
            ptrs = _poison(cuda, N * Cn * H * W * _esize(dtype))
            dx = C.gap_bwd(dyd, H, W)
            _landed(ptrs, dx)
            assert dx.dtype == dtype and tuple(dx.shape) == (N, Cn, H, W)
            assert dx.stride() == (H * W * Cn, 1, W * Cn, Cn), dx.stride()  # channels_last
            po.assert_same(dx, po.gap_bwd_ref(dy, H, W, dtype), f"gap_bwd {(N, Cn, H, W)} {dtype}")
