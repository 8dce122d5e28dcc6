"""Bucket gather / scatter (PackTable, pack_list: csrc/kernels/multi_tensor.hip) and the elementwise reduce
(reduce_sum_, scale_: csrc/kernels/reduce.hip) on the GPU against references that are derivable bit for bit.

Pack and unpack are one fp32 multiply and one round-to-nearest-even per element, so the expected flat buffer
and the expected tensors are computed on the CPU in exactly that form and compared on the bits (NaN by
position). reduce_sum_ adds in a fixed order -- the destination (or 0), then source 0, 1, ... -- multiplies
by the scale and rounds once; an add followed by a multiply cannot be contracted into an fma, so that too is
derivable bitwise. Everything outside the written ranges must keep its sentinel.

One chunk of the multi-tensor kernels is 4096 elements; the vector path needs a full chunk and 16-byte
aligned addresses, so every case runs once with slots padded to 64 elements and once with slot i shifted by
i elements, which sends full chunks down the scalar path."""
import functools

import pytest
import torch

import list_shapes

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
SENTINEL = 7.0
SCALES = (1.0, 2.0, 1.0 / 3.0)
SPECIALS = [0.0, -0.0, float("inf"), float("-inf"), float("nan")]


def _C():
    from distributed_learning_amd.ops import _ext

    return _ext.require()


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _assert_bitwise(got, want, what=""):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), what
    assert torch.equal(_bits(got)[~nan], _bits(want)[~nan]), what  # the sign of zero included


def _raw(t):
    """The elements of a dense tensor in storage order."""
    return t.permute(0, 2, 3, 1).reshape(-1) if t.dim() == 4 else t.reshape(-1)


def _scaled(x, scale, dtype):
    """One fp32 multiply, one rounding: what every kernel of this file does to an element."""
    return (x.detach().cpu().float() * scale).to(dtype)


def _bucket(dev, dtype, gen, specials):
    ts = [torch.randn(n, generator=gen) for n in (1, 63, 4096, 10000, 5, 4096 + 4)]
    if specials:
        ts[1][:5] = torch.tensor(SPECIALS)       # scalar tail
        ts[2][100:105] = torch.tensor(SPECIALS)  # inside a full chunk
    ts = [t.to(dev, dtype) for t in ts]
    ts.append(torch.randn(8, 16, 3, 3, generator=gen).to(dev, dtype).contiguous(memory_format=torch.channels_last))
    return ts


def _offsets(ts, odd):
    """Slots padded to 64 elements; ``odd``: slot i starts i elements later."""
    offs, o = [], 0
    for i, t in enumerate(ts):
        offs.append(o + (i if odd else 0))
        o += (t.numel() + 63) // 64 * 64 + 64
    return offs, o


def _expected_flat(ts, offs, total, flat_dtype, scale):
    want = torch.full((total,), SENTINEL, dtype=flat_dtype)
    for t, off in zip(ts, offs):
        want[off:off + t.numel()] = _scaled(_raw(t), scale, flat_dtype)
    return want


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("flat_dtype", DTYPES)
@pytest.mark.parametrize("grad_dtype", DTYPES)
def test_pack_table_and_list(cuda, grad_dtype, flat_dtype, odd):
    C = _C()
    for scale in SCALES:
        gen = torch.Generator().manual_seed(1)
        ts = _bucket(cuda, grad_dtype, gen, specials=scale == 1.0)
        offs, total = _offsets(ts, odd)
        if odd:
            assert (offs[3] * ts[3].element_size()) % 16 != 0 and ts[3].numel() > 4096
        want = _expected_flat(ts, offs, total, flat_dtype, scale)
        before = [t.clone() for t in ts]
        by_table = torch.full((total,), SENTINEL, device=cuda, dtype=flat_dtype)
        by_list = by_table.clone()
        table = C.PackTable(ts, offs)
        assert table.total_numel() == offs[-1] + ts[-1].numel()
        table.pack(by_table, scale)
        C.pack_list(ts, offs, by_list, scale)
        _assert_bitwise(by_table, want, f"PackTable.pack scale {scale}")
        _assert_bitwise(by_list, want, f"pack_list scale {scale}")
        for t, b in zip(ts, before):
            _assert_bitwise(t, b, "pack changed a source")


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("flat_dtype", DTYPES)
@pytest.mark.parametrize("grad_dtype", DTYPES)
def test_unpack_table(cuda, grad_dtype, flat_dtype, odd):
    C = _C()
    for scale in SCALES:
        gen = torch.Generator().manual_seed(2)
        ts = _bucket(cuda, grad_dtype, gen, specials=False)
        offs, total = _offsets(ts, odd)
        src = torch.randn(total, generator=gen)
        if scale == 1.0:
            src[offs[1]:offs[1] + 5] = torch.tensor(SPECIALS)
            src[offs[2] + 100:offs[2] + 105] = torch.tensor(SPECIALS)
        flat = src.to(cuda, flat_dtype)
        flat0 = flat.clone()
        bystander = torch.full((4096 + 4,), SENTINEL, device=cuda, dtype=grad_dtype)
        table = C.PackTable(ts, offs)
        table.unpack(flat, scale)
        for t, off in zip(ts, offs):
            _assert_bitwise(_raw(t), _scaled(flat0[off:off + t.numel()], scale, grad_dtype), f"unpack scale {scale}")
        _assert_bitwise(flat, flat0, "unpack changed the flat buffer")
        assert bool((bystander == SENTINEL).all())


def _cycle(dev, dtypes, count, gen, empty=()):
    """count tensors of sizes cycling (5, 4096, 5000) and of dtypes[t]; zero elements at the indices of ``empty``."""
    return [torch.randn(0 if t in empty else (5, 4096, 5000)[t % 3], generator=gen).to(dev, dtypes[t])
            for t in range(count)]


@pytest.mark.parametrize("flat_dtype", DTYPES)
@pytest.mark.parametrize("count,layout", [(33, "fp32"), (70, "bf16"), (70, "runs"), (40, "empties"), (40, "edges")])
def test_pack_list_splits(cuda, count, layout, flat_dtype):
    """More than 32 tensors per list, a dtype that changes twice along the list, zero-element tensors; "edges":
    the list of tests/list_shapes.py."""
    C = _C()
    gen = torch.Generator().manual_seed(count)
    f, b = torch.float32, torch.bfloat16
    dtypes = {"fp32": [f] * count, "bf16": [b] * count, "runs": [f] * 20 + [b] * 35 + [f] * 15,
              "empties": [f] * 10 + [b] * 30, "edges": list_shapes.mixed_dtypes()}[layout]
    empty = (3, 17, 18, 31, 32) if layout == "empties" else ()
    if layout == "edges":
        ts = list_shapes.edge_list(cuda, dtypes, gen)
    else:
        ts = _cycle(cuda, dtypes, count, gen, empty)
    offs, total = _offsets(ts, odd=False)
    flat = torch.full((total,), SENTINEL, device=cuda, dtype=flat_dtype)
    C.pack_list(ts, offs, flat, 1.0 / 3.0)
    _assert_bitwise(flat, _expected_flat(ts, offs, total, flat_dtype, 1.0 / 3.0))


@pytest.mark.parametrize("grad_dtype", DTYPES)
def test_pack_list_bad_slot_late_in_the_list_packs_nothing(cuda, grad_dtype):
    """All slots are checked before the first launch: an out-of-range 36th slot leaves the buffer untouched."""
    C = _C()
    gen = torch.Generator().manual_seed(3)
    ts = _cycle(cuda, [grad_dtype] * 40, 40, gen)
    offs, total = _offsets(ts, odd=False)
    flat = torch.full((total,), SENTINEL, device=cuda)
    bad = list(offs)
    bad[35] = total - ts[35].numel() + 1
    with pytest.raises(RuntimeError, match="out of range"):
        C.pack_list(ts, bad, flat, 2.0)
    torch.cuda.synchronize(cuda)
    assert bool((flat == SENTINEL).all())
    bad[35] = -1
    with pytest.raises(RuntimeError, match="out of range"):
        C.pack_list(ts, bad, flat, 2.0)
    torch.cuda.synchronize(cuda)
    assert bool((flat == SENTINEL).all())
    C.pack_list(ts, offs, flat, 2.0)
    _assert_bitwise(flat, _expected_flat(ts, offs, total, torch.float32, 2.0))


# ---------------------------------------------------------------------------------------------------------
# reduce_sum_ / scale_
# ---------------------------------------------------------------------------------------------------------
BIG = 2048 * 256 * 4 + 5  # past the 2048-block grid cap for fp32: the grid-stride loop runs a second round
REDUCE_NS = (1, 3, 7, 8, 9, 1000, BIG)


@functools.lru_cache(maxsize=None)
def _pool():
    """Nine rows of BIG + 16 normal values, drawn once and never modified: row 0 feeds the destination."""
    return torch.randn(9, BIG + 16, generator=torch.Generator().manual_seed(4))


def _reduce_ref(dst, srcs, accumulate, scale, n):
    """The kernel's order in fp32 on the CPU, and the same sum in float64."""
    acc = dst[:n].float() if accumulate else torch.zeros(n)
    acc64 = acc.double()
    for s in srcs:
        acc = acc + s[:n].float()
        acc64 = acc64 + s[:n].double()
    return (acc * scale).to(dst.dtype), acc64 * scale


def _tol(dtype):  # the tolerance of test_gpu_kernels.py::test_reduce_sum
    return dict(rtol=1e-2, atol=2e-2) if dtype == torch.bfloat16 else dict(rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("nsrc", [0, 1, 3, 8])
@pytest.mark.parametrize("accumulate", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_reduce_sum_bitwise(cuda, dtype, accumulate, nsrc):
    C = _C()
    for n in REDUCE_NS:
        for scale in ((0.25, 1.0 / 3.0) if n <= 1000 else (0.25,)):
            rows = [_pool()[r, :n + (13 if r == 1 else 0)].to(dtype) for r in range(nsrc + 1)]  # source 0 is longer
            guard = torch.full((n + 8,), SENTINEL, device=cuda, dtype=dtype)
            dst = guard[:n]
            dst.copy_(rows[0])
            srcs = [r.to(cuda) for r in rows[1:]]
            C.reduce_sum_(dst, srcs, accumulate, scale)
            want, want64 = _reduce_ref(rows[0], rows[1:], accumulate, scale, n)
            _assert_bitwise(dst, want, f"n {n} scale {scale}")
            torch.testing.assert_close(dst.cpu().double(), want64, **_tol(dtype))
            assert bool((guard[n:] == SENTINEL).all())
            for s, r in zip(srcs, rows[1:]):
                _assert_bitwise(s, r, "a source changed")


def test_reduce_sum_rejects_nine_sources(cuda):
    C = _C()
    dst = torch.ones(16, device=cuda)
    with pytest.raises(RuntimeError, match="at most"):
        C.reduce_sum_(dst, [torch.ones(16, device=cuda) for _ in range(9)], True, 1.0)
    with pytest.raises(RuntimeError, match="shorter"):
        C.reduce_sum_(dst, [torch.ones(15, device=cuda)], True, 1.0)
    torch.cuda.synchronize(cuda)
    assert bool((dst == 1.0).all())


@pytest.mark.parametrize("which", ["dst", "src"])
@pytest.mark.parametrize("accumulate", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_reduce_sum_misaligned(cuda, dtype, accumulate, which):
    """A destination or a source one element past an aligned address: the scalar kernel."""
    C = _C()
    n = 4099
    rows = [_pool()[r, :n].to(dtype) for r in range(3)]
    guard = torch.full((n + 9,), SENTINEL, device=cuda, dtype=dtype)
    lead = 1 if which == "dst" else 0
    dst = guard[lead:lead + n]
    dst.copy_(rows[0])
    holder = torch.full((n + 1,), SENTINEL, device=cuda, dtype=dtype)
    holder[1:] = rows[2].to(cuda)
    srcs = [rows[1].to(cuda), holder[1:] if which == "src" else rows[2].to(cuda)]
    assert (dst.data_ptr() % 16 != 0) == (which == "dst") and (srcs[1].data_ptr() % 16 != 0) == (which == "src")
    C.reduce_sum_(dst, srcs, accumulate, 1.0 / 3.0)
    want, want64 = _reduce_ref(rows[0], rows[1:], accumulate, 1.0 / 3.0, n)
    _assert_bitwise(dst, want)
    torch.testing.assert_close(dst.cpu().double(), want64, **_tol(dtype))
    assert bool((guard[:lead] == SENTINEL).all()) and bool((guard[lead + n:] == SENTINEL).all())
    assert float(holder[0]) == SENTINEL


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_scale_bitwise(cuda, dtype, aligned):
    C = _C()
    lead = 0 if aligned else 1
    for n in (1, 7, 4099):
        for s in (2.0, 1.0 / 3.0):
            src = _pool()[5, :n].to(dtype)
            guard = torch.full((n + 9,), SENTINEL, device=cuda, dtype=dtype)
            t = guard[lead:lead + n]
            t.copy_(src)
            assert (t.data_ptr() % 16 == 0) == aligned
            C.scale_(t, s)
            _assert_bitwise(t, _scaled(src, s, dtype), f"n {n} scale {s}")
            assert bool((guard[:lead] == SENTINEL).all()) and bool((guard[lead + n:] == SENTINEL).all())
