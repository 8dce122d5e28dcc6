"""The Philox fills (csrc/kernels/synthetic.hip: uniform_, randint_) and SyntheticBatches on the GPU against
tests/philox_ref.py, bit for bit: round constants, key schedule, the 64-bit counter, the element order, the
tail and the ``offset + step * per_step`` position are all pinned, not just the moments of the output.

Sizes: 1, 3, 4, 5 (one group, with and without a tail), 1023 (one block, a tail), and one size past each
kernel's grid cap (4096 blocks of 256 groups of 4 for uniform_, 1024 blocks of 256 for randint_), where the
grid-stride loop runs a second round. Offsets: 0, 12345 and 2^32 - 2, where the counter's high word changes
inside the fill. Seeds: 42 and one with a non-zero high key word."""
import functools

import numpy as np
import pytest
import torch

from philox_ref import randint_ref, uniform_ref

pytestmark = pytest.mark.gpu

OFFSETS = (0, 12345, 2 ** 32 - 2)
SEEDS = (42, 0x123456789ABCDEF0)
UNIFORM_NS = (1, 3, 4, 5, 1023, 4 * 256 * 4096 + 5)
RANDINT_NS = (1, 255, 262144 + 3)


def _C():
    from distributed_learning_amd.ops import _ext

    return _ext.require()


@functools.lru_cache(maxsize=None)
def _uref(n, seed, offset):
    return uniform_ref(n, seed, offset)  # fp32; never modified


def _bits(t):
    return t.cpu().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", UNIFORM_NS)
def test_uniform_bitwise(cuda, dtype, n):
    C = _C()
    for seed in SEEDS:
        for offset in OFFSETS:
            out = torch.full((n + 8,), -7.0, device=cuda, dtype=dtype)
            C.uniform_(out[:n], seed, offset, 0.0, 1.0)  # lo + span * u = u whether fused or not: derivable bitwise
            ref = _uref(n, seed, offset).to(dtype)
            assert torch.equal(_bits(out[:n]), _bits(ref)), (seed, offset)
            assert bool((out[n:] == -7.0).all()), "wrote past the end"


def test_uniform_general_range(cuda):
    """lo = -1, hi = 3. The compiler may contract ``lo + span * u`` into an fma (the kernels are built with
    -ffp-contract=fast) while the reference rounds the product first, so bitwise equality is not derivable in
    general; the two forms differ by at most the rounding of the product, bounded here by 1 ulp of fp32 at the
    value's magnitude."""
    C = _C()
    for n in (1023, 4 * 4096 + 5):
        out = torch.empty(n, device=cuda)
        C.uniform_(out, 42, 12345, -1.0, 3.0)
        ref = uniform_ref(n, 42, 12345, -1.0, 3.0).numpy()
        got = out.cpu().numpy()
        assert got.min() >= -1.0 and got.max() < 3.0
        assert np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= np.spacing(np.abs(ref)))
        outb = torch.empty(n, device=cuda, dtype=torch.bfloat16)
        C.uniform_(outb, 42, 12345, -1.0, 3.0)
        assert torch.equal(_bits(outb), _bits(out.to(torch.bfloat16)))  # the same fp32 value, rounded once


def test_uniform_bf16_range(cuda):
    """The contract: fp32 fills are in [0, 1); bf16 fills are the fp32 stream rounded to nearest, so they are
    in [0, 1] and are exactly 1.0 where the fp32 value is >= 1 - 2^-9 (probability 2^-9 per element)."""
    C = _C()
    n = 1 << 18
    f, b = torch.empty(n, device=cuda), torch.empty(n, device=cuda, dtype=torch.bfloat16)
    C.uniform_(f, 42, 0, 0.0, 1.0)
    C.uniform_(b, 42, 0, 0.0, 1.0)
    ref = _uref(n, 42, 0)
    assert float(f.min()) >= 0.0 and float(f.max()) < 1.0
    assert float(b.float().min()) >= 0.0 and float(b.float().max()) <= 1.0
    ones = ref >= 1.0 - 2.0 ** -9
    assert 256 < int(ones.sum()) < 1024  # 2^18 * 2^-9 = 512 expected
    assert torch.equal(b.cpu().float() == 1.0, ones)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_uniform_stream_algebra(cuda, dtype):
    C = _C()
    n, k, o = 4 * 4096 + 5, 300, 12345
    whole, parts = torch.empty(n, device=cuda, dtype=dtype), torch.empty(n, device=cuda, dtype=dtype)
    C.uniform_(whole, 42, o, 0.0, 1.0)
    C.uniform_(parts[:4 * k], 42, o, 0.0, 1.0)
    C.uniform_(parts[4 * k:], 42, o + k, 0.0, 1.0)
    assert torch.equal(whole, parts)
    per = (n + 3) // 4
    for s in (0, 1, 5):
        step = torch.tensor([s], dtype=torch.long, device=cuda)
        a, b = torch.empty(n, device=cuda, dtype=dtype), torch.empty(n, device=cuda, dtype=dtype)
        C.uniform_(a, 42, o, 0.0, 1.0, step, per)
        C.uniform_(b, 42, o + s * per, 0.0, 1.0)
        assert torch.equal(a, b), s
        assert torch.equal(_bits(a), _bits(_uref(n, 42, o + s * per).to(dtype))), s
        assert int(step) == s  # the fill reads the counter, it does not advance it


@pytest.mark.parametrize("n", RANDINT_NS)
def test_randint_bitwise(cuda, n):
    C = _C()
    for high in (10, 1000, 2 ** 40 + 7):
        for seed in SEEDS:
            for offset in OFFSETS:
                out = torch.full((n + 4,), -1, device=cuda, dtype=torch.long)
                C.randint_(out[:n], high, seed, offset)
                assert torch.equal(out[:n].cpu(), randint_ref(n, high, seed, offset)), (high, seed, offset)
                assert bool((out[n:] == -1).all())
    for s in (0, 1, 5):
        step = torch.tensor([s], dtype=torch.long, device=cuda)
        out = torch.empty(n, device=cuda, dtype=torch.long)
        C.randint_(out, 1000, 42, 12345, step, n)
        assert torch.equal(out.cpu(), randint_ref(n, 1000, 42, 12345 + s * n)), s


def test_randint_rejects_bad_high(cuda):
    C = _C()
    out = torch.zeros(8, device=cuda, dtype=torch.long)
    for high in (0, -5):
        with pytest.raises(RuntimeError, match="high must be positive"):
            C.randint_(out, high, 42, 0)
    assert bool((out == 0).all())


@pytest.mark.parametrize("dtype,channels_last", [(torch.bfloat16, True), (torch.float32, False)])
def test_synthetic_batches_follow_the_stream(cuda, dtype, channels_last):
    from distributed_learning_amd.data import SyntheticBatches

    batch, shape, classes, seed, rank = 3, (3, 5, 7), 1000, 1234, 2
    numel = batch * 3 * 5 * 7
    per_x = (numel + 3) // 4  # 79 groups: the last one is a tail

    def want(s, sd):
        x = uniform_ref(numel, sd, s * per_x, dtype=dtype)
        x = x.view(batch, 5, 7, 3).permute(0, 3, 1, 2) if channels_last else x.view(batch, 3, 5, 7)
        return x, randint_ref(batch, classes, sd, s * batch)

    def check(gen, s, sd):
        x, y = gen.next()
        assert x.shape == (batch, 3, 5, 7) and x.dtype == dtype
        assert x.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
        wx, wy = want(s, sd)
        assert torch.equal(x.cpu(), wx) and torch.equal(y.cpu(), wy), s

    for device_step in (False, True):
        kw = dict(dtype=dtype, seed=seed, channels_last=channels_last, device_step=device_step)
        gen = SyntheticBatches(batch, shape, classes, cuda, rank=rank, **kw)
        for s in range(3):
            check(gen, s, seed + 7919 * rank)
        gen.seek(7)
        check(gen, 7, seed + 7919 * rank)
        check(gen, 8, seed + 7919 * rank)
        same = SyntheticBatches(batch, shape, classes, cuda, rank=rank, identical=True, **kw)
        check(same, 0, seed)
