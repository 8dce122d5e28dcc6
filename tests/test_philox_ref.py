"""tests/philox_ref.py on the CPU: the generic Philox-4x32-10 core against the published known-answer
vectors (Random123's kat_vectors: zeros, all ones, digits of pi), and the stream mapping's own algebra. The
GPU tests (tests/test_gpu_synthetic.py) compare the kernels with this helper bit for bit."""
import numpy as np
import pytest
import torch

from philox_ref import philox4x32_10, randint_ref, uniform_ref

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_known_answers(ctr, key, want):
    got = philox4x32_10(ctr, key)
    assert tuple(int(w[0]) for w in got) == want


def test_vectorised_equals_scalar():
    """Arrays of counters give what the same counters give one at a time (the KAT covers the scalar form)."""
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 1 << 32, size=(4, 50), dtype=np.uint64)
    vec = philox4x32_10(tuple(ctr), (0xA4093822, 0x299F31D0))
    for i in (0, 17, 49):
        one = philox4x32_10(tuple(int(ctr[w, i]) for w in range(4)), (0xA4093822, 0x299F31D0))
        assert [int(w[i]) for w in vec] == [int(w[0]) for w in one]


def test_uniform_ref_mapping():
    a = uniform_ref(23, 42, 5)
    assert a.dtype == torch.float32 and a.shape == (23,)
    assert float(a.min()) >= 0.0 and float(a.max()) < 1.0
    # seekable: elements 8.. of a fill at offset 5 are a fill at offset 7, and a tail repeats no group
    assert torch.equal(a[8:], uniform_ref(15, 42, 7))
    assert len(set(a.tolist())) == 23
    # the counter carries into its high word: position 2^32 follows 2^32 - 1
    b = uniform_ref(16, 42, 2 ** 32 - 2)
    assert torch.equal(b[8:], uniform_ref(8, 42, 2 ** 32))
    assert not torch.equal(b[8:], uniform_ref(8, 42, 0))
    # the high key word matters
    assert not torch.equal(uniform_ref(8, 0x123456789ABCDEF0, 0), uniform_ref(8, 0x9ABCDEF0, 0))
    # bf16 is one rounding of the fp32 value; the largest fp32 draw rounds up to exactly 1
    assert torch.equal(uniform_ref(23, 42, 5, dtype=torch.bfloat16), a.to(torch.bfloat16))
    assert torch.tensor((2 ** 24 - 1) / 2 ** 24, dtype=torch.float32).to(torch.bfloat16) == 1.0
    # affine map in fp32
    c = uniform_ref(23, 42, 5, -1.0, 3.0)
    assert torch.equal(c, a * 4 - 1)  # span 4 scales exactly, so this holds to the bit


def test_randint_ref_mapping():
    y = randint_ref(300, 1000, 7, 3)
    assert y.dtype == torch.int64 and int(y.min()) >= 0 and int(y.max()) < 1000
    assert torch.equal(y[10:], randint_ref(290, 1000, 7, 13))
    big = randint_ref(300, 2 ** 40 + 7, 7, 3)
    assert int(big.max()) >= 2 ** 32 and int(big.max()) < 2 ** 40 + 7  # uses more than one output word
    # written out for one element: the label key is seed ^ 0x1abe1, the value (r0 << 32 | r1) % high
    r = philox4x32_10((3, 0, 0x5EED, 0xDA7A), (7 ^ 0x1ABE1, 0))
    assert int(y[0]) == ((int(r[0][0]) << 32) | int(r[1][0])) % 1000
