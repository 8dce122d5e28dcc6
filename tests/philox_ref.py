"""Philox-4x32-10 in vectorised numpy, and the element mappings of csrc/kernels/synthetic.hip on top of it.

Written from the published algorithm (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
and from the mapping the kernel file documents; it shares no code with the package. The generic core is
checked against the published known-answer vectors in tests/test_philox_ref.py (CPU), so a GPU test that
compares the kernels with ``uniform_ref`` / ``randint_ref`` bit for bit pins the round constants, the key
schedule, the 64-bit counter and the element order of the stream."""
import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57   # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85   # key increments (Weyl sequence)
MASK32 = np.uint64(0xFFFFFFFF)
MASK64 = (1 << 64) - 1


def philox4x32_10(ctr, key):
    """``ctr``: four uint32-valued arrays (or ints) of one shape, ``key``: two ints. Returns the four output
    words as uint64 arrays holding 32-bit values."""
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) & MASK32 for w in ctr]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]  # 32 x 32 -> 64 bits: never wraps in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def _stream(count, seed, offset):
    """The kernels' use of the core: counter (ctr_lo, ctr_hi, 0x5eed, 0xda7a) for the 64-bit positions
    ``offset .. offset + count - 1`` (wrapping at 2^64), key (seed_lo, seed_hi)."""
    seed, offset = int(seed) & MASK64, int(offset) & MASK64
    with np.errstate(over="ignore"):
        pos = np.uint64(offset) + np.arange(count, dtype=np.uint64)  # uint64 addition wraps like the kernel's
    fixed = np.full(count, 0x5EED, dtype=np.uint64), np.full(count, 0xDA7A, dtype=np.uint64)
    return philox4x32_10((pos & MASK32, pos >> np.uint64(32), *fixed), (seed & 0xFFFFFFFF, seed >> 32))


def uniform_ref(n, seed, offset, lo=0.0, hi=1.0, dtype=torch.float32):
    """What ``uniform_`` writes into ``n`` elements in storage order: group ``gi`` (stream position
    ``offset + gi``) fills elements ``4 gi .. 4 gi + 3`` with ``lo + (hi - lo) * ((r >> 8) * 2^-24)``, every
    operation in fp32 and unfused, then one round-to-nearest-even to bf16 where asked."""
    groups = (n + 3) // 4
    r = np.stack(_stream(groups, seed, offset), axis=1).reshape(-1)[:n]
    unit = (r >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)  # 24 bits: exact
    lo32, hi32 = np.float32(lo), np.float32(hi)
    v = lo32 + (hi32 - lo32) * unit
    out = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    return out if dtype == torch.float32 else out.to(dtype)


def randint_ref(n, high, seed, offset):
    """What ``randint_`` writes: element ``i`` is ``((r0 << 32) | r1) % high`` of stream position ``offset + i``
    under the key ``seed ^ 0x1abe1``."""
    r = _stream(n, (int(seed) & MASK64) ^ 0x1ABE1, offset)
    x = (r[0] << np.uint64(32)) | r[1]
    return torch.from_numpy((x % np.uint64(high)).astype(np.int64))
