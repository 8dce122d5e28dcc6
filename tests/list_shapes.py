"""The tensor list on which every by-value list op (sgd_step_list, the LARS lists, the EMA lists, pack_list) meets
all of its host-side boundaries at once (csrc/include/dla_lists.h cuts such a list into launches of 32):

* 40 tensors: two launches, three where the dtype changes along the list;
* sizes cycling 1, 4095, 4096, 4097 and 2 * 4096 + 3: below, at and above one 4096-element chunk, and a tail after
  two full chunks;
* tensor ``EMPTY`` has zero elements (skipped by every op but the LARS lists, where it keeps its slot);
* tensor ``MISALIGNED`` is a dense 4096-element view one element past an aligned address: a full chunk that fails
  the 16-byte test and takes the scalar path;
* ``mixed_dtypes()`` changes from fp32 to bf16 at tensor ``DTYPE_CHANGE``, part-way through the first launch.
"""
import torch

COUNT = 40
SIZES = (1, 4095, 4096, 4097, 2 * 4096 + 3)
EMPTY, DTYPE_CHANGE, MISALIGNED = 6, 21, 34


def mixed_dtypes():
    return [torch.float32] * DTYPE_CHANGE + [torch.bfloat16] * (COUNT - DTYPE_CHANGE)


def edge_list(dev, dtypes, gen, two_d=False, scale=lambda t: 1.0):
    """The list above with ``scale(t) * randn`` values of dtype ``dtypes[t]`` (one dtype for all when not a list);
    ``two_d``: shapes (1, n), which LARS adapts, instead of (n,)."""
    if not isinstance(dtypes, (list, tuple)):
        dtypes = [dtypes] * COUNT
    out = []
    for t in range(COUNT):
        n = 0 if t == EMPTY else 4096 if t == MISALIGNED else SIZES[t % len(SIZES)]
        x = (torch.randn(n + (t == MISALIGNED), generator=gen) * scale(t)).to(dev, dtypes[t])
        if t == MISALIGNED:
            x = x[1:]
            assert x.data_ptr() % 16 != 0 and x.numel() == 4096
        out.append(x.view(1, n) if two_d else x)
    return out
