"""``augment(index=)`` and ``augment_mix(index=)`` on the CPU: the torch implementation on ``store[index]``, and the
checks the Python entry points make on the host before anything runs."""
import pytest
import torch

import augment_oracle as ao
import mix_oracle as mo

DTYPES = [torch.float32, torch.bfloat16]
INDEX = (7, 2, 7, 0, 8)


def _u8(v):
    return torch.as_tensor(v, dtype=torch.uint8)


@pytest.fixture(scope="module")
def store():
    return ao.noise_source(9, seed=23)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_indexed_equals_the_call_on_the_gathered_batch(store, dtype):
    from distributed_learning_amd.ops.augment import augment, augment_mix

    idx = torch.tensor(INDEX, dtype=torch.int32)
    batch = store[idx.long()]
    for geom, flip, hw, pad in ((ao.int_geom(mo.INT_PAD4_5), _u8(mo.FLIP5), ao.INT_HW, 4),
                                (ao.interp_geom(), _u8(ao.INTERP_FLIP), ao.INTERP_HW, 0)):
        out = augment(store, geom, flip, ao.MEAN, ao.STD, hw, dtype, pad, index=idx)
        assert out.shape == (5, 3) + hw and out.dtype == dtype
        assert torch.equal(out, augment(batch, geom, flip, ao.MEAN, ao.STD, hw, dtype, pad))
        boxes = mo.BOXES5 if hw == ao.INT_HW else mo.INTERP_BOX
        for lams, blend in (((1.0,) * 5, False), (mo.INTERP_LAM, True)):
            partner, lam, box = mo.tensors(mo.PARTNER5, lams, boxes)
            out = augment_mix(store, geom, flip, partner, lam, box, ao.MEAN, ao.STD, hw, dtype, pad, blend, index=idx)
            want = augment_mix(batch, geom, flip, partner, lam, box, ao.MEAN, ao.STD, hw, dtype, pad, blend)
            assert torch.equal(out, want)
    # integer geometry against the formula, through the index
    out = augment(store, ao.int_geom(mo.INT_INSIDE5), _u8(mo.FLIP5), ao.MEAN, ao.STD, ao.INT_HW, dtype, index=idx)
    ao.assert_bitwise(out.contiguous(memory_format=torch.channels_last),
                      ao.expected_int(batch, mo.INT_INSIDE5, mo.FLIP5, ao.INT_HW, 0))


def test_more_samples_than_rows(store):
    from distributed_learning_amd.ops.augment import augment

    idx = torch.tensor((8, 0, 3, 3, 1, 7, 2, 6, 5, 4, 8, 0), dtype=torch.int32)
    rows = [i % 5 for i in range(12)]
    geom, flip = ao.interp_geom()[rows], _u8([ao.INTERP_FLIP[i] for i in rows])
    out = augment(store, geom, flip, ao.MEAN, ao.STD, ao.INTERP_HW, torch.float32, index=idx)
    assert out.shape[0] == 12
    assert torch.equal(out, augment(store[idx.long()], geom, flip, ao.MEAN, ao.STD, ao.INTERP_HW, torch.float32))


def test_host_index_is_checked(store):
    from distributed_learning_amd.ops.augment import augment, augment_mix

    geom, flip = ao.interp_geom(), _u8(ao.INTERP_FLIP)
    partner, lam, box = mo.tensors(mo.PARTNER5, (1.0,) * 5, mo.INTERP_BOX)
    good = torch.tensor(INDEX, dtype=torch.int32)
    bad = {
        "index == P": torch.tensor((7, 2, 9, 0, 8), dtype=torch.int32),
        "negative index": torch.tensor((7, 2, -1, 0, 8), dtype=torch.int32),
        "int64 index": good.long(),
        "float index": good.float(),
        "two-dimensional index": good.reshape(5, 1),
        "index longer than geom": torch.tensor(INDEX + (1,), dtype=torch.int32),
        "index shorter than geom": good[:4],
    }
    for what, idx in bad.items():
        with pytest.raises((ValueError, TypeError)):
            augment(store, geom, flip, ao.MEAN, ao.STD, ao.INTERP_HW, torch.float32, index=idx)
            pytest.fail(f"{what}: accepted by augment")
        with pytest.raises((ValueError, TypeError)):
            augment_mix(store, geom, flip, partner, lam, box, ao.MEAN, ao.STD, ao.INTERP_HW, torch.float32, 0, False,
                        index=idx)
            pytest.fail(f"{what}: accepted by augment_mix")
    with pytest.raises(ValueError, match=r"index must be in \[0, 9\)"):
        augment(store, geom, flip, ao.MEAN, ao.STD, ao.INTERP_HW, torch.float32, index=bad["index == P"])
    augment(store, geom, flip, ao.MEAN, ao.STD, ao.INTERP_HW, torch.float32, index=good)  # the unchanged call passes


def test_element_limit_is_per_image_not_per_store():
    """A store may hold any number of bytes: the 2^31 limit applies to one image and to the output (checked on
    storage-less tensors, with a device index so that nothing is read)."""
    from distributed_learning_amd.ops.augment import augment
    from distributed_learning_amd.ops.limits import NativeLimitError

    p, n = 21850, 4  # 21850 * 256 * 256 * 3 = 4.30e9 bytes
    big = torch.empty(p, 256, 256, 3, dtype=torch.uint8, device="meta")
    assert big.numel() > 2 ** 32
    geom, flip = torch.empty(n, 4, device="meta"), torch.empty(n, device="meta", dtype=torch.uint8)
    index = torch.empty(n, dtype=torch.int32, device="meta")
    with pytest.raises(NativeLimitError, match="src"):  # the same tensor as a batch is refused ...
        augment(big, torch.empty(p, 4, device="meta"), torch.empty(p, device="meta", dtype=torch.uint8), ao.MEAN,
                ao.STD, (224, 224), torch.bfloat16)
    # ... and as a store it passes: the torch path then runs shape-only on the storage-less tensors
    out = augment(big, geom, flip, ao.MEAN, ao.STD, (224, 224), torch.bfloat16, index=index)
    assert out.shape == (n, 3, 224, 224) and out.dtype == torch.bfloat16
    huge = torch.empty(2, 32768, 32768, 3, dtype=torch.uint8, device="meta")  # one image of 3 * 2^30 bytes
    with pytest.raises(NativeLimitError, match="src"):
        augment(huge, geom, flip, ao.MEAN, ao.STD, (224, 224), torch.bfloat16, index=index)
    many = torch.empty(10923, dtype=torch.int32, device="meta")  # 10923 * 256 * 256 * 3 = 2^31 + 1536 outputs
    with pytest.raises(NativeLimitError, match="out"):
        augment(big, torch.empty(10923, 4, device="meta"), torch.empty(10923, device="meta", dtype=torch.uint8),
                ao.MEAN, ao.STD, (256, 256), torch.bfloat16, index=many)
