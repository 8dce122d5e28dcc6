"""The torch CPU implementation of the Mixup / CutMix augmentation (ops/augment.py ``augment_mix``) against the
float64 oracle in mix_oracle.py: the cases of tests/test_gpu_augment_mix.py on the CPU path."""
import numpy as np
import pytest
import torch

import augment_oracle as ao
import mix_oracle as mo

DTYPES = [torch.float32, torch.bfloat16]


def _run(src, geom, flip, partner, lam, box, out_hw, dtype, pad=0, blend=True):
    from distributed_learning_amd.ops.augment import augment_mix

    return augment_mix(src, geom, torch.as_tensor(flip, dtype=torch.uint8), partner, lam, box, ao.MEAN, ao.STD,
                       out_hw, dtype, pad, blend)


def _plain(src, geom, flip, out_hw, dtype, pad=0):
    from distributed_learning_amd.ops.augment import augment

    return augment(src, geom, torch.as_tensor(flip, dtype=torch.uint8), ao.MEAN, ao.STD, out_hw, dtype, pad)


@pytest.fixture(scope="module")
def src():
    return ao.noise_source(6)  # shared, never written


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_identity_equals_plain_augment(src, dtype):
    mo.check_identity(_run, _plain, src, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("offsets,pad", [(mo.INT_INSIDE5, 0), (mo.INT_PAD4_5, 4)], ids=["inside", "pad4"])
def test_cutmix_integer_geometry_bitwise(src, offsets, pad, dtype):
    mo.check_cutmix_int(_run, src, offsets, pad, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("lams", mo.LAMS, ids=["lams0", "lams1"])
def test_mixup_integer_geometry(src, lams, dtype):
    mo.check_mixup_int(_run, src, lams, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_interpolated(src, dtype):
    mo.check_interpolated(_run, src, dtype)


def test_interpolated_over_black_border(src):
    mo.check_black_border(_run, src)


def test_sample_permutation(src):
    mo.check_permutation(_run, src)


def test_imagenet_shape():
    mo.check_imagenet_shape(_run, "cpu")


def test_guards(src):
    mo.check_python_guards(_run, src)


def test_oracle_selects_and_blends():
    """The oracle on values small enough to check by hand."""
    a = np.arange(2 * 2 * 2 * 3, dtype=np.float64).reshape(2, 2, 2, 3)
    out = mo.mix(a, (1, 0), (0.25, 1.0), ((0, 0, 0, 0), (0, 1, 2, 2)))
    assert np.array_equal(out[0], 0.25 * a[0] + 0.75 * a[1])
    assert np.array_equal(out[1, :, 0], a[1, :, 0]) and np.array_equal(out[1, :, 1], a[0, :, 1])
    assert mo.is_exact_sum(np.float64(0.5), np.float64(0.25)) and not mo.is_exact_sum(np.float64(1.0), np.float64(2.0 ** -60))
