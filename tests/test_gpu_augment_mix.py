"""The mixed forms of the augmentation kernel (csrc/kernels/augment.hip, ``augment_mix_``) against the float64 numpy
oracle in mix_oracle.py.

Integer geometry is checked bit for bit wherever the definition is exact (CutMix; Mixup with lam in {0, 1, 0.5})
and within 2^-21 elsewhere; interpolated geometry within the tolerance of augment_oracle.assert_close. 7 x 9 x 3 =
189 elements per image put image boundaries inside 16-byte groups, where the per-image reload of the partner's
parameters can go wrong.
"""
import numpy as np
import pytest
import torch

import augment_oracle as ao
import mix_oracle as mo

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


def _run(src, geom, flip, partner, lam, box, out_hw, dtype, pad=0, blend=True):
    from distributed_learning_amd.ops.augment import augment_mix

    return augment_mix(src, geom, torch.as_tensor(flip, dtype=torch.uint8), partner, lam, box, ao.MEAN, ao.STD,
                       out_hw, dtype, pad, blend)


def _plain(src, geom, flip, out_hw, dtype, pad=0):
    from distributed_learning_amd.ops.augment import augment

    return augment(src, geom, torch.as_tensor(flip, dtype=torch.uint8), ao.MEAN, ao.STD, out_hw, dtype, pad)


@pytest.fixture(scope="module")
def src(cuda):
    return ao.noise_source(6).to(cuda)  # shared, never written


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_identity_equals_plain_augment(cuda, src, dtype):
    mo.check_identity(_run, _plain, src, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("offsets,pad", [(mo.INT_INSIDE5, 0), (mo.INT_PAD4_5, 4)], ids=["inside", "pad4"])
def test_cutmix_integer_geometry_bitwise(cuda, src, offsets, pad, dtype):
    mo.check_cutmix_int(_run, src, offsets, pad, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("lams", mo.LAMS, ids=["lams0", "lams1"])
def test_mixup_integer_geometry(cuda, src, lams, dtype):
    mo.check_mixup_int(_run, src, lams, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_interpolated(cuda, src, dtype):
    mo.check_interpolated(_run, src, dtype)


def test_interpolated_over_black_border(cuda, src):
    mo.check_black_border(_run, src)


def test_sample_permutation(cuda, src):
    mo.check_permutation(_run, src)


def test_imagenet_shape(cuda):
    mo.check_imagenet_shape(_run, cuda)


def _binding_args(cuda, src, dtype=torch.float32):
    from distributed_learning_amd.ops.augment import scale_bias

    geom = ao.interp_geom().to(cuda)
    flip = torch.tensor(ao.INTERP_FLIP, dtype=torch.uint8, device=cuda)
    scale, bias = (t.to(cuda) for t in scale_bias(ao.MEAN, ao.STD))
    # identity parameters: lam = 1 and empty boxes (away from the origin), an arbitrary partner
    partner, lam, box = (t.to(cuda) for t in mo.tensors(mo.PARTNER5, (1.0,) * 5, ((2, 3, 2, 7),) * 5))
    return dict(src=src[:5], geom=geom, flip=flip, partner=partner, lam=lam, box=box, scale=scale, bias=bias, pad=0)


@pytest.mark.parametrize("blend", [False, True], ids=["select", "blend"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_writes_stay_inside_out(cuda, src, dtype, blend):
    """``out`` between two NaN guard rows, its base off 16-byte alignment (the construction of
    test_gpu_augment.py::test_writes_stay_inside_out): the guards stay NaN and, with identity parameters, the
    inside equals the plain call bit for bit."""
    from distributed_learning_amd.ops import _ext

    C = _ext.require()
    ho, wo = ao.INTERP_HW
    row, n = wo * 3, 5 * ho * wo * 3
    buf = torch.full((row + n + row,), float("nan"), dtype=dtype, device=cuda)
    out = buf[row:row + n].view(5, ho, wo, 3).permute(0, 3, 1, 2)
    assert out.data_ptr() % 16 != 0
    C.augment_mix_(out=out, blend=blend, **_binding_args(cuda, src))
    assert bool(buf[:row].isnan().all()) and bool(buf[-row:].isnan().all())
    assert not bool(buf[row:row + n].isnan().any())
    plain = _plain(src[:5], ao.interp_geom(), ao.INTERP_FLIP, ao.INTERP_HW, dtype)
    assert np.array_equal(ao.bits_of(out), ao.bits_of(plain))


def test_guards_raise_before_launch(cuda, src):
    from distributed_learning_amd.ops import _ext

    mo.check_python_guards(_run, src)
    C = _ext.require()
    good = _binding_args(cuda, src)
    ho, wo = ao.INTERP_HW
    out = torch.full((5, ho, wo, 3), float("nan"), device=cuda).permute(0, 3, 1, 2)
    box6 = torch.zeros(6, 4, dtype=torch.int32, device=cuda)
    bad = {
        "host partner": dict(partner=good["partner"].cpu()),
        "host lam": dict(lam=good["lam"].cpu()),
        "host box": dict(box=good["box"].cpu()),
        "short partner": dict(partner=good["partner"][:4].contiguous()),
        "short lam": dict(lam=good["lam"][:4].contiguous()),
        "short box": dict(box=good["box"][:4].contiguous()),
        "int64 partner": dict(partner=good["partner"].long()),
        "float64 lam": dict(lam=good["lam"].double()),
        "float box": dict(box=good["box"].float()),
        "box off 16-byte alignment": dict(box=box6.view(-1)[2:22].view(5, 4)),
        "non-contiguous box": dict(box=torch.zeros(5, 8, dtype=torch.int32, device=cuda)[:, :4]),
        "geom of the wrong length": dict(geom=good["geom"][:4].contiguous()),
        "float source": dict(src=good["src"].float()),
        "NCHW-dense out": dict(out=torch.full((5, 3, ho, wo), float("nan"), device=cuda)),
    }
    assert bad["box off 16-byte alignment"]["box"].data_ptr() % 16 == 8
    for what, change in bad.items():
        for blend in (False, True):
            args = dict(good, out=out, blend=blend)
            args.update(change)
            with pytest.raises((RuntimeError, ValueError, TypeError)):
                C.augment_mix_(**args)
                pytest.fail(f"{what}: the binding accepted it")
            torch.cuda.synchronize()
            assert bool(args["out"].isnan().all()), f"{what}: out was written"
    # the Python entry point's refusals leave nothing behind either: it allocates its own output after the checks
    C.augment_mix_(out=out, blend=False, **good)  # and the unchanged arguments pass
    mo.assert_same_bits(out, _plain(src[:5], ao.interp_geom(), ao.INTERP_FLIP, ao.INTERP_HW, torch.float32),
                        "identity through the binding")
