"""The augmentation kernel (csrc/kernels/augment.hip) against the float64 numpy oracle in augment_oracle.py.

Sources are uint8 random noise, so a half-pixel, tap or axis error is of order 1. Integer geometry is checked
bit for bit (the blend is one source byte, the result one fmaf); interpolated geometry within the tolerance
derived in augment_oracle.assert_close.
"""
import numpy as np
import pytest
import torch

import augment_oracle as ao

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


def _augment(src, geom, flip, out_hw, dtype, pad=0):
    from distributed_learning_amd.ops.augment import augment

    return augment(src, geom, torch.tensor(flip, dtype=torch.uint8), ao.MEAN, ao.STD, out_hw, dtype, pad)


@pytest.fixture(scope="module")
def src(cuda):
    return ao.noise_source(6).to(cuda)  # shared, never written


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("offsets,pad", [(ao.INT_INSIDE, 0), (ao.INT_PAD4, 4)], ids=["inside", "pad4"])
def test_integer_geometry_bitwise(cuda, src, offsets, pad, dtype):
    s = src[:3]
    out = _augment(s, ao.int_geom(offsets), ao.FLIP3, ao.INT_HW, dtype, pad)
    assert out.shape == (3, 3) + ao.INT_HW and out.dtype == dtype
    assert out.is_contiguous(memory_format=torch.channels_last)
    want = ao.expected_int(s.cpu(), offsets, ao.FLIP3, ao.INT_HW, pad)
    if pad:
        black = ao.scale_bias64()[1].astype(np.float32)  # a border pixel is fmaf(0, scale, bias) = bias
        assert (want[0, 0, 0] == black).all() and (want[2, -1, -1] == black).all()
    ao.assert_bitwise(out, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_interpolated(cuda, src, dtype):
    s, geom = src[:5], ao.interp_geom()
    assert not bool((geom[:, 2:] == geom[:, 2:].round()).all())  # non-integer steps, both directions
    assert float(geom[:, 2:].min()) < 1.0 < float(geom[:, 2:].max())
    out = _augment(s, geom, ao.INTERP_FLIP, ao.INTERP_HW, dtype)
    ao.assert_close(out, ao.oracle(s.cpu(), geom, ao.INTERP_FLIP, ao.INTERP_HW, 0))


def test_interpolated_over_black_border(cuda, src):
    """Non-integer boxes reaching into the pad: blends of source pixels with black, and taps past the pad."""
    from distributed_learning_amd.ops.augment import boxes_to_geom

    s = src[:2]
    geom = boxes_to_geom(torch.tensor([-2.5, 10.0]), torch.tensor([-3.25, 12.5]), torch.tensor([12.0, 14.0]),
                         torch.tensor([15.0, 16.5]), ao.INTERP_HW)
    out = _augment(s, geom, (1, 0), ao.INTERP_HW, torch.float32, pad=2)
    ao.assert_close(out, ao.oracle(s.cpu(), geom, (1, 0), ao.INTERP_HW, 2))


def test_imagenet_shape(cuda):
    """256^2 -> 224^2 bf16 once: a random-resized crop within the tolerance, the centre crop bit for bit."""
    from distributed_learning_amd.ops.augment import AugmentParams

    hw = (224, 224)
    s = ao.noise_source(2, 256, 256, seed=11)
    g_rrc, f_rrc = AugmentParams("rrc", (256, 256), hw, seed=3, stream=1).params(5, 1)
    g_c, f_c = AugmentParams("center", (256, 256), hw).params(0, 1)
    assert g_c.tolist() == [[16.0, 16.0, 1.0, 1.0]] and f_c.tolist() == [0]
    assert g_rrc[0, 2:].tolist() != [1.0, 1.0]
    geom, flip = torch.cat([g_rrc, g_c]), torch.cat([f_rrc, f_c]).tolist()
    out = _augment(s.to(cuda), geom, flip, hw, torch.bfloat16)
    assert out.shape == (2, 3, 224, 224)
    ao.assert_close(out[:1], ao.oracle(s[:1], geom[:1], flip[:1], hw, 0))
    ao.assert_bitwise(out[1:], ao.expected_int(s[1:], [(16, 16)], [0], hw, 0))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_writes_stay_inside_out(cuda, src, dtype):
    """``out`` between two NaN guard rows: one row (30 elements) in front puts its base off 16-byte alignment (the launch
    starts and ends with scalar stores); the guards stay NaN and the inside equals the plain call bit for bit."""
    from distributed_learning_amd.ops import _ext
    from distributed_learning_amd.ops.augment import scale_bias

    C = _ext.require()
    s, geom = src[:5], ao.interp_geom().to(cuda)
    flip = torch.tensor(ao.INTERP_FLIP, dtype=torch.uint8, device=cuda)
    ho, wo = ao.INTERP_HW
    row, n = wo * 3, 5 * ho * wo * 3
    buf = torch.full((row + n + row,), float("nan"), dtype=dtype, device=cuda)
    out = buf[row:row + n].view(5, ho, wo, 3).permute(0, 3, 1, 2)
    assert out.data_ptr() % 16 != 0
    scale, bias = (t.to(cuda) for t in scale_bias(ao.MEAN, ao.STD))
    C.augment_(s, out, geom, flip, scale, bias, 0)
    assert bool(buf[:row].isnan().all()) and bool(buf[-row:].isnan().all())
    assert not bool(buf[row:row + n].isnan().any())
    plain = _augment(s, geom, ao.INTERP_FLIP, ao.INTERP_HW, dtype)
    assert np.array_equal(ao.bits_of(out), ao.bits_of(plain))


def test_samples_are_independent(cuda, src):
    """Each sample's output depends only on its own geom / flip row: a permuted batch gives the permuted output."""
    s, geom = src[:5], ao.interp_geom()
    perm = [3, 0, 4, 2, 1]
    out = _augment(s, geom, ao.INTERP_FLIP, ao.INTERP_HW, torch.bfloat16)
    outp = _augment(s[perm].contiguous(), geom[perm], [ao.INTERP_FLIP[i] for i in perm], ao.INTERP_HW, torch.bfloat16)
    assert np.array_equal(ao.bits_of(out)[perm], ao.bits_of(outp))
    assert not np.array_equal(ao.bits_of(out), ao.bits_of(outp))


def test_guards_raise_before_launch(cuda, src):
    from distributed_learning_amd.ops import _ext
    from distributed_learning_amd.ops.augment import augment, scale_bias

    C = _ext.require()
    s, geom = src[:3], ao.int_geom(ao.INT_INSIDE).to(cuda)
    flip = torch.tensor(ao.FLIP3, dtype=torch.uint8, device=cuda)
    scale, bias = (t.to(cuda) for t in scale_bias(ao.MEAN, ao.STD))
    ho, wo = ao.INT_HW
    out = torch.full((3, ho, wo, 3), float("nan"), device=cuda).permute(0, 3, 1, 2)
    wide = ao.noise_source(3, ao.HS, 2 * ao.WS).to(cuda)
    bad = {
        "float source": dict(src=s.float()),
        "C = 4": dict(src=torch.zeros(3, ao.HS, ao.WS, 4, dtype=torch.uint8, device=cuda)),
        "non-contiguous src": dict(src=wide[:, :, ::2]),
        "NCHW-dense out": dict(out=torch.full((3, 3, ho, wo), float("nan"), device=cuda)),
        "geom of the wrong length": dict(geom=geom[:2].contiguous()),
        "flip of the wrong length": dict(flip=flip[:2].contiguous()),
    }
    for what, change in bad.items():
        args = dict(src=s, out=out, geom=geom, flip=flip, scale=scale, bias=bias, pad=0)
        args.update(change)
        with pytest.raises((RuntimeError, ValueError, TypeError)):
            C.augment_(**args)
            pytest.fail(f"{what}: the binding accepted it")
        torch.cuda.synchronize()
        assert bool(args["out"].isnan().all()), f"{what}: out was written"
    # the Python entry point refuses the same before it allocates or launches
    f8 = torch.tensor(ao.FLIP3, dtype=torch.uint8)
    for kw in (dict(src=s.float()), dict(src=bad["C = 4"]["src"]), dict(src=wide[:, :, ::2]), dict(geom=geom[:2].cpu())):
        a = dict(src=s, geom=geom.cpu(), flip=f8)
        a.update(kw)
        with pytest.raises((RuntimeError, ValueError, TypeError)):
            augment(a["src"], a["geom"], a["flip"], ao.MEAN, ao.STD, ao.INT_HW, torch.float32)
    C.augment_(s, out, geom, flip, scale, bias, 0)  # and the unchanged arguments pass
    ao.assert_bitwise(out, ao.expected_int(s.cpu(), ao.INT_INSIDE, ao.FLIP3, ao.INT_HW, 0))
