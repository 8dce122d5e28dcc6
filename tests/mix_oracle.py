"""Float64 numpy oracle and shared cases of the Mixup / CutMix augmentation tests (test_gpu_augment_mix.py,
test_augment_mix_cpu.py).

Written from the definition in ops/augment.py's ``augment_mix`` docstring, independently of the kernel and of the
torch CPU path; ``A(j)``, the sources and the geometries come from augment_oracle.py. Each implementation is
compared with this oracle, never one with the other. For output ``(n, oy, ox, c)`` with ``p = partner[n]``::

    w   = 0 if y0 <= oy < y1 and x0 <= ox < x1 else lam[n]        (output coordinates)
    out = fmaf(w, A(n), (1 - w) * A(p))                            each image with its OWN geom and flip

The cases are functions of ``run(src, geom, flip, partner, lam, box, out_hw, dtype, pad, blend) -> out`` so that
both test files drive the same parameters.
"""
import numpy as np
import torch

import augment_oracle as ao

MIX_TOL = 2.0 ** -21  # two half-ulp roundings at magnitude below 4 plus the rounding of 1 - w (see check_mixup_int)

# five samples: partner has a fixed point (1), a 2-cycle (2 <-> 3), and sample 0 and the last sample point at each
# other; the flips of every pair differ
PARTNER5 = (4, 1, 3, 2, 0)
FLIP5 = (1, 1, 0, 1, 0)
INT_INSIDE5 = (ao.INT_INSIDE[0], ao.INT_INSIDE[1], ao.INT_INSIDE[2], ao.INT_INSIDE[1], ao.INT_INSIDE[2])
INT_PAD4_5 = (ao.INT_PAD4[0], ao.INT_PAD4[1], ao.INT_PAD4[2], ao.INT_PAD4[1], ao.INT_PAD4[2])
HO, WO = ao.INT_HW
# full image (sample 0 takes all of the last image: its last pixel is the source tensor's last three bytes), the
# single pixels (0, 0) and (Ho-1, Wo-1), empty, and an interior box whose edges fall inside 16-byte groups (element
# (2 * 9 + 3) * 3 = 63) on the last sample, which keeps its own bottom-right corner
BOXES5 = ((0, 0, HO, WO), (0, 0, 1, 1), (HO - 1, WO - 1, HO, WO), (3, 3, 3, 7), (2, 3, 5, 7))
LAMS = ((0.0, 1.0, 0.5, 0.25, 0.9), (2.0 ** -20, 0.3137, 0.5, 1.0, 0.0))
EXACT_LAMS = (0.0, 1.0, 0.5)


def tensors(partner, lam, box):
    """The host tensors ``augment_mix`` takes."""
    return (torch.tensor(partner, dtype=torch.int32), torch.tensor(lam, dtype=torch.float32),
            torch.tensor(box, dtype=torch.int32).reshape(-1, 4))


def weights(lam, box, out_hw) -> np.ndarray:
    """``w`` as float64 [N, Ho, Wo, 1] from the fp32 ``lam`` values."""
    ho, wo = out_hw
    lam64 = np.asarray(lam, np.float32).astype(np.float64)
    w = np.empty((len(lam64), ho, wo, 1), np.float64)
    for n, (y0, x0, y1, x1) in enumerate(box):
        w[n] = lam64[n]
        w[n, y0:y1, x0:x1] = 0.0
    return w


def mix(a: np.ndarray, partner, lam, box) -> np.ndarray:
    """The definition in float64 from ``A`` [N, Ho, Wo, 3] (float64, or exact fp32 values): float64."""
    a = np.asarray(a, np.float64)
    w = weights(lam, box, a.shape[1:3])
    return w * a + (1.0 - w) * a[list(partner)]


def is_exact_sum(x: np.ndarray, y: np.ndarray) -> bool:
    """Whether the float64 sum x + y was exact everywhere (Knuth's TwoSum error term is zero)."""
    s = x + y
    bb = s - x
    err = (x - (s - bb)) + (y - bb)
    return bool((err == 0).all())


def bf16_round(x64: np.ndarray) -> np.ndarray:
    """float64 -> the bf16 value nearest the fp32 rounding of x, as float64 (x finite)."""
    bits = ao.bf16_bits(x64.astype(np.float32)).astype(np.uint32) << 16
    return bits.view(np.float32).astype(np.float64)


def assert_within(out: torch.Tensor, want64: np.ndarray, tol: float = MIX_TOL) -> float:
    """fp32: |out - oracle| <= tol. bf16: out is the rounding of some value in [oracle - tol, oracle + tol];
    rounding is monotonic, so that is round(oracle - tol) <= out <= round(oracle + tol)."""
    got = ao.dense(out).cpu().to(torch.float64).numpy()
    err = float(np.abs(got - want64).max())
    print(f"augment_mix {out.dtype}: max |out - oracle| {err:.3e} (tol {tol:.3e})")
    if out.dtype == torch.bfloat16:
        # tol is a multiple of 2^-21 and the oracle has far fewer than 53 bits: oracle +- tol is exact in float64
        # and its fp32 rounding followed by the bf16 rounding stays monotonic
        lo, hi = bf16_round(want64 - tol), bf16_round(want64 + tol)
        bad = int(((got < lo) | (got > hi)).sum())
        assert bad == 0, f"{bad} bf16 elements are no rounding of a value within {tol:.3e} of the oracle"
    else:
        assert err <= tol, f"max |out - oracle| {err:.3e} exceeds {tol:.3e}"
    return err


def assert_same_bits(a: torch.Tensor, b: torch.Tensor, what: str = "") -> None:
    bad = int((ao.bits_of(a) != ao.bits_of(b)).sum())
    assert bad == 0, f"{what}: {bad} elements differ bitwise"


# --- shared cases ----------------------------------------------------------------------------------
def check_identity(run, plain, src, dtype):
    """lam = 1 and an empty box: both forms equal the plain augmentation bit for bit, whatever the partner."""
    cases = ((ao.int_geom(INT_INSIDE5), FLIP5, ao.INT_HW, 0), (ao.interp_geom(), ao.INTERP_FLIP, ao.INTERP_HW, 0))
    for geom, flip, hw, pad in cases:
        partner, lam, box = tensors(PARTNER5, (1.0,) * 5, ((0, 0, 0, 0), (3, 3, 3, 3), (2, 5, 2, 9), (7, 9, 7, 9),
                                                          (0, 4, 6, 4)))
        want = plain(src[:5], geom, flip, hw, dtype, pad)
        for blend in (False, True):
            out = run(src[:5], geom, flip, partner, lam, box, hw, dtype, pad, blend)
            assert out.shape == want.shape and out.dtype == dtype
            assert_same_bits(out, want, f"identity, blend={blend}")


def check_cutmix_int(run, src, offsets, pad, dtype):
    """CutMix on integer geometry: every output is one exact fmaf taken from n or p."""
    s = src[:5]
    a = ao.expected_int(s.cpu(), offsets, FLIP5, ao.INT_HW, pad)
    want = mix(a, PARTNER5, (1.0,) * 5, BOXES5)
    assert np.array_equal(want, want.astype(np.float32))  # w in {0, 1}: a selection, exact
    assert (want[0] == a[4]).all() and (want[3] == a[3]).all() and (want[1] == a[1]).all()
    assert (want[4, 2:5, 3:7] == a[0, 2:5, 3:7]).all() and (want[4, -1, -1] == a[4, -1, -1]).all()
    if pad == 0:  # the boxes do move pixels
        assert (want[2, -1, -1] != a[2, -1, -1]).any() and (want[4, 2:5, 3:7] != a[4, 2:5, 3:7]).any()
    partner, lam, box = tensors(PARTNER5, (1.0,) * 5, BOXES5)
    outs = [run(s, ao.int_geom(offsets), FLIP5, partner, lam, box, ao.INT_HW, dtype, pad, b) for b in (False, True)]
    for out in outs:
        assert out.shape == (5, 3) + ao.INT_HW and out.dtype == dtype
        ao.assert_bitwise(out, want.astype(np.float32))
    assert_same_bits(outs[0], outs[1], "select vs blend")


def check_mixup_int(run, src, lams, dtype):
    """Mixup on integer geometry. lam in {0, 1, 0.5} is bitwise: for 0.5 both products are exact and the sum rounds
    once. Otherwise |out - oracle| <= 2^-21: |A| < 2.7, so w * a and (1 - w) * b are below 4 and each of the two
    roundings (the product (1 - w) * b, the fmaf) is at most half an ulp of [2, 4), 2^-23 = 1.2e-7; the fp32
    rounding of 1 - w is at most 2^-25, times |b| < 2.7: 8e-8. Sum 3.2e-7 < 2^-21 = 4.8e-7."""
    s = src[:5]
    a = ao.expected_int(s.cpu(), INT_INSIDE5, FLIP5, ao.INT_HW, 0)
    assert float(np.abs(a).max()) < 2.7
    boxes = ((0, 0, 0, 0),) * 5
    want = mix(a, PARTNER5, lams, boxes)
    partner, lam, box = tensors(PARTNER5, lams, boxes)
    out = run(s, ao.int_geom(INT_INSIDE5), FLIP5, partner, lam, box, ao.INT_HW, dtype, 0, True)
    assert_within(out, want)
    exact = [i for i, v in enumerate(lams) if v in EXACT_LAMS]
    assert exact and len(exact) < 5
    w = weights(lams, boxes, ao.INT_HW)[exact]
    a64 = a.astype(np.float64)
    assert is_exact_sum(w * a64[exact], (1.0 - w) * a64[[PARTNER5[i] for i in exact]])
    idx = torch.tensor(exact)
    ao.assert_bitwise(out.index_select(0, idx.to(out.device)).contiguous(memory_format=torch.channels_last),
                      want[exact].astype(np.float32))
    # and the mixing did happen: a lam of 0.5 differs from both images
    half = lams.index(0.5)
    assert (want[half] != a64[half]).any() and (want[half] != a64[PARTNER5[half]]).any()


INTERP_LAM = (0.3, 1.0, 0.7, 1.0, 0.55)
INTERP_BOX = ((0, 0, 0, 0), (1, 2, 6, 9), (4, 4, 4, 4), (0, 0, 8, 10), (0, 3, 8, 4))


def check_interpolated(run, src, dtype):
    """Interpolated geometry with Mixup and CutMix parameters on different samples, under the tolerance of
    augment_oracle.assert_close unchanged: a convex combination cannot enlarge that error."""
    s, geom = src[:5], ao.interp_geom()
    a = ao.oracle(s.cpu(), geom, ao.INTERP_FLIP, ao.INTERP_HW, 0)
    want = mix(a, PARTNER5, INTERP_LAM, INTERP_BOX)
    assert float(np.abs(want - a).max()) > 0.5  # the partner's pixels are in there
    partner, lam, box = tensors(PARTNER5, INTERP_LAM, INTERP_BOX)
    out = run(s, geom, ao.INTERP_FLIP, partner, lam, box, ao.INTERP_HW, dtype, 0, True)
    ao.assert_close(out, want)


def check_black_border(run, src):
    """Non-integer boxes reaching into the pad (test_interpolated_over_black_border's), each sample mixed with the
    other: one by Mixup, one by a CutMix box."""
    from distributed_learning_amd.ops.augment import boxes_to_geom

    s = src[:2]
    geom = boxes_to_geom(torch.tensor([-2.5, 10.0]), torch.tensor([-3.25, 12.5]), torch.tensor([12.0, 14.0]),
                         torch.tensor([15.0, 16.5]), ao.INTERP_HW)
    flip = (1, 0)
    a = ao.oracle(s.cpu(), geom, flip, ao.INTERP_HW, 2)
    lams, boxes = (0.4, 1.0), ((0, 0, 0, 0), (2, 1, 6, 7))
    partner, lam, box = tensors((1, 0), lams, boxes)
    out = run(s, geom, flip, partner, lam, box, ao.INTERP_HW, torch.float32, 2, True)
    ao.assert_close(out, mix(a, (1, 0), lams, boxes))


def check_permutation(run, src):
    """Permuting the batch and remapping ``partner`` permutes the output bits."""
    s, geom = src[:5], ao.interp_geom()
    perm = [3, 0, 4, 2, 1]  # new sample i is old sample perm[i]
    inv = [perm.index(i) for i in range(5)]
    partner, lam, box = tensors(PARTNER5, INTERP_LAM, INTERP_BOX)
    out = run(s, geom, ao.INTERP_FLIP, partner, lam, box, ao.INTERP_HW, torch.bfloat16, 0, True)
    partner_p = torch.tensor([inv[PARTNER5[perm[i]]] for i in range(5)], dtype=torch.int32)
    outp = run(s[perm].contiguous(), geom[perm], [ao.INTERP_FLIP[i] for i in perm], partner_p, lam[perm],
               box[perm].contiguous(), ao.INTERP_HW, torch.bfloat16, 0, True)
    assert np.array_equal(ao.bits_of(out)[perm], ao.bits_of(outp))
    assert not np.array_equal(ao.bits_of(out), ao.bits_of(outp))


def check_imagenet_shape(run, device):
    """256^2 -> 224^2 bf16, two images that are each other's partner: a random-resized crop with Mixup within the
    tolerance; the centre crop with a CutMix box bit for bit."""
    from distributed_learning_amd.ops.augment import AugmentParams

    hw = (224, 224)
    s = ao.noise_source(2, 256, 256, seed=11)
    g_rrc, f_rrc = AugmentParams("rrc", (256, 256), hw, seed=3, stream=1).params(5, 1)
    g_c, f_c = AugmentParams("center", (256, 256), hw).params(0, 2)
    assert g_rrc[0, 2:].tolist() != [1.0, 1.0]
    geom, flip = torch.cat([g_rrc, g_c[:1]]), torch.cat([f_rrc, f_c[:1]]).tolist()
    lams, boxes = (0.35, 0.8), ((0, 0, 0, 0), (0, 0, 0, 0))
    partner, lam, box = tensors((1, 0), lams, boxes)
    out = run(s.to(device), geom, flip, partner, lam, box, hw, torch.bfloat16, 0, True)
    assert out.shape == (2, 3, 224, 224)
    ao.assert_close(out, mix(ao.oracle(s, geom, flip, hw, 0), (1, 0), lams, boxes))
    # both images centre-cropped: the box (edges inside 16-byte groups) swaps exact values
    boxes = ((50, 61, 150, 200), (0, 0, 224, 3))
    partner, lam, box = tensors((1, 0), (1.0, 1.0), boxes)
    a = ao.expected_int(s, [(16, 16), (16, 16)], [0, 0], hw, 0)
    want = mix(a, (1, 0), (1.0, 1.0), boxes).astype(np.float32)
    assert (want[0, 50:150, 61:200] == a[1, 50:150, 61:200]).all() and (want[0, 49] == a[0, 49]).all()
    for blend in (False, True):
        ao.assert_bitwise(run(s.to(device), g_c, f_c.tolist(), partner, lam, box, hw, torch.bfloat16, 0, blend), want)


def check_python_guards(run, src):
    """What ``augment_mix`` refuses on host parameters, before anything is computed."""
    import pytest

    s, geom = src[:3], ao.int_geom(ao.INT_INSIDE)
    good = dict(partner=(2, 1, 0), lam=(1.0, 1.0, 1.0), box=((0, 0, 1, 1),) * 3, blend=False)
    bad = {
        "partner == N": dict(partner=(3, 1, 0)),
        "negative partner": dict(partner=(-1, 1, 0)),
        "lam > 1": dict(lam=(1.5, 1.0, 1.0), blend=True),
        "lam < 0": dict(lam=(-0.25, 1.0, 1.0), blend=True),
        "NaN lam": dict(lam=(float("nan"), 1.0, 1.0), blend=True),
        "box past the grid": dict(box=((0, 0, HO + 1, 1),) * 3),
        "box past the grid in x": dict(box=((0, 0, 1, WO + 1),) * 3),
        "negative box": dict(box=((-1, 0, 1, 1),) * 3),
        "y1 < y0": dict(box=((3, 0, 2, 1),) * 3),
        "x1 < x0": dict(box=((0, 4, 1, 3),) * 3),
        "select with lam != 1": dict(lam=(1.0, 0.5, 1.0)),
    }
    for what, change in bad.items():
        a = dict(good)
        a.update(change)
        partner, lam, box = tensors(a["partner"], a["lam"], a["box"])
        with pytest.raises(ValueError):
            run(s, geom, ao.FLIP3, partner, lam, box, ao.INT_HW, torch.float32, 0, a["blend"])
            pytest.fail(f"{what}: accepted")
    partner, lam, box = tensors(good["partner"], good["lam"], good["box"])
    for what, (p, l, b) in {
        "short partner": (partner[:2], lam, box), "short lam": (partner, lam[:2], box),
        "short box": (partner, lam, box[:2]), "box [N, 3]": (partner, lam, box[:, :3]),
        "int64 partner": (partner.long(), lam, box), "float64 lam": (partner, lam.double(), box),
        "int64 box": (partner, lam, box.long()), "float box": (partner, lam, box.float()),
    }.items():
        with pytest.raises((ValueError, TypeError)):
            run(s, geom, ao.FLIP3, p, l, b, ao.INT_HW, torch.float32, 0, False)
            pytest.fail(f"{what}: accepted")
    run(s, geom, ao.FLIP3, partner, lam, box, ao.INT_HW, torch.float32, 0, False)  # the unchanged arguments pass
