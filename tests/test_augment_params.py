"""AugmentParams: the per-batch crop boxes and flips are a pure function of (seed, stream, step) -- CPU only."""
import pytest
import torch

from distributed_learning_amd.ops.augment import AugmentParams, boxes_to_geom

SRC, OUT = (256, 256), (224, 224)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("kind,pad", [("rrc", 0), ("padcrop", 4)])
def test_params_are_a_pure_function_of_seed_stream_step(kind, pad):
    rng = torch.get_rng_state().clone()
    make = lambda **kw: AugmentParams(kind, SRC, OUT, **{"seed": 1234, "stream": 2, "pad": pad, **kw})  # noqa: E731
    a = make().params(7, 64)
    assert a[0].shape == (64, 4) and a[0].dtype == torch.float32 and a[1].shape == (64,) and a[1].dtype == torch.uint8
    assert _same(a, make().params(7, 64))  # a fresh object, the same draw
    p = make()
    p.params(3, 64)
    assert _same(a, p.params(7, 64))  # no state carried from call to call: a resumed run at batch 7 draws batch 7
    assert not _same(a, make().params(8, 64))
    assert not _same(a, make(stream=3).params(7, 64))
    assert not _same(a, make(seed=1235).params(7, 64))
    assert torch.equal(torch.get_rng_state(), rng)  # nothing drawn from the global stream


def test_rrc_boxes():
    n, smin = 4096, 0.08
    y0, x0, h, w, flip = AugmentParams("rrc", SRC, OUT, seed=5, scale_min=smin).boxes(0, n)
    for t in (y0, x0, h, w):
        assert t.dtype == torch.int64 and t.shape == (n,)
    assert bool(((h >= 1) & (w >= 1) & (y0 >= 0) & (x0 >= 0) & (y0 + h <= 256) & (x0 + w <= 256)).all())
    # h = round(sqrt(area / r)) and w = round(sqrt(area * r)) are each within half a pixel of the real-valued side,
    # so the drawn area lies in [(h - 1/2)(w - 1/2), (h + 1/2)(w + 1/2)] and the drawn ratio in
    # [(w - 1/2) / (h + 1/2), (w + 1/2) / (h - 1/2)]; the draws are area in [smin, 1] * 65536, ratio in [3/4, 4/3]
    hf, wf = h.double(), w.double()
    assert bool(((hf + 0.5) * (wf + 0.5) >= smin * 65536).all())
    assert bool(((hf - 0.5) * (wf - 0.5) <= 65536).all())
    assert bool(((wf - 0.5) / (hf + 0.5) <= 4 / 3).all())
    assert bool(((wf + 0.5) / (hf - 0.5) >= 3 / 4).all())
    # the draws spread over the range rather than sitting at one end
    frac = hf * wf / 65536
    assert float(frac.min()) < 0.15 and float(frac.max()) > 0.9
    assert float((wf / hf).min()) < 0.8 and float((wf / hf).max()) > 1.25
    assert len(set(y0.tolist())) > 50 and len(set(x0.tolist())) > 50
    flips = int(flip.sum())
    assert set(flip.tolist()) == {0, 1} and abs(flips - 2048) <= 192  # 6 sigma of Binomial(4096, 1/2) (sigma 32)
    geom, f2 = AugmentParams("rrc", SRC, OUT, seed=5, scale_min=smin).params(0, n)
    assert torch.equal(f2, flip)
    assert torch.equal(geom, torch.stack([y0.double(), x0.double(), hf / 224, wf / 224], 1).float())


def test_rrc_scale_min_one_is_the_whole_image():
    y0, x0, h, w, _ = AugmentParams("rrc", SRC, OUT, scale_min=1.0).boxes(3, 4096)
    assert bool(((y0 == 0) & (x0 == 0) & (h == 256) & (w == 256)).all())


def test_rrc_fallback_is_the_ratio_clamped_centre_crop():
    # a 40 x 400 source: no attempt with ratio <= 4/3 and area >= 0.9 * 16000 fits (h > 40), so every row falls back
    y0, x0, h, w, _ = AugmentParams("rrc", (40, 400), (32, 32), scale_min=0.9).boxes(0, 256)
    assert bool(((h == 40) & (w == 53) & (y0 == 0) & (x0 == (400 - 53) // 2)).all())


def test_padcrop_offsets():
    y0, x0, h, w, flip = AugmentParams("padcrop", (32, 32), (32, 32), pad=4).boxes(1, 4096)
    assert y0.dtype == torch.int64 and x0.dtype == torch.int64
    assert set(y0.tolist()) == set(range(-4, 5)) and set(x0.tolist()) == set(range(-4, 5))
    assert bool(((h == 32) & (w == 32)).all()) and set(flip.tolist()) == {0, 1}
    geom, _ = AugmentParams("padcrop", (32, 32), (32, 32), pad=4).params(1, 4096)
    assert bool((geom[:, 2:] == 1.0).all()) and torch.equal(geom[:, 0], y0.float())


def test_center_is_the_fixed_box_without_flip():
    for step in (0, 9):
        geom, flip = AugmentParams("center", SRC, OUT, seed=step).params(step, 5)
        assert geom.tolist() == [[16.0, 16.0, 1.0, 1.0]] * 5 and flip.tolist() == [0] * 5


def test_boxes_to_geom_rounds_the_float64_step():
    geom = boxes_to_geom(torch.tensor([3]), torch.tensor([4]), torch.tensor([11]), torch.tensor([13]), (8, 10))
    assert geom.dtype == torch.float32
    assert geom.tolist() == [[3.0, 4.0, 1.375, float(torch.tensor(13 / 10, dtype=torch.float64).float())]]


def test_bad_arguments():
    with pytest.raises(ValueError):
        AugmentParams("mixup", SRC, OUT)
    for smin in (0.0, 1.5):
        with pytest.raises(ValueError):
            AugmentParams("rrc", SRC, OUT, scale_min=smin)
