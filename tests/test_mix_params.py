"""``MixParams`` (ops/augment.py): the per-batch Mixup / CutMix parameters as a pure function of
(seed, stream, step), their construction, and the distributions they are drawn from."""
import numpy as np
import pytest
import torch

HW = (224, 224)


def _mp(**kw):
    from distributed_learning_amd.ops.augment import MixParams

    a = dict(out_hw=HW, mixup_alpha=0.2, cutmix_alpha=1.0, seed=1234, stream=0)
    a.update(kw)
    return MixParams(**a)


def _same(a, b):
    return all(torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y for x, y in zip(a, b))


def test_pure_function_of_seed_stream_step():
    torch.manual_seed(99)
    np.random.seed(99)
    t_state, n_state = torch.get_rng_state().clone(), np.random.get_state()
    p = _mp()
    a = p.params(7, 16)
    partner, lam, box, target, blend = a
    assert partner.dtype == torch.int32 and partner.shape == (16,)
    assert lam.dtype == torch.float32 and lam.shape == (16,)
    assert box.dtype == torch.int32 and box.shape == (16, 4)
    assert target.dtype == torch.float32 and target.shape == (16,) and isinstance(blend, bool)
    assert all(t.device.type == "cpu" for t in (partner, lam, box, target))
    assert _same(a, p.params(7, 16)) and _same(a, _mp().params(7, 16))
    assert not any(_same(a, p.params(s, 16)) for s in (6, 8, 9))
    assert not _same(a, _mp(seed=1235).params(7, 16)) and not _same(a, _mp(stream=1).params(7, 16))
    assert torch.equal(torch.get_rng_state(), t_state)
    now = np.random.get_state()
    assert now[0] == n_state[0] and np.array_equal(now[1], n_state[1]) and now[2:] == n_state[2:]


def test_crops_and_flips_are_the_same_with_and_without_mixing():
    from distributed_learning_amd.ops.augment import AugmentParams

    ap = AugmentParams("rrc", (256, 256), HW, seed=1234, stream=2)
    before = [ap.params(s, 8) for s in range(4)]
    mp = _mp(stream=2)
    for s in range(4):
        mp.params(s, 8)
        geom, flip = AugmentParams("rrc", (256, 256), HW, seed=1234, stream=2).params(s, 8)
        assert torch.equal(geom, before[s][0]) and torch.equal(flip, before[s][1])
    # and the private generators differ: same seed, stream and step, another stream of numbers
    assert mp._generator(3).initial_seed() != ap._generator(3).initial_seed()


def test_partner_is_a_permutation():
    for step in range(5):
        partner = _mp().params(step, 33)[0]
        assert sorted(partner.tolist()) == list(range(33))
    assert _mp().params(0, 33)[0].tolist() != list(range(33))


def test_mixup_only():
    p = _mp(cutmix_alpha=0.0)
    seen = set()
    for step in range(20):
        partner, lam, box, target, blend = p.params(step, 6)
        assert blend is True
        assert bool((box[:, 0] == box[:, 2]).all()) and bool((box[:, 1] == box[:, 3]).all())  # empty
        assert torch.equal(lam, target) and float(lam.min()) == float(lam.max())
        assert 0.0 <= float(lam[0]) <= 1.0
        seen.add(float(lam[0]))
    assert len(seen) == 20


def test_cutmix_only():
    ho, wo = 32, 48
    p = _mp(out_hw=(ho, wo), mixup_alpha=0.0)
    areas = set()
    for step in range(50):
        partner, lam, box, target, blend = p.params(step, 6)
        assert blend is False and bool((lam == 1).all())
        assert bool((box == box[0]).all())
        y0, x0, y1, x1 = box[0].tolist()
        assert 0 <= y0 <= y1 <= ho and 0 <= x0 <= x1 <= wo
        want = torch.tensor(1.0 - (y1 - y0) * (x1 - x0) / (ho * wo), dtype=torch.float64).to(torch.float32)
        assert bool((target == want).all())
        # the usual construction: int(size * sqrt(1 - lam0)) around a centre on the grid, clipped
        cut, lam0 = p.draw(step)
        assert cut is True
        r = np.sqrt(1.0 - lam0)
        assert y1 - y0 <= int(ho * r) and x1 - x0 <= int(wo * r)
        areas.add((y1 - y0) * (x1 - x0))
    assert len(areas) > 10 and max(areas) > 0


@pytest.mark.parametrize("alpha", [0.2, 0.4, 1.0])
def test_lam0_is_beta_distributed(alpha):
    """20,000 batch draws: the mean within 0.015 of 0.5 (5 standard errors at alpha = 0.2) and the variance within
    5 % of Beta(alpha, alpha)'s 1 / (4 (2 alpha + 1))."""
    p = _mp(mixup_alpha=alpha, cutmix_alpha=0.0)
    lam0 = np.array([p.draw(step)[1] for step in range(20000)])
    assert lam0.min() >= 0.0 and lam0.max() <= 1.0
    var = 1.0 / (4.0 * (2.0 * alpha + 1.0))
    print(f"alpha {alpha}: mean {lam0.mean():.4f}, variance {lam0.var():.4f} (Beta: 0.5, {var:.4f})")
    assert abs(lam0.mean() - 0.5) <= 0.015
    assert abs(lam0.var() - var) <= 0.05 * var


@pytest.mark.parametrize("switch_prob", [0.5, 0.2])
def test_switch_probability(switch_prob):
    """Both alphas set: the CutMix share over 2,000 steps within 0.056 of switch_prob (5 standard errors at 0.5)."""
    p = _mp(switch_prob=switch_prob)
    share = np.mean([p.draw(step)[0] for step in range(2000)])
    print(f"CutMix share {share:.4f} at switch_prob {switch_prob}")
    assert abs(share - switch_prob) <= 0.056
    # the mode decides the form of the whole batch
    for step in range(10):
        cut = p.draw(step)[0]
        partner, lam, box, target, blend = p.params(step, 4)
        assert blend is (not cut) and bool((lam == 1).all()) is cut
    assert all(_mp(switch_prob=1.0).draw(s)[0] for s in range(20))
    assert not any(_mp(switch_prob=0.0).draw(s)[0] for s in range(20))


def test_argument_checks():
    for kw in (dict(mixup_alpha=-0.1), dict(cutmix_alpha=-1.0), dict(mixup_alpha=0.0, cutmix_alpha=0.0),
               dict(switch_prob=1.5), dict(switch_prob=-0.1), dict(out_hw=(0, 4)), dict(mixup_alpha=float("nan"))):
        with pytest.raises(ValueError):
            _mp(**kw)


def test_params_feed_augment_mix():
    """What params() returns is what augment_mix takes: the CPU path accepts it as it is."""
    import augment_oracle as ao
    from distributed_learning_amd.ops.augment import augment_mix

    src = ao.noise_source(5)
    for p in (_mp(out_hw=ao.INTERP_HW, cutmix_alpha=0.0), _mp(out_hw=ao.INTERP_HW, mixup_alpha=0.0)):
        partner, lam, box, target, blend = p.params(3, 5)
        out = augment_mix(src, ao.interp_geom(), torch.tensor(ao.INTERP_FLIP, dtype=torch.uint8), partner, lam, box,
                          ao.MEAN, ao.STD, ao.INTERP_HW, torch.float32, 0, blend)
        assert out.shape == (5, 3) + ao.INTERP_HW and bool(torch.isfinite(out).all())
