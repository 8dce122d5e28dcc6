"""Conditions on the loss oracle itself (tests/loss_oracle.py), on the CPU.

1. The fp32 emulation of the documented formulas, with correctly rounded exp / log standing in for the hardware
   and no fault, meets every criterion on every input of tests/test_gpu_loss_exact.py within a quarter of each
   bound (for a gradient entry: inside the interval built with a quarter of the assumed exp error).
2. Each listed fault, injected alone, fails at least one criterion on at least one of those inputs.
3. Which of the faults the tolerances of tests/test_loss_metrics.py (LOSS_TOL, GRAD_TOL, exact counts) let through
   at that file's own shapes, both dtypes, eps 0 and 0.1: asserted, so the record in
   profiles/loss_oracle/README.md cannot drift.
"""
import functools

import numpy as np
import pytest
import torch

import loss_oracle as lo
from test_loss_metrics import GRAD_TOL, LOSS_TOL, make_case, oracle_counts, oracle_loss_grad
from test_loss_mix import make_mix_case
from test_loss_mix import oracle_loss_grad as mix_oracle_loss_grad

NAMES = lo.case_names()


def test_case_list_covers_the_paths():
    cs = [lo.get_case(n) for n in NAMES if "-metrics-eps0.1" in n]
    for dt in ("f32", "bf16"):
        own = [c for c in cs if c.dt == dt]
        # C = 64 stands in the scalar list but its pitch is a multiple of 16 bytes in both dtypes: 16-byte path
        assert {c.C for c in own if c.vec and c.kind == "sweep"} == set(lo.VEC_C[dt]) | {64}
        assert {c.C for c in own if not c.vec and c.kind == "sweep"} == (set(lo.SCALAR_C[dt]) - {64}) | {2056}
        assert {c.B for c in own if c.kind == "rows"} == set(lo.ROW_COUNTS)
        assert any(c.B * c.C > 2048 * 256 for c in own)
        N = lo.elems(dt)
        big = next(c for c in own if c.kind == "sweep" and c.C == lo.VEC_C[dt][-1])
        assert 0 in big.ta and big.C - 1 in big.ta and all(big.C - N + j in big.ta for j in range(N))
        assert any(256 * N <= t < 512 * N for t in big.ta)  # a target inside a second-trip vector
    assert {c.gout for c in cs} == set(lo.GOUTS)
    assert all(len(lo.get_case(n).x) * lo.get_case(n).C <= 700_000 for n in NAMES)


def test_bf16_rounding_helper():
    g = torch.Generator().manual_seed(0)
    a = torch.cat([torch.randn(4096, generator=g) * 10, torch.tensor([0.0, -0.0, 1.00390625, 1.01171875, 3e38, -3e38])])
    assert np.array_equal(lo.bf16_rne(a.numpy()), a.bfloat16().float().numpy())


@pytest.mark.parametrize("name", NAMES)
def test_emulation_is_within_a_quarter_of_every_bound(name):
    c = lo.get_case(name)
    ratios = lo.check(c, lo.emulate(c), share=0.25)
    assert ratios["lse"] <= 1.0 and ratios["row"] <= 1.0


# One input per fault on which it must fail (any criterion). Every name is an input of the GPU test.
CAUGHT_ON = {
    "drop_uni": "sweep-16x1028-f32-metrics-eps0.1",
    "hot_one": "sweep-16x2056-bf16-metrics-eps0.1",
    "uni_c_minus_1": "sweep-16x1028-f32-metrics-eps0.1",
    "gout_ignored": "sweep-16x1028-f32-metrics-eps0.1",
    "g_over_B": "sweep-16x1028-f32-metrics-eps0.1",
    "expsum_skip_last_vec": "sweep-16x1028-f32-metrics-eps0.1",
    "sum_skip_last_vec": "sweep-16x1028-f32-metrics-eps0.1",
    "rank_skip_last_vec": "sweep-16x2056-bf16-metrics-eps0",
    "second_trip_alias": "sweep-16x1028-f32-mix-eps0.1",
    "batch_sum_256": "rows-257x40-f32-metrics-eps0",
    "target_lane_shift": "sweep-16x2056-bf16-mix-eps0",
    "ignored_not_zeroed": "rows-5x40-bf16-metrics-eps0.1",
    "no_rescale_lane": "structured-12x1028-f32-metrics-eps0",
    "no_rescale_merge": "structured-12x2056-bf16-mix-eps0.1",
    "smooth_at_eps0": "structured-12x1028-f32-metrics-eps0",
    "bf16_truncate": "sweep-16x2056-bf16-metrics-eps0.1",
    "mix_swap_hab": "sweep-16x1028-f32-mix-eps0.1",
    "mix_same_target_not_added": "sweep-16x1028-f32-mix-eps0.1",
    "mix_zero_weight_kept": "structured-12x1028-f32-mix-eps0",
}


@pytest.mark.parametrize("fault", lo.FAULTS)
def test_every_fault_is_caught(fault):
    c = lo.get_case(CAUGHT_ON[fault])
    assert CAUGHT_ON[fault] in NAMES
    fails, _ = lo.criteria(c, lo.emulate(c, fault))
    print(fault, "->", fails)
    assert fails, f"{fault} passes every criterion on {c.name}"
    assert not lo.criteria(c, lo.emulate(c))[0]  # the same input passes without the fault


def test_gout_fault_is_caught_at_every_value_but_one():
    for name in NAMES:
        c = lo.get_case(name)
        if c.kind == "sweep" and c.C == 64 and c.gout != 1.0:
            assert lo.criteria(c, lo.emulate(c, "gout_ignored"))[0], name


# ------------------------------------------------------------------------------------------------- the old tolerances
OLD_SHAPES = [(3, 10), (4, 8), (5, 1000), (129, 4097), (256, 1000)]
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


@functools.lru_cache(maxsize=None)
def _old_case(B, C, dt, pair, eps):
    from types import SimpleNamespace

    if pair == "mix":
        x, ta, tb, lam = make_mix_case(B, C, DT[dt])
        ref, gref, _ = mix_oracle_loss_grad(x, ta, tb, lam, eps)
    else:
        x, ta = make_case(B, C, DT[dt])
        tb = lam = None
        ref, gref = oracle_loss_grad(x, ta, eps)
    c = SimpleNamespace(name=f"old-{B}x{C}-{dt}-{pair}-{eps}", kind="old", pair=pair, dt=dt, B=B, C=C, off=0, eps=eps,
                        k=5, x=x.float().numpy(), ta=ta.numpy(), tb=None if tb is None else tb.numpy(),
                        lam=None if lam is None else lam.numpy(), gout=1.0,
                        vec=(C * (4 if dt == "f32" else 2)) % 16 == 0)
    counts = oracle_counts(x, ta, 5) if pair == "metrics" else None
    return c, float(ref), gref, counts


def _old_tolerances_pass(fault, pair, dt, shapes):
    """True iff the emulation with ``fault`` passes the tolerance checks of the older tests at all of ``shapes``."""
    for B, C in shapes:
        for eps in (0.0, 0.1):
            c, ref, gref, counts = _old_case(B, C, dt, pair, eps)
            out = lo.emulate(c, fault)
            try:
                torch.testing.assert_close(torch.tensor(float(out.mean), dtype=torch.float64),
                                           torch.tensor(ref, dtype=torch.float64), **LOSS_TOL)
                torch.testing.assert_close(torch.from_numpy(out.grad).double(), gref, **GRAD_TOL[DT[dt]])
                if counts is not None:
                    assert out.sums[1:].tolist() == [float(v) for v in counts]
            except AssertionError:
                return False
    return True


# Faults that LOSS_TOL, GRAD_TOL and the exact counts accept at every shape of the older tests (make_case /
# make_mix_case at seed 0, eps 0 and 0.1), per logits dtype. gout is always 1 there, no row count exceeds 256 and no
# 16-byte row has a second trip, so those three cannot show; make_case holds no -inf logit, so the two 0 * inf faults
# do not show under the tolerances either (the older files catch them with dedicated -inf cases).
OLD_TOLERANCES_PASS = {
    "f32": ["gout_ignored", "second_trip_alias", "batch_sum_256", "smooth_at_eps0", "mix_zero_weight_kept"],
    "bf16": ["gout_ignored", "second_trip_alias", "batch_sum_256", "smooth_at_eps0", "bf16_truncate",
             "mix_zero_weight_kept"],
}
# At the training shape (256, 1000) alone, in bf16, more get through: the smoothing term eps / C = 1e-4 times g sits
# far below atol 1e-4, and 254 valid rows of 256 move g by 0.8 % against rtol 2e-2.
OLD_TOLERANCES_PASS_BF16_TRAINING_SHAPE = ["drop_uni", "uni_c_minus_1", "gout_ignored", "g_over_B",
                                           "second_trip_alias", "batch_sum_256", "smooth_at_eps0", "bf16_truncate",
                                           "mix_zero_weight_kept"]


def _passed(dt, shapes):
    return [f for f in lo.FAULTS if not (dt == "f32" and f == "bf16_truncate")  # no effect on fp32 logits
            and _old_tolerances_pass(f, "mix" if f.startswith("mix_") else "metrics", dt, shapes)]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_record_of_what_the_old_tolerances_let_through(dt):
    passed = _passed(dt, OLD_SHAPES)
    print("the old tolerances pass:", passed)
    assert passed == OLD_TOLERANCES_PASS[dt]


def test_record_of_what_the_old_tolerances_let_through_at_the_training_shape():
    passed = _passed("bf16", [(256, 1000)])
    print("the old tolerances pass:", passed)
    assert passed == OLD_TOLERANCES_PASS_BF16_TRAINING_SHAPE
