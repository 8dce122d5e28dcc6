"""CPU self-tests of tests/pool_oracle.py: the oracle against PyTorch and a brute-force loop, the coverage of every
case of test_gpu_pool_exact.py from the oracle alone, the kernel emulation with each planted fault under the very
assertions the GPU test applies, and the multiply-shift division outside its domain."""
import pytest
import torch
import torch.nn.functional as F

import pool_oracle as po
from bn_oracle import pool_out

CASES = po.cases()
IDS = ["n{}c{}-{}x{}-k{}s{}p{}{}".format(*c[:7], "c" if c[7] else "") for c in CASES]


def test_case_list_reaches_every_kernel():
    """Forward K in {2, 3, runtime}, backward R in {1, 2, 3, runtime}, stride > window, the ceil drop rule."""
    assert len(CASES) > 80
    assert {po.fwd_kernel(c[4]) for c in CASES} == {0, 2, 3}
    assert {po.bwd_kernel(c[4], c[5]) for c in CASES} == {0, 1, 2, 3}
    assert any(c[5] > c[4] for c in CASES)
    # (2, 2, 1, ceil) at H = 5, W = 6: the drop rule fires on H only
    assert (5 + 2 - 2 + 1) // 2 + 1 == 4 and pool_out(5, 2, 2, 1, True) == 3
    assert (6 + 2 - 2 + 1) // 2 + 1 == 4 and pool_out(6, 2, 2, 1, True) == 4
    assert any(c[2:] == (5, 6, 2, 2, 1, True) for c in CASES)
    # strips of 4 and of 7 rows: output heights with remainders 0, 1 and k - 1 = 2 among the 3x3/s1 cases
    ohs = {pool_out(c[2], 3, 1, c[6], False) for c in CASES if c[4:6] == (3, 1)}
    assert {o % 4 for o in ohs} >= {0, 1, 2} and {o % 7 for o in ohs} >= {0, 1, 2}
    assert {c[1] // 8 for c in CASES} == {1, 3, 5}


def _finite_distinct(N, C, H, W, seed):
    n = N * C * H * W
    return (torch.randperm(n, generator=po.gen(seed)).float() / 8).reshape(N, C, H, W)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_matches_torch_on_tie_free_data(case):
    N, C, H, W, k, s, p, ceil = case
    x = _finite_distinct(N, C, H, W, 3).requires_grad_(True)
    yr = F.max_pool2d(x, k, s, p, 1, ceil)
    y, pos = po.maxpool_ref(x.detach(), k, s, p, ceil)
    assert torch.equal(y, yr.detach())
    dy = torch.randint(-3, 4, y.shape, generator=po.gen(4)).float()
    yr.backward(dy)
    assert torch.equal(po.maxpool_bwd_ref(dy, pos, H, W, k, s, p), x.grad.double())
    th, tw = po.targets(pos, k, s, p)
    assert bool(((th >= 0) & (th < H) & (tw >= 0) & (tw < W)).all())  # finite data: never a padding tap


def test_oracle_matches_a_brute_force_loop():
    N, C, H, W, k, s, p, ceil = 1, 8, 5, 6, 3, 2, 1, True
    c = po.make_case(N, C, H, W, k, s, p, ceil)
    dx = torch.zeros(N, C, H, W, dtype=torch.float64)
    for n in range(N):
        for ch in range(C):
            for oh in range(c.OH):
                for ow in range(c.OW):
                    best, bq = float("-inf"), 0
                    for q in range(k * k):
                        h, w = oh * s - p + q // k, ow * s - p + q % k
                        if not (0 <= h < H and 0 <= w < W):
                            continue
                        v = float(c.x[n, ch, h, w])
                        if v > best or (v != v and best == best):
                            best, bq = v, q
                    want = float(c.y[n, ch, oh, ow])
                    assert (best != best and want != want) or best == want
                    assert bq == int(c.pos[n, ch, oh, ow])
                    h, w = oh * s - p + bq // k, ow * s - p + bq % k
                    if 0 <= h < H and 0 <= w < W:
                        dx[n, ch, h, w] += float(c.dy[n, ch, oh, ow])
    assert torch.equal(dx, c.dx[torch.float32])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_coverage_holds_and_the_emulation_passes(case):
    """make_case asserts the coverage shares; the fault-free emulation passes every assertion in both dtypes."""
    c = po.make_case(*case)
    assert c.cov.all_neg >= 1
    if c.k == 1:  # the one excuse: a single tap per window, nothing can tie
        assert c.cov.taps == 1 and c.cov.multi_share == 0 and c.cov.tie_share == 0
    else:  # over ALL windows, all -inf windows not counted as tied
        assert c.cov.tie_share >= 0.25 and c.cov.nan2 >= 1 and c.cov.first_not_last >= 1
    for dt in (torch.float32, torch.bfloat16):
        po.check_maxpool(c, *po.emu_pair(c, dt), dt, "emulation")


# fault -> the cases it must be caught at (every one of them), chosen where the fault changes anything
def _applies(fault, c):
    if fault == "no_ceil_drop":
        return c.ceil and (po._out_nodrop(c.H, c.k, c.s, c.p, True) != c.OH or po._out_nodrop(c.W, c.k, c.s, c.p, True) != c.OW)
    if fault == "strip_remainder":
        return c.k == 3 and c.s == 1 and c.OH % po.STRIP != 0
    if fault == "uncovered_unwritten":
        return not bool(c.covered.all())
    if fault == "pad_zero":  # the all -inf window of the padded corner then gives 0
        return c.p > 0
    if fault in ("last_max", "last_nan", "nan_not_sticky", "credit_ties", "mask_multiply"):
        return c.cov.taps >= 2
    return True


@pytest.mark.parametrize("fault", po.FAULTS)
def test_every_fault_is_caught(fault):
    hit = 0
    for case in CASES:
        c = po.make_case(*case)
        if not _applies(fault, c):
            continue
        hit += 1
        with pytest.raises(AssertionError):
            po.check_maxpool(c, *po.emu_pair(c, torch.bfloat16, fault), torch.bfloat16, fault)
    assert hit >= 3, f"{fault}: only {hit} cases can show it"


def test_mask_multiply_is_invisible_to_finite_gradients():
    """Why the second dy exists: with integer dy alone a multiply-by-mask backward equals the select."""
    c = po.make_case(3, 24, 9, 7, 3, 2, 1, False)
    ref_pos = c.pos.to(torch.uint8)
    assert torch.equal(po.emu_bwd(c.dy, ref_pos, c.x, 3, 2, 1, fault="mask_multiply").double(), c.dx[torch.float32])
    leaked = po.emu_bwd(c.dy2, ref_pos, c.x, 3, 2, 1, fault="mask_multiply")
    assert int(torch.isnan(leaked).sum()) > 3


# ------------------------------------------------------------------------------------- global average pool
@pytest.mark.parametrize("hw", [(1, 1), (1, 2), (1, 3), (5, 1), (7, 7), (8, 8)])
def test_gap_oracle(hw):
    H, W = hw
    x = torch.randint(-8, 9, (3, 8, H, W), generator=po.gen(H * W)).float()
    for dt in (torch.float32, torch.bfloat16):
        y = po.gap_fwd_ref(x, dt)
        torch.testing.assert_close(y, x.double().mean((2, 3)), rtol=2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -22, atol=0)
        dy = torch.randint(-8, 9, (3, 8), generator=po.gen(1)).float()
        dx = po.gap_bwd_ref(dy, H, W, dt)
        assert dx.shape == (3, 8, H, W)
        torch.testing.assert_close(dx, (dy.double() / (H * W))[:, :, None, None].expand(-1, -1, H, W),
                                   rtol=2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -22, atol=0)
    if H * W in (1, 2, 64):  # 1 / HW exact: the mean itself
        assert torch.equal(po.gap_fwd_ref(x, torch.float32), x.double().mean((2, 3)))


# ------------------------------------------------------------------------------ multiply-shift division
def test_fdiv_is_exact_inside_its_domain_only():
    """n < 2^24 and d < 2^16: exact at every multiple of d and just below it. d = 65536 is still exact (the bound is
    tight at d <= 2^16); d = 1048577 fails at n = d - 1 -- below 2^24, so `work < 2^24` alone did not protect it."""
    for d in (3, 24, 2365, 65535, 65536):
        for q in range(1, (1 << 24) // d + 1, 1 if d > 1000 else 997):
            for n in (q * d - 1, q * d):
                if n < (1 << 24):
                    assert po.emu_fdiv(n, d) == n // d, (n, d)
        assert po.emu_fdiv((1 << 24) - 1, d) == ((1 << 24) - 1) // d
    # the smallest divisor with a wrong quotient below 2^24 is only 475 past 2^16
    assert 254 * 66011 - 1 < (1 << 24) and po.emu_fdiv(254 * 66011 - 1, 66011) == 254
    d = 1048577
    assert d - 1 < (1 << 24) and po.emu_fdiv(d - 1, d) == 1 and (d - 1) // d == 0
    assert all(po.emu_fdiv(n, d) == 0 for n in (0, 1, 65535, 1 << 19))


def test_wide_image_decode():
    """[1, 8, 2, 1048577]: cg = 1, cols = 1048577, rows = 2 (or 1 strip). The multiply-shift decode sends flat pixel
    1048576 to (row 1, col -1) -- with one strip to image 1 of a batch of 1 --, the guarded launchers divide in
    hardware there."""
    W = 1048577
    assert po.emu_decode(W - 1, 1, W, 2, fast=True) == (0, 1, -1, 0)
    assert po.emu_decode(W - 1, 1, W, 1, fast=True) == (1, 0, -1, 0)  # separable 3x3/s1: nstrip = 1
    assert po.emu_decode(W - 1, 1, W, 2, fast=False) == (0, 0, W - 1, 0)
