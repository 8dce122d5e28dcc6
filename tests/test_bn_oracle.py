"""The BatchNorm oracle (bn_oracle.py) checked on the CPU: a plain fp32 emulation of the documented formulas meets
every criterion with room to spare, each listed defect is caught by the new criteria, and the record of what the
tolerances of test_gpu_bn_act.py / test_gpu_pool.py do with the same defect (on their own kind of data) is
asserted, so the table in profiles/bn_oracle/README.md cannot drift from the code."""
import pytest
import torch

import bn_oracle as bo

SHAPES = [(1, 8), (2, 8), (135, 24), (256, 64), (1568, 24), (4096, 8)]
KINDS = {"plain": dict(), "relu": dict(relu=True), "res_relu": dict(relu=True, use_res=True),
         "res": dict(use_res=True), "dual_relu": dict(relu=True, dual=True), "dual": dict(dual=True)}


def emu_case(c, dtype, fault=None):
    """The whole emulated forward + backward of a case through the checks the GPU tests use."""
    rep = bo.Report(c.M, c.C)
    K, S, Q = bo.emu_stats(c.x)
    ws, rm, rv = bo.emu_finalize(K, S, Q, c.M, c.p, c.eps, c.momentum, fault, c.momentum_d)
    bo.check_ws_fwd(rep, ws, c.rf, K, rm, rv)
    wsd = None
    if c.xd is not None:
        Kd, Sd, Qd = bo.emu_stats(c.xd)
        wsd, rmd, rvd = bo.emu_finalize(Kd, Sd, Qd, c.M, c.pd, c.eps_d, c.momentum_d)
        bo.check_ws_fwd(rep, wsd, c.rfd, Kd, rmd, rvd, "d.")
    y, mask = bo.emu_apply(c.x, ws, c.relu, dtype, c.res, c.xd, wsd, fault)
    bo.check_apply(rep, y, mask, c.x, ws, c.rf, c.relu, c.res, c.xd, wsd)
    bits = None
    if c.relu:
        bits = bo.unpack_bits(mask, c.M, c.C) if mask is not None else bo.replay_fwd(c.x, ws, True, dtype)[1]
    dx, dres, dg, db, wsb = bo.emu_bwd(c.x, c.dy, ws, c.p, dtype, bits, fault)
    bo.check_bwd_coefs(rep, torch.cat([ws, wsb]), dg, db, c.rf, c.rb)
    bo.check_dx(rep, dx, c.rb)
    if c.res is not None:
        rep.equal("dres", dres.double(), c.rb.dyp)
    if c.xd is not None:
        dxd, _, dgd, dbd, wsbd = bo.emu_bwd(c.xd, c.dy, wsd, c.pd, dtype, bits)
        bo.check_bwd_coefs(rep, torch.cat([wsd, wsbd]), dgd, dbd, c.rfd, c.rbd, "d.")
        bo.check_dx(rep, dxd, c.rbd, "dxd")
    return rep


HALF = {"invstd": bo.B_INVSTD / 2, "scale": bo.B_COEF / 2, "shift": bo.B_COEF / 2, "running_mean": bo.B_COEF / 2,
        "running_var": bo.B_COEF / 2, "k1": bo.B_COEF / 2, "m1": bo.B_COEF / 2, "k2": bo.B_COEF / 2,
        "dgamma": bo.B_DGAMMA_RAGGED / 2, "mean": bo.B_MEAN_RAGGED / 2, "dx (t)": 0.5, "dxd (t)": 0.5}
# k2 = invstd * invstd * Q / M carries invstd's error twice (a 1-ulp rsqrt after the rounding of var + eps: about
# 1 ulp each) and two roundings of its own: 3 ulp in the worst case, which a 4-ulp bound cannot hold at half. The
# emulation (torch's fp32 rsqrt) reaches 2.05; it must stay under 3 of the 4.
HALF["k2"] = 3.0


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("M,C", SHAPES)
def test_emulation_meets_every_criterion(M, C, kind):
    for eps, mom, seed in ((1e-5, 0.1, 11), (1e-3, 0.01, 12)):
        c = bo.make_case(M, C, seed, eps=eps, momentum=mom, eps_d=1e-3 if eps == 1e-5 else 1e-5,
                         momentum_d=0.01 if mom == 0.1 else 0.1, **KINDS[kind])
        for dtype in (torch.bfloat16, torch.float32):
            rep = emu_case(c, dtype)
            rep.assert_ok(f"{kind} M={M} C={C} {dtype}")
            for name, w in rep.worst.items():
                key = name[2:] if name.startswith("d.") else name
                if key in HALF:
                    assert w <= HALF[key], f"{name}: the emulation's worst {w:.3g} is over half its bound"


def test_data_properties():
    for M in (135, 256, 4096):
        x, mu = bo.channel_data(M, 64, bo.gen(3))
        mean, var, _ = bo.stats64(x, 1e-5)
        assert torch.equal(mean, mu.double()) and float(var[0]) == 0.0 and mu[2] == 2 and mu[1] == 0
        assert 1 / 80 <= float(var[1]) <= 1 / 50
        assert float((x[0] - mu).abs().max()) <= 1
        assert torch.equal(x, x.to(torch.bfloat16).float())
        # eps = 1e-5 moves the low-variance channel's invstd by about 3e-4
        d = 1 - float(((var[1] + 1e-5) / var[1]).rsqrt())
        assert 2e-4 < d < 5e-4


def test_replay_refuses_an_inexact_fma_and_reports_like_the_exact_oracle():
    with pytest.raises(AssertionError, match="inexact"):
        bo.fma64(torch.tensor([[3.0]]), torch.tensor([1.0 + 2.0 ** -23]), torch.tensor([2.0 ** -60]))
    rep = bo.Report(300, 16, 128)
    got = torch.zeros(300, 16)
    got[129, 3] = got[257, 11] = 1.0
    rep.equal("y", got, torch.zeros(300, 16))
    assert not rep.ok() and "2 of 4800 differ" in rep.failures[0] and "channels [3, 11]" in rep.failures[0]
    assert "row blocks of 128: [1, 2]" in rep.failures[0]
    rep = bo.Report(8, 8)
    rep.within("invstd", torch.tensor([1.0 + 5 * bo.ULP, float("nan")]), torch.ones(2), torch.ones(2), 4.0)
    assert "2 of 2 differ" in rep.failures[0] and rep.worst["invstd"] == float("inf")
    bits = torch.rand(6, 16, generator=bo.gen(2)) > 0.5
    assert torch.equal(bo.unpack_bits(bo.pack_bits(bits), 6, 16), bits)


def test_pool_reference_matches_emulation_and_gather_is_exact():
    g = bo.gen(5)
    for (N, C, H, W), k, s, p, ceil in (((2, 8, 8, 8), 3, 2, 1, False), ((1, 16, 6, 10), 3, 2, 0, True),
                                        ((2, 8, 7, 9), 3, 2, 1, False), ((2, 8, 6, 6), 2, 2, 0, False),
                                        ((2, 8, 5, 7), 3, 1, 1, False)):
        a = bo.ints((N, C, H, W), g, 0, 3)
        v, pos = bo.pool_ref(a, k, s, p, ceil)
        ve, pe = bo.emu_pool_fwd(a, k, s, p, ceil)
        assert torch.equal(v, ve) and torch.equal(pos, pe)
        assert torch.equal(v, torch.nn.functional.max_pool2d(a, k, s, p, ceil_mode=ceil))
        dyp = bo.ints(v.shape, g)
        full = bo.pool_gather(dyp, pos, H, W, k, s, p)
        assert float(full.sum()) == float(dyp.sum())  # every window's gradient lands on exactly one pixel
        ar = a.double().requires_grad_(True)
        # where no window has a tie, autograd's routing is the same
        if int((bo._windows(a, k, s, p, ceil) == v.unsqueeze(-1)).sum(-1).max()) == 1:
            torch.nn.functional.max_pool2d(ar, k, s, p, ceil_mode=ceil).backward(dyp.double())
            assert torch.equal(ar.grad, full)


# ------------------------------------------------------------------------------------------- the defects
def _present_tolerances(fault):
    """What the tolerances of test_gpu_bn_act.py do with the defect on that file's kind of data ((8, 64, 14, 14)
    bf16 randn * 2 + 0.7, both BNs at the default eps / momentum): True when an assertion there would fail.
    y / dx / dres: rtol 2e-2, atol 3e-2 (dx, dres: a 1e-5 share excluded); running statistics: rtol 1e-4 / 1e-3;
    dgamma, dbeta: rtol 2e-2, atol 5e-2. The reference backward uses the output's own ReLU mask, as there."""
    g = bo.gen(0)
    M, C = 8 * 14 * 14, 64
    bf = lambda t: t.to(torch.bfloat16).float()  # noqa: E731
    x, res, dy = bf(torch.randn(M, C, generator=g) * 2 + 0.7), bf(torch.randn(M, C, generator=g)), \
        bf(torch.randn(M, C, generator=g))
    p = bo.SimpleNamespace(gamma=torch.rand(C, generator=g) + 0.5, beta=torch.rand(C, generator=g) - 0.5,
                           rm0=torch.zeros(C), rv0=torch.ones(C))
    eps, mom = 1e-5, 0.1
    K, S, Q = bo.emu_stats(x)
    ws, rm, rv = bo.emu_finalize(K, S, Q, M, p, eps, mom, fault, momentum_other=mom)  # the other BN's: the same
    y, mask = bo.emu_apply(x, ws, True, torch.bfloat16, res, fault=fault)
    bits = bo.unpack_bits(mask, M, C)
    dx, dres, dg, db, _ = bo.emu_bwd(x, dy, ws, p, torch.bfloat16, bits, fault)
    rf = bo.ref_fwd(x, p, eps, mom, False, res)
    yr = rf.pre.clamp(min=0)
    own = (y.float() > 0)  # the reference backward takes the kernel's own ReLU decisions
    dyp = dy.double() * own
    xc = x.double() - rf.mean
    Sr, Qr = dyp.sum(0), (dyp * xc).sum(0)
    k1 = rf.gamma * rf.invstd
    dxr = k1 * (dyp - Sr / M - xc * rf.invstd ** 2 * Qr / M)
    close = lambda a, b, rt, at: torch.isclose(a.double(), b, rtol=rt, atol=at)  # noqa: E731
    caught = []
    if not bool(close(y, yr, 2e-2, 3e-2).all()):
        caught.append("y")
    if not bool(close(rm, rf.rm, 1e-4, 1e-4).all()):
        caught.append("running_mean")
    if not bool(close(rv, rf.rv, 1e-3, 1e-4).all()):
        caught.append("running_var")
    if float((~close(dx, dxr, 2e-2, 3e-2)).float().mean()) > 1e-5:
        caught.append("dx")
    if float((~close(dres, dyp, 2e-2, 3e-2)).float().mean()) > 1e-5:
        caught.append("dres")
    if not bool(close(dg, Qr * rf.invstd, 2e-2, 5e-2).all()):
        caught.append("dgamma")
    if not bool(close(db, Sr, 2e-2, 5e-2).all()):
        caught.append("dbeta")
    return caught


def _present_pool(fault):
    """What test_gpu_pool.py's fused-stem test does with a pooling defect ((2, 16, 16, 16) bf16 randn, eps 1e-3):
    the pooled output must equal the unfused one bitwise, and dx may be 1.5x + 1e-3 as far (relative L2) from an
    fp32 reference, which pools the unrounded values, as the unfused bf16 path is."""
    g = bo.gen(1)
    N, C, H, W = 2, 16, 16, 16
    M = N * H * W
    x = (torch.randn(M, C, generator=g)).to(torch.bfloat16).float()
    p = bo.SimpleNamespace(gamma=torch.rand(C, generator=g) + 0.5, beta=torch.rand(C, generator=g) - 0.5,
                           rm0=torch.zeros(C), rv0=torch.ones(C))
    K, S, Q = bo.emu_stats(x)
    ws, _, _ = bo.emu_finalize(K, S, Q, M, p, 1e-3, 0.1)
    y, _ = bo.emu_apply(x, ws, True, torch.bfloat16)
    a = bo.nchw(y.float(), N, H, W)
    v0, pos0 = bo.emu_pool_fwd(a, 3, 2, 1)
    v1, pos1 = bo.emu_pool_fwd(a, 3, 2, 1, fault=fault)
    caught = [] if torch.equal(v0, v1) else ["y"]
    dyp = torch.randn(v0.shape, generator=g).to(torch.bfloat16).float()
    rf = bo.ref_fwd(x, p, 1e-3, 0.1)
    a64 = bo.nchw(rf.bn.clamp(min=0), N, H, W)
    _, posr = bo.pool_ref(a64, 3, 2, 1)

    def dx_of(pos, dtype):
        dy = bo.rows(bo.pool_gather(dyp, pos, H, W, 3, 2, 1)).float()
        bits = bo.replay_fwd(x, ws, True, torch.bfloat16)[1]
        return bo.emu_bwd(x, dy, ws, p, dtype, bits)[0].double()

    ref = dx_of(posr, torch.float32)
    err = lambda d: float((d - ref).norm() / ref.norm())  # noqa: E731
    if err(dx_of(pos1, torch.bfloat16)) > 1.5 * err(dx_of(pos0, torch.bfloat16)) + 1e-3:
        caught.append("dx")
    return caught


def _new_criteria(fault):
    """The failures the new criteria report for the defect, over an exact and a ragged case."""
    if fault in ("tap_dropped", "tie_last"):
        c = bo.make_case(2 * 8 * 8, 8, 21, relu=True, eps=1e-3)
        K, S, Q = bo.emu_stats(c.x)
        ws, _, _ = bo.emu_finalize(K, S, Q, c.M, c.p, c.eps, c.momentum)
        y, _ = bo.replay_fwd(c.x, ws, True, torch.bfloat16)
        a = bo.nchw(y.float(), 2, 8, 8)
        rep = bo.Report(c.M, c.C)
        v, pos = bo.emu_pool_fwd(a, 3, 2, 1, fault=fault)
        vr, pr = bo.pool_ref(a, 3, 2, 1)
        rep.equal("pooled y", v, vr)
        rep.equal("pos", pos, pr)
        return rep.failures
    out = []
    kind = {"momentum_other": "dual_relu", "mask_neighbour": "res_relu"}.get(fault, "res_relu")
    for M, C in ((256, 24), (135, 24)):
        c = bo.make_case(M, C, 31, **KINDS[kind])
        out += emu_case(c, torch.bfloat16, fault).failures
    return out


# fault -> the quantities on which the present tolerances of test_gpu_bn_act.py / test_gpu_pool.py fail on their own
# data ([]: the defect passes today). Measured by _present_tolerances / _present_pool and asserted below.
PRESENT = {
    "eps_dropped": [],
    "eps_swapped": [],
    "momentum_other": [],
    "no_bessel": [],
    "row_dropped": ["dgamma", "dbeta"],   # caught today as well (a row of N(0, 1) gradients against atol 5e-2)
    "row_twice": ["dgamma", "dbeta"],     # caught today as well
    "m1_dropped": [],
    "k2_dropped": ["dx"],                 # caught today as well
    "truncate": [],
    "mask_neighbour": ["dx", "dres", "dgamma", "dbeta"],  # caught today as well
    "tap_dropped": ["y", "dx"],           # caught today as well (fused == unfused pooled output)
    "tie_last": ["dx"],                   # caught today as well
}


@pytest.mark.parametrize("fault", bo.FAULTS)
def test_fault_is_caught_by_the_new_criteria(fault):
    failures = _new_criteria(fault)
    assert failures, f"{fault}: not caught"
    present = _present_pool(fault) if fault in ("tap_dropped", "tie_last") else _present_tolerances(fault)
    print(f"{fault}: new criteria: {len(failures)} failures, e.g. {failures[0][:120]}; present tolerances: "
          f"{present or 'pass'}")
    assert present == PRESENT[fault], (fault, present)


def test_record_shows_what_passes_today():
    for fault in ("eps_dropped", "eps_swapped", "momentum_other", "no_bessel", "truncate"):
        assert PRESENT[fault] == []
    assert set(PRESENT) == set(bo.FAULTS)
