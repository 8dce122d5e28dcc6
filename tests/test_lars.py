"""FusedLARS on the CPU: the torch fallback against a float64 oracle of the formula, the learning-rate
schedule, checkpoints, the DistributedOptimizer wrapper and the CLI flags.

``lars_oracle_step`` below is the oracle of both LARS test files (tests/test_gpu_lars.py imports it); it
is written from the formula of the issue and shares no code with the package."""
import math
import os
import subprocess
import sys

import pytest
import torch

from dist_util import free_port, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 1e-5, 1e-6  # the FusedSGD bound of tests/test_gpu_kernels.py


def lars_oracle_step(P, M, grads, hp, grad_scale=1.0, max_grad_norm=0.0):
    """One LARS step in float64, in place. ``P``, ``M``: lists of float64 tensors (parameter or master,
    momentum); ``grads``: one tensor (any dtype) or None per parameter; ``hp``: one dict per parameter with
    lr, momentum, weight_decay, eta, eps, adapt. Returns (G, per-tensor ||g||, trust ratios) of the stepped
    tensors (None for the skipped ones)."""
    gs = [None if g is None else g.detach().double().cpu() for g in grads]
    total = sum(float((g * g).sum()) for g in gs if g is not None)
    G = grad_scale * math.sqrt(total)
    clip = min(1.0, max_grad_norm / (G + 1e-6)) if max_grad_norm > 0 else 1.0
    c = grad_scale * clip
    gnorms, trusts = [], []
    for p, m, g, h in zip(P, M, gs, hp):
        if g is None:
            gnorms.append(None)
            trusts.append(None)
            continue
        graw = math.sqrt(float((g * g).sum()))
        wn, gn = math.sqrt(float((p * p).sum())), c * graw
        wd = h["weight_decay"] if h["adapt"] else 0.0
        trust = 1.0
        if h["adapt"] and wn > 0 and gn > 0:
            trust = h["eta"] * wn / (gn + wd * wn + h["eps"])
        d = c * g.reshape(p.shape) + wd * p
        m.mul_(h["momentum"]).add_(d, alpha=h["lr"] * trust)
        p.sub_(m)
        gnorms.append(graw)
        trusts.append(trust)
    return G, gnorms, trusts


def hyper(opt):
    """The oracle's per-parameter hyper-parameters of a FusedLARS, in param_groups order."""
    out = []
    for g in opt.param_groups:
        for p in g["params"]:
            out.append(dict(lr=g["lr"], momentum=g["momentum"], weight_decay=g["weight_decay"], eta=g["eta"],
                            eps=g["eps"], adapt=not (g["exclude_bias_and_norm"] and p.ndim <= 1)))
    return out


SHAPES = [(5,), (7, 3), (33, 17), (4, 3, 3, 3), (64,), (130, 70)]


def _make(dtype, seed=0, **kw):
    from distributed_learning_amd.ops.optim import FusedLARS

    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(s, generator=g).to(dtype).requires_grad_() for s in SHAPES]
    opt = FusedLARS([dict(params=ps[:3], lr=0.3, weight_decay=1e-4), dict(params=ps[3:], lr=0.05, weight_decay=5e-3)],
                    lr=0.1, momentum=0.9, **kw)
    return ps, opt


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("max_grad_norm", [0.0, 0.5])
def test_fallback_matches_oracle(dtype, max_grad_norm):
    ps, opt = _make(dtype, grad_scale=0.5, max_grad_norm=max_grad_norm, master_weights=dtype != torch.float32)
    P = [p.detach().double().clone() for p in ps]
    M = [torch.zeros_like(p) for p in P]
    g = torch.Generator().manual_seed(1)
    for step in range(3):
        grads = [(torch.randn(p.shape, generator=g) * (i + 1)).to(dtype) for i, p in enumerate(ps)]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        opt.step()
        G, _, trusts = lars_oracle_step(P, M, grads, hyper(opt), 0.5, max_grad_norm)
        assert all(t == 1.0 for t, p in zip(trusts, ps) if p.ndim <= 1) and trusts[1] != 1.0
        torch.testing.assert_close(opt.last_grad_norm, torch.tensor([G], dtype=torch.float32), rtol=RTOL, atol=ATOL)
        for p, ref, mref in zip(ps, P, M):
            st = opt.state[p]
            got = st["master"] if dtype != torch.float32 else p.detach()
            assert got.dtype == torch.float32 and st["momentum_buffer"].dtype == torch.float32
            torch.testing.assert_close(got, ref.float(), rtol=RTOL, atol=ATOL)
            torch.testing.assert_close(st["momentum_buffer"], mref.float(), rtol=RTOL, atol=ATOL)
            if dtype != torch.float32:
                assert torch.equal(p.detach(), st["master"].to(torch.bfloat16))  # the shadow, bitwise


def test_excluded_tensors_get_plain_momentum_sgd():
    """ndim <= 1: trust 1 and no weight decay, whatever the group's weight decay is."""
    from distributed_learning_amd.ops.optim import FusedLARS

    torch.manual_seed(0)
    b, w = torch.randn(40).requires_grad_(), torch.randn(8, 5).requires_grad_()
    b0 = b.detach().double().clone()
    opt = FusedLARS([b, w], lr=0.1, momentum=0.9, weight_decay=0.1)
    m = torch.zeros_like(b0)
    for _ in range(3):
        b.grad, w.grad = torch.randn(40), torch.randn(8, 5)
        m = 0.9 * m + 0.1 * b.grad.double()
        b0 = b0 - m
        opt.step()
        torch.testing.assert_close(b.detach(), b0.float(), rtol=RTOL, atol=ATOL)
    # and with the exclusion off the same tensor is scaled layer-wise: a different trajectory
    b2 = torch.randn(40).requires_grad_()
    start = b2.detach().clone()
    opt2 = FusedLARS([b2], lr=0.1, momentum=0.9, weight_decay=0.1, exclude_bias_and_norm=False)
    b2.grad = torch.randn(40)
    plain = start - 0.1 * b2.grad
    opt2.step()
    assert not torch.allclose(b2.detach(), plain, rtol=1e-3, atol=1e-4)


def test_zero_norms_give_trust_one():
    from distributed_learning_amd.ops.optim import FusedLARS

    w0, w1 = torch.zeros(6, 4).requires_grad_(), torch.randn(6, 4).requires_grad_()
    keep = w1.detach().clone()
    opt = FusedLARS([w0, w1], lr=0.1, momentum=0.0)
    w0.grad, w1.grad = torch.ones(6, 4), torch.zeros(6, 4)
    opt.step()
    torch.testing.assert_close(w0.detach(), torch.full((6, 4), -0.1))  # zero weight: trust 1
    assert torch.equal(w1.detach(), keep) and torch.isfinite(w0).all()  # zero gradient: unchanged, finite


def test_poly_warmup_lr():
    from distributed_learning_amd.ops.optim import poly_warmup_lr

    base, warm, total = 3.2, 10, 110
    assert poly_warmup_lr(0, base, warm, total) == 0.0
    assert poly_warmup_lr(warm, base, warm, total) == base
    assert poly_warmup_lr(5, base, warm, total) == pytest.approx(base / 2)
    assert poly_warmup_lr(total, base, warm, total) == 0.0
    assert poly_warmup_lr(total + 50, base, warm, total, end_lr=0.01) == pytest.approx(0.01)
    assert poly_warmup_lr(60, base, warm, total, power=2.0) == pytest.approx(base * 0.25)
    assert poly_warmup_lr(60, base, warm, total, power=1.0, end_lr=0.2) == pytest.approx(0.2 + (base - 0.2) * 0.5)
    lrs = [poly_warmup_lr(s, base, warm, total) for s in range(total + 1)]
    assert all(a < b for a, b in zip(lrs[:warm], lrs[1:warm + 1]))  # warmup rises
    assert all(a > b for a, b in zip(lrs[warm:-1], lrs[warm + 1:]))  # decay falls
    assert all(poly_warmup_lr(s, base, 0, 0) == base for s in (0, 1, 1000))  # no schedule: constant
    assert poly_warmup_lr(50, base, warm, 0) == base  # warmup only


def test_set_lr_updates_groups():
    _, opt = _make(torch.float32)
    opt.set_lr(0.7)
    assert [g["lr"] for g in opt.param_groups] == [0.7, 0.7]
    opt.set_lr(0.2, group=1)
    assert [g["lr"] for g in opt.param_groups] == [0.7, 0.2]


def test_checkpoint_roundtrip_continues_bit_exactly(tmp_path):
    from distributed_learning_amd.models import create_network
    from distributed_learning_amd.ops.optim import FusedLARS
    from distributed_learning_amd.train import load_checkpoint, save_checkpoint

    def grads(model, seed):
        g = torch.Generator().manual_seed(seed)
        for p in model.parameters():
            p.grad = torch.randn(p.shape, generator=g).to(p.dtype)

    def make():
        torch.manual_seed(3)
        m = create_network("basicnet").to(torch.bfloat16)
        return m, FusedLARS(m.parameters(), lr=0.2, momentum=0.9, weight_decay=1e-4, master_weights=True)

    m, opt = make()
    for s in range(2):
        grads(m, s)
        opt.step()
    path = str(tmp_path / "lars.pt")
    save_checkpoint(path, m, opt, 2)
    m2, opt2 = make()
    assert load_checkpoint(path, m2, opt2) == 2
    for p in m2.parameters():
        st = opt2.state[p]
        assert st["master"].dtype == torch.float32 and st["momentum_buffer"].dtype == torch.float32
    for mod, o in ((m, opt), (m2, opt2)):
        grads(mod, 2)
        o.step()
    for a, b in zip(m.parameters(), m2.parameters()):
        assert torch.equal(a, b)
        assert torch.equal(opt.state[a]["master"], opt2.state[b]["master"])
        assert torch.equal(opt.state[a]["momentum_buffer"], opt2.state[b]["momentum_buffer"])


def _train_wrapped(rank, world, steps):
    import distributed_learning_amd as dla
    from distributed_learning_amd.ops.loss import cross_entropy
    from distributed_learning_amd.ops.optim import FusedLARS
    from test_wrappers_dist import TinyNet, _data

    torch.manual_seed(rank)  # different init per rank: the broadcast must make them equal
    model = TinyNet()
    dla.broadcast_parameters(model.state_dict(), root_rank=0)
    opt = dla.DistributedOptimizer(FusedLARS(model.parameters(), lr=0.5, momentum=0.9, weight_decay=1e-4,
                                             max_grad_norm=1.0),
                                   named_parameters=model.named_parameters(), bucket_cap_mb=0.001)
    start = {n: p.detach().clone() for n, p in model.named_parameters()}
    for s in range(steps):
        x, y = _data(rank, seed=s)
        opt.zero_grad()
        cross_entropy(model(x), y).backward()
        opt.step()
    return start, {n: p.detach().clone() for n, p in model.named_parameters()}


def test_distributed_optimizer_wraps_fused_lars():
    res = run(_train_wrapped, 2, 3)
    (start, end0), (_, end1) = res
    for k in end0:
        assert torch.equal(end0[k], end1[k]), k  # bitwise equal across ranks
        assert not torch.equal(end0[k], start[k]), k  # and trained


POSITIONALS = ["1", "0", "1", "1", "127.0.0.1", "lo", "mnist", "/nonexistent", "0"]


def test_parser_accepts_lars_flags():
    from distributed_learning_amd.config import parse_args

    c = parse_args(POSITIONALS)
    assert (c.optimizer, c.lars_eta, c.max_grad_norm, c.warmup_steps, c.total_steps, c.lr_power) == \
        ("sgd", 1e-3, 0.0, 0, 0, 2.0)
    c = parse_args(POSITIONALS + ["--optimizer", "lars", "--lars_eta", "0.002", "--max_grad_norm", "1.5",
                                  "--warmup_steps", "5", "--total_steps", "100", "--lr_power", "1"])
    assert (c.optimizer, c.lars_eta, c.max_grad_norm, c.warmup_steps, c.total_steps, c.lr_power) == \
        ("lars", 0.002, 1.5, 5, 100, 1.0)
    c = parse_args(POSITIONALS + ["--warmup_steps", "5"])  # a schedule alone is fine with SGD
    assert c.optimizer == "sgd" and c.warmup_steps == 5


def test_parser_rejects_clipping_with_sgd(capsys):
    from distributed_learning_amd.config import parse_args

    with pytest.raises(SystemExit) as e:
        parse_args(POSITIONALS + ["--optimizer", "sgd", "--max_grad_norm", "1"])
    assert e.value.code == 2 and "--max_grad_norm needs --optimizer lars" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_args(POSITIONALS + ["--max_grad_norm", "1"])  # sgd is the default
    assert "needs --optimizer lars" in capsys.readouterr().err


def test_worker_optimizer_and_schedule_selection():
    """Defaults build today's FusedSGD with no schedule; the flags select FusedLARS and a schedule."""
    from distributed_learning_amd.config import parse_args
    from distributed_learning_amd.ops.optim import FusedLARS, FusedSGD
    from distributed_learning_amd.train import lr_schedule, make_optimizer, set_lr

    ps = [torch.zeros(3, 3, requires_grad=True)]
    c = parse_args(POSITIONALS)
    opt = make_optimizer(c, ps, False)
    assert type(opt) is FusedSGD and lr_schedule(c) is None
    assert opt.defaults["lr"] == c.lr and opt.defaults["momentum"] == c.momentum and not opt.master_weights
    c = parse_args(POSITIONALS + ["--optimizer", "lars", "--lars_eta", "0.01", "--max_grad_norm", "2", "--lr", "1.0",
                                  "--warmup_steps", "4", "--total_steps", "8"])
    opt = make_optimizer(c, ps, True)
    assert type(opt) is FusedLARS and opt.defaults["eta"] == 0.01 and opt.max_grad_norm == 2 and opt.master_weights
    sched = lr_schedule(c)
    # batch b runs at the schedule's step b + 1: the first batch already updates
    assert [sched(b) for b in (0, 1, 3, 5, 7, 20)] == [0.25, 0.5, 1.0, 0.25, 0.0, 0.0]
    set_lr(opt, sched(1))
    assert opt.param_groups[0]["lr"] == 0.5
    sgd = FusedSGD(ps, lr=0.1)
    set_lr(sgd, 0.3)
    assert sgd.param_groups[0]["lr"] == 0.3


@pytest.mark.slow
def test_main_cli_lars_two_workers(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "distributed_learning_amd.main", "1", "0", "2", "2", "127.0.0.1", "lo", "mnist",
           "/nonexistent", "0", "--optimizer", "lars", "--max_grad_norm", "1", "--warmup_steps", "2", "--total_steps",
           "10", "--random_input", "1", "--limit_batches", "3", "--batch_size", "8", "--master_port", str(free_port()),
           "--results_root", str(tmp_path), "--job_id", "t"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    files = sorted(tmp_path.glob("*/*_loss.txt"))
    assert len(files) == 2, files
    for w, f in enumerate(files):
        lines = f.read_text().splitlines()
        assert len(lines) == 3 and lines[0].startswith(f"Worker 0:{w} loss for batch 0: ")
        assert all(math.isfinite(float(ln.rsplit(": ", 1)[1])) for ln in lines)
