"""FusedLAMB and FusedAdamW on the CPU: the torch fallback against the float64 oracle of tests/lamb_oracle.py, the
faults that the bound catches, the bias-correction formula, checkpoints, the DistributedOptimizer wrapper and
the CLI flags.

Bound: the FusedSGD / FusedLARS bound, rtol 1e-5 and atol 1e-6 against the oracle rounded to fp32 (imported from
tests/test_lars.py). The fp32 emulation of tests/lamb_oracle.py meets it on these inputs (test_fault_record, the
``None`` case), so it is attainable; each injected fault misses it.

Inputs: (1, n) tensors of 1, 17, 4096, 3 * 4096 + 5 and 123457 elements, which LAMB adapts, and a 300-element
vector, which it excludes; lr 2e-2 / 1e-2, betas (0.9, 0.999), eps 1e-6, wd 1e-2 / 3e-2, grad_scale 0.5. Four
steps; in step 2 tensor 1 has no gradient, in step 3 tensor 2 has a zero gradient."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dist_util import free_port, run
from lamb_oracle import FAULTS, hyper, lamb_emulate_step, lamb_oracle_step, worst_ratio
from test_lars import ATOL, POSITIONALS, RTOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 17, 4096, 3 * 4096 + 5, 123457]
KW = dict(lr=2e-2, betas=(0.9, 0.999), eps=1e-6, weight_decay=1e-2, grad_scale=0.5)
STEPS = 4


def _cls(name):
    from distributed_learning_amd.ops import optim

    return {"lamb": optim.FusedLAMB, "adamw": optim.FusedAdamW}[name]


def _params(dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(1, n, generator=g).to(dtype) for n in SIZES] + [torch.randn(300, generator=g).to(dtype)]


def _grads(ps, step, gen):
    """The gradients of step ``step`` (from 1): bf16-valued where the parameter is; None / zero as the module
    docstring says."""
    out = [torch.randn(p.shape, generator=gen).to(p.dtype) for p in ps]
    if step == 2:
        out[1] = None
    if step == 3:
        out[2] = torch.zeros_like(out[2])
    return out


def _make(name, dtype, **kw):
    ps = [p.requires_grad_() for p in _params(dtype)]
    opt = _cls(name)([dict(params=ps[:3]), dict(params=ps[3:], lr=1e-2, weight_decay=3e-2)],
                     master_weights=dtype != torch.float32, **{**KW, **kw})
    return ps, opt


def _close(got, ref64):
    torch.testing.assert_close(got.detach().float().cpu(), ref64.float().reshape(got.shape), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("max_grad_norm", [0.0, 1.0])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["lamb", "adamw"])
def test_fallback_matches_oracle(name, dtype, max_grad_norm):
    ps, opt = _make(name, dtype, max_grad_norm=max_grad_norm)
    P = [p.detach().double().clone() for p in ps]
    M, V, K = [torch.zeros_like(p) for p in P], [torch.zeros_like(p) for p in P], [0] * len(P)
    gen = torch.Generator().manual_seed(1)
    for step in range(1, STEPS + 1):
        grads = _grads(ps, step, gen)
        for p, g in zip(ps, grads):
            p.grad = None if g is None else g.clone()
        opt.step()
        G, trusts, _ = lamb_oracle_step(P, M, V, K, grads, hyper(opt), name == "lamb", KW["grad_scale"], max_grad_norm)
        assert opt.last_launches == 0 and opt.last_plan is None
        if max_grad_norm > 0:
            assert G > 10 * max_grad_norm  # the clip binds
            _close(opt.last_grad_norm, torch.tensor([G]))
        else:
            assert opt.last_grad_norm is None
        if name == "lamb":
            assert trusts[-1] == 1.0 and trusts[0] != 1.0  # the vector is excluded
        else:
            assert all(t in (None, 1.0) for t in trusts)
        for i, (p, ref, mref, vref) in enumerate(zip(ps, P, M, V)):
            st = opt.state[p]
            if K[i] == 0:
                assert "exp_avg" not in st  # never stepped yet
                continue
            got = st["master"] if dtype != torch.float32 else p.detach()
            assert got.dtype == st["exp_avg"].dtype == st["exp_avg_sq"].dtype == torch.float32
            assert st["step"].dtype == torch.int32 and st["step"].shape == (1,) and int(st["step"]) == K[i]
            _close(got, ref)
            _close(st["exp_avg"], mref)
            _close(st["exp_avg_sq"], vref)
            if dtype != torch.float32:
                assert torch.equal(p.detach(), st["master"].to(torch.bfloat16))  # the shadow, bitwise
    assert K == [4, 3, 4, 4, 4, 4]


def _fault_run(name, fault, max_grad_norm=0.0):
    """Worst error, in units of the bound, of the fp32 emulation (with ``fault``) against the oracle over the
    test's four steps: (p, m, v) maxima."""
    ps, opt = _make(name, torch.float32, max_grad_norm=max_grad_norm)
    hp = hyper(opt)
    P = [p.detach().double().clone() for p in ps]
    M, V, K = [torch.zeros_like(p) for p in P], [torch.zeros_like(p) for p in P], [0] * len(P)
    Pe = [p.detach().clone() for p in ps]
    Me, Ve, Ke = [torch.zeros_like(p) for p in Pe], [torch.zeros_like(p) for p in Pe], [0] * len(Pe)
    gen = torch.Generator().manual_seed(1)
    worst = [0.0, 0.0, 0.0]
    for step in range(1, STEPS + 1):
        grads = _grads(ps, step, gen)
        lamb_oracle_step(P, M, V, K, grads, hp, name == "lamb", KW["grad_scale"], max_grad_norm)
        lamb_emulate_step(Pe, Me, Ve, Ke, grads, hp, name == "lamb", KW["grad_scale"], max_grad_norm, fault)
        for j, (got, ref) in enumerate(((Pe, P), (Me, M), (Ve, V))):
            worst[j] = max([worst[j]] + [worst_ratio(a, b, RTOL, ATOL) for a, b in zip(got, ref)])
    return worst


@pytest.mark.parametrize("fault", [None] + list(FAULTS))
@pytest.mark.parametrize("name", ["lamb", "adamw"])
def test_fault_record(name, fault):
    """The bound is attainable in fp32 (fault None) and catches every injected fault on these inputs (figures:
    profiles/lamb/README.md). ``trust_from_grad`` does not exist in AdamW."""
    if name == "adamw" and fault == "trust_from_grad":
        assert max(_fault_run(name, fault)) <= 1.0  # no trust ratio to get wrong
        return
    worst = _fault_run(name, fault)
    print(f"fault record: {name} {fault}: worst |err| / bound  p {worst[0]:.3g}  m {worst[1]:.3g}  v {worst[2]:.3g}")
    if fault is None:
        assert max(worst) <= 1.0
    else:
        assert worst[0] > 1.0  # the parameters miss the bound


def test_excluded_tensors_get_plain_adamw():
    """ndim <= 1: trust 1 and no weight decay, whatever the group's weight decay is; both optimizers agree there."""
    outs = {}
    for name in ("lamb", "adamw"):
        g = torch.Generator().manual_seed(0)
        b, w = torch.randn(40, generator=g).requires_grad_(), torch.randn(8, 5, generator=g).requires_grad_()
        P, M, V, K = [b.detach().double().clone()], [torch.zeros(40).double()], [torch.zeros(40).double()], [0]
        opt = _cls(name)([b, w], lr=0.05, weight_decay=0.1)
        for _ in range(3):
            b.grad, w.grad = torch.randn(40, generator=g), torch.randn(8, 5, generator=g)
            hp = [dict(lr=0.05, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay=0.0, adapt=False)]
            lamb_oracle_step(P, M, V, K, [b.grad], hp, False)
            opt.step()
            _close(b, P[0])
        outs[name] = (b.detach().clone(), w.detach().clone())
    assert torch.equal(outs["lamb"][0], outs["adamw"][0]) and not torch.equal(outs["lamb"][1], outs["adamw"][1])
    # with the exclusion off the same vector is decayed (and in LAMB scaled): a different trajectory
    b2 = outs["lamb"][0].clone().requires_grad_()
    start = b2.detach().clone()
    opt2 = _cls("adamw")([b2], lr=0.05, weight_decay=0.1, exclude_bias_and_norm=False)
    b2.grad = torch.ones(40)
    opt2.step()
    torch.testing.assert_close(b2.detach(), start - 0.05 * (1.0 + 0.1 * start), rtol=1e-5, atol=1e-6)


def test_zero_norms_give_trust_one():
    w0, w1 = torch.zeros(6, 4).requires_grad_(), torch.randn(6, 4).requires_grad_()
    keep = w1.detach().clone()
    opt = _cls("lamb")([w0, w1], lr=0.1)
    w0.grad, w1.grad = torch.ones(6, 4), torch.zeros(6, 4)
    opt.step()
    # zero weight: trust 1, u = 1 / (1 + eps); zero gradient without weight decay: u = 0, unchanged, finite
    torch.testing.assert_close(w0.detach(), torch.full((6, 4), -0.1), rtol=1e-5, atol=1e-6)
    assert torch.equal(w1.detach(), keep) and torch.isfinite(w0).all()
    assert all(torch.isfinite(opt.state[w][k]).all() for w in (w0, w1) for k in ("exp_avg", "exp_avg_sq"))


def test_argument_checks():
    p = [torch.zeros(3, 3, requires_grad=True)]
    for name in ("lamb", "adamw"):
        with pytest.raises(ValueError, match="eps > 0"):
            _cls(name)(p, lr=0.1, eps=0.0)
        for betas in ((1.0, 0.999), (0.9, 1.0), (-0.1, 0.999)):
            with pytest.raises(ValueError, match="betas"):
                _cls(name)(p, lr=0.1, betas=betas)
        opt = _cls(name)(p, lr=0.1)
        assert opt.defaults["betas"] == (0.9, 0.999) and opt.defaults["eps"] == 1e-6
        assert opt.defaults["weight_decay"] == 0 and opt.defaults["exclude_bias_and_norm"]


KS = (1, 2, 3, 10, 10 ** 3, 10 ** 5)
BETAS = (0.9, 0.999, 0.9999)


def test_bias_correction_formula_in_fp32():
    """1 - beta^k as -expm1(k * ln beta) with everything rounded to fp32 (the kernels' form) is within 1e-6 of
    float64 over the grid; the running fp32 product beta^k is not: at beta = 0.999 it misses the bound at every
    k <= 1e3 of the grid (1.3e-5 at k = 1, 7.6e-6 at k = 1e3; at k = 1e5 beta^k has vanished against 1 and both
    forms return exactly 1)."""
    f = np.float32
    for beta in BETAS:
        ln = f(math.log(beta))
        prod, running = f(1.0), {}
        for k in range(1, max(KS) + 1):
            prod = f(prod * f(beta))
            if k in KS:
                running[k] = f(1.0) - prod
        for k in KS:
            exact = -math.expm1(k * math.log(beta))
            got = -np.expm1(f(f(k) * ln), dtype=f)
            assert got.dtype == f and abs(float(got) - exact) <= 1e-6 * exact, (beta, k, got, exact)
            if beta == 0.999 and k <= 10 ** 3:
                assert abs(float(running[k]) - exact) > 1e-6 * exact, (beta, k, running[k], exact)


def test_checkpoint_roundtrip_continues_bit_exactly(tmp_path):
    from distributed_learning_amd.models import create_network
    from distributed_learning_amd.train import load_checkpoint, save_checkpoint

    def grads(model, seed):
        g = torch.Generator().manual_seed(seed)
        for p in model.parameters():
            p.grad = torch.randn(p.shape, generator=g).to(p.dtype)

    for name in ("lamb", "adamw"):
        def make():
            torch.manual_seed(3)
            m = create_network("basicnet").to(torch.bfloat16)
            return m, _cls(name)(m.parameters(), lr=0.02, weight_decay=1e-2, max_grad_norm=1.0, master_weights=True)

        m, opt = make()
        for s in range(2):
            grads(m, s)
            opt.step()
        path = str(tmp_path / f"{name}.pt")
        save_checkpoint(path, m, opt, 2)
        m2, opt2 = make()
        assert load_checkpoint(path, m2, opt2) == 2
        for p, q in zip(m.parameters(), m2.parameters()):
            st = opt2.state[q]
            assert st["master"].dtype == st["exp_avg"].dtype == st["exp_avg_sq"].dtype == torch.float32
            assert st["step"].dtype == torch.int32 and st["step"].device == q.device and int(st["step"]) == 2
            assert st["step"].data_ptr() != opt.state[p]["step"].data_ptr()
        for mod, o in ((m, opt), (m2, opt2)):
            grads(mod, 2)
            o.step()
        for a, b in zip(m.parameters(), m2.parameters()):
            assert torch.equal(a, b)
            for k in ("master", "exp_avg", "exp_avg_sq", "step"):
                assert torch.equal(opt.state[a][k], opt2.state[b][k]), k
            assert int(opt2.state[b]["step"]) == 3


def test_model_ema_exchanges_masters():
    """ModelEMA.applied() under the new class: masters and shadows are exchanged with the averages and restored."""
    from distributed_learning_amd.models import create_network
    from distributed_learning_amd.ops.optim import ModelEMA

    torch.manual_seed(4)
    m = create_network("basicnet").to(torch.bfloat16)
    opt = _cls("lamb")(m.parameters(), lr=0.02, master_weights=True, ema_decay=0.5)
    ema = ModelEMA(m, opt, 0.5)
    g = torch.Generator().manual_seed(5)
    for s in range(2):
        for p in m.parameters():
            p.grad = torch.randn(p.shape, generator=g).to(p.dtype)
        ema.step(s)
    before = [(p.detach().clone(), opt.state[p]["master"].clone(), opt.state[p]["ema"].clone()) for p in m.parameters()]
    with ema.applied():
        for p, (_, master, avg) in zip(m.parameters(), before):
            assert torch.equal(opt.state[p]["master"], avg) and torch.equal(opt.state[p]["ema"], master)
            assert torch.equal(p.detach(), avg.to(torch.bfloat16)) and not torch.equal(avg, master)
    for p, (shadow, master, avg) in zip(m.parameters(), before):
        assert torch.equal(p.detach(), shadow) and torch.equal(opt.state[p]["master"], master)
        assert torch.equal(opt.state[p]["ema"], avg)


def _train_wrapped(rank, world, steps, name):
    import distributed_learning_amd as dla
    from distributed_learning_amd.ops.loss import cross_entropy
    from test_wrappers_dist import TinyNet, _data

    torch.manual_seed(rank)  # different init per rank: the broadcast must make them equal
    model = TinyNet()
    dla.broadcast_parameters(model.state_dict(), root_rank=0)
    opt = dla.DistributedOptimizer(_cls(name)(model.parameters(), lr=0.05, weight_decay=1e-2, max_grad_norm=1.0),
                                   named_parameters=model.named_parameters(), bucket_cap_mb=0.001)
    start = {n: p.detach().clone() for n, p in model.named_parameters()}
    for s in range(steps):
        x, y = _data(rank, seed=s)
        opt.zero_grad()
        cross_entropy(model(x), y).backward()
        opt.step()
    return start, {n: p.detach().clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize("name", ["lamb", "adamw"])
def test_distributed_optimizer_wraps(name):
    res = run(_train_wrapped, 2, 3, name)
    (start, end0), (_, end1) = res
    for k in end0:
        assert torch.equal(end0[k], end1[k]), k  # bitwise equal across ranks
        assert not torch.equal(end0[k], start[k]), k  # and trained


def test_parser_accepts_adam_flags(capsys):
    from distributed_learning_amd.config import parse_args

    c = parse_args(POSITIONALS)
    assert (c.optimizer, c.beta1, c.beta2, c.opt_eps) == ("sgd", 0.9, 0.999, 1e-6)
    for name in ("lamb", "adamw"):
        c = parse_args(POSITIONALS + ["--optimizer", name, "--beta1", "0.8", "--beta2", "0.99", "--opt_eps", "1e-8",
                                      "--max_grad_norm", "1.5", "--warmup_steps", "5"])
        assert (c.optimizer, c.beta1, c.beta2, c.opt_eps, c.max_grad_norm) == (name, 0.8, 0.99, 1e-8, 1.5)
    with pytest.raises(SystemExit) as e:
        parse_args(POSITIONALS + ["--optimizer", "sgd", "--max_grad_norm", "1"])
    assert e.value.code == 2 and "--max_grad_norm needs --optimizer lars" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        parse_args(POSITIONALS + ["--optimizer", "lamb", "--opt_eps", "0"])
    assert e.value.code == 2 and "--opt_eps must be > 0" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_args(POSITIONALS + ["--optimizer", "adamw", "--beta2", "1.0"])
    assert "--beta1 and --beta2 must be in [0, 1)" in capsys.readouterr().err


def test_worker_optimizer_selection():
    from distributed_learning_amd.config import parse_args
    from distributed_learning_amd.train import make_optimizer, set_lr

    ps = [torch.zeros(3, 3, requires_grad=True)]
    for name in ("lamb", "adamw"):
        c = parse_args(POSITIONALS + ["--optimizer", name, "--beta1", "0.8", "--opt_eps", "1e-5", "--max_grad_norm", "2",
                                      "--lr", "0.004", "--weight_decay", "0.02", "--ema_decay", "0.99"])
        opt = make_optimizer(c, ps, True)
        assert type(opt) is _cls(name) and opt.defaults["betas"] == (0.8, 0.999) and opt.defaults["eps"] == 1e-5
        assert opt.defaults["weight_decay"] == 0.02 and opt.max_grad_norm == 2 and opt.master_weights
        assert opt.ema_enabled
        set_lr(opt, 0.5)
        assert opt.param_groups[0]["lr"] == 0.5


@pytest.mark.slow
def test_main_cli_lamb_two_workers(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "distributed_learning_amd.main", "1", "0", "2", "2", "127.0.0.1", "lo", "mnist",
           "/nonexistent", "0", "--optimizer", "lamb", "--lr", "0.002", "--weight_decay", "0.01", "--max_grad_norm", "1",
           "--warmup_steps", "2", "--total_steps", "10", "--random_input", "1", "--limit_batches", "3", "--batch_size",
           "8", "--master_port", str(free_port()), "--results_root", str(tmp_path), "--job_id", "t"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    files = sorted(tmp_path.glob("*/*_loss.txt"))
    assert len(files) == 2, files
    for w, f in enumerate(files):
        lines = f.read_text().splitlines()
        assert len(lines) == 3 and lines[0].startswith(f"Worker 0:{w} loss for batch 0: ")
        assert all(math.isfinite(float(ln.rsplit(": ", 1)[1])) for ln in lines)
