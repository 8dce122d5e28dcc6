"""The weight EMA on the CPU: the torch fallback of FusedSGD / FusedLARS against the float64 oracle and the
replay criteria of tests/ema_oracle.py, the decay schedule, ModelEMA, checkpoints, the CLI flags, and the proof
that the criteria catch the faults that can be injected into the oracle's fp32 emulation.

With EMA off nothing is new: no state, no checkpoint key, no eval_ema line."""
import os
import subprocess
import sys

import pytest
import torch

import dist_util
from ema_oracle import (EXACT_DECAYS, FAULTS, GENERAL_DECAYS, Emulation, check_step, ema_oracle_step, omd32)
from test_gpu_sgd import sgd_oracle_step
from test_lars import ATOL, POSITIONALS, RTOL, hyper, lars_oracle_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5,), (7, 3), (33, 17), (4, 3, 3, 3), (64,), (130, 70)]
NO_GRAD = {1: {2}, 2: {2, 4}}  # step -> tensors without a gradient in it


def _params(dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).to(dtype).requires_grad_() for s in SHAPES]


def _snapshot(opt, ps):
    out = []
    for p in ps:
        st = opt.state[p]
        target = st["master"] if "master" in st else p.detach().float()
        out.append((target.clone(), st["ema"].clone() if "ema" in st else None))
    return out


def _run(make, oracle, decay, dtype):
    """4 steps of the optimizer and of the float64 oracle; every step is held to the replay criteria, the end to
    RTOL / ATOL against the oracle."""
    ps = _params(dtype)
    opt = make(ps, decay)
    omd = omd32(decay)
    P = [p.detach().double().clone() for p in ps]
    E = [None] * len(ps)
    gen = torch.Generator().manual_seed(1)
    for step in range(4):
        grads = [None if i in NO_GRAD.get(step, ()) else torch.randn(p.shape, generator=gen).to(dtype)
                 for i, p in enumerate(ps)]
        for p, g in zip(ps, grads):
            p.grad = g
        before = _snapshot(opt, ps)
        opt.step()
        after = _snapshot(opt, ps)
        assert check_step(before, after, [g is not None for g in grads], omd, decay in EXACT_DECAYS) == set()
        P_old = [p.clone() for p in P]
        oracle(P, grads, opt)
        ema_oracle_step(E, P_old, P, grads, omd)
    for p, e64 in zip(ps, E):
        e = opt.state[p]["ema"]
        assert e.dtype == torch.float32
        torch.testing.assert_close(e, e64.float(), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("decay", EXACT_DECAYS + GENERAL_DECAYS)
def test_sgd_fallback_matches_oracle(decay, dtype):
    from distributed_learning_amd.ops.optim import FusedSGD

    kw = dict(lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True)
    M = [None] * len(SHAPES)
    hp = dict(kw, dampening=0.0, grad_scale=1.0)

    def oracle(P, grads, opt):
        sgd_oracle_step(P, M, grads, [hp] * len(P))

    _run(lambda ps, d: FusedSGD(ps, master_weights=dtype != torch.float32, ema_decay=d, **kw), oracle, decay, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("decay", EXACT_DECAYS + GENERAL_DECAYS)
def test_lars_fallback_matches_oracle(decay, dtype):
    from distributed_learning_amd.ops.optim import FusedLARS

    M = [torch.zeros(s, dtype=torch.float64) for s in SHAPES]

    def oracle(P, grads, opt):
        lars_oracle_step(P, M, grads, hyper(opt), 0.5, 0.5)

    _run(lambda ps, d: FusedLARS(ps, lr=0.3, momentum=0.9, weight_decay=1e-4, grad_scale=0.5, max_grad_norm=0.5,
                                 master_weights=dtype != torch.float32, ema_decay=d), oracle, decay, dtype)


def test_ema_does_not_perturb_the_update():
    from distributed_learning_amd.ops.optim import FusedLARS, FusedSGD

    for cls, kw in ((FusedSGD, dict(lr=0.1, momentum=0.9)), (FusedLARS, dict(lr=0.3, weight_decay=1e-4))):
        a, b = _params(torch.bfloat16), _params(torch.bfloat16)
        oa, ob = cls(a, master_weights=True, **kw), cls(b, master_weights=True, ema_decay=0.99, **kw)
        gen = torch.Generator().manual_seed(2)
        for _ in range(3):
            for p, q in zip(a, b):
                p.grad = torch.randn(p.shape, generator=gen).to(p.dtype)
                q.grad = p.grad.clone()
            oa.step()
            ob.step()
            for p, q in zip(a, b):
                assert torch.equal(p, q)
                for k in ("master", "momentum_buffer"):
                    assert torch.equal(oa.state[p][k], ob.state[q][k])
                assert "ema" not in oa.state[p] and ob.state[q]["ema"].dtype == torch.float32


def test_ema_decay_at():
    from distributed_learning_amd.ops.optim import ema_decay_at

    assert [ema_decay_at(t, 0.9999, False) for t in (0, 1, 10 ** 6)] == [0.9999] * 3
    assert ema_decay_at(0, 0.9999, True) == 0.1
    assert ema_decay_at(1, 0.9999, True) == 2 / 11
    assert ema_decay_at(90, 0.9999, True) == 0.91
    assert ema_decay_at(90, 0.9, True) == 0.9
    assert ema_decay_at(10 ** 7, 0.9999, True) == 0.9999
    vals = [ema_decay_at(t, 0.999, True) for t in range(20000)]
    assert all(a <= b for a, b in zip(vals, vals[1:])) and vals[-1] == 0.999


def test_constructor_and_set_ema_decay_reject_bad_values():
    from distributed_learning_amd.ops.optim import FusedLARS, FusedSGD, ModelEMA

    ps = _params(torch.float32)
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError):
            FusedSGD(ps, ema_decay=bad)
        with pytest.raises(ValueError):
            FusedLARS(ps, lr=0.1, ema_decay=bad)
    off = FusedSGD(ps)
    with pytest.raises(ValueError):
        off.set_ema_decay(0.9)
    with pytest.raises(ValueError):
        ModelEMA(torch.nn.Linear(2, 2), off, 0.9)
    on = FusedSGD(ps, ema_decay=0.9)
    on.set_ema_decay(0.5)
    assert on.ema_decay == 0.5
    with pytest.raises(ValueError):
        on.set_ema_decay(1.0)


def _bn_model(dtype=torch.float32, seed=3):
    torch.manual_seed(seed)
    m = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.BatchNorm2d(8), torch.nn.ReLU(),
                            torch.nn.Flatten(), torch.nn.Linear(8 * 6 * 6, 5))
    if dtype != torch.float32:
        for mod in m:
            if isinstance(mod, (torch.nn.Conv2d, torch.nn.Linear)):
                mod.to(dtype)
    return m


def _train_step(model, seed):
    """Gradients from a seed (no autograd: bf16 convolutions are not the point), and new BatchNorm statistics."""
    g = torch.Generator().manual_seed(seed)
    for p in model.parameters():
        p.grad = torch.randn(p.shape, generator=g).to(p.dtype)
    bn = model[1]
    with torch.no_grad():
        bn.running_mean.add_(torch.randn(8, generator=g))
        bn.running_var.mul_(1 + 0.1 * torch.rand(8, generator=g))
        bn.num_batches_tracked.add_(1)


def _everything(model, opt, ema):
    out = [p.detach().clone() for p in model.parameters()] + [b.clone() for b in model.buffers()]
    for p in model.parameters():
        out += [v.clone() for k, v in sorted(opt.state[p].items()) if torch.is_tensor(v)]
    return out + [e.clone() for _, e in sorted(ema.buffers.items())]


def test_model_ema_step_buffers_and_applied():
    from distributed_learning_amd.ops.optim import FusedSGD, ModelEMA

    model = _bn_model(torch.bfloat16)
    opt = FusedSGD(model.parameters(), lr=0.1, momentum=0.9, master_weights=True, ema_decay=0.5)
    ema = ModelEMA(model, opt, 1 - 2.0 ** -3, warmup=True)
    assert sorted(ema.buffers) == ["1.running_mean", "1.running_var"]  # num_batches_tracked is left alone
    rm0 = model[1].running_mean.clone()
    for s in range(3):
        _train_step(model, s)
        e_old = ema.buffers["1.running_mean"].clone()
        ema.step(s)
        d = min(1 - 2.0 ** -3, (1 + s) / (10 + s))
        assert opt.ema_decay == d
        want = e_old + (model[1].running_mean - e_old) * omd32(d)
        torch.testing.assert_close(ema.buffers["1.running_mean"], want, rtol=2.0 ** -22, atol=0)
    assert not torch.equal(ema.buffers["1.running_mean"], rm0)
    before = _everything(model, opt, ema)
    tracked = model[1].num_batches_tracked.clone()
    with ema.applied():
        for p in model.parameters():
            st = opt.state[p]
            if p.dtype == torch.bfloat16:
                assert torch.equal(p.detach(), st["master"].to(torch.bfloat16))
            assert not torch.equal(st["ema"], (st["master"] if "master" in st else p.detach()))
        inside = _everything(model, opt, ema)
        assert torch.equal(model[1].num_batches_tracked, tracked)
    # masters / fp32 parameters / buffers held the averages inside, and everything is back
    n = len(list(model.parameters()))
    for i, p in enumerate(model.parameters()):
        st_before = {k: v for k, v in opt.state[p].items()}
        target_inside = inside[i] if p.dtype == torch.float32 else None
        if target_inside is not None:
            assert torch.equal(target_inside, st_before["ema"])
    assert torch.equal(inside[n], before[-2]) and torch.equal(inside[n + 1], before[-1])  # buffers held their EMAs
    after = _everything(model, opt, ema)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    exported = ema.model_state_dict()
    assert torch.equal(exported["1.running_mean"], ema.buffers["1.running_mean"])
    assert torch.equal(exported["0.weight"], opt.state[model[0].weight]["ema"].to(torch.bfloat16))
    assert all(torch.equal(a, b) for a, b in zip(before, _everything(model, opt, ema)))


def test_applied_restores_after_an_exception():
    from distributed_learning_amd.ops.optim import FusedLARS, ModelEMA

    model = _bn_model(torch.bfloat16)
    opt = FusedLARS(model.parameters(), lr=0.3, master_weights=True, ema_decay=0.9)
    ema = ModelEMA(model, opt, 0.9)
    for s in range(2):
        _train_step(model, s)
        ema.step(s)
    before = _everything(model, opt, ema)
    with pytest.raises(ZeroDivisionError):
        with ema.applied():
            assert not all(torch.equal(a, b) for a, b in zip(before, _everything(model, opt, ema)))
            1 / 0
    assert all(torch.equal(a, b) for a, b in zip(before, _everything(model, opt, ema)))


def test_default_off_adds_nothing(tmp_path):
    from distributed_learning_amd.ops.optim import FusedLARS, FusedSGD
    from distributed_learning_amd.train import save_checkpoint

    model = _bn_model()
    for opt in (FusedSGD(model.parameters(), lr=0.1, momentum=0.9), FusedLARS(model.parameters(), lr=0.1)):
        _train_step(model, 0)
        opt.step()
        sd = opt.state_dict()
        assert all("ema" not in st for st in sd["state"].values()) and "ema" not in sd
        assert all("ema" not in k for g in sd["param_groups"] for k in g)
        path = str(tmp_path / "off.pt")
        save_checkpoint(path, model, opt, 1)
        assert sorted(torch.load(path, weights_only=True)) == ["extra", "model", "optimizer", "rng", "step"]


def _six_steps(tmp_path, cls, kw, split):
    from distributed_learning_amd.ops.optim import ModelEMA
    from distributed_learning_amd.train import load_checkpoint, save_checkpoint

    def make():
        model = _bn_model(torch.bfloat16)
        opt = cls(model.parameters(), master_weights=True, ema_decay=0.999, **kw)
        return model, opt, ModelEMA(model, opt, 0.999, warmup=True)

    model, opt, ema = make()
    for s in range(6):
        if split and s == 3:
            path = str(tmp_path / "ema.pt")
            save_checkpoint(path, model, opt, 3, ema=ema)
            assert "ema" in torch.load(path, weights_only=True)
            model, opt, ema = make()
            model[1].running_mean.fill_(7.0)  # the load must bring the buffers and their averages back
            assert load_checkpoint(path, model, opt, ema=ema) == 3
            assert all(opt.state[p]["ema"].dtype == torch.float32 for p in model.parameters())
        _train_step(model, s)
        ema.step(s)  # the global batch number: the warmup continues where it was
    return _everything(model, opt, ema)


@pytest.mark.parametrize("name", ["sgd", "lars"])
def test_checkpoint_roundtrip_continues_bit_exactly(tmp_path, name):
    from distributed_learning_amd.ops.optim import FusedLARS, FusedSGD

    cls, kw = {"sgd": (FusedSGD, dict(lr=0.1, momentum=0.9)), "lars": (FusedLARS, dict(lr=0.3, weight_decay=1e-4))}[name]
    whole, resumed = _six_steps(tmp_path, cls, kw, False), _six_steps(tmp_path, cls, kw, True)
    assert len(whole) == len(resumed) and all(torch.equal(a, b) for a, b in zip(whole, resumed))


def test_resume_without_ema_state_starts_from_the_loaded_weights(tmp_path):
    from distributed_learning_amd.ops.optim import FusedSGD, ModelEMA
    from distributed_learning_amd.train import load_checkpoint, save_checkpoint

    model = _bn_model()
    opt = FusedSGD(model.parameters(), lr=0.1, momentum=0.9)
    for s in range(2):
        _train_step(model, s)
        opt.step()
    path = str(tmp_path / "plain.pt")
    save_checkpoint(path, model, opt, 2)
    m2 = _bn_model(seed=4)
    o2 = FusedSGD(m2.parameters(), lr=0.1, momentum=0.9, ema_decay=0.75)
    e2 = ModelEMA(m2, o2, 0.75)
    assert load_checkpoint(path, m2, o2, ema=e2) == 2
    assert torch.equal(e2.buffers["1.running_mean"], model[1].running_mean)
    loaded = [p.detach().clone() for p in m2.parameters()]
    _train_step(m2, 2)
    e2.step(2)
    for p, p0 in zip(m2.parameters(), loaded):  # e = p0 + omd * (p1 - p0): omd = 2^-2, exact
        assert torch.equal(o2.state[p]["ema"], p0 + (p.detach() - p0) * 0.25)


def test_parser_accepts_and_rejects_ema_flags(capsys):
    from distributed_learning_amd.config import parse_args
    from distributed_learning_amd.ops.optim import FusedLARS, FusedSGD
    from distributed_learning_amd.train import _config_text, make_optimizer

    c = parse_args(POSITIONALS)
    assert (c.ema_decay, c.ema_warmup) == (0.0, 0)
    assert "ema" not in _config_text(c)
    ps = [torch.zeros(3, 3, requires_grad=True)]
    assert not make_optimizer(c, ps, False).ema_enabled
    c = parse_args(POSITIONALS + ["--ema_decay", "0.9999", "--ema_warmup", "1"])
    assert (c.ema_decay, c.ema_warmup) == (0.9999, 1) and "ema_decay=0.9999" in _config_text(c)
    opt = make_optimizer(c, ps, False)
    assert type(opt) is FusedSGD and opt.ema_enabled and opt.ema_decay == 0.9999
    c = parse_args(POSITIONALS + ["--ema_decay", "0.5", "--optimizer", "lars"])
    opt = make_optimizer(c, ps, True)
    assert type(opt) is FusedLARS and opt.ema_enabled and opt.master_weights
    for bad in ("1", "-0.1"):
        with pytest.raises(SystemExit) as e:
            parse_args(POSITIONALS + ["--ema_decay", bad])
        assert e.value.code == 2 and "--ema_decay must be in [0, 1)" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_args(POSITIONALS + ["--ema_warmup", "2"])


def _wrapped(rank, world):
    import distributed_learning_amd as dla
    from distributed_learning_amd.ops.optim import FusedSGD
    from test_wrappers_dist import TinyNet

    torch.manual_seed(0)
    model = TinyNet()
    inner = FusedSGD(model.parameters(), lr=0.1, ema_decay=0.9)
    opt = dla.DistributedOptimizer(inner, named_parameters=model.named_parameters())
    opt.set_ema_decay(0.75)
    return inner.ema_decay


def test_distributed_optimizer_forwards_set_ema_decay():
    assert dist_util.run(_wrapped, 1) == [0.75]


def _cli(tmp_path, sub, workers, *extra):
    out = tmp_path / sub
    out.mkdir()
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "distributed_learning_amd.main", "1", "0", str(workers), str(workers), "127.0.0.1",
           "lo", "mnist", "/nonexistent", "0", "--random_input", "1", "--limit_batches", "2", "--batch_size", "8",
           "--eval_batches", "1", "--eval_every", "1", "--master_port", str(dist_util.free_port()),
           "--results_root", str(out), "--job_id", "t", *extra]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(out))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return out


@pytest.mark.slow
def test_main_cli_ema_two_workers(tmp_path):
    out = _cli(tmp_path, "ema", 2, "--ema_decay", "0.9", "--ema_warmup", "1", "--optimizer", "lars")
    files = sorted(out.glob("*/*_eval.txt"))
    assert len(files) == 2, files
    values = []
    for w, f in enumerate(files):
        lines = f.read_text().splitlines()
        assert [ln.split()[2] for ln in lines] == ["eval", "eval_ema"] * 2
        for b, ln in zip((1, 1, 2, 2), lines):
            assert ln.startswith(f"Worker 0:{w} {ln.split()[2]} at batch {b}: loss ") and ln.endswith(" samples 16")
        assert lines[0].split()[3:] != lines[1].split()[3:]  # the averaged model is another model
        values.append([ln.split()[3:] for ln in lines])
    assert values[0] == values[1]  # all-reduced metrics, identical weights and averages on both ranks


@pytest.mark.slow
def test_cli_without_ema_writes_no_eval_ema(tmp_path):
    out = _cli(tmp_path, "off", 1, "--experiment", "experiment_single")
    lines = next(out.glob("*/*_eval.txt")).read_text().splitlines()
    assert [ln.split()[2] for ln in lines] == ["eval", "eval"]
    assert "ema_decay" not in next(out.glob("*/*_config.txt")).read_text()


def test_worker_result_and_checkpoint_keys_with_and_without_ema(tmp_path):
    """The training loop in this process (no process group): the result, the eval file and the checkpoint."""
    from distributed_learning_amd.config import parse_args
    from distributed_learning_amd.experiments import main_single

    def run(name, *extra):
        c = parse_args(POSITIONALS + ["--random_input", "1", "--limit_batches", "2", "--batch_size", "8",
                                      "--eval_batches", "1", "--checkpoint", str(tmp_path / f"{name}.pt"), *extra])
        c.folder = str(tmp_path / name)
        r = main_single(c)
        lines = (tmp_path / name / "single_0_0_eval.txt").read_text().splitlines()
        return r, lines, torch.load(str(tmp_path / f"{name}.pt"), weights_only=True)

    r, lines, ck = run("off")
    assert "evals_ema" not in r and len(r["evals"]) == 1 and [ln.split()[2] for ln in lines] == ["eval"]
    assert sorted(ck) == ["extra", "model", "optimizer", "rng", "step"]
    assert all("ema" not in st for st in ck["optimizer"]["state"].values())
    r2, lines, ck = run("on", "--ema_decay", "0.9")
    assert r2["losses"] == r["losses"] and r2["evals"][0]["loss"] == r["evals"][0]["loss"]  # the run is the same run
    assert len(r2["evals_ema"]) == 1 and r2["evals_ema"][0]["batch"] == 2
    assert r2["evals_ema"][0]["loss"] != r2["evals"][0]["loss"]
    assert [ln.split()[2] for ln in lines] == ["eval", "eval_ema"]
    assert sorted(ck) == ["ema", "extra", "model", "optimizer", "rng", "step"]
    assert all(st["ema"].dtype == torch.float32 for st in ck["optimizer"]["state"].values())
    # resumed with the schedule position: batches 2 and 3
    c = parse_args(POSITIONALS + ["--random_input", "1", "--limit_batches", "2", "--batch_size", "8", "--ema_decay",
                                  "0.9", "--resume", str(tmp_path / "on.pt")])
    c.folder = str(tmp_path / "resumed")
    assert main_single(c)["start_step"] == 2


def _emulate(decay, fault, steps=4):
    """The emulation with one fault against the criteria and against RTOL / ATOL alone: (criteria that failed,
    whether the RTOL / ATOL comparison with the float64 oracle passed)."""
    g = torch.Generator().manual_seed(5)
    start = [torch.randn(s, generator=g) for s in SHAPES]
    emu = Emulation(start, decay, fault=fault)
    omd = omd32(decay)
    P = [t.double() for t in start]
    E = [None] * len(start)
    failed = set()
    for step in range(steps):
        grads = [None if i in NO_GRAD.get(step, ()) else torch.randn(p.shape, generator=g)
                 for i, p in enumerate(start)]
        before = emu.snapshot()
        emu.step(grads)
        failed |= check_step(before, emu.snapshot(), [x is not None for x in grads], omd, decay in EXACT_DECAYS)
        P_old = [p.clone() for p in P]
        P = [p if x is None else (p.float() - 0.1 * x).double() for p, x in zip(P, grads)]  # the emulation's own p
        ema_oracle_step(E, P_old, P, grads, omd)
    tol_ok = all(torch.allclose(e, e64.float(), rtol=RTOL, atol=ATOL) for e, e64 in zip(emu.e, E))
    return failed, tol_ok


@pytest.mark.parametrize("decay", EXACT_DECAYS + GENERAL_DECAYS)
def test_criteria_catch_injected_faults(decay):
    failed, tol_ok = _emulate(decay, None)
    assert failed == set() and tol_ok  # the formula itself passes everything
    caught_by = {"decay_for_omd": {"replay", "first"}, "from_p_old": {"replay", "first"},
                 "from_shadow": {"replay", "first"}, "no_init": {"first"}, "advance_without_grad": {"untouched"}}
    report = {}
    for fault in FAULTS:
        failed, tol_ok = _emulate(decay, fault)
        report[fault] = (sorted(failed), tol_ok)
        assert failed & caught_by[fault], (fault, decay, failed)
    print(f"decay {decay}: " + "; ".join(f"{k}: criteria {v[0]}, RTOL/ATOL alone {'passes' if v[1] else 'fails'}"
                                         for k, v in report.items()))
    # faults of the size of the weights are outside any tolerance
    assert not report["no_init"][1] and not report["decay_for_omd"][1]
    if decay == 0.9999:
        # omd * 2^-9 relative, about 2e-7: under RTOL. Only the replay criteria see this one.
        assert report["from_shadow"][1]
