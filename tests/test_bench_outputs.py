"""``bench.py --dump-outputs`` / ``--full``: the options parse to a lean default, and the dump writes the same
bounded float32 arrays for the same state (whole small tensors, a fixed sample of large ones)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def bench(monkeypatch, tmp_path):
    # bench.py picks its MIOpen user database at import unless one is set: keep that out of this process
    monkeypatch.setenv("MIOPEN_USER_DB_PATH", str(tmp_path / "miopen_db"))
    monkeypatch.syspath_prepend(ROOT)
    import bench as b

    return b


def test_plain_run_is_the_default(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs, a.phases, a.bucket_mb_sweep) == (7, 2, False, None, 0, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "out"


class _Opt:
    def __init__(self, params):
        self.state = {p: {"master": p.detach().double().float() * 2} for p in params}


def test_dump_outputs_is_bounded_sampled_and_repeatable(bench, tmp_path, monkeypatch):
    torch.manual_seed(0)
    small, big = torch.nn.Linear(7, 5), torch.nn.Linear(300, 1000, bias=False)  # 35 + 5 and 300,000 elements
    model = torch.nn.Sequential(small, big).to(torch.bfloat16)
    params = list(model.parameters())
    for p in params:
        p.grad = torch.randn_like(p)
    params[1].grad = None  # a parameter without a gradient is left out of grads.npy only
    opt = _Opt(params)
    logits, loss = torch.randn(9, 11).to(torch.bfloat16), torch.tensor(6.90625)
    monkeypatch.setattr(bench, "DUMP_LOGITS_BYTES", 4 * 11 * 4)  # room for 4 of the 9 rows
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), loss, logits, model.named_parameters(), opt)
    got = {}
    for n in sorted(os.listdir(tmp_path / "a")):
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype == np.float32 and np.array_equal(x, y), n
        got[n[:-4]] = x
    assert sorted(got) == ["grads", "logits", "loss", "masters", "params"]
    cap = 1 << 16
    assert got["params"].shape == (35 + 5 + cap,) and got["masters"].shape == got["params"].shape
    assert got["grads"].shape == (35 + cap,)
    assert np.array_equal(got["params"][:35], params[0].detach().float().reshape(-1).numpy())
    assert np.array_equal(got["masters"], got["params"] * 2)  # the same elements of every set
    flat = params[2].detach().float().reshape(-1).numpy()
    assert np.isin(got["params"][40:], flat).all() and len(np.unique(got["params"][40:])) > 1
    assert got["logits"].shape == (4, 11) and got["loss"].tolist() == [6.90625]
    rows = logits.float().numpy()
    assert all(any(np.array_equal(r, q) for q in rows) for r in got["logits"])
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in os.listdir(tmp_path / "a")) < 64e6


def test_dump_sample_shrinks_to_the_byte_budget(bench, tmp_path, monkeypatch):
    model = torch.nn.Sequential(*[torch.nn.Linear(256, 256, bias=False) for _ in range(4)])  # 4 x 65,536
    monkeypatch.setattr(bench, "DUMP_SAMPLE_BYTES", 4 * 4 * 20000)  # one set (params) of 4 tensors
    bench.dump_outputs(str(tmp_path), torch.tensor(1.0), torch.zeros(2, 3), model.named_parameters(), _Opt([]))
    assert np.load(tmp_path / "params.npy").shape == (4 * 16384,)  # the cap halves from 65,536 until it fits


def test_miopen_db_copy_falls_back_when_build_cannot_be_written(bench, tmp_path, monkeypatch):
    root = tmp_path / "tree"
    (root / "miopen_db").mkdir(parents=True)
    (root / "miopen_db" / "x.udb.txt").write_text("tuned\n")
    monkeypatch.setattr(bench, "_ROOT", str(root))
    got = bench._miopen_user_db()
    assert os.path.dirname(got) == str(root / "build") and bench._miopen_user_db() == got
    assert open(os.path.join(got, "x.udb.txt")).read() == "tuned\n"
    (root / "miopen_db" / "x.udb.txt").write_text("retuned\n")  # a changed shipped database: a new copy
    assert bench._miopen_user_db() not in (got, str(root / "miopen_db"))
    blocked = tmp_path / "blocked"
    (blocked / "miopen_db").mkdir(parents=True)
    (blocked / "miopen_db" / "x.udb.txt").write_text("tuned\n")
    (blocked / "build").write_text("a file where the directory would go")
    monkeypatch.setattr(bench, "_ROOT", str(blocked))
    monkeypatch.setenv("XDG_CACHE_HOME", str(tmp_path / "cache"))
    got = bench._miopen_user_db()
    assert got.startswith(str(tmp_path / "cache" / "distributed_learning_amd"))
    assert open(os.path.join(got, "x.udb.txt")).read() == "tuned\n"
    assert open(blocked / "miopen_db" / "x.udb.txt").read() == "tuned\n" and os.path.isfile(blocked / "build")
