"""Label-smoothed cross-entropy with top-1 / top-k counts, the evaluation pass and its data (CPU).

Oracles: the loss and its gradient are float64 ``F.cross_entropy(label_smoothing=eps, ignore_index=-100)``;
the counts are the tie rule written out below in float64 (``rank = #{c: x_c > x_t} + #{c < t: x_c == x_t}``,
a valid row is top-k correct iff ``rank < k``, a NaN target logit is never correct).

Bounds (also used by tests/test_gpu_loss_metrics.py): those of tests/test_gpu_kernels.py::test_xent_vs_torch
-- loss rtol/atol 1e-5; gradient rtol 1e-4 / atol 1e-7 in fp32 and rtol 2e-2 / atol 1e-4 in bf16.

Count inputs: random targets on random logits are correct in no row, which a kernel that writes zeros would
pass. So row i's target logit is overwritten with the row's (i mod 10)-th largest value: ranks fall on both
sides of k = 1 and k = 5 and every row holds an exact tie.
"""
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import dist_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LOSS_TOL = dict(rtol=1e-5, atol=1e-5)
GRAD_TOL = {torch.float32: dict(rtol=1e-4, atol=1e-7), torch.bfloat16: dict(rtol=2e-2, atol=1e-4)}


def make_case(B, C, dtype=torch.float32, seed=0, scale=3.0, ignore=True):
    """(logits, targets) on the CPU: logits as stored in ``dtype``; targets -100 and >= C among them."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, C, generator=g) * scale).to(dtype)
    y = torch.randint(0, C, (B,), generator=g)
    for i in range(B):
        x[i, y[i]] = torch.sort(x[i].float(), descending=True).values[i % min(10, C)].to(dtype)
    if ignore and B > 3:
        y[1] = -100
    if ignore and B > 4:
        y[3] = C + 3
    return x, y


def oracle_counts(x, y, k):
    """(valid rows, top-1 correct, top-k correct) by the tie rule, in float64."""
    x64 = x.detach().double().cpu()
    C = x64.shape[1]
    n = c1 = ck = 0
    for i, t in enumerate(y.cpu().tolist()):
        if not 0 <= t < C:
            continue
        n += 1
        xt = x64[i, t]
        if math.isnan(float(xt)):
            continue
        rank = int((x64[i] > xt).sum()) + int((x64[i, :t] == xt).sum())
        c1 += rank < 1
        ck += rank < k
    return n, c1, ck


def oracle_loss_grad(x, y, eps):
    """float64 loss and gradient of the stored logits."""
    C = x.shape[1]
    x64 = x.detach().double().cpu().requires_grad_(True)
    t = y.cpu().clone()
    t[(t < 0) | (t >= C)] = -100
    loss = F.cross_entropy(x64, t, label_smoothing=eps, ignore_index=-100)
    loss.backward()
    return loss.detach(), x64.grad


def check_against_oracle(x, y, eps, k, dtype, strict=True):
    """Run cross_entropy_with_metrics on (x, y) where they live and compare everything with the oracles."""
    from distributed_learning_amd.ops import cross_entropy_with_metrics

    n, c1, ck = oracle_counts(x, y, k)
    c5 = oracle_counts(x, y, 5)[2]
    assert 0 < c5 <= n  # a count that is always zero cannot pass
    if strict:  # enough rows: top-1 and top-5 both strictly between none and all of the valid rows
        assert 0 < c1 < n and c5 < n
    xr = x.detach().requires_grad_(True)  # the same storage: a test may depend on its alignment
    loss, stats = cross_entropy_with_metrics(xr, y, eps, k)
    loss.backward()
    assert stats.dtype == torch.float32 and stats.shape == (4,) and stats.device == x.device
    assert not stats.requires_grad and xr.grad.dtype == x.dtype
    assert stats[1:].tolist() == [float(n), float(c1), float(ck)]
    ref, gref = oracle_loss_grad(x, y, eps)
    print(f"loss err {abs(float(loss.detach()) - float(ref)):.3g}, worst grad err "
          f"{float((xr.grad.double().cpu() - gref).abs().max()):.3g}")
    torch.testing.assert_close(loss.detach().double().cpu(), ref, **LOSS_TOL)
    torch.testing.assert_close((stats[0] / stats[1]).double().cpu(), ref, **LOSS_TOL)
    torch.testing.assert_close(xr.grad.double().cpu(), gref, **GRAD_TOL[dtype])
    return loss.detach(), stats, xr.grad


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("B,C", [(256, 1000), (129, 4097)])
def test_fallback_matches_oracles(B, C, eps, k):
    x, y = make_case(B, C)
    check_against_oracle(x, y, eps, k, torch.float32)


def test_fallback_float64_and_bf16_inputs():
    x, y = make_case(64, 100, seed=3)
    loss, _, _ = check_against_oracle(x.double(), y, 0.1, 5, torch.float32)
    assert loss.dtype == torch.float64
    xb, yb = make_case(64, 100, torch.bfloat16, seed=4)
    check_against_oracle(xb, yb, 0.1, 5, torch.bfloat16)


def edge_case_counts(device, dtype):
    """The tie, ignored-row, NaN and all-equal cases; shared with the GPU file."""
    from distributed_learning_amd.ops import cross_entropy_with_metrics

    def counts(x, y, k):
        return cross_entropy_with_metrics(x.to(device, dtype), y.to(device), 0.0, k)[1][1:].tolist()

    # all-equal rows: correct at k iff t < k
    x = torch.full((12, 12), 0.5)
    y = torch.arange(12)
    for k in (1, 5, 11):
        assert counts(x, y, k) == [12.0, 1.0, float(k)]
    # k >= C: every valid row, and only those
    x, y = make_case(9, 10, dtype, seed=5)
    for k in (10, 11, 1 << 30):
        got = counts(x, y, k)
        assert got[0] == 7.0 and got[2] == 7.0, got
    # targets -100, -1 and >= C are ignored: the counts equal those of the remaining rows alone
    x, y = make_case(40, 37, dtype, seed=6, ignore=False)
    y2 = y.clone()
    y2[0], y2[5], y2[6], y2[39] = -100, 37, -1, 1 << 40
    keep = torch.tensor([i for i in range(40) if i not in (0, 5, 6, 39)])
    assert counts(x, y2, 5) == counts(x[keep], y[keep], 5) == [float(v) for v in oracle_counts(x, y2, 5)]
    # an exact tie: the smaller class index wins
    x = torch.tensor([[1.0, 2.0, 2.0, 0.0], [1.0, 2.0, 2.0, 0.0]])
    assert counts(x, torch.tensor([1, 2]), 1) == [2.0, 1.0, 1.0]
    assert counts(x, torch.tensor([1, 2]), 2) == [2.0, 1.0, 2.0]
    # a NaN target logit is wrong at every k; the row stays valid
    x, y = make_case(8, 20, dtype, seed=7, ignore=False)
    base = counts(x, y, 20)
    assert base == [8.0, oracle_counts(x, y, 20)[1], 8.0]
    x[2, y[2]] = float("nan")
    assert counts(x, y, 20) == [8.0, float(oracle_counts(x, y, 20)[1]), 7.0]
    assert counts(x, y, 1 << 30)[2] == 7.0


def test_edge_cases_fallback():
    edge_case_counts("cpu", torch.float32)
    edge_case_counts("cpu", torch.bfloat16)


def test_zero_valid_rows_and_argument_checks():
    from distributed_learning_amd.ops import cross_entropy, cross_entropy_with_metrics

    x, _ = make_case(4, 10)
    loss, stats = cross_entropy_with_metrics(x, torch.full((4,), -100), 0.1, 5)
    assert math.isnan(float(loss)) and stats.tolist() == [0.0, 0.0, 0.0, 0.0]
    y = torch.zeros(4, dtype=torch.long)
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            cross_entropy_with_metrics(x, y, bad)
        with pytest.raises(ValueError):
            cross_entropy(x, y, bad)
    with pytest.raises(ValueError):
        cross_entropy_with_metrics(x, y, 0.0, 0)


def test_default_cross_entropy_is_unchanged():
    """No argument: the value of the formula the fallback always used, bit for bit; eps > 0: the smoothed loss."""
    from distributed_learning_amd.ops import cross_entropy

    g = torch.Generator().manual_seed(11)
    x = torch.randn(33, 50, generator=g) * 3
    y = torch.randint(0, 50, (33,), generator=g)
    assert torch.equal(cross_entropy(x, y), F.nll_loss(F.log_softmax(x.float(), dim=1), y))
    assert torch.equal(cross_entropy(x, y, 0.0), cross_entropy(x, y))
    torch.testing.assert_close(cross_entropy(x, y, 0.1).double(), F.cross_entropy(x.double(), y, label_smoothing=0.1),
                               **LOSS_TOL)


# --- evaluate() -----------------------------------------------------------------------------------
def _basicnet_and_streams(seed=0):
    from distributed_learning_amd.data import SyntheticBatches
    from distributed_learning_amd.models import create_network

    torch.manual_seed(seed)
    model = create_network("basicnet")
    train = SyntheticBatches(8, (1, 28, 28), 10, "cpu", seed=1)
    val = SyntheticBatches(8, (1, 28, 28), 10, "cpu", seed=2)
    return model, train, val


def test_evaluate_equals_a_loop_and_leaves_training_alone():
    from distributed_learning_amd.data import SyntheticBatches
    from distributed_learning_amd.ops import cross_entropy_with_metrics
    from distributed_learning_amd.train import evaluate

    model, train, val = _basicnet_and_streams()
    model.train()
    for _ in range(2):
        train.next()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    rng = torch.get_rng_state().clone()
    got = evaluate(model, val, "cpu", "fp32", 3, topk=3)
    again = evaluate(model, val, "cpu", "fp32", 3, topk=3)  # rewound: the same batches every time
    assert got == again and got["samples"] == 24 and got["k"] == 3
    assert model.training and all(m.training for m in model.modules())
    assert torch.equal(torch.get_rng_state(), rng) and train.step == 2
    for k, v in model.state_dict().items():
        assert torch.equal(v, state[k]), k
    # by hand
    ref = SyntheticBatches(8, (1, 28, 28), 10, "cpu", seed=2)
    total = torch.zeros(4, dtype=torch.float64)
    model.eval()
    with torch.no_grad():
        for _ in range(3):
            x, y = ref.next()
            total += cross_entropy_with_metrics(model(x), y, 0.0, 3)[1].double()
    model.train()
    assert got["samples"] == int(total[1])
    assert got["loss"] == pytest.approx(float(total[0] / total[1]), rel=1e-6)
    assert got["top1"] == float(total[2] / total[1]) and got["topk"] == float(total[3] / total[1])
    assert 0.0 <= got["top1"] <= got["topk"] <= 1.0 and got["topk"] > 0.0
    # a module frozen in eval mode stays frozen
    model.dropout1.eval()
    frozen = [m.training for m in model.modules()]
    evaluate(model, val, "cpu", "fp32", 1)
    assert [m.training for m in model.modules()] == frozen


def _eval_rank(rank, world):
    from distributed_learning_amd.data import SyntheticBatches
    from distributed_learning_amd.train import evaluate

    model, _, _ = _basicnet_and_streams()
    both = evaluate(model, SyntheticBatches(8, (1, 28, 28), 10, "cpu", seed=2, rank=rank), "cpu", "fp32", 2, topk=5)
    # this rank's own share, without the collective
    own = _own_stats(model, SyntheticBatches(8, (1, 28, 28), 10, "cpu", seed=2, rank=rank), 2)
    return both, own


def _own_stats(model, val, batches):
    from distributed_learning_amd.ops import cross_entropy_with_metrics

    total = torch.zeros(4, dtype=torch.float64)
    model.eval()
    with torch.no_grad():
        for _ in range(batches):
            x, y = val.next()
            total += cross_entropy_with_metrics(model(x), y, 0.0, 5)[1].double()
    model.train()
    return total


@pytest.mark.slow
def test_evaluate_two_gloo_ranks():
    (a, own0), (b, own1) = dist_util.run(_eval_rank, 2)
    assert a == b
    total = own0 + own1
    assert a["samples"] == int(total[1]) == 32
    assert a["loss"] == pytest.approx(float(total[0] / total[1]), rel=1e-6)
    assert a["top1"] == pytest.approx(float(total[2] / total[1])) and a["topk"] == pytest.approx(float(total[3] / total[1]))
    assert not torch.equal(own0, own1)  # the ranks did see different batches


# --- held-out data --------------------------------------------------------------------------------
def test_padded_partition_counts_every_sample_once():
    from distributed_learning_amd.data import TensorDataset, get_eval_loader

    n, bs, world = 23, 4, 2
    ds = TensorDataset(torch.arange(n, dtype=torch.float32).reshape(n, 1, 1, 1).expand(n, 1, 2, 2).contiguous() + 1.0,
                       torch.arange(n) % 10)
    seen, lengths = [], []
    rng = torch.get_rng_state().clone()
    for r in range(world):
        loader = get_eval_loader(ds, r, world, bs)
        batches = list(loader)
        lengths.append(len(batches))
        assert len(loader) == len(batches)
        for x, y in batches:
            assert x.shape == (bs, 1, 2, 2) and y.shape == (bs,) and y.dtype == torch.long
            real = y != -100
            assert torch.equal(real, x[:, 0, 0, 0] != 0)  # padding rows: zero image and target -100
            assert (x[~real] == 0).all()
            idx = (x[real, 0, 0, 0] - 1).long()
            assert torch.equal(y[real], idx % 10)
            assert all(int(i) % world == r for i in idx)  # rank r takes r, r + W, ... in file order
            seen += idx.tolist()
        own = [i for i in seen if i % world == r]
        assert own == sorted(own)
    assert torch.equal(torch.get_rng_state(), rng)  # iterating draws nothing from the global stream
    assert sorted(seen) == list(range(n))
    assert lengths == [3, 3]
    # a rank whose share ends a whole batch early still runs every batch: 9 samples, batch 4, 2 ranks -> 5 + 4
    ds9 = TensorDataset(torch.ones(9, 1, 2, 2), torch.zeros(9, dtype=torch.long))
    per = [[int((y != -100).sum()) for _, y in get_eval_loader(ds9, r, 2, 4)] for r in range(2)]
    assert per == [[4, 1], [4, 0]]
    # more ranks than samples
    per = [[int((y != -100).sum()) for _, y in get_eval_loader(ds9, r, 12, 4)] for r in (0, 8, 11)]
    assert per == [[1], [1], [0]]


def test_load_dataset_held_out_splits(tmp_path):
    import struct

    from distributed_learning_amd.data import load_dataset

    d = tmp_path / "mnist" / "MNIST" / "raw"
    d.mkdir(parents=True)
    for stem, n in (("train", 6), ("t10k", 4)):
        with open(d / f"{stem}-images-idx3-ubyte", "wb") as f:
            f.write(struct.pack(">IIII", 0x0803, n, 28, 28) + bytes(n * 28 * 28))
        with open(d / f"{stem}-labels-idx1-ubyte", "wb") as f:
            f.write(struct.pack(">II", 0x0801, n) + bytes(range(n)))
    assert len(load_dataset("mnist", str(tmp_path))) == 6
    assert len(load_dataset("mnist", str(tmp_path), train=False)) == 4
    c = tmp_path / "cifar-10-batches-bin"
    c.mkdir()
    (c / "test_batch.bin").write_bytes(bytes(3 * 3073))
    assert len(load_dataset("cifar10", str(tmp_path), train=False)) == 3
    with pytest.raises(FileNotFoundError, match="ImageFolderVal"):
        load_dataset("imagenet", str(tmp_path), train=False)


# --- command line ---------------------------------------------------------------------------------
def _cli(tmp_path, sub, *extra):
    out = tmp_path / sub
    out.mkdir()
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "distributed_learning_amd.main", "1", "0", "1", "1", "127.0.0.1", "lo", "mnist",
           "/nonexistent", "0", "--experiment", "experiment_single", "--random_input", "1", "--limit_batches", "3",
           "--batch_size", "8", "--master_port", str(dist_util.free_port()), "--results_root", str(out),
           "--job_id", "t", *extra]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(out))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return out / "experiment_single_1_t"


@pytest.mark.slow
def test_cli_evaluation_leaves_the_run_alone(tmp_path):
    plain = _cli(tmp_path, "plain")
    evald = _cli(tmp_path, "eval", "--eval_every", "1", "--eval_batches", "2", "--topk", "3")
    assert not list(plain.glob("*_eval.txt"))
    assert (plain / "single_0_0_loss.txt").read_bytes() == (evald / "single_0_0_loss.txt").read_bytes()
    assert sorted(p.name for p in plain.iterdir()) == sorted(p.name for p in evald.iterdir() if "_eval" not in p.name)
    lines = (evald / "single_0_0_eval.txt").read_text().splitlines()
    assert len(lines) == 3
    for b, line in enumerate(lines, start=1):
        assert line.startswith(f"Worker 0:0 eval at batch {b}: loss ") and line.endswith(" samples 16")
        words = line.split()
        assert words[8] == "top1" and words[10] == "top3" and 0.0 <= float(words[9]) <= float(words[11]) <= 1.0
    # once after the last batch
    once = _cli(tmp_path, "once", "--eval_batches", "2")
    assert len((once / "single_0_0_eval.txt").read_text().splitlines()) == 1
    # label smoothing changes the training loss and nothing else about the run
    smooth = _cli(tmp_path, "smooth", "--label_smoothing", "0.1")
    assert (smooth / "single_0_0_loss.txt").read_bytes() != (plain / "single_0_0_loss.txt").read_bytes()
    assert not list(smooth.glob("*_eval.txt"))


@pytest.mark.parametrize("args", [["--label_smoothing", "1"], ["--label_smoothing", "-0.1"], ["--eval_batches", "-1"],
                                  ["--topk", "0"]])
def test_cli_parse_errors(args):
    from distributed_learning_amd.config import parse_args

    with pytest.raises(SystemExit):
        parse_args(args)


def test_cli_defaults():
    from distributed_learning_amd.config import parse_args

    c = parse_args([])
    assert (c.label_smoothing, c.eval_batches, c.eval_every, c.topk) == (0.0, 0, 0, 5)
