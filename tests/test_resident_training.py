"""``--resident 1`` and ``--staged_dir`` through the command line, on the CPU (the store lives in host memory there):
the run must be the ``--augment standard`` run, file for file, because batch k holds the same samples in the same
order and the CPU transform of ``store[index]`` is the transform of the loader's batch."""
import copy
import re

import pytest

from test_augment_cpu import _cli, _losses, _write_cifar

AUG = ("--augment", "standard")
MIX = ("--mixup_alpha", "0.2", "--cutmix_alpha", "1.0")
# 40 training samples at batch 8: 7 batches cross an epoch boundary; evaluation over the 8 test samples
SEVEN = ("--limit_batches", "7", "--epoch_count", "2", "--eval_batches", "1", "--eval_every", "4")


@pytest.mark.slow
@pytest.mark.parametrize("mix", [(), MIX], ids=["plain", "mixed"])
def test_resident_run_equals_the_loader_run(tmp_path, mix):
    data = _write_cifar(tmp_path / "data")
    a = _cli(tmp_path, "loader", data, *AUG, *SEVEN, *mix)
    b = _cli(tmp_path, "resident", data, *AUG, *SEVEN, *mix, "--resident", "1")
    assert len(_losses(a)) == 7
    for name in ("single_0_0_loss.txt", "single_0_0_eval.txt"):
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
    assert len((a / "single_0_0_eval.txt").read_text().splitlines()) == 2  # after batches 4 and 7
    assert sorted(p.name for p in a.iterdir()) == sorted(p.name for p in b.iterdir())
    rows_a, rows_b = ((d / "single_0_0_times.csv").read_text().splitlines() for d in (a, b))
    assert rows_a[0] == rows_b[0] and len(rows_a) == len(rows_b)  # the same columns, a row per batch
    col = rows_a[0].split(", ").index("data_len")
    assert [r.split(", ")[col] for r in rows_a[1:]] == [r.split(", ")[col] for r in rows_b[1:]] == ["8"] * 7
    assert "resident=1" in (b / "single_config.txt").read_text()
    assert "resident=" not in (a / "single_config.txt").read_text()


@pytest.mark.slow
def test_resident_resume_equals_the_uninterrupted_run(tmp_path):
    data = _write_cifar(tmp_path / "data")
    ck = tmp_path / "ck.pt"
    res = (*AUG, "--resident", "1", "--epoch_count", "2")
    whole = _cli(tmp_path, "whole", data, *res, "--limit_batches", "7")
    first = _cli(tmp_path, "first", data, *res, "--limit_batches", "3", "--checkpoint", str(ck))
    second = _cli(tmp_path, "second", data, *res, "--limit_batches", "4", "--resume", str(ck))
    assert len(_losses(whole)) == 7
    assert _losses(first) + _losses(second) == _losses(whole)


def test_flags_and_parser_errors(tmp_path, capsys):
    from distributed_learning_amd.config import parse_args

    c = parse_args([])
    assert (c.staged_dir, c.resident) == (None, 0)
    c = parse_args(["--model", "resnet50", "--augment", "standard", "--resident", "1", "--staged_dir", "/x"])
    assert (c.staged_dir, c.resident) == ("/x", 1)
    assert parse_args(["--model", "resnet18_cifar", "--augment", "standard", "--resident", "1"]).resident == 1
    for bad, said in ((["--model", "resnet18_cifar", "--resident", "1"], "--resident 1 needs --augment standard"),
                      (["--model", "resnet50", "--staged_dir", "/x"], "--staged_dir needs --augment standard"),
                      (["--model", "resnet18_cifar", "--augment", "standard", "--staged_dir", "/x"],
                       "--staged_dir needs an ImageNet model"),
                      (["--model", "resnet50", "--augment", "standard", "--resident", "2"], "invalid choice")):
        with pytest.raises(SystemExit):
            parse_args(bad)
        assert said in capsys.readouterr().err, bad
    r = _cli(tmp_path, "err", tmp_path, "--resident", "1", ok=False)
    assert r.returncode != 0 and "--resident 1 needs --augment standard" in r.stderr


def test_config_text_hides_the_unset_flags():
    from distributed_learning_amd.config import parse_args
    from distributed_learning_amd.train import _config_text

    base = ["--model", "resnet50", "--augment", "standard"]
    off = _config_text(parse_args(base))
    assert "staged_dir=" not in off and "resident=" not in off
    on = _config_text(parse_args(base + ["--resident", "1", "--staged_dir", "/x"]))
    assert "resident=1" in on and "staged_dir='/x'" in on
    # taking the two flags out gives the text of a run that never heard of them
    assert re.sub(r",? ?(resident=1|staged_dir='/x')", "", on) == off
    only = _config_text(parse_args(base + ["--staged_dir", "/x"]))
    assert "staged_dir='/x'" in only and "resident" not in only
    none = _config_text(parse_args([]))
    assert "staged_dir" not in none and "resident" not in none and "augment" not in none


def test_synthetic_input_ignores_the_flag(tmp_path, capsys):
    """Synthetic batches are generated on the device already: the flag warns and changes nothing."""
    from distributed_learning_amd import experiments
    from distributed_learning_amd.config import parse_args

    def run(sub, *extra):
        cfg = parse_args(["1", "0", "1", "1", "127.0.0.1", "lo", "resnet18_cifar", "/nonexistent", "0", "--random_input",
                          "1", "--limit_batches", "2", "--batch_size", "4", *extra])
        cfg.folder = str(tmp_path / sub)
        return experiments.main_single(copy.copy(cfg))["losses"]

    plain = run("plain")
    capsys.readouterr()
    assert run("res", *AUG, "--resident", "1") == plain
    assert "--resident 1 ignored" in "".join(capsys.readouterr())
