"""Mixup / CutMix in the training loop and on the command line (``--mixup_alpha``, ``--cutmix_alpha``,
``--mix_switch_prob``): the CPU runs are subprocess tests on a tiny CIFAR fixture written into ``tmp_path`` (the
helpers of tests/test_augment_cpu.py), the GPU run is in-process on the bf16 native path."""
import copy
import re

import numpy as np
import pytest

from test_augment_cpu import _cli, _losses, _write_cifar

MIX = ("--mixup_alpha", "0.2", "--cutmix_alpha", "1.0")


def _same(text, sub):
    return re.sub(r"master_port=\d+", "", text).replace(f"/{sub}", "/run")


@pytest.mark.slow
def test_cli_mix(tmp_path):
    data = _write_cifar(tmp_path / "data")
    std = ("--augment", "standard", "--eval_batches", "1")
    a = _cli(tmp_path, "a", data, *std, *MIX)
    la = _losses(a)
    assert len(la) == 2 and all(np.isfinite(la))
    cfg = (a / "single_config.txt").read_text()
    assert "mixup_alpha=0.2" in cfg and "cutmix_alpha=1.0" in cfg and "mix_switch_prob=0.5" in cfg
    b = _cli(tmp_path, "b", data, *std, *MIX)
    assert _losses(b) == la
    plain = _cli(tmp_path, "plain", data, *std)
    assert _losses(plain) != la  # the mixing did change what the model saw and was scored against
    # the first batch starts from the same weights: mixing alone moved its loss
    assert _losses(plain)[0] != la[0]
    # the evaluation is the plain one either way: the same file, one line of the same form over the same samples
    # (its numbers follow the weights, which the mixed batches trained)
    assert sorted(p.name for p in a.iterdir()) == sorted(p.name for p in plain.iterdir())
    for run in (a, b, plain):
        ev = (run / "single_0_0_eval.txt").read_text().splitlines()
        assert len(ev) == 1 and ev[0].endswith(" samples 8") and np.isfinite(float(ev[0].split()[7]))
    assert (a / "single_0_0_eval.txt").read_bytes() == (b / "single_0_0_eval.txt").read_bytes()
    # flags absent, or both alphas at 0: the files of --augment standard alone, byte for byte
    zero = _cli(tmp_path, "zero", data, *std, "--mixup_alpha", "0", "--cutmix_alpha", "0", "--mix_switch_prob", "0.3")
    for name in ("single_0_0_loss.txt", "single_0_0_eval.txt"):
        assert (zero / name).read_bytes() == (plain / name).read_bytes()
    assert (zero / "single_0_0_times.csv").read_text().splitlines()[0] == \
        (plain / "single_0_0_times.csv").read_text().splitlines()[0] == \
        (a / "single_0_0_times.csv").read_text().splitlines()[0]
    zcfg, pcfg = (zero / "single_config.txt").read_text(), (plain / "single_config.txt").read_text()
    assert "mixup_alpha" not in pcfg and "cutmix_alpha" not in pcfg and "mix_switch_prob" not in pcfg
    assert _same(zcfg, "zero") == _same(pcfg, "plain")
    assert "augment='standard'" in pcfg


@pytest.mark.slow
def test_cli_mix_resume(tmp_path):
    data = _write_cifar(tmp_path / "data")
    ck = tmp_path / "ck.pt"
    std = ("--augment", "standard", *MIX)
    whole = _cli(tmp_path, "whole", data, *std, "--limit_batches", "4")
    first = _cli(tmp_path, "first", data, *std, "--checkpoint", str(ck))
    second = _cli(tmp_path, "second", data, *std, "--resume", str(ck))
    assert len(_losses(whole)) == 4
    assert _losses(first) + _losses(second) == _losses(whole)


@pytest.mark.parametrize("args", [["--mixup_alpha", "0.2"], ["--cutmix_alpha", "1.0"],
                                  ["--augment", "standard", "--mixup_alpha", "-0.1"],
                                  ["--augment", "standard", "--cutmix_alpha", "-1"],
                                  ["--augment", "standard", "--mixup_alpha", "0.2", "--mix_switch_prob", "1.5"],
                                  ["--augment", "standard", "--mix_switch_prob", "-0.1"]])
def test_cli_parse_errors(args):
    from distributed_learning_amd.config import parse_args

    with pytest.raises(SystemExit):
        parse_args(["--model", "resnet18_cifar", *args])


def test_cli_flags():
    from distributed_learning_amd.config import parse_args

    c = parse_args([])
    assert (c.mixup_alpha, c.cutmix_alpha, c.mix_switch_prob) == (0.0, 0.0, 0.5)
    c = parse_args(["--model", "resnet50", "--augment", "standard", "--mixup_alpha", "0.2", "--cutmix_alpha", "1",
                    "--mix_switch_prob", "0.25"])
    assert (c.mixup_alpha, c.cutmix_alpha, c.mix_switch_prob) == (0.2, 1.0, 0.25)


def test_config_text_shows_the_flags_only_when_set():
    from distributed_learning_amd.config import parse_args
    from distributed_learning_amd.train import _config_text

    off = _config_text(parse_args(["--model", "resnet18_cifar", "--augment", "standard"]))
    assert "mixup_alpha" not in off and "cutmix_alpha" not in off and "mix_switch_prob" not in off
    assert "augment='standard'" in off
    on = _config_text(parse_args(["--model", "resnet18_cifar", "--augment", "standard", "--cutmix_alpha", "1"]))
    assert "mixup_alpha=0.0" in on and "cutmix_alpha=1.0" in on and "mix_switch_prob=0.5" in on


def test_synthetic_input_ignores_the_flags(tmp_path, capsys):
    """Synthetic batches are generated in the model's form: the flags warn and change nothing."""
    from distributed_learning_amd import experiments
    from distributed_learning_amd.config import parse_args

    def run(sub, *extra):
        cfg = parse_args(["1", "0", "1", "1", "127.0.0.1", "lo", "resnet18_cifar", "/nonexistent", "0", "--random_input",
                          "1", "--limit_batches", "2", "--batch_size", "4", *extra])
        cfg.folder = str(tmp_path / sub)
        return experiments.main_single(copy.copy(cfg))["losses"]

    plain = run("plain")
    capsys.readouterr()
    assert run("mix", "--augment", "standard", *MIX) == plain
    said = "".join(capsys.readouterr())
    assert "--mixup_alpha / --cutmix_alpha ignored" in said


@pytest.mark.gpu
def test_gpu_training_with_mixing(cuda, tmp_path):
    """experiments.main_single on the fixture, resnet18_cifar, batch 8, 2 batches, the bf16 native path: finite
    losses, the same on a second run, and not those of the unmixed run."""
    from distributed_learning_amd import experiments
    from distributed_learning_amd.config import parse_args

    data = _write_cifar(tmp_path / "data")

    def run(sub, *extra):
        cfg = parse_args(["1", "0", "1", "1", "127.0.0.1", "lo", "resnet18_cifar", str(data), "1", "--limit_batches",
                          "2", "--batch_size", "8", "--augment", "standard", *extra])
        assert cfg.precision == "bf16" and cfg.kernels == "native"
        cfg.folder = str(tmp_path / sub)
        return experiments.main_single(copy.copy(cfg))["losses"]

    mixed = run("a", *MIX)
    assert len(mixed) == 2 and all(np.isfinite(mixed))
    assert run("b", *MIX) == mixed
    plain = run("plain")
    assert len(plain) == 2 and plain != mixed and plain[0] != mixed[0]
