"""CPU side of the device augmentation: the torch implementation of the transform against the float64 oracle, the
raw (uint8) loaders against today's normalised ones, and the command line (``--augment``) end to end."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import augment_oracle as ao
import dist_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.bfloat16]


def _augment(src, geom, flip, out_hw, dtype, pad=0, mean=ao.MEAN, std=ao.STD):
    from distributed_learning_amd.ops.augment import augment

    return augment(src, geom, torch.tensor(flip, dtype=torch.uint8), mean, std, out_hw, dtype, pad)


@pytest.fixture(scope="module")
def src():
    return ao.noise_source(6)


# --- the torch implementation against the oracle ---------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("offsets,pad", [(ao.INT_INSIDE, 0), (ao.INT_PAD4, 4)], ids=["inside", "pad4"])
def test_integer_geometry_bitwise(src, offsets, pad, dtype):
    out = _augment(src[:3], ao.int_geom(offsets), ao.FLIP3, ao.INT_HW, dtype, pad)
    assert out.shape == (3, 3) + ao.INT_HW and out.dtype == dtype
    ao.assert_bitwise(out, ao.expected_int(src[:3], offsets, ao.FLIP3, ao.INT_HW, pad))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_interpolated(src, dtype):
    geom = ao.interp_geom()
    out = _augment(src[:5], geom, ao.INTERP_FLIP, ao.INTERP_HW, dtype)
    ao.assert_close(out, ao.oracle(src[:5], geom, ao.INTERP_FLIP, ao.INTERP_HW, 0))


def test_oracle_agrees_with_the_integer_formula(src):
    """The two references are written separately (sampling vs slicing a padded copy); they must agree exactly."""
    for offsets, pad in ((ao.INT_INSIDE, 0), (ao.INT_PAD4, 4)):
        sampled = ao.oracle(src[:3], ao.int_geom(offsets), ao.FLIP3, ao.INT_HW, pad).astype(np.float32)
        assert np.array_equal(sampled, ao.expected_int(src[:3], offsets, ao.FLIP3, ao.INT_HW, pad))


def test_guards(src):
    from distributed_learning_amd.ops.augment import augment

    geom, flip = ao.int_geom(ao.INT_INSIDE), torch.tensor(ao.FLIP3, dtype=torch.uint8)
    wide = ao.noise_source(3, ao.HS, 2 * ao.WS)
    for kw in (dict(src=src[:3].float()), dict(src=torch.zeros(3, ao.HS, ao.WS, 4, dtype=torch.uint8)),
               dict(src=wide[:, :, ::2]), dict(geom=geom[:2]), dict(flip=flip[:2]), dict(dtype=torch.float16)):
        a = dict(src=src[:3], geom=geom, flip=flip, dtype=torch.float32)
        a.update(kw)
        with pytest.raises((ValueError, TypeError)):
            augment(a["src"], a["geom"], a["flip"], ao.MEAN, ao.STD, ao.INT_HW, a["dtype"])


def test_element_count_limit():
    """2^31 or more elements on either side are refused before anything is allocated or launched (the kernel
    indexes elements with 32 bits); checked on storage-less tensors."""
    from distributed_learning_amd.ops.augment import augment
    from distributed_learning_amd.ops.limits import NativeLimitError

    n = 10923  # 10923 * 256 * 256 * 3 = 2^31 + 1536
    geom, flip = torch.empty(n, 4, device="meta"), torch.empty(n, device="meta", dtype=torch.uint8)
    big = torch.empty(n, 256, 256, 3, dtype=torch.uint8, device="meta")
    with pytest.raises(NativeLimitError, match="src"):
        augment(big, geom, flip, ao.MEAN, ao.STD, (224, 224), torch.bfloat16)
    small = torch.empty(n, 8, 8, 3, dtype=torch.uint8, device="meta")
    with pytest.raises(NativeLimitError, match="out"):
        augment(small, geom, flip, ao.MEAN, ao.STD, (256, 256), torch.bfloat16)


# --- raw loaders -----------------------------------------------------------------------------------
def _center(x_u8, src_hw, out_hw, mean, std):
    from distributed_learning_amd.ops.augment import AugmentParams, augment

    geom, flip = AugmentParams("center", src_hw, out_hw).params(0, x_u8.shape[0])
    return augment(x_u8, geom, flip, mean, std, out_hw, torch.float32)


def test_imagefolder_raw_matches_the_evaluation_transform(tmp_path):
    from PIL import Image

    from distributed_learning_amd.data import ImageFolder
    from distributed_learning_amd.ops.augment import IMAGENET_MEAN, IMAGENET_STD

    rng = np.random.default_rng(3)
    for cls, (w, h) in (("a", (300, 260)), ("b", (200, 333)), ("b", (256, 256))):
        (tmp_path / cls).mkdir(exist_ok=True)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(tmp_path / cls / f"{w}x{h}.png")
    today, raw = ImageFolder(str(tmp_path)), ImageFolder(str(tmp_path), raw=True)
    assert len(today) == len(raw) == 3
    for i in range(3):
        (x, label), (u8, label_raw) = today[i], raw[i]
        assert label == label_raw
        assert u8.dtype == torch.uint8 and u8.shape == (256, 256, 3) and u8.is_contiguous()
        out = _center(u8[None], (256, 256), (224, 224), IMAGENET_MEAN, IMAGENET_STD)[0]
        assert out.shape == x.shape == (3, 224, 224)
        # both are a few fp32 roundings (each <= 1.6e-7 at values below 2.7) of the same real number
        assert float((out - x).abs().max()) <= 1e-6


def _write_cifar(root, per_file=8):
    d = root / "cifar-10-batches-bin"
    d.mkdir(parents=True)
    rng = np.random.default_rng(1)
    for name in [f"data_batch_{i}.bin" for i in range(1, 6)] + ["test_batch.bin"]:
        rec = rng.integers(0, 256, (per_file, 3073), dtype=np.uint8)
        rec[:, 0] = rng.integers(0, 10, per_file)
        (d / name).write_bytes(rec.tobytes())
    return root


def test_cifar_raw_matches_the_normalised_tensor(tmp_path):
    from distributed_learning_amd.data import load_cifar10, load_dataset
    from distributed_learning_amd.ops.augment import CIFAR10_MEAN, CIFAR10_STD

    root = str(_write_cifar(tmp_path))
    for train, n in ((True, 40), (False, 8)):
        today, raw = load_cifar10(root, train), load_cifar10(root, train, raw=True)
        assert raw.x.dtype == torch.uint8 and raw.x.shape == (n, 32, 32, 3) and raw.x.is_contiguous()
        assert today.x.shape == (n, 3, 32, 32) and torch.equal(today.y, raw.y)
        out = _center(raw.x, (32, 32), (32, 32), CIFAR10_MEAN, CIFAR10_STD)
        assert float((out - today.x).abs().max()) <= 1e-6
    assert load_dataset("cifar10", root, raw=True).x.dtype == torch.uint8
    assert load_dataset("cifar10", root).x.dtype == torch.float32
    with pytest.raises(ValueError, match="MNIST"):
        load_dataset("mnist", root, raw=True)


# --- command line ----------------------------------------------------------------------------------
def _cli(tmp_path, sub, data, *extra, model="resnet18_cifar", ok=True):
    out = tmp_path / sub
    out.mkdir()
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "distributed_learning_amd.main", "1", "0", "1", "1", "127.0.0.1", "lo", model,
           str(data), "0", "--experiment", "main_single", "--limit_batches", "2", "--batch_size", "8",
           "--master_port", str(dist_util.free_port()), "--results_root", str(out), "--job_id", "t", *extra]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(out))
    if ok:
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return out / "main_single_1_t"
    return r


def _losses(folder):
    lines = (folder / "single_0_0_loss.txt").read_text().splitlines()
    return [float(line.rsplit(": ", 1)[1]) for line in lines]


@pytest.mark.slow
def test_cli_augment_standard(tmp_path):
    data = _write_cifar(tmp_path / "data")
    a = _cli(tmp_path, "a", data, "--augment", "standard", "--eval_batches", "1")
    la = _losses(a)
    assert len(la) == 2 and all(np.isfinite(la))
    ev = (a / "single_0_0_eval.txt").read_text().splitlines()
    assert len(ev) == 1 and ev[0].endswith(" samples 8") and np.isfinite(float(ev[0].split()[7]))
    assert "augment='standard'" in (a / "single_config.txt").read_text()
    b = _cli(tmp_path, "b", data, "--augment", "standard", "--eval_batches", "1")
    assert _losses(b) == la and (b / "single_0_0_eval.txt").read_text() == "\n".join(ev) + "\n"
    # off: the files of a run that never heard of the flag, with the same contents
    none = _cli(tmp_path, "none", data, "--augment", "none", "--eval_batches", "1")
    plain = _cli(tmp_path, "plain", data, "--eval_batches", "1")
    assert sorted(p.name for p in none.iterdir()) == sorted(p.name for p in plain.iterdir()) \
        == sorted(p.name for p in a.iterdir())
    for name in ("single_0_0_loss.txt", "single_0_0_eval.txt"):
        assert (none / name).read_bytes() == (plain / name).read_bytes()
    cfg = (none / "single_config.txt").read_text()
    assert "augment=" not in cfg and "aug_scale_min" not in cfg  # the file a run without the flags always wrote
    same = lambda text, sub: re.sub(r"master_port=\d+", "", text).replace(f"/{sub}", "/run")  # noqa: E731
    assert same(cfg, "none") == same((plain / "single_config.txt").read_text(), "plain")
    assert _losses(none) != la  # and the augmentation did change what the model saw
    # a timer row per batch with the same columns either way
    assert (a / "single_0_0_times.csv").read_text().splitlines()[0] == \
        (plain / "single_0_0_times.csv").read_text().splitlines()[0]


@pytest.mark.slow
def test_cli_augment_resume(tmp_path):
    data = _write_cifar(tmp_path / "data")
    ck = tmp_path / "ck.pt"
    whole = _cli(tmp_path, "whole", data, "--augment", "standard", "--limit_batches", "4")
    first = _cli(tmp_path, "first", data, "--augment", "standard", "--checkpoint", str(ck))
    second = _cli(tmp_path, "second", data, "--augment", "standard", "--resume", str(ck))
    assert len(_losses(whole)) == 4
    assert _losses(first) + _losses(second) == _losses(whole)


def test_cli_augment_needs_a_three_channel_dataset(tmp_path):
    from distributed_learning_amd.config import parse_args

    with pytest.raises(SystemExit):
        parse_args(["--model", "mnist", "--augment", "standard"])
    r = _cli(tmp_path, "mnist", tmp_path, "--augment", "standard", model="mnist", ok=False)
    assert r.returncode != 0 and "MNIST has no raw" in r.stderr


def test_cli_flags():
    from distributed_learning_amd.config import parse_args

    c = parse_args([])
    assert (c.augment, c.aug_scale_min) == ("none", 0.08)
    c = parse_args(["--model", "resnet50", "--augment", "standard", "--aug_scale_min", "0.25"])
    assert (c.augment, c.aug_scale_min) == ("standard", 0.25)
    for bad in (["--aug_scale_min", "0"], ["--aug_scale_min", "1.5"], ["--augment", "mixup"]):
        with pytest.raises(SystemExit):
            parse_args(bad)


def test_synthetic_input_ignores_the_flag(tmp_path, capsys):
    """Synthetic batches are generated in the model's form: the flag warns and changes nothing."""
    import copy

    from distributed_learning_amd import experiments
    from distributed_learning_amd.config import parse_args

    def run(sub, *extra):
        cfg = parse_args(["1", "0", "1", "1", "127.0.0.1", "lo", "resnet18_cifar", "/nonexistent", "0", "--random_input",
                          "1", "--limit_batches", "2", "--batch_size", "4", *extra])
        cfg.folder = str(tmp_path / sub)
        return experiments.main_single(copy.copy(cfg))["losses"]

    plain = run("plain")
    capsys.readouterr()
    assert run("aug", "--augment", "standard") == plain
    assert "ignored" in "".join(capsys.readouterr())
