"""The staging tool (distributed_learning_amd/stage.py) and its reader (data.StagedImages): one decode through
``ImageFolder(raw=True)`` itself, then a memory-mapped array."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

pytest.importorskip("PIL.Image")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ("train_images.npy", "train_labels.npy", "train_meta.json")


def _tree(root, split="ImageFolder"):
    from PIL import Image

    rng = np.random.default_rng(5)
    sizes = {"beta": ((300, 260), (200, 333), (256, 256)), "alpha": ((257, 400), (512, 300))}  # (w, h), none staged as is
    for cls, whs in sizes.items():
        (root / split / cls).mkdir(parents=True)
        for w, h in whs:
            Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(root / split / cls / f"{w}x{h}.png")
    return root


def _stage(root, out, *extra):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "distributed_learning_amd.stage", str(root), "--out", str(out), *extra]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def staged(tmp_path_factory):
    base = tmp_path_factory.mktemp("stage")
    root = _tree(base / "data")
    for w in ("1", "2"):
        r = _stage(root, base / f"w{w}", "--split", "train", "--workers", w)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return base


def test_staged_items_equal_the_image_folder(staged):
    from distributed_learning_amd.data import ImageFolder, StagedImages

    folder = ImageFolder(str(staged / "data" / "ImageFolder"), raw=True)
    ds = StagedImages(str(staged / "w1"), "train")
    assert len(ds) == len(folder) == 5 and ds.classes == folder.classes == ["alpha", "beta"]
    assert ds.images.dtype == np.uint8 and ds.images.shape == (5, 256, 256, 3) and isinstance(ds.images, np.memmap)
    assert ds.labels.dtype == np.int64 and ds.labels.tolist() == [0, 0, 1, 1, 1]
    for i in range(5):
        (x, y), (xf, yf) = ds[i], folder[i]
        assert x.dtype == torch.uint8 and x.shape == (256, 256, 3) and x.is_contiguous()
        assert torch.equal(x, xf) and y == yf and isinstance(y, int)
    meta = json.loads((staged / "w1" / "train_meta.json").read_text())
    assert meta["count"] == 5 and meta["stage"] == 256 and meta["classes"] == ["alpha", "beta"]
    assert len(meta["names_sha256"]) == 64


def test_output_does_not_depend_on_the_worker_count(staged):
    for name in FILES:
        assert (staged / "w1" / name).read_bytes() == (staged / "w2" / name).read_bytes(), name


def test_resident_store_fills_from_the_staged_array(staged):
    from distributed_learning_amd.data import ResidentStore, StagedImages

    ds = StagedImages(str(staged / "w2"), "train")
    store = ResidentStore.from_dataset(ds, [4, 1, 1], "cpu")
    assert torch.equal(store.images[:3], torch.from_numpy(np.array(ds.images[[4, 1, 1]])))
    assert store.labels.tolist() == [1, 0, 0, -100]


def test_a_pickled_dataset_maps_the_file_again(staged):
    """What a spawned loader worker receives holds no copy of the array."""
    import pickle

    from distributed_learning_amd.data import StagedImages

    ds = StagedImages(str(staged / "w1"), "train")
    x, y = ds[2]
    blob = pickle.dumps(ds)
    assert len(blob) < 256 * 256 * 3
    again = pickle.loads(blob)
    assert torch.equal(again[2][0], x) and again[2][1] == y and len(again) == 5


def test_mismatching_files_raise(staged, tmp_path):
    from distributed_learning_amd.data import StagedImages

    def copy(sub):
        d = tmp_path / sub
        shutil.copytree(staged / "w1", d)
        return d

    d = copy("short_labels")
    np.save(d / "train_labels.npy", np.load(d / "train_labels.npy")[:-1])
    with pytest.raises(ValueError, match="train_labels.npy"):
        StagedImages(str(d), "train")
    d = copy("short_images")
    np.save(d / "train_images.npy", np.load(d / "train_images.npy")[:-1])
    with pytest.raises(ValueError, match="train_images.npy"):
        StagedImages(str(d), "train")
    d = copy("labels_out_of_range")
    np.save(d / "train_labels.npy", np.load(d / "train_labels.npy") + 1)
    with pytest.raises(ValueError, match="outside"):
        StagedImages(str(d), "train")
    with pytest.raises(FileNotFoundError):
        StagedImages(str(staged / "w1"), "val")


def test_load_dataset_needs_no_image_tree(staged, tmp_path):
    from distributed_learning_amd.data import ImageFolder, StagedImages, load_dataset

    root = _tree(tmp_path / "data")
    _tree(root, "ImageFolderVal")
    for split in ("train", "val"):
        r = _stage(root, tmp_path / "st", "--split", split, "--workers", "1")
        assert r.returncode == 0, r.stderr[-2000:]
    want = [ImageFolder(str(root / "ImageFolder"), raw=True)[i] for i in range(5)]
    shutil.rmtree(root)
    for train in (True, False):
        ds = load_dataset("imagenet", str(root), train, raw=True, staged_dir=str(tmp_path / "st"))
        assert isinstance(ds, StagedImages) and len(ds) == 5
        for i in range(5):
            assert torch.equal(ds[i][0], want[i][0]) and ds[i][1] == want[i][1]
    with pytest.raises(ValueError):
        load_dataset("imagenet", str(root), raw=False, staged_dir=str(tmp_path / "st"))
    with pytest.raises(ValueError):
        load_dataset("cifar10", str(root), raw=True, staged_dir=str(tmp_path / "st"))


def test_tool_refuses_a_missing_tree(tmp_path):
    r = _stage(tmp_path, tmp_path / "out", "--split", "val")
    assert r.returncode != 0 and "image tree not found" in r.stderr
    assert _stage(tmp_path, tmp_path / "out", "--split", "test").returncode != 0
