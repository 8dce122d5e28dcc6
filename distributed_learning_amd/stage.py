"""Decode an ImageNet tree once into the staged files :class:`~distributed_learning_amd.data.StagedImages` reads.

``python -m distributed_learning_amd.stage ROOT --split train|val --out DIR [--workers W]`` runs
``ImageFolder(raw=True)`` -- the loader's own decode, resize and centre 256x256 crop, no second implementation --
over ``ROOT/ImageFolder`` (train) or ``ROOT/ImageFolderVal`` (val) and writes

* ``DIR/{split}_images.npy``  uint8 ``[N, 256, 256, 3]`` (through ``numpy.lib.format.open_memmap``),
* ``DIR/{split}_labels.npy``  int64 ``[N]``,
* ``DIR/{split}_meta.json``   count, stage size, class names and a SHA-256 over the sorted relative file names.

Every item is a function of its file alone, so the output is the same for every ``W``. A training run then
passes ``--staged_dir DIR`` and never opens a JPEG again.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import multiprocessing as mp
import os
from pathlib import Path
from typing import List, Optional, Tuple

import numpy as np

from .data import ImageFolder

SPLITS = {"train": "ImageFolder", "val": "ImageFolderVal"}
_DATASET: Optional[ImageFolder] = None


def _init(root: str) -> None:
    global _DATASET
    _DATASET = ImageFolder(root, raw=True)


def _decode(i: int) -> Tuple[int, np.ndarray]:
    return i, _DATASET[i][0].numpy()


def names_digest(dataset: ImageFolder) -> str:
    """SHA-256 over the sorted file names relative to the tree's root, one per line."""
    names = sorted(os.path.relpath(path, dataset.root).replace(os.sep, "/") for path, _ in dataset.samples)
    return hashlib.sha256("\n".join(names).encode()).hexdigest()


def stage(root: str, split: str, out: str, workers: Optional[int] = None) -> dict:
    """Write the three files of ``split`` under ``out``; returns the meta dictionary."""
    if split not in SPLITS:
        raise ValueError(f"unknown split {split!r}; choose from {sorted(SPLITS)}")
    tree = os.path.join(root, SPLITS[split])
    if not os.path.isdir(tree):
        raise FileNotFoundError(f"image tree not found: {tree}")
    workers = min(16, os.cpu_count() or 1) if workers is None else int(workers)
    if workers < 1:
        raise ValueError(f"--workers must be >= 1, got {workers}")
    _init(tree)
    ds = _DATASET
    n, s = len(ds), ImageFolder.STAGE
    if n == 0:
        raise ValueError(f"no images under {tree}")
    d = Path(out)
    d.mkdir(parents=True, exist_ok=True)
    images = np.lib.format.open_memmap(d / f"{split}_images.npy", mode="w+", dtype=np.uint8, shape=(n, s, s, 3))
    if workers == 1:
        for i in range(n):
            images[i] = _decode(i)[1]
    else:
        with mp.get_context("spawn").Pool(workers, initializer=_init, initargs=(tree,)) as pool:
            for i, x in pool.imap_unordered(_decode, range(n), chunksize=16):
                images[i] = x
    images.flush()
    del images
    np.save(d / f"{split}_labels.npy", np.asarray([label for _, label in ds.samples], dtype=np.int64))
    meta = {"count": n, "stage": s, "classes": list(ds.classes), "names_sha256": names_digest(ds), "split": split}
    with open(d / f"{split}_meta.json", "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    return meta


def main(argv: Optional[List[str]] = None) -> None:
    p = argparse.ArgumentParser(prog="python -m distributed_learning_amd.stage", description=__doc__.split("\n")[0])
    p.add_argument("root", help="dataset root holding ImageFolder/ and ImageFolderVal/")
    p.add_argument("--split", required=True, choices=sorted(SPLITS))
    p.add_argument("--out", required=True, help="directory the staged files are written to")
    p.add_argument("--workers", type=int, default=None, help="decoding processes (default min(16, cpu count))")
    a = p.parse_args(argv)
    meta = stage(a.root, a.split, a.out, a.workers)
    print(f"staged {meta['count']} images of {len(meta['classes'])} classes ({a.split}) into {a.out}")


if __name__ == "__main__":
    main()
