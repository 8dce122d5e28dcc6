"""Datasets: partitioning, on-device synthetic batches, and offline loaders.

Reference (/root/reference/src/data.py):
* ``DataPartitioner`` — ``randperm(len)`` under the global seed, ``total_dev`` disjoint partitions
  of ``batches_per_dev * batch_size`` samples, partition index ``node_id*node_dev + worker_id``
  (data.py:26-41,58-68). Kept with identical semantics.
* MNIST / ImageFolder loaders via torchvision with downloads (data.py:71-127). torchvision is not
  installed and there is no network, so this module reads the on-disk formats directly: MNIST idx
  files, CIFAR-10 binary batches, and ImageFolder trees (PIL), each optional.
* ``random_data_generator`` — CPU ``rand_like``/``randint_like`` per step from a real template
  batch (data.py:129-132; ~130 ms/step on the reference's hardware). Replaced by
  :class:`SyntheticBatches`, which generates each batch directly in HBM with the native Philox
  kernel (csrc/kernels/synthetic.hip) and needs no dataset on disk.
"""
from __future__ import annotations

import os
import struct
from pathlib import Path
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .ops import _ext

PER_WORKER_BATCH_SIZE = 128


class Partition(torch.utils.data.Dataset):
    """Index view over a dataset (reference data.py:10-23)."""

    def __init__(self, data, index: Sequence[int]):
        self.data = data
        self.index = index

    def __len__(self):
        return len(self.index)

    def __getitem__(self, i):
        return self.data[int(self.index[i])]


class DataPartitioner:
    """``total_dev`` disjoint, equally sized partitions (reference data.py:26-41)."""

    def __init__(self, data, total_dev: int, batch_size: int, seed: int = 1234):
        self.data = data
        n = len(data)
        batches_per_dev = n // total_dev // batch_size
        part_len = batches_per_dev * batch_size
        g = torch.Generator().manual_seed(seed)
        idx = torch.randperm(n, generator=g)
        self.partitions: List[torch.Tensor] = [idx[i * part_len:(i + 1) * part_len] for i in range(total_dev)]

    def use(self, partition: int) -> Partition:
        return Partition(self.data, self.partitions[partition])


class EpochSampler(torch.utils.data.Sampler):
    """Shuffled order drawn from (seed, epoch) alone, with a start offset.

    The reference shuffles with ``DataLoader(shuffle=True)`` (data.py:67), whose order depends on the
    global RNG state at the moment each epoch starts, so a run cannot be resumed mid-epoch on the same
    sequence. Here epoch e's permutation is a pure function of (seed, e): a resumed run at global
    batch k sets epoch k // batches_per_epoch and starts k % batches_per_epoch batches into it,
    without loading or decoding the skipped samples."""

    def __init__(self, n: int, seed: int = 1234):
        self.n, self.seed = n, seed
        self.epoch, self.start = 0, 0

    def set_epoch(self, epoch: int, start: int = 0) -> None:
        self.epoch, self.start = int(epoch), int(start)

    def order(self, epoch: int) -> List[int]:
        g = torch.Generator().manual_seed(self.seed * 1_000_003 + epoch)
        return torch.randperm(self.n, generator=g).tolist()

    def __iter__(self):
        return iter(self.order(self.epoch)[self.start:])

    def __len__(self):
        return self.n - self.start


def resume_position(start_step: int, batches_per_epoch: int) -> Tuple[int, int]:
    """(epoch, batches to skip inside it) of global batch ``start_step``."""
    if batches_per_epoch <= 0:
        return 0, 0
    return start_step // batches_per_epoch, start_step % batches_per_epoch


def get_partition_loader(dataset, node_id: int, worker_id: int, node_dev: int, total_dev: int,
                         batch_size: int = PER_WORKER_BATCH_SIZE, num_workers: int = 2, seed: int = 1234):
    part = DataPartitioner(dataset, total_dev, batch_size, seed).use(node_id * node_dev + worker_id)
    sampler = EpochSampler(len(part), seed + node_id * node_dev + worker_id)
    # own generator: the loader's per-iterator worker seed must not be drawn from the global RNG, or every
    # epoch start (and a resume's first iterator) would shift the model's dropout stream
    loader = torch.utils.data.DataLoader(part, batch_size=batch_size, sampler=sampler, num_workers=num_workers,
                                         drop_last=True, generator=torch.Generator().manual_seed(seed))
    loader.epoch_sampler = sampler
    return loader


# ------------------------------------------------------------------------------------------------
# Offline dataset readers (no torchvision, no downloads)
# ------------------------------------------------------------------------------------------------
class TensorDataset(torch.utils.data.Dataset):
    def __init__(self, x: torch.Tensor, y: torch.Tensor):
        self.x, self.y = x, y

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        return self.x[i], self.y[i]


def _read_idx(path: Path) -> np.ndarray:
    with open(path, "rb") as f:
        magic = struct.unpack(">I", f.read(4))[0]
        ndim = magic & 0xFF
        dims = struct.unpack(">" + "I" * ndim, f.read(4 * ndim))
        return np.frombuffer(f.read(), dtype=np.uint8).reshape(dims)


def load_mnist(root: str, train: bool = True) -> TensorDataset:
    """MNIST from idx files under ``root/mnist/MNIST/raw`` (torchvision layout) or ``root/mnist``."""
    stem = "train" if train else "t10k"
    for d in (Path(root) / "mnist" / "MNIST" / "raw", Path(root) / "mnist", Path(root)):
        img, lab = d / f"{stem}-images-idx3-ubyte", d / f"{stem}-labels-idx1-ubyte"
        if img.exists() and lab.exists():
            x = torch.from_numpy(_read_idx(img).astype(np.float32) / 255.0).unsqueeze(1)
            x = (x - 0.1307) / 0.3081  # reference normalisation (data.py:78-79)
            y = torch.from_numpy(_read_idx(lab).astype(np.int64))
            return TensorDataset(x, y)
    raise FileNotFoundError(f"MNIST idx files not found under {root}")


def load_cifar10(root: str, train: bool = True, raw: bool = False) -> TensorDataset:
    """CIFAR-10 binary batches (``cifar-10-batches-bin``); never unpickles anything. ``raw``: the images as
    stored, uint8 ``[N, 32, 32, 3]`` (HWC), for the device-side transform (ops/augment.py) instead of the
    normalised fp32 ``[N, 3, 32, 32]`` tensor."""
    d = Path(root) / "cifar-10-batches-bin"
    files = [d / f"data_batch_{i}.bin" for i in range(1, 6)] if train else [d / "test_batch.bin"]
    if not all(f.exists() for f in files):
        raise FileNotFoundError(f"CIFAR-10 binary batches not found under {d}")
    records = np.concatenate([np.fromfile(f, dtype=np.uint8).reshape(-1, 3073) for f in files])
    y = torch.from_numpy(records[:, 0].astype(np.int64))
    if raw:
        return TensorDataset(torch.from_numpy(np.ascontiguousarray(
            records[:, 1:].reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1))), y)
    x = torch.from_numpy(records[:, 1:].reshape(-1, 3, 32, 32).astype(np.float32) / 255.0)
    mean = torch.tensor([0.4914, 0.4822, 0.4465]).view(1, 3, 1, 1)
    std = torch.tensor([0.2470, 0.2435, 0.2616]).view(1, 3, 1, 1)
    return TensorDataset((x - mean) / std, y)


class ImageFolder(torch.utils.data.Dataset):
    """``root/<class>/<image>`` tree; Resize(256) -> CenterCrop(224) -> normalise (data.py:116-125).

    ``raw=True`` stops after the resize and hands over a uint8 ``[256, 256, 3]`` (HWC) staging image: the same
    bilinear resize of the shorter side to 256, then the centre 256x256 crop. Crop, flip, normalisation and
    layout then happen on the device (ops/augment.py). The centre 224 box of the staging image is pixel for
    pixel the default's crop, since ``(w - 256) // 2 + 16 == (w - 224) // 2``. The trade-off: a random-resized
    crop is drawn from this 256x256 staging image, not from the full-resolution original as torchvision's is,
    so it never sees the parts of a non-square image outside the centre square nor more than 256 pixels of
    detail per side; in exchange every sample has one fixed size and the batch is a single uint8 copy."""

    EXT = (".jpg", ".jpeg", ".png", ".bmp", ".ppm", ".webp")
    STAGE = 256

    def __init__(self, root: str, raw: bool = False):
        self.root = Path(root)
        self.raw = bool(raw)
        self.classes = sorted(p.name for p in self.root.iterdir() if p.is_dir())
        self.samples = [(str(f), ci) for ci, c in enumerate(self.classes) for f in sorted((self.root / c).rglob("*"))
                        if f.suffix.lower() in self.EXT]
        self.mean = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1)
        self.std = torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        from PIL import Image

        path, label = self.samples[i]
        img = Image.open(path).convert("RGB")
        w, h = img.size
        s = 256 / min(w, h)
        img = img.resize((max(1, round(w * s)), max(1, round(h * s))), Image.BILINEAR)
        w, h = img.size
        if self.raw:
            left, top = (w - self.STAGE) // 2, (h - self.STAGE) // 2
            img = img.crop((left, top, left + self.STAGE, top + self.STAGE))
            return torch.from_numpy(np.array(img, dtype=np.uint8)), label
        left, top = (w - 224) // 2, (h - 224) // 2
        img = img.crop((left, top, left + 224, top + 224))
        x = torch.from_numpy(np.asarray(img, dtype=np.float32) / 255.0).permute(2, 0, 1)
        return (x - self.mean) / self.std, label


class StagedImages(torch.utils.data.Dataset):
    """The files ``python -m distributed_learning_amd.stage`` writes, as a dataset: ``ImageFolder(raw=True)``'s
    items ``(uint8 [256, 256, 3], label)`` and ``.classes`` without the JPEG tree or a decode. ``.images`` is the
    memory-mapped uint8 ``[N, 256, 256, 3]`` array and ``.labels`` int64 ``[N]`` (:class:`ResidentStore`'s bulk
    fill slices them). The arrays are checked against ``{split}_meta.json``; a mismatch raises."""

    def __init__(self, directory: str, split: str = "train"):
        import json

        d = Path(directory)
        with open(d / f"{split}_meta.json") as f:
            self.meta = json.load(f)
        self._path, self._images = str(d / f"{split}_images.npy"), None
        self.labels = np.load(d / f"{split}_labels.npy")
        self.classes = list(self.meta["classes"])
        n, stage = int(self.meta["count"]), int(self.meta["stage"])
        if self.images.dtype != np.uint8 or tuple(self.images.shape) != (n, stage, stage, 3):
            raise ValueError(f"{d}/{split}_images.npy is {self.images.dtype} {tuple(self.images.shape)}, but "
                             f"{split}_meta.json describes uint8 {(n, stage, stage, 3)}")
        if self.labels.dtype != np.int64 or tuple(self.labels.shape) != (n,):
            raise ValueError(f"{d}/{split}_labels.npy is {self.labels.dtype} {tuple(self.labels.shape)}, but "
                             f"{split}_meta.json describes int64 {(n,)}")
        if n and not (0 <= int(self.labels.min()) and int(self.labels.max()) < len(self.classes)):
            raise ValueError(f"{d}/{split}_labels.npy holds labels outside the {len(self.classes)} classes")

    @property
    def images(self) -> np.ndarray:
        if self._images is None:
            self._images = np.load(self._path, mmap_mode="r")
        return self._images

    def __getstate__(self):
        # a loader worker maps the file itself: pickling a memory map would copy the whole array
        return dict(self.__dict__, _images=None)

    def __len__(self):
        return len(self.labels)

    def __getitem__(self, i):
        return torch.from_numpy(np.array(self.images[i])), int(self.labels[i])


def load_dataset(kind: str, root: str, train: bool = True, raw: bool = False, staged_dir: Optional[str] = None):
    """The training split, or with ``train=False`` the held-out one: MNIST ``t10k``, CIFAR-10
    ``test_batch.bin``, ImageNet ``root/ImageFolderVal``. ``raw``: uint8 HWC images for the device-side
    transform (CIFAR-10 and ImageNet; MNIST has no raw form). ``staged_dir`` (ImageNet, raw): the staged files of
    ``distributed_learning_amd.stage`` instead of the JPEG tree, which is then not needed."""
    if staged_dir:
        if kind != "imagenet" or not raw:
            raise ValueError("staged_dir holds raw (uint8 HWC) ImageNet staging images: it needs kind 'imagenet' "
                             "and raw=True")
        return StagedImages(staged_dir, "train" if train else "val")
    if kind == "mnist":
        if raw:
            raise ValueError("MNIST has no raw (uint8 HWC) form: the device-side augmentation serves the "
                             "3-channel CIFAR-10 and ImageNet models only")
        return load_mnist(root, train)
    if kind == "cifar10":
        return load_cifar10(root, train, raw)
    if kind == "imagenet":
        if train:
            return ImageFolder(os.path.join(root, "ImageFolder"), raw)
        val = os.path.join(root, "ImageFolderVal")
        if not os.path.isdir(val):
            raise FileNotFoundError(f"ImageNet validation tree not found: {val}")
        return ImageFolder(val, raw)
    raise ValueError(f"unknown dataset kind {kind!r}")


class EvalPartition:
    """A rank's share of a held-out set as equally shaped batches, every sample counted exactly once.

    Rank ``r`` of ``W`` takes samples ``r, r+W, ...`` in file order (no shuffle, nothing dropped). Every rank
    runs ``len(self)`` batches, the number the largest share needs; what a rank lacks is padded with zero
    images and target -100, which the loss and the accuracy counts ignore. So collectives inside a batch
    line up across ranks and the all-reduced counts cover the set exactly."""

    IGNORE = -100

    def __init__(self, dataset, rank: int, world: int, batch_size: int, num_workers: int = 0):
        if not 0 <= rank < world:
            raise ValueError(f"rank {rank} outside a world of {world}")
        self.dataset, self.batch_size, self.num_workers = dataset, int(batch_size), num_workers
        n = len(dataset)
        self.index = range(rank, n, world)
        largest = (n + world - 1) // world
        self.batches = (largest + self.batch_size - 1) // self.batch_size

    def __len__(self) -> int:
        return self.batches

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        # own generator: the loader's per-iterator seed must not be drawn from the global RNG (an evaluation
        # leaves the training run's random streams where they were)
        loader = torch.utils.data.DataLoader(Partition(self.dataset, self.index), batch_size=self.batch_size,
                                             shuffle=False, num_workers=self.num_workers, drop_last=False,
                                             generator=torch.Generator().manual_seed(0))
        shape, dtype, done = None, None, 0
        for x, y in loader:
            shape, dtype = tuple(x.shape[1:]), x.dtype
            y = y.to(torch.long)
            short = self.batch_size - x.shape[0]
            if short:
                x = torch.cat([x, x.new_zeros((short,) + shape)])
                y = torch.cat([y, y.new_full((short,), self.IGNORE)])
            done += 1
            yield x, y
        if done < self.batches:  # a rank whose share ends a whole batch early
            if shape is None:
                x0 = torch.as_tensor(self.dataset[0][0])
                shape, dtype = tuple(x0.shape), x0.dtype
            for _ in range(self.batches - done):
                yield (torch.zeros((self.batch_size,) + shape, dtype=dtype),
                       torch.full((self.batch_size,), self.IGNORE, dtype=torch.long))


def get_eval_loader(dataset, rank: int, world: int, batch_size: int = PER_WORKER_BATCH_SIZE,
                    num_workers: int = 0) -> EvalPartition:
    return EvalPartition(dataset, rank, world, batch_size, num_workers)


# ------------------------------------------------------------------------------------------------
# Device-resident shards (--resident 1): the augmentation kernel reads its samples in place, by index
# ------------------------------------------------------------------------------------------------
def _bulk_images(dataset):
    """The dataset's images as one uint8 ``[n, Hs, Ws, 3]`` array when it exposes one (``TensorDataset.x`` of
    ``load_cifar10(raw=True)``, ``StagedImages.images``), with its labels; else ``(None, None)``."""
    for images, labels in ((getattr(dataset, "images", None), getattr(dataset, "labels", None)),
                           (getattr(dataset, "x", None), getattr(dataset, "y", None))):
        if images is not None and labels is not None and len(images.shape) == 4 and images.shape[3] == 3 \
                and str(images.dtype).endswith("uint8"):
            return images, labels
    return None, None


class ResidentStore:
    """A rank's data shard held on its training device for the whole run: ``images`` uint8 ``[P + 1, Hs, Ws, 3]``
    and, on the host, ``labels`` int64 ``[P + 1]``. Row ``P`` is the padding sample of an evaluation -- a zero
    image with label :attr:`EvalPartition.IGNORE`. ``ops.augment.augment(store.images, ..., index=)`` reads a
    batch's rows in place: after the fill there is no decode, no collate and no host-to-device image copy.

    ``images`` (uint8 ``[P, Hs, Ws, 3]``, a tensor or a numpy array, memory-mapped or not) is copied in chunks of at
    most :attr:`CHUNK_BYTES`; :meth:`from_dataset` fills from any dataset and an index list. On a GPU a store
    larger than ``max_fraction`` of the memory free at construction is refused: the shard either fits beside the
    step or the run stops -- there is no fallback to host memory. The 0.5 is a policy default, not a measurement;
    it keeps a store from silently crowding out the step."""

    CHUNK_BYTES = 256 << 20

    def __init__(self, images, labels, device, max_fraction: float = 0.5):
        shape = tuple(int(v) for v in images.shape)
        if len(shape) != 4 or shape[3] != 3 or not str(images.dtype).endswith("uint8"):
            raise ValueError(f"ResidentStore: images must be uint8 [P, Hs, Ws, 3], got {images.dtype} {shape}")
        labels = torch.as_tensor(np.asarray(labels)).to(torch.int64).reshape(-1)
        if labels.shape[0] != shape[0]:
            raise ValueError(f"ResidentStore: {shape[0]} images but {labels.shape[0]} labels")
        self._allocate(shape[0], shape[1:3], device, max_fraction)
        self._fill(lambda lo, hi: (torch.as_tensor(np.ascontiguousarray(images[lo:hi])), labels[lo:hi]))

    @classmethod
    def from_dataset(cls, dataset, index: Sequence[int], device, max_fraction: float = 0.5) -> "ResidentStore":
        """Row ``i`` is ``dataset[index[i]]`` (items ``(uint8 [Hs, Ws, 3], label)``). A dataset that exposes its
        images as one array is sliced in bulk; any other is read item by item, once."""
        index = [int(i) for i in index]
        images, labels = _bulk_images(dataset)
        self = cls.__new__(cls)
        if images is not None:
            hw = tuple(images.shape[1:3])
            labels = torch.as_tensor(np.asarray(labels)).to(torch.int64)

            def chunk(lo, hi):
                rows = np.asarray(index[lo:hi], dtype=np.int64)
                block = images[torch.from_numpy(rows)] if torch.is_tensor(images) else images[rows]
                return torch.as_tensor(np.ascontiguousarray(block)), labels[torch.from_numpy(rows)]
        else:
            if len(dataset) == 0:
                raise ValueError("ResidentStore: empty dataset")
            hw = tuple(torch.as_tensor(dataset[index[0] if index else 0][0]).shape[:2])

            def chunk(lo, hi):
                items = [dataset[i] for i in index[lo:hi]]
                return (torch.stack([torch.as_tensor(x) for x, _ in items]),
                        torch.tensor([int(y) for _, y in items], dtype=torch.int64))
        self._allocate(len(index), hw, device, max_fraction)
        self._fill(chunk)
        return self

    @staticmethod
    def check_fits(nbytes: int, device, max_fraction: float) -> None:
        device = torch.device(device)
        if device.type != "cuda":
            return
        free, total = torch.cuda.mem_get_info(device)
        if nbytes > max_fraction * free:
            raise RuntimeError(
                f"resident store of {nbytes} bytes exceeds {max_fraction} of the {free} bytes free on {device} "
                f"({total} in all): the shard does not fit beside the training step. Use more ranks (a rank holds "
                f"1/world of the set) or run without --resident 1; there is no host-memory fallback")

    def _allocate(self, rows: int, hw, device, max_fraction: float) -> None:
        self.device = torch.device(device)
        self.rows, self.hw = int(rows), (int(hw[0]), int(hw[1]))
        self.check_fits((self.rows + 1) * self.hw[0] * self.hw[1] * 3, self.device, max_fraction)
        self.images = torch.empty((self.rows + 1,) + self.hw + (3,), dtype=torch.uint8, device=self.device)
        self.images[self.rows].zero_()
        self.labels = torch.full((self.rows + 1,), EvalPartition.IGNORE, dtype=torch.int64)

    def _fill(self, chunk) -> None:
        """``chunk(lo, hi) -> (uint8 [hi - lo, Hs, Ws, 3], int64 [hi - lo])`` on the host, at most CHUNK_BYTES each."""
        step = max(1, self.CHUNK_BYTES // (self.hw[0] * self.hw[1] * 3))
        for lo in range(0, self.rows, step):
            hi = min(lo + step, self.rows)
            x, y = chunk(lo, hi)
            if tuple(x.shape) != (hi - lo,) + self.hw + (3,) or x.dtype != torch.uint8:
                raise ValueError(f"ResidentStore: rows {lo}..{hi} are {x.dtype} {tuple(x.shape)}, expected uint8 "
                                 f"{(hi - lo,) + self.hw + (3,)}")
            self.images[lo:hi].copy_(x)
            self.labels[lo:hi] = y

    def __len__(self) -> int:
        return self.rows

    @property
    def nbytes(self) -> int:
        return self.images.numel()


class ResidentBatches:
    """The training iterator over a :class:`ResidentStore`, in the exact order of :func:`get_partition_loader`'s
    loader: it owns an ``EpochSampler(P, seed)`` (``.epoch_sampler``, driven by the training loop's ``set_epoch``
    the same way) and one iteration walks ``order(epoch)[start:]`` in consecutive chunks of ``batch_size``, a short
    tail dropped. It yields ``(index int32 [B], y int64 [B])`` on the host: batch ``k`` of a run names the samples
    the ``DataLoader`` path would have loaded, in the same order, resume offsets included."""

    def __init__(self, store: ResidentStore, batch_size: int, seed: int = 1234):
        self.store, self.batch_size = store, int(batch_size)
        self.epoch_sampler = EpochSampler(len(store), seed)

    def __len__(self) -> int:
        return len(self.store) // self.batch_size

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        order = torch.tensor(list(self.epoch_sampler), dtype=torch.int64)
        b = self.batch_size
        for lo in range(0, len(order) - b + 1, b):
            rows = order[lo:lo + b]
            yield rows.to(torch.int32), self.store.labels[rows]


def get_resident_batches(dataset, node_id: int, worker_id: int, node_dev: int, total_dev: int,
                         batch_size: int = PER_WORKER_BATCH_SIZE, device="cpu", seed: int = 1234,
                         max_fraction: float = 0.5) -> ResidentBatches:
    """:func:`get_partition_loader` with the rank's partition held on ``device``: the same partition, the same
    sampler seed, so the same samples in every batch."""
    stream = node_id * node_dev + worker_id
    part = DataPartitioner(dataset, total_dev, batch_size, seed).use(stream)
    store = ResidentStore.from_dataset(dataset, part.index.tolist(), device, max_fraction)
    return ResidentBatches(store, batch_size, seed + stream)


class ResidentEval:
    """:class:`EvalPartition`'s rule over a :class:`ResidentStore`: rank ``r`` of ``W`` takes samples ``r, r + W,
    ...`` of the held-out set, every rank runs the batch count of the largest share, and what a rank lacks is
    index ``P`` -- the store's zero row, target ``IGNORE``. Yields ``(index int32 [B], y int64 [B])`` on the host.

    ``total``: the size of the whole held-out set when ``store`` holds this rank's share only, in that order
    (:meth:`from_dataset`); without it the store holds the whole set and the rank indexes its share."""

    IGNORE = EvalPartition.IGNORE

    def __init__(self, store: ResidentStore, rank: int, world: int, batch_size: int, total: Optional[int] = None):
        if not 0 <= rank < world:
            raise ValueError(f"rank {rank} outside a world of {world}")
        self.store, self.batch_size = store, int(batch_size)
        p = len(store)
        if total is None:
            total, share = p, list(range(rank, p, world))
        else:
            share = list(range(p))
            if p != len(range(rank, int(total), world)):
                raise ValueError(f"ResidentEval: a store of {p} rows is not rank {rank}'s share of {total} samples "
                                 f"over {world} ranks")
        largest = (int(total) + world - 1) // world
        self.batches = (largest + self.batch_size - 1) // self.batch_size
        self.index = torch.full((self.batches * self.batch_size,), p, dtype=torch.int64)
        self.index[:len(share)] = torch.tensor(share, dtype=torch.int64)

    @classmethod
    def from_dataset(cls, dataset, rank: int, world: int, batch_size: int, device,
                     max_fraction: float = 0.5) -> "ResidentEval":
        """Holds only the rank's share ``dataset[r], dataset[r + W], ...``."""
        store = ResidentStore.from_dataset(dataset, range(rank, len(dataset), world), device, max_fraction)
        return cls(store, rank, world, batch_size, total=len(dataset))

    def __len__(self) -> int:
        return self.batches

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        b = self.batch_size
        for k in range(self.batches):
            rows = self.index[k * b:(k + 1) * b]
            yield rows.to(torch.int32), self.store.labels[rows]


# ------------------------------------------------------------------------------------------------
# Synthetic batches
# ------------------------------------------------------------------------------------------------
class SyntheticBatches:
    """Uniform images + uniform labels, generated on the training device every step. fp32 images are in
    [0, 1); bf16 images are the same fp32 stream rounded to nearest, so they are in [0, 1] -- a draw of
    1 - 2^-9 or more becomes exactly 1.0 (probability 2^-9 per element).

    ``per_rank_seed``: by default each rank draws a different stream (seed + rank), which is what
    data parallelism actually sees; set ``identical=True`` to reproduce the reference, where every
    rank seeds 1234 and draws bit-identical batches.
    """

    def __init__(self, batch_size: int, shape: Tuple[int, int, int], num_classes: int, device,
                 dtype: torch.dtype = torch.float32, seed: int = 1234, rank: int = 0, identical: bool = False,
                 channels_last: bool = False, regenerate: bool = True, device_step: bool = False):
        self.batch_size = batch_size
        self.shape = tuple(shape)
        self.num_classes = num_classes
        self.device = torch.device(device)
        self.dtype = dtype
        self.seed = seed if identical else seed + 7919 * rank
        self.channels_last = channels_last and len(shape) == 3
        self.regenerate = regenerate
        self.step = 0
        n, (c, h, w) = batch_size, self.shape
        if self.channels_last:
            self._x = torch.empty((n, h, w, c), device=self.device, dtype=dtype).permute(0, 3, 1, 2)
        else:
            self._x = torch.empty((n, c, h, w), device=self.device, dtype=dtype)
        self._y = torch.empty((n,), device=self.device, dtype=torch.long)
        self._native = self.device.type == "cuda" and _ext.available()
        if self.device.type == "cuda" and not self._native:
            _ext.require()  # fail loudly on a GPU box without the extension
        # device_step: the stream position lives in a device counter advanced by a kernel, so the
        # generation can be captured in a HIP graph and still draw a new batch on every replay
        self._step_dev = (torch.zeros((1,), dtype=torch.long, device=self.device)
                          if device_step and self._native else None)
        self._fill()
        if self._step_dev is not None:
            self._step_dev.zero_()  # same stream positions as the host-stepped generator

    def _fill(self):
        if self._native:
            C = _ext.require()
            flat = self._x if not self.channels_last else self._x.permute(0, 2, 3, 1)
            per_x, per_y = (flat.numel() + 3) // 4, self.batch_size
            if self._step_dev is not None:
                C.uniform_(flat, self.seed, 0, 0.0, 1.0, self._step_dev, per_x)
                C.randint_(self._y, self.num_classes, self.seed, 0, self._step_dev, per_y)
                self._step_dev.add_(1)
            else:
                C.uniform_(flat, self.seed, self.step * per_x, 0.0, 1.0)
                C.randint_(self._y, self.num_classes, self.seed, self.step * per_y)
        else:
            # one generator per step position, so the stream is seekable (checkpoint resume)
            g = torch.Generator().manual_seed(self.seed + 1_000_003 * self.step)
            self._x.copy_(torch.rand(self._x.shape, generator=g).to(self.dtype))
            self._y.copy_(torch.randint(0, self.num_classes, self._y.shape, generator=g))

    def seek(self, step: int) -> None:
        """Continue the stream at batch ``step`` (a resumed run draws the batches it has not seen)."""
        self.step = int(step)
        if self._step_dev is not None:
            self._step_dev.fill_(self.step)

    def next(self) -> Tuple[torch.Tensor, torch.Tensor]:
        if self.regenerate:
            self._fill()
        self.step += 1
        return self._x, self._y

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        while True:
            yield self.next()


def random_data_generator(data_pair):
    """Reference-compatible generator (data.py:129-132): CPU tensors shaped like a template."""
    data, target = data_pair
    while True:
        yield torch.rand_like(data), torch.randint_like(target, high=int(target.max()) + 1)
