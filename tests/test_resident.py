"""The resident store and its iterators (data.py) on the CPU: the store lives in host memory there, the order and
padding rules are the same."""
import numpy as np
import pytest
import torch

from test_augment_cpu import _write_cifar


def _order(batches, epochs, first=0, batch=8):
    """The (index or image, label) batches of ``epochs`` epochs from global batch ``first``, as the training loop
    drives the sampler."""
    from distributed_learning_amd.data import resume_position

    epoch0, skip = resume_position(first, len(batches))
    out = []
    for epoch in range(epoch0, epochs):
        batches.epoch_sampler.set_epoch(epoch, skip * batch if epoch == epoch0 else 0)
        out.extend(batches)
    return out


def test_resident_batches_follow_the_loader_order(tmp_path):
    from distributed_learning_amd import data as D

    ds = D.load_cifar10(str(_write_cifar(tmp_path)), raw=True)
    for total_dev, part, batch in ((1, 0, 8), (2, 1, 6)):  # 40 samples: 5 batches of 8; 2 x 18 samples, 3 of 6
        loader = D.get_partition_loader(ds, 0, part, total_dev, total_dev, batch, num_workers=0)
        res = D.get_resident_batches(ds, 0, part, total_dev, total_dev, batch, "cpu")
        assert isinstance(res.epoch_sampler, D.EpochSampler) and res.epoch_sampler.seed == loader.epoch_sampler.seed
        assert len(res) == len(loader) == len(res.store) // batch
        for first in (0, 2):
            want, got = _order(loader, 2, first, batch), _order(res, 2, first, batch)
            assert len(want) == len(got) == 2 * len(loader) - first
            for (x, y), (index, y2) in zip(want, got):
                assert index.dtype == torch.int32 and tuple(index.shape) == (batch,) and index.device.type == "cpu"
                assert y2.dtype == torch.int64 and torch.equal(y, y2)
                assert torch.equal(res.store.images[index.long()], x)
        epochs = [torch.cat([i for i, _ in _order(res, e + 1)[-len(res):]]) for e in range(2)]
        assert not torch.equal(epochs[0], epochs[1])  # a new order every epoch
        assert sorted(epochs[0].tolist()) == list(range(len(res.store)))  # and each sample once (no tail here)


def test_short_tail_is_dropped():
    from distributed_learning_amd.data import ResidentBatches, ResidentStore

    store = ResidentStore(torch.zeros(11, 2, 2, 3, dtype=torch.uint8), torch.arange(11), "cpu")
    res = ResidentBatches(store, 4, seed=5)
    got = list(res)
    assert len(res) == len(got) == 2 and all(i.numel() == 4 for i, _ in got)
    assert torch.equal(torch.cat([i for i, _ in got]).long(), torch.tensor(res.epoch_sampler.order(0)[:8]))
    res.epoch_sampler.set_epoch(0, 4)
    assert [i.tolist() for i, _ in res] == [got[1][0].tolist()]


def test_store_rows_labels_and_zero_row(tmp_path):
    from distributed_learning_amd import data as D

    ds = D.load_cifar10(str(_write_cifar(tmp_path)), raw=True)
    index = [5, 0, 39, 5, 17]
    bulk = D.ResidentStore.from_dataset(ds, index, "cpu")

    class Items:  # no array to slice: the item-by-item path
        def __len__(self):
            return len(ds)

        def __getitem__(self, i):
            return ds[i]

    items = D.ResidentStore.from_dataset(Items(), index, "cpu")
    direct = D.ResidentStore(ds.x[index].numpy(), ds.y[index], "cpu")
    for s in (bulk, items, direct):
        assert len(s) == 5 and s.images.shape == (6, 32, 32, 3) and s.images.dtype == torch.uint8
        assert torch.equal(s.images[:5], ds.x[index]) and torch.equal(s.labels[:5], ds.y[index])
        assert not bool(s.images[5].any()) and s.labels.dtype == torch.int64
        assert int(s.labels[5]) == D.EvalPartition.IGNORE == -100
        assert s.nbytes == 6 * 32 * 32 * 3
    with pytest.raises(ValueError):
        D.ResidentStore(ds.x.float(), ds.y, "cpu")
    with pytest.raises(ValueError):
        D.ResidentStore(ds.x, ds.y[:-1], "cpu")


def test_fill_in_chunks(monkeypatch):
    from distributed_learning_amd.data import ResidentStore

    g = torch.Generator().manual_seed(0)
    x = torch.randint(0, 256, (7, 4, 5, 3), generator=g, dtype=torch.uint8)
    monkeypatch.setattr(ResidentStore, "CHUNK_BYTES", 2 * 4 * 5 * 3 + 1)  # two images per chunk, a chunk of one last
    s = ResidentStore(x.numpy(), np.arange(7), "cpu")
    assert torch.equal(s.images[:7], x) and s.labels[:7].tolist() == list(range(7))
    assert ResidentStore.CHUNK_BYTES != 256 << 20
    monkeypatch.undo()
    assert ResidentStore.CHUNK_BYTES == 256 << 20


def test_resident_eval_covers_the_set_once():
    from distributed_learning_amd.data import EvalPartition, ResidentEval, ResidentStore, TensorDataset

    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, 256, (8, 4, 4, 3), generator=g, dtype=torch.uint8)
    ds = TensorDataset(x, torch.arange(10, 18))
    seen = []
    for rank in range(3):
        ev = ResidentEval.from_dataset(ds, rank, 3, 2, "cpu")
        ref = EvalPartition(ds, rank, 3, 2)
        p = len(ev.store)
        assert p == len(range(rank, 8, 3)) and len(ev) == len(ref) == 2  # the largest share is 3: two batches
        assert torch.equal(ev.store.images[:p], x[rank::3])  # only its share, in that order
        got = list(ev)
        assert len(got) == 2
        for (index, y), (xr, yr) in zip(got, ref):
            assert index.dtype == torch.int32 and y.dtype == torch.int64
            assert torch.equal(y, yr) and torch.equal(ev.store.images[index.long()], xr)
        index, y = torch.cat([i for i, _ in got]), torch.cat([t for _, t in got])
        pad = index == p
        assert int(pad.sum()) == 4 - p and bool((y[pad] == -100).all()) and not bool((y[~pad] == -100).any())
        seen += y[~pad].tolist()
    assert sorted(seen) == list(range(10, 18))
    # rank 1 of 3: samples 1, 4, 7, then one padding sample
    ev = ResidentEval.from_dataset(ds, 1, 3, 2, "cpu")
    assert [i.tolist() for i, _ in ev] == [[0, 1], [2, 3]] and [y.tolist() for _, y in ev] == [[11, 14], [17, -100]]
    # a store of the whole set: the rank indexes its share
    whole = ResidentEval(ResidentStore(x, ds.y, "cpu"), 1, 3, 2)
    assert [i.tolist() for i, _ in whole] == [[1, 4], [7, 8]] and [y.tolist() for _, y in whole] == [[11, 14], [17, -100]]
    with pytest.raises(ValueError):
        ResidentEval(ResidentStore(x, ds.y, "cpu"), 3, 3, 2)
    with pytest.raises(ValueError):
        ResidentEval(ResidentStore(x[:2], ds.y[:2], "cpu"), 1, 3, 2, total=8)


def test_store_larger_than_the_allowed_fraction_is_refused(monkeypatch):
    from distributed_learning_amd.data import ResidentStore

    free, total = 1000 * 2 ** 20, 4000 * 2 ** 20
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (free, total))
    nbytes = 501 * 2 ** 20
    with pytest.raises(RuntimeError) as e:
        ResidentStore.check_fits(nbytes, "cuda:0", 0.5)
    msg = str(e.value)
    assert str(nbytes) in msg and str(free) in msg and "0.5" in msg and "no host-memory fallback" in msg
    ResidentStore.check_fits(500 * 2 ** 20, "cuda:0", 0.5)  # exactly the fraction fits
    ResidentStore.check_fits(nbytes, "cuda:0", 0.75)
    ResidentStore.check_fits(10 ** 15, "cpu", 0.5)  # host memory is not policed
    # the constructor asks before it allocates: on a "GPU" with nothing free it raises without touching the device
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (0, total))
    with pytest.raises(RuntimeError, match="resident store of"):
        ResidentStore(torch.zeros(3, 2, 2, 3, dtype=torch.uint8), torch.zeros(3), "cuda:0")
