"""The indexed forms of the augmentation kernel (csrc/kernels/augment.hip, ``augment_gather_`` and
``augment_mix_gather_``) and the resident store on top of them.

The oracle is the kernel that test_gpu_augment.py and test_gpu_augment_mix.py already prove: for any store and
index the indexed form must equal the existing form run on ``store[index].contiguous()`` bit for bit -- the source
bytes are the same, so there is no tolerance and no excluded share. Integer geometry is also compared with the
numpy formula directly. 7 x 9 x 3 = 189 elements per image put image boundaries inside 16-byte groups, where the
per-image reload of the index and the image base can go wrong.
"""
import copy

import numpy as np
import pytest
import torch

import augment_oracle as ao
import mix_oracle as mo
from test_augment_cpu import _write_cifar

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
P = 9
INDEX5 = (7, 2, 7, 0, 8)  # a repeat, not sorted, the store's first and last rows
INDEX12 = (8, 0, 3, 3, 1, 7, 2, 6, 5, 4, 8, 0)  # N > P
INDEXES = {"n5": INDEX5, "n12": INDEX12}


def _u8(v, dev=None):
    return torch.as_tensor(v, dtype=torch.uint8, device=dev)


def _plain(src, geom, flip, out_hw, dtype, pad=0, index=None):
    from distributed_learning_amd.ops.augment import augment

    return augment(src, geom, _u8(flip), ao.MEAN, ao.STD, out_hw, dtype, pad, index=index)


def _mix(src, geom, flip, partner, lam, box, out_hw, dtype, pad=0, blend=True, index=None):
    from distributed_learning_amd.ops.augment import augment_mix

    return augment_mix(src, geom, _u8(flip), partner, lam, box, ao.MEAN, ao.STD, out_hw, dtype, pad, blend,
                       index=index)


def _cycle(seq, n):
    return [seq[i % len(seq)] for i in range(n)]


@pytest.fixture(scope="module")
def store(cuda):
    return ao.noise_source(P, seed=23).to(cuda)  # shared, never written


def _gathered(store, index):
    return store[torch.tensor(index, device=store.device)].contiguous()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("index", INDEXES.values(), ids=INDEXES.keys())
@pytest.mark.parametrize("offsets,pad", [(ao.INT_INSIDE, 0), (ao.INT_PAD4, 4)], ids=["inside", "pad4"])
def test_integer_geometry_bitwise(cuda, store, offsets, pad, index, dtype):
    n = len(index)
    offs, flips = _cycle(offsets, n), _cycle(ao.FLIP3, n)
    idx = torch.tensor(index, dtype=torch.int32)
    out = _plain(store, ao.int_geom(offs), flips, ao.INT_HW, dtype, pad, index=idx)
    assert out.shape == (n, 3) + ao.INT_HW and out.dtype == dtype
    assert out.is_contiguous(memory_format=torch.channels_last)
    batch = _gathered(store, index)
    mo.assert_same_bits(out, _plain(batch, ao.int_geom(offs), flips, ao.INT_HW, dtype, pad), "indexed vs gathered")
    ao.assert_bitwise(out, ao.expected_int(batch.cpu(), offs, flips, ao.INT_HW, pad))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("index", INDEXES.values(), ids=INDEXES.keys())
def test_interpolated_bitwise(cuda, store, index, dtype):
    """Interpolated boxes, among them the one flush bottom-right that reads an image's very last pixel: in the
    indexed form every image, not just the batch's last, ends at the clamp of the 8-byte load."""
    n = len(index)
    rows = _cycle(range(5), n)
    geom, flips = ao.interp_geom()[rows], [ao.INTERP_FLIP[i] for i in rows]
    out = _plain(store, geom, flips, ao.INTERP_HW, dtype, index=torch.tensor(index, dtype=torch.int32))
    mo.assert_same_bits(out, _plain(_gathered(store, index), geom, flips, ao.INTERP_HW, dtype), "indexed vs gathered")
    # a device index is taken as it is
    dev = _plain(store, geom, flips, ao.INTERP_HW, dtype, index=torch.tensor(index, dtype=torch.int32, device=cuda))
    mo.assert_same_bits(out, dev, "host vs device index")


# partner has a fixed point (position 1) and positions 0 and 2 index the same store row (7): the partner's image is
# row index[partner[n]], its geom and flip are rows partner[n] of the batch's arrays
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("blend", [False, True], ids=["select", "blend"])
def test_cutmix_bitwise(cuda, store, blend, dtype):
    assert mo.PARTNER5[1] == 1 and INDEX5[0] == INDEX5[2]
    batch = _gathered(store, INDEX5)
    idx = torch.tensor(INDEX5, dtype=torch.int32)
    partner, lam, box = mo.tensors(mo.PARTNER5, (1.0,) * 5, mo.BOXES5)
    for geom, flips, hw, pad in ((ao.int_geom(mo.INT_INSIDE5), mo.FLIP5, ao.INT_HW, 0),
                                 (ao.int_geom(mo.INT_PAD4_5), mo.FLIP5, ao.INT_HW, 4),
                                 (ao.interp_geom(), ao.INTERP_FLIP, ao.INTERP_HW, 0)):
        bx = box if hw == ao.INT_HW else mo.tensors(mo.PARTNER5, (1.0,) * 5, mo.INTERP_BOX)[2]
        out = _mix(store, geom, flips, partner, lam, bx, hw, dtype, pad, blend, index=idx)
        want = _mix(batch, geom, flips, partner, lam, bx, hw, dtype, pad, blend)
        mo.assert_same_bits(out, want, f"cutmix blend={blend} pad={pad}")
        assert not np.array_equal(ao.bits_of(out), ao.bits_of(_plain(batch, geom, flips, hw, dtype, pad)))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_mixup_bitwise(cuda, store, dtype):
    batch = _gathered(store, INDEX5)
    idx = torch.tensor(INDEX5, dtype=torch.int32)
    for lams in mo.LAMS + (mo.INTERP_LAM,):
        for geom, flips, hw in ((ao.int_geom(mo.INT_INSIDE5), mo.FLIP5, ao.INT_HW),
                                (ao.interp_geom(), ao.INTERP_FLIP, ao.INTERP_HW)):
            boxes = mo.INTERP_BOX if hw == ao.INTERP_HW else ((0, 0, 0, 0),) * 5
            partner, lam, box = mo.tensors(mo.PARTNER5, lams, boxes)
            out = _mix(store, geom, flips, partner, lam, box, hw, dtype, 0, True, index=idx)
            mo.assert_same_bits(out, _mix(batch, geom, flips, partner, lam, box, hw, dtype, 0, True), f"mixup {lams}")


def test_mix_with_more_samples_than_rows(cuda, store):
    """N = 12 > P = 9 through both mixed forms, with a partner permutation that has no fixed structure."""
    n = len(INDEX12)
    batch, idx = _gathered(store, INDEX12), torch.tensor(INDEX12, dtype=torch.int32)
    rows = _cycle(range(5), n)
    geom, flips = ao.interp_geom()[rows], [ao.INTERP_FLIP[i] for i in rows]
    partner = torch.tensor([5, 11, 2, 0, 9, 3, 10, 1, 8, 6, 4, 7], dtype=torch.int32)
    box = torch.tensor(_cycle(mo.INTERP_BOX, n), dtype=torch.int32)
    for blend, lam in ((False, torch.ones(n)), (True, torch.tensor(_cycle(mo.INTERP_LAM, n)))):
        out = _mix(store, geom, flips, partner, lam, box, ao.INTERP_HW, torch.bfloat16, 0, blend, index=idx)
        want = _mix(batch, geom, flips, partner, lam, box, ao.INTERP_HW, torch.bfloat16, 0, blend)
        mo.assert_same_bits(out, want, f"N > P, blend={blend}")


def _binding_args(cuda, store):
    from distributed_learning_amd.ops.augment import scale_bias

    scale, bias = (t.to(cuda) for t in scale_bias(ao.MEAN, ao.STD))
    return dict(store=store, index=torch.tensor(INDEX5, dtype=torch.int32, device=cuda),
                geom=ao.interp_geom().to(cuda), flip=_u8(ao.INTERP_FLIP, cuda), scale=scale, bias=bias, pad=0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("form", ["plain", "select", "blend"])
def test_writes_stay_inside_out(cuda, store, form, dtype):
    """``out`` between two NaN guard rows, its base off 16-byte alignment (the construction of
    test_gpu_augment.py::test_writes_stay_inside_out): the guards stay NaN and the inside equals the call that
    allocates its own output bit for bit."""
    from distributed_learning_amd.ops import _ext

    C = _ext.require()
    ho, wo = ao.INTERP_HW
    row, n = wo * 3, 5 * ho * wo * 3
    buf = torch.full((row + n + row,), float("nan"), dtype=dtype, device=cuda)
    out = buf[row:row + n].view(5, ho, wo, 3).permute(0, 3, 1, 2)
    assert out.data_ptr() % 16 != 0
    args = _binding_args(cuda, store)
    idx = args["index"].cpu()
    if form == "plain":
        C.augment_gather_(out=out, **args)
        want = _plain(store, ao.interp_geom(), ao.INTERP_FLIP, ao.INTERP_HW, dtype, index=idx)
    else:
        lams = (1.0,) * 5 if form == "select" else mo.INTERP_LAM
        partner, lam, box = mo.tensors(mo.PARTNER5, lams, mo.INTERP_BOX)
        C.augment_mix_gather_(out=out, partner=partner.to(cuda), lam=lam.to(cuda), box=box.to(cuda),
                              blend=form == "blend", **args)
        want = _mix(store, ao.interp_geom(), ao.INTERP_FLIP, partner, lam, box, ao.INTERP_HW, dtype, 0,
                    form == "blend", index=idx)
    assert bool(buf[:row].isnan().all()) and bool(buf[-row:].isnan().all())
    assert not bool(buf[row:row + n].isnan().any())
    assert np.array_equal(ao.bits_of(out), ao.bits_of(want))


BIG_ROWS = 21850  # x 256 x 256 x 3 = 4.30 GB
NOISE_ROWS = (0, 10922, 10923, 21845, 21849)


def test_store_beyond_32_bit_byte_offsets(cuda):
    """A 4.30 GB store: row 10922 straddles byte 2^31 (at its image row 170), row 21845 byte 2^32, row 21849 is the
    last. Identity geometry reads every byte of the indexed rows; a zero row between them comes out as bias."""
    img = 256 * 256 * 3
    assert 10922 * img < 2 ** 31 < 10923 * img and (2 ** 31 - 10922 * img) // 768 == 170
    assert 21845 * img < 2 ** 32 < 21846 * img and BIG_ROWS * img > 2 ** 32
    free, _ = torch.cuda.mem_get_info(cuda)
    if free < 6 * 2 ** 30:
        pytest.skip(f"needs 6 GB of free device memory, {free} bytes are free")
    big = torch.zeros((BIG_ROWS, 256, 256, 3), dtype=torch.uint8, device=cuda)
    noise = ao.noise_source(len(NOISE_ROWS), 256, 256, seed=31)
    big[torch.tensor(NOISE_ROWS, device=cuda)] = noise.to(cuda)
    index = torch.tensor(NOISE_ROWS[:2] + (5,) + NOISE_ROWS[2:], dtype=torch.int32)  # row 5 is all zeros
    n = index.numel()
    offs, flips = [(0, 0)] * n, [0] * n
    src = torch.cat([noise[:2], torch.zeros_like(noise[:1]), noise[2:]])
    want = ao.expected_int(src, offs, flips, (256, 256), 0)
    black = ao.scale_bias64()[1].astype(np.float32)
    assert (want[2] == black).all()
    for dtype in DTYPES:
        out = _plain(big, ao.int_geom(offs), flips, (256, 256), dtype, index=index)
        ao.assert_bitwise(out, want)
    # the mixed forms form the partner's base the same way: each noise row pasted over its neighbour
    partner, lam, box = mo.tensors((1, 0, 2, 4, 5, 3), (1.0,) * n, ((64, 64, 192, 192),) * n)
    mixed = mo.mix(want, partner.tolist(), (1.0,) * n, box.tolist()).astype(np.float32)
    for blend in (False, True):
        ao.assert_bitwise(_mix(big, ao.int_geom(offs), flips, partner, lam, box, (256, 256), torch.float32, 0, blend,
                               index=index), mixed)
    del big
    torch.cuda.empty_cache()


def test_guards_raise_before_launch(cuda, store):
    from distributed_learning_amd.ops import _ext

    C = _ext.require()
    good = _binding_args(cuda, store)
    ho, wo = ao.INTERP_HW
    out = torch.full((5, ho, wo, 3), float("nan"), device=cuda).permute(0, 3, 1, 2)
    wide = ao.noise_source(P, ao.HS, 2 * ao.WS).to(cuda)
    partner, lam, box = (t.to(cuda) for t in mo.tensors(mo.PARTNER5, (1.0,) * 5, mo.INTERP_BOX))
    bad = {
        "int64 index": dict(index=good["index"].long()),
        "short index": dict(index=good["index"][:4].contiguous()),
        "long index": dict(index=torch.zeros(6, dtype=torch.int32, device=cuda)),
        "host index": dict(index=good["index"].cpu()),
        "non-contiguous index": dict(index=torch.zeros(10, dtype=torch.int32, device=cuda)[::2]),
        "non-contiguous store": dict(store=wide[:, :, ::2]),
        "image of 2 pixels": dict(store=torch.zeros(P, 1, 2, 3, dtype=torch.uint8, device=cuda)),
        "empty store": dict(store=torch.zeros(0, ao.HS, ao.WS, 3, dtype=torch.uint8, device=cuda)),
        "geom of the wrong length": dict(geom=good["geom"][:4].contiguous()),
        "flip of the wrong length": dict(flip=good["flip"][:4].contiguous()),
    }
    for what, change in bad.items():
        args = dict(good, out=out)
        args.update(change)
        for call, extra in ((C.augment_gather_, {}),
                            (C.augment_mix_gather_, dict(partner=partner, lam=lam, box=box, blend=True))):
            with pytest.raises((RuntimeError, ValueError, TypeError)):
                call(**args, **extra)
                pytest.fail(f"{what}: the binding accepted it")
            torch.cuda.synchronize()
            assert bool(out.isnan().all()), f"{what}: out was written"
    for what, change in {"short partner": dict(partner=partner[:4].contiguous()),
                         "short lam": dict(lam=lam[:4].contiguous()),
                         "short box": dict(box=box[:4].contiguous())}.items():
        args = dict(good, out=out, partner=partner, lam=lam, box=box, blend=True)
        args.update(change)
        with pytest.raises((RuntimeError, ValueError, TypeError)):
            C.augment_mix_gather_(**args)
            pytest.fail(f"{what}: the binding accepted it")
        torch.cuda.synchronize()
        assert bool(out.isnan().all()), f"{what}: out was written"
    C.augment_gather_(out=out, **good)  # and the unchanged arguments pass
    mo.assert_same_bits(out, _plain(_gathered(store, INDEX5), ao.interp_geom(), ao.INTERP_FLIP, ao.INTERP_HW,
                                    torch.float32), "through the binding")


# --- the resident store and its iterator -------------------------------------------------------------
def test_resident_batches_equal_the_loader_path(cuda, tmp_path):
    """CIFAR fixture, 40 samples, batch 8, 7 batches (an epoch boundary after 5): each resident batch's indexed
    output and labels equal the plain kernel on what the DataLoader path yields for that batch, bit for bit --
    from the start, and from batch 3 through set_epoch."""
    from distributed_learning_amd import data as D
    from distributed_learning_amd.ops.augment import CIFAR10_MEAN, CIFAR10_STD, AugmentParams, augment

    ds = D.load_cifar10(str(_write_cifar(tmp_path)), raw=True)
    loader = D.get_partition_loader(ds, 0, 0, 1, 1, 8, num_workers=0)
    res = D.get_resident_batches(ds, 0, 0, 1, 1, 8, cuda)
    assert isinstance(res.store, D.ResidentStore) and res.store.images.device == cuda
    assert res.store.images.shape == (41, 32, 32, 3) and len(res) == len(loader) == 5
    assert not bool(res.store.images[40].any()) and int(res.store.labels[40]) == D.EvalPartition.IGNORE
    params = AugmentParams("padcrop", (32, 32), (32, 32), pad=4)

    def walk(batches, first, count):
        got, k = [], first
        epoch, skip = D.resume_position(first, len(batches))
        while len(got) < count:
            batches.epoch_sampler.set_epoch(epoch, skip * 8)
            for item in batches:
                got.append((k, item))
                k += 1
                if len(got) == count:
                    break
            epoch, skip = epoch + 1, 0
        return got

    for first, count in ((0, 7), (3, 4)):
        for (k, (x, y)), (k2, (index, y2)) in zip(walk(loader, first, count), walk(res, first, count)):
            assert k == k2 and index.dtype == torch.int32 and index.shape == (8,) and y2.dtype == torch.int64
            assert torch.equal(y, y2)
            geom, flip = params.params(k, 8)
            for dtype in DTYPES:
                want = augment(x.to(cuda), geom, flip, CIFAR10_MEAN, CIFAR10_STD, (32, 32), dtype, 4)
                got = augment(res.store.images, geom, flip, CIFAR10_MEAN, CIFAR10_STD, (32, 32), dtype, 4, index=index)
                mo.assert_same_bits(got, want, f"batch {k}")


def test_native_run_resident_equals_the_loader_path(cuda, tmp_path):
    """One in-process bf16 native run of resnet18_cifar, 3 batches with CutMix: the resident run's first loss is
    bitwise the loader path's (the model input is the same bits), and every loss is equal wherever two loader-path
    runs equal one another (the control: the native step itself may not be run-to-run deterministic)."""
    from distributed_learning_amd import experiments
    from distributed_learning_amd.config import parse_args

    data = _write_cifar(tmp_path / "data")

    def run(sub, *extra):
        cfg = parse_args(["1", "0", "1", "1", "127.0.0.1", "lo", "resnet18_cifar", str(data), "1", "--limit_batches",
                          "3", "--batch_size", "8", "--augment", "standard", "--cutmix_alpha", "1", *extra])
        cfg.folder = str(tmp_path / sub)
        return experiments.main_single(copy.copy(cfg))["losses"]

    # the training loop turns torch.backends.cudnn.benchmark on for its process; put it back, or every fp32 torch
    # reference convolution of the tests that run after this one would start with an exhaustive MIOpen search
    tuned = torch.backends.cudnn.benchmark
    try:
        a, b = run("a"), run("b")
        r = run("r", "--resident", "1")
    finally:
        torch.backends.cudnn.benchmark = tuned
    assert len(a) == len(r) == 3 and all(np.isfinite(r))
    print(f"loader {a}\nloader {b}\nresident {r}")
    assert r[0] == a[0] == b[0]
    for i in range(3):
        if a[i] == b[i]:
            assert r[i] == a[i], f"batch {i}: resident {r[i]} vs loader {a[i]}"
