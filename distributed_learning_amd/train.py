"""The per-worker training loop (reference: ``worker_process``, /root/reference/src/main.py:29-107).

Per batch, identical phase structure and timer names to the reference:
``batch`` ⊃ ``get_data`` -> ``data2dev`` -> ``zero_grad`` -> ``forward`` (model + loss) -> ``backprop``
-> ``sync`` (``model.sync_gradients()``) -> ``optimizer_step``, then one row appended with
``batch_count`` and ``data_len``; at the end ``{exp}_{node}_{worker}_times.csv``,
``{exp}_{node}_{worker}_loss.txt`` and ``{exp}_config.txt``.

Differences by design:
* errors propagate (the reference printed and swallowed them, main.py:109-114, which left the
  node pump blocked forever);
* the loss line is formatted from device values collected without a per-step host sync (the
  reference's f-string forced ``.item()`` every batch) unless ``--sync_timers 1``;
* a device-accurate ``*_device_times.csv`` (HIP events) is written beside the parity CSV;
* only one process writes ``{exp}_config.txt`` (the reference raced all workers on it);
* optional checkpoint save/resume (the reference had none);
* optional label smoothing (``--label_smoothing``) and evaluation on held-out data (``--eval_batches``,
  ``--eval_every``, ``--topk``): :func:`evaluate` runs between two batches, outside every timer row, and
  appends one line per evaluation to ``{exp}_{node}_{worker}_eval.txt``; without the flags nothing of it runs;
* optional training augmentation (``--augment standard``): the loaders hand over raw uint8 HWC images, ``data2dev``
  is one uint8 copy plus one kernel (ops/augment.py) that crops, resamples, flips, normalises, casts and lays out
  the batch with parameters drawn from (seed, partition, batch number); evaluation uses the centre crop through
  the same kernel; without the flag nothing of it runs;
* optional Mixup / CutMix on top of it (``--mixup_alpha``, ``--cutmix_alpha``, ``--mix_switch_prob``): the same
  kernel pass mixes every sample with a partner (parameters from (seed, partition, batch number) as well) and the
  loss is the pair-target ``ops.cross_entropy_mix``; without the flags nothing of it runs;
* optional weight averaging (``--ema_decay``, ``--ema_warmup``): the optimizer's update kernels also advance an
  exponential moving average of every weight (ops/optim.py ``ModelEMA``), every evaluation runs a second time
  from the averages (``eval_ema`` lines), and checkpoints carry them; without the flag nothing of it runs;
* optional Adam-family optimizers (``--optimizer lamb`` / ``adamw`` with ``--beta1``, ``--beta2``, ``--opt_eps``): the
  fused LAMB / AdamW of ops/optim.py under the same schedule, clipping (``--max_grad_norm``), weight averaging and
  checkpoint code as LARS; with ``sgd`` or ``lars`` nothing of it runs;
* optional staged and device-resident data (``--staged_dir``, ``--resident 1``, both on top of ``--augment
  standard``): the ImageNet staging images come from the files of ``distributed_learning_amd.stage`` instead of a
  per-epoch JPEG decode, and with ``--resident 1`` the rank's shard lives on the device (``data.ResidentStore``),
  ``get_data`` yields an index list in the loader's exact order and ``data2dev`` is the indexed form of the
  augmentation kernel reading its samples in place; without the flags nothing of it runs;
* on GPU the step is the framework's measured headline path (the one ``bench.py`` times): native
  MFMA convolutions / FC heads and fused BN kernels, bf16 weights with fp32 master weights in the
  fused SGD (``--precision bf16``, default), on-device synthetic batches, and every gradient
  collective on the C++ RCCL engine's comm stream. ``--precision fp32`` runs the reference's
  numerics (fp32 weights and activations on MIOpen / torch kernels); ``--precision autocast`` keeps
  fp32 parameters under bf16 autocast.
"""
from __future__ import annotations

import copy
import datetime
import itertools
import os
import time
from typing import Callable, Optional

import torch
import torch.distributed as dist
import torch.nn as nn

from . import data as D
from .models import get_spec
from .ops import augment as aug
from .ops import nn as dnn
from .ops.loss import cross_entropy, cross_entropy_mix, cross_entropy_with_metrics
from .ops.optim import FusedAdamW, FusedLAMB, FusedLARS, FusedSGD, ModelEMA, poly_warmup_lr
from .timing import EventTimers, Timers
from .utils.log import Level, print_d


def _model_for(config, device):
    spec = get_spec(config.model_name)
    torch.manual_seed(config.seed)  # identical init on all ranks (reference main.py:31) ...
    model = spec.build().to(device)
    if _channels_last(config, device):
        model = model.to(memory_format=torch.channels_last)
    return spec, model


def _precision(config, device) -> str:
    return getattr(config, "precision", "fp32") if device.type == "cuda" else "fp32"


def _channels_last(config, device) -> bool:
    """NHWC on the GPU for the native (bf16) kernels; the fp32 reference-precision path keeps the
    reference's NCHW layout, where MIOpen has its tuned fp32 kernels (fp32 NHWC fell back to kernels
    that needed minutes per GoogLeNet step)."""
    return device.type == "cuda" and _precision(config, device) != "fp32"


def setup_compute_path(config, device) -> str:
    """Select the kernels of the step; returns the precision in effect (bf16 | autocast | fp32)."""
    prec = _precision(config, device)
    if device.type != "cuda":
        dnn.set_backend("torch")
        dnn.set_native_conv(False)
        return prec
    # MIOpen's exhaustive find for the fp32 reference-precision path costs minutes of tuning per new
    # shape; its default (immediate-mode) choice is what the reference's own runs used
    torch.backends.cudnn.benchmark = prec != "fp32"
    native = config.kernels == "native" and prec != "fp32"  # the native kernels are bf16 kernels
    dnn.set_backend("native" if native else "torch")
    dnn.set_native_conv(native and getattr(config, "conv", "native") == "native")
    return prec


def _no_dataset(config) -> bool:
    """Synthetic input: asked for, or no dataset to read (a staged directory stands in for the dataset root)."""
    if config.random_input:
        return True
    if getattr(config, "staged_dir", None):
        return False
    return not config.dataset_root or not os.path.isdir(config.dataset_root)


def _data_for(config, spec, device, rank: int, node_id: int, worker_id: int, dtype=torch.float32):
    if _no_dataset(config):
        if not config.random_input:
            print_d(f"dataset root {config.dataset_root!r} not found: using synthetic data", Level.WARNING)
        return D.SyntheticBatches(config.batch_size, spec.input_shape, spec.num_classes, device,
                                  dtype=dtype, seed=config.seed, rank=rank,
                                  channels_last=_channels_last(config, device))
    ds = D.load_dataset(spec.dataset, config.dataset_root, raw=_augmenting(config),
                        staged_dir=getattr(config, "staged_dir", None))
    if _resident(config):
        return D.get_resident_batches(ds, node_id, worker_id, config.node_dev, config.total_dev, config.batch_size,
                                      device)
    return D.get_partition_loader(ds, node_id, worker_id, config.node_dev, config.total_dev, config.batch_size)


def _augmenting(config) -> bool:
    return getattr(config, "augment", "none") != "none"


def _resident(config) -> bool:
    return bool(getattr(config, "resident", 0))


def _mixing(config) -> bool:
    return getattr(config, "mixup_alpha", 0.0) > 0 or getattr(config, "cutmix_alpha", 0.0) > 0


def _augmenters(config, spec, device, prec: str, stream: int):
    """``--augment standard``: the (training, evaluation) transforms ``(raw uint8 batch on the device, batch
    number) -> model input`` in the step's dtype and layout, through ops/augment.py: random-resized crop 256 -> 224
    plus flip (ImageNet models) or pad-4 random crop plus flip (CIFAR models) for training, the centre crop for
    evaluation. The training parameters are a function of (seed, partition ``stream``, batch number) alone.
    ``index=`` (``--resident 1``): ``x`` is a resident store's images and the batch its rows ``index``."""
    if spec.dataset == "imagenet":
        kind, src_hw, pad = "rrc", (D.ImageFolder.STAGE, D.ImageFolder.STAGE), 0
        mean, std = aug.IMAGENET_MEAN, aug.IMAGENET_STD
    elif spec.dataset == "cifar10":
        kind, src_hw, pad = "padcrop", tuple(spec.input_shape[1:]), 4
        mean, std = aug.CIFAR10_MEAN, aug.CIFAR10_STD
    else:
        raise ValueError(f"--augment {config.augment} needs a CIFAR-10 or ImageNet model, not {spec.dataset!r}")
    out_hw = tuple(spec.input_shape[1:])
    dtype = torch.bfloat16 if prec == "bf16" else torch.float32
    cl = _channels_last(config, device)

    def make(kind: str, pad: int):
        p = aug.AugmentParams(kind, src_hw, out_hw, seed=config.seed, stream=stream,
                              scale_min=getattr(config, "aug_scale_min", 0.08), pad=pad)

        def apply(x, batch: int, mix=None, index=None):
            """``mix``: ``(partner, lam, box, blend)`` of :class:`~.ops.augment.MixParams` -- Mixup / CutMix in
            the same kernel pass."""
            n = x.shape[0] if index is None else index.shape[0]
            if mix is None:
                x = aug.augment(x, *p.params(batch, n), mean, std, out_hw, dtype, pad, index=index)
            else:
                x = aug.augment_mix(x, *p.params(batch, n), *mix[:3], mean, std, out_hw, dtype, pad, mix[3],
                                    index=index)
            return x if cl else x.contiguous()  # the fp32 reference-precision path runs NCHW

        return apply

    return make(kind, pad), make("center", 0)


def _indexed(apply: Callable, store) -> Callable:
    """``apply`` over a resident store: the batch it is handed is the int32 row index."""
    return lambda index, batch, mix=None: apply(store.images, batch, mix, index=index)


def _config_text(config) -> str:
    """``{exp}_config.txt``: the augmentation, mixing and weight-average flags appear only when set, so a run
    without them writes the file it always did."""
    shown = copy.copy(config)
    if not _augmenting(config):
        for k in ("augment", "aug_scale_min"):
            shown.__dict__.pop(k, None)
    if not _mixing(config):
        for k in ("mixup_alpha", "cutmix_alpha", "mix_switch_prob"):
            shown.__dict__.pop(k, None)
    if not getattr(config, "ema_decay", 0.0) > 0:
        for k in ("ema_decay", "ema_warmup"):
            shown.__dict__.pop(k, None)
    for k in ("staged_dir", "resident"):
        if not getattr(config, k, None):
            shown.__dict__.pop(k, None)
    return str(shown)


def _eval_data_for(config, spec, device, rank: int, node_id: int, worker_id: int, dtype=torch.float32):
    """Held-out batches of ``--eval_batches``: a synthetic stream of its own (rewound before every evaluation,
    so each one sees the same batches), or this rank's share of the dataset's test split."""
    if _no_dataset(config):
        return D.SyntheticBatches(config.batch_size, spec.input_shape, spec.num_classes, device,
                                  dtype=dtype, seed=config.seed + 104729, rank=rank,
                                  channels_last=_channels_last(config, device))
    ds = D.load_dataset(spec.dataset, config.dataset_root, train=False, raw=_augmenting(config),
                        staged_dir=getattr(config, "staged_dir", None))
    if _resident(config):
        return D.ResidentEval.from_dataset(ds, node_id * config.node_dev + worker_id, config.total_dev,
                                           config.batch_size, device)
    return D.get_eval_loader(ds, node_id * config.node_dev + worker_id, config.total_dev, config.batch_size,
                             num_workers=2 if spec.dataset == "imagenet" else 0)


def evaluate(model: nn.Module, batches, device, precision: str = "fp32", max_batches: int = 0, topk: int = 5,
             transform: Optional[Callable] = None) -> dict:
    """Loss and top-1 / top-k accuracy of ``model`` over up to ``max_batches`` (0 = all) of ``batches``.

    The inner module runs in ``eval()`` mode under ``no_grad`` with the training loop's dtype and layout
    handling; each batch's ``[loss sum, valid rows, top-1, top-k]`` is added on the device, all-reduced once
    over the process group if there is one, and read once. Nothing of the training run moves: no parameter,
    BatchNorm running statistic or optimizer state is written, no global random stream is drawn from, and
    every module is put back in the mode it had (``train()`` in the training loop). ``transform`` (``--augment``):
    the batches are raw uint8 images; ``transform(batch on the device, index)`` makes the model input."""
    inner = getattr(model, "module", model)
    device = torch.device(device)
    prec = precision if device.type == "cuda" else "fp32"
    cl = device.type == "cuda" and prec != "fp32"
    autocast = torch.autocast("cuda", dtype=torch.bfloat16) if prec == "autocast" \
        else torch.autocast("cpu", enabled=False)
    if isinstance(batches, D.SyntheticBatches):
        batches.seek(0)
    it = iter(batches)
    if max_batches and max_batches > 0:
        it = itertools.islice(it, int(max_batches))
    total = torch.zeros(4, dtype=torch.float32, device=device)
    modes = [(m, m.training) for m in inner.modules()]
    inner.eval()
    try:
        with torch.no_grad():
            for i, (x, y) in enumerate(it):
                x = x.to(device, non_blocking=True)
                y = y.to(device, non_blocking=True)
                if transform is not None:
                    x = transform(x, i)  # already in the step's dtype and layout: what follows leaves it alone
                if prec == "bf16" and x.is_floating_point() and x.dtype != torch.bfloat16:
                    x = x.to(torch.bfloat16)
                if x.dim() == 4 and cl:
                    x = x.contiguous(memory_format=torch.channels_last)
                with autocast:
                    total += cross_entropy_with_metrics(inner(x), y, 0.0, topk)[1]
    finally:
        for m, mode in modes:
            m.training = mode
    if dist.is_initialized():
        dist.all_reduce(total, op=dist.ReduceOp.SUM)
    loss_sum, n, top1, topk_n = total.tolist()  # the one host read
    nan = float("nan")
    return {"loss": loss_sum / n if n else nan, "top1": top1 / n if n else nan, "topk": topk_n / n if n else nan,
            "samples": int(n), "k": int(topk)}


def save_checkpoint(path: str, model: nn.Module, optimizer, step: int, extra: Optional[dict] = None,
                    ema: Optional[ModelEMA] = None) -> None:
    """Rank-0 checkpoint: plain ``torch.save`` of state dicts (new functionality vs the reference). ``ema``: the
    buffer averages go under the key ``"ema"`` (the parameter averages are optimizer state); without it the
    checkpoint has the keys it always had."""
    if dist.is_initialized() and dist.get_rank() != 0:
        return
    inner = getattr(model, "module", model)
    rng = {"cpu": torch.get_rng_state()}
    if torch.cuda.is_available() and torch.cuda.is_initialized():
        rng["cuda"] = torch.cuda.get_rng_state()
    # the RNG state makes a resumed run draw the same dropout masks as an uninterrupted one
    state = {"model": inner.state_dict(), "optimizer": optimizer.state_dict(), "step": step, "extra": extra or {},
             "rng": rng}
    if ema is not None:
        state["ema"] = ema.state_dict()
    tmp = path + ".tmp"
    torch.save(state, tmp)
    os.replace(tmp, path)


def load_checkpoint(path: str, model: nn.Module, optimizer=None, map_location=None,
                    ema: Optional[ModelEMA] = None) -> int:
    """Load on every rank (``weights_only=True``: tensors and plain containers only). ``ema``: its buffer averages
    are loaded too; from a checkpoint without any, the average starts from the loaded weights."""
    state = torch.load(path, map_location=map_location or "cpu", weights_only=True)
    inner = getattr(model, "module", model)
    inner.load_state_dict(state["model"])
    if optimizer is not None and "optimizer" in state:
        optimizer.load_state_dict(state["optimizer"])
    if ema is not None:
        if "ema" in state:
            ema.load_state_dict(state["ema"])
        else:
            ema.reset_buffers()
            print_d(f"{path} holds no weight average: it starts from the loaded weights", Level.INFO)
    rng = state.get("rng") or {}
    if "cpu" in rng:
        torch.set_rng_state(rng["cpu"].cpu())
    if "cuda" in rng and torch.cuda.is_available():
        torch.cuda.set_rng_state(rng["cuda"].cpu())
    return int(state.get("step", 0))


def make_optimizer(config, params, master_weights: bool):
    """``--optimizer sgd`` (default): the reference's momentum SGD; ``lars``: the fused LARS; ``lamb`` / ``adamw``:
    the fused LAMB / AdamW (``--beta1``, ``--beta2``, ``--opt_eps``; ``--momentum`` is not theirs)."""
    ema = dict(ema_decay=config.ema_decay) if getattr(config, "ema_decay", 0.0) > 0 else {}
    kind = getattr(config, "optimizer", "sgd")
    if kind in ("lamb", "adamw"):
        return (FusedLAMB if kind == "lamb" else FusedAdamW)(
            params, lr=config.lr, betas=(getattr(config, "beta1", 0.9), getattr(config, "beta2", 0.999)),
            eps=getattr(config, "opt_eps", 1e-6), weight_decay=config.weight_decay,
            max_grad_norm=getattr(config, "max_grad_norm", 0.0), master_weights=master_weights, **ema)
    if getattr(config, "optimizer", "sgd") == "lars":
        return FusedLARS(params, lr=config.lr, momentum=config.momentum, weight_decay=config.weight_decay,
                         eta=getattr(config, "lars_eta", 1e-3), max_grad_norm=getattr(config, "max_grad_norm", 0.0),
                         master_weights=master_weights, **ema)
    return FusedSGD(params, lr=config.lr, momentum=config.momentum, weight_decay=config.weight_decay,
                    master_weights=master_weights, **ema)


def lr_schedule(config) -> Optional[Callable[[int], float]]:
    """batch number (from 0) -> learning rate for ``--warmup_steps`` / ``--total_steps``; None (the learning
    rate is never touched) without them. Batch ``b`` runs at the schedule's value for step ``b + 1``: the first
    batch of a warmup already updates (at ``lr / warmup_steps``) instead of spending a forward and backward pass
    on a zero learning rate, and batch ``warmup_steps - 1`` is the first at the full rate."""
    warmup, total = getattr(config, "warmup_steps", 0), getattr(config, "total_steps", 0)
    if warmup <= 0 and total <= 0:
        return None
    power = getattr(config, "lr_power", 2.0)
    return lambda batch: poly_warmup_lr(batch + 1, config.lr, warmup, total, power)


def set_lr(optimizer, lr: float) -> None:
    if hasattr(optimizer, "set_lr"):
        optimizer.set_lr(lr)  # FusedLARS / FusedLAMB / FusedAdamW: also the device scalar their kernels read
    else:
        for group in optimizer.param_groups:
            group["lr"] = lr


def worker_process(config, distribute_model: Callable, reducer, experiment_name: str,
                   node_id: Optional[int] = None, worker_id: Optional[int] = None) -> dict:
    rank = dist.get_rank() if dist.is_initialized() else 0
    node_id = rank // max(1, config.node_dev) if node_id is None else node_id
    worker_id = rank % max(1, config.node_dev) if worker_id is None else worker_id
    device = torch.device(f"cuda:{torch.cuda.current_device()}") if config.use_gpu else torch.device("cpu")
    print_d(f"Starting experiment {experiment_name} ({config.experiment}), {datetime.datetime.now()}", Level.INFO)
    prec = setup_compute_path(config, device)

    spec, model = _model_for(config, device)
    if prec == "bf16":
        dnn.bf16_weights(model)  # bf16 weights, fp32 masters in the optimizer (bench.py's path)
    model = distribute_model(model, reducer, config.grouping_size, device)
    params = list(getattr(model, "module", model).parameters())
    optimizer = make_optimizer(config, params, master_weights=prec == "bf16")
    schedule = lr_schedule(config)
    # --ema_decay: the averages of the weights (in the optimizer) and of the floating-point buffers
    ema = ModelEMA(model, optimizer, config.ema_decay, bool(getattr(config, "ema_warmup", 0))) \
        if getattr(config, "ema_decay", 0.0) > 0 else None
    start_step = 0
    if getattr(config, "resume", None):
        start_step = load_checkpoint(config.resume, model, optimizer, map_location=device, ema=ema)
        print_d(f"resumed from {config.resume} at step {start_step}", Level.INFO)

    os.makedirs(config.folder, exist_ok=True)
    if rank == 0:
        with open(f"{config.folder}/{experiment_name}_config.txt", "w") as f:
            f.write(_config_text(config))
    stem = f"{config.folder}/{experiment_name}_{node_id}_{worker_id}"
    sync_mode = int(config.sync_timers or 0)
    timers = Timers(sync=sync_mode == 1)
    batch_sync = sync_mode == 2 and device.type == "cuda"
    cl = _channels_last(config, device)
    ev = EventTimers() if device.type == "cuda" else None
    train_set = _data_for(config, spec, device, rank, node_id, worker_id,
                          dtype=torch.bfloat16 if prec == "bf16" else torch.float32)
    autocast = torch.autocast("cuda", dtype=torch.bfloat16) if prec == "autocast" \
        else torch.autocast("cpu", enabled=False)
    model.train()
    smoothing = float(getattr(config, "label_smoothing", 0.0))
    eval_batches, eval_every = int(getattr(config, "eval_batches", 0)), int(getattr(config, "eval_every", 0))
    eval_set = _eval_data_for(config, spec, device, rank, node_id, worker_id,
                              dtype=torch.bfloat16 if prec == "bf16" else torch.float32) if eval_batches > 0 else None
    evals, evals_ema = [], []
    train_aug = eval_aug = None
    if _augmenting(config):
        train_aug, eval_aug = _augmenters(config, spec, device, prec, node_id * config.node_dev + worker_id)
        if isinstance(train_set, D.SyntheticBatches):
            print_d(f"--augment {config.augment} ignored: synthetic input is generated in the model's form",
                    Level.WARNING)
            train_aug = None
        if isinstance(eval_set, D.SyntheticBatches):
            eval_aug = None
    if _resident(config):
        if isinstance(train_set, D.SyntheticBatches):
            print_d("--resident 1 ignored: synthetic input is generated on the device already", Level.WARNING)
        # a resident batch is an index list: the transforms read the store's rows in place
        if isinstance(train_set, D.ResidentBatches):
            train_aug = _indexed(train_aug, train_set.store)
        if isinstance(eval_set, D.ResidentEval):
            eval_aug = _indexed(eval_aug, eval_set.store)
    train_mix = None  # --mixup_alpha / --cutmix_alpha: per-batch partners, weights and boxes for train_aug and the loss
    if _mixing(config):
        if train_aug is None:
            print_d("--mixup_alpha / --cutmix_alpha ignored: the mixing lives in the augmentation kernel, which "
                    "synthetic input does not run", Level.WARNING)
        else:
            train_mix = aug.MixParams(tuple(spec.input_shape[1:]), config.mixup_alpha, config.cutmix_alpha,
                                      seed=config.seed, stream=node_id * config.node_dev + worker_id,
                                      switch_prob=getattr(config, "mix_switch_prob", 0.5))

    def run_eval(done: int) -> None:
        """One evaluation after ``done`` training batches: between two ``batch`` timer rows, never inside one."""
        t0 = time.time()
        r = evaluate(model, eval_set, device, prec, eval_batches, getattr(config, "topk", 5), eval_aug)
        r["batch"], r["seconds"] = done, time.time() - t0
        evals.append(r)
        with open(f"{stem}_eval.txt", "a") as f:
            f.write(f"Worker {node_id}:{worker_id} eval at batch {done}: loss {r['loss']} top1 {r['top1']} "
                    f"top{r['k']} {r['topk']} samples {r['samples']}\n")
        if ema is None:
            return
        t0 = time.time()
        with ema.applied():  # the same evaluation from the averaged weights; they are swapped back on exit
            r = evaluate(model, eval_set, device, prec, eval_batches, getattr(config, "topk", 5), eval_aug)
        r["batch"], r["seconds"] = done, time.time() - t0
        evals_ema.append(r)
        with open(f"{stem}_eval.txt", "a") as f:
            f.write(f"Worker {node_id}:{worker_id} eval_ema at batch {done}: loss {r['loss']} top1 {r['top1']} "
                    f"top{r['k']} {r['topk']} samples {r['samples']}\n")

    if eval_set is not None:
        open(f"{stem}_eval.txt", "w").close()  # this run's evaluations only

    losses = []
    # a resumed run continues the original sequence: batch numbering, and the data stream position
    batch_count = start_step
    end_batch = start_step + config.limit_batches
    epoch0, skip = 0, 0
    sampler = getattr(train_set, "epoch_sampler", None)
    if isinstance(train_set, D.SyntheticBatches):
        train_set.seek(start_step)
    elif sampler is not None:
        # resume inside the same per-epoch order without loading the skipped batches
        epoch0, skip = D.resume_position(start_step, len(train_set))
    t_start = time.time()
    for epoch in range(epoch0, config.epoch_count):
        if batch_count >= end_batch:
            break
        if sampler is not None:
            sampler.set_epoch(epoch, skip * config.batch_size if epoch == epoch0 else 0)
        gen = iter(train_set)
        while batch_count < end_batch:
            timers.start("batch")
            ev and ev.start("batch")
            timers.start("get_data")
            nx = next(gen, None)
            if nx is None:
                break
            x, y = nx
            timers.end("get_data")

            timers.start("data2dev")
            x = x.to(device, non_blocking=True)
            y = y.to(device, non_blocking=True)
            y_b = mix_lam = None
            if train_mix is not None:
                partner, lam, box, mix_lam, blend = train_mix.params(batch_count, x.shape[0])
                x = train_aug(x, batch_count, (partner, lam, box, blend))
                y_b = y.index_select(0, partner.to(device, non_blocking=True))
                mix_lam = mix_lam.to(device, non_blocking=True)
            elif train_aug is not None:
                x = train_aug(x, batch_count)  # uint8 in, the step's dtype and layout out: no cast, no re-layout
            else:
                if prec == "bf16" and x.is_floating_point() and x.dtype != torch.bfloat16:
                    x = x.to(torch.bfloat16)
                if x.dim() == 4 and cl:
                    x = x.contiguous(memory_format=torch.channels_last)
            timers.end("data2dev")

            timers.start("zero_grad")
            optimizer.zero_grad(set_to_none=True)
            timers.end("zero_grad")

            timers.start("forward")
            ev and ev.start("forward")
            with autocast:
                out = model(x)
                loss = cross_entropy(out, y, smoothing) if y_b is None \
                    else cross_entropy_mix(out, y, y_b, mix_lam, smoothing)
            ev and ev.end("forward")
            timers.end("forward")

            timers.start("backprop")
            ev and ev.start("backprop")
            loss.backward()
            ev and ev.end("backprop")
            timers.end("backprop")

            timers.start("sync")
            ev and ev.start("sync")
            model.sync_gradients()
            ev and ev.end("sync")
            timers.end("sync")

            timers.start("optimizer_step")
            ev and ev.start("optimizer_step")
            if schedule is not None:
                set_lr(optimizer, schedule(batch_count))
            if ema is not None:
                ema.step(batch_count)  # the global batch number: a resumed run continues the decay warmup
            else:
                optimizer.step()
            ev and ev.end("optimizer_step")
            timers.end("optimizer_step")

            losses.append(loss.detach().float())
            if sync_mode == 1:
                print_d(f"Worker {node_id}:{worker_id} loss for batch {batch_count}: {losses[-1].item()}", Level.DEBUG)
            elif batch_sync:
                torch.cuda.synchronize()  # the reference's per-batch loss print synchronised here (main.py:94-96)
            timers.end("batch")
            ev and ev.end("batch")
            extra = {"batch_count": batch_count, "data_len": x.size(0)}
            timers.end_experiment(experiment_name, extra)
            if ev:
                ev.end_experiment(experiment_name, extra)
            batch_count += 1
            if eval_set is not None and eval_every > 0 and batch_count % eval_every == 0:
                run_eval(batch_count)

    if device.type == "cuda":
        torch.cuda.synchronize()
    wall = time.time() - t_start - sum(r["seconds"] for r in evals + evals_ema)  # training time: evaluations taken out
    if eval_set is not None and (not evals or evals[-1]["batch"] != batch_count):
        run_eval(batch_count)  # --eval_every 0, or a last batch that is no multiple of it
    values = torch.stack(losses).cpu().tolist() if losses else []
    with open(f"{stem}_loss.txt", "w") as f:
        for i, v in enumerate(values):
            f.write(f"Worker {node_id}:{worker_id} loss for batch {start_step + i}: {v}\n")
    rows = timers.rows()
    timers.writeout(f"{stem}_times.csv")
    if ev:
        ev.writeout(f"{stem}_device_times.csv")
    if device.type == "cuda":
        from .ops import conv as nconv

        print_d(f"native conv dispatches ({experiment_name}): {dict(sorted(nconv.CALLS.items()))} "
                f"[precision {prec}, ops backend {dnn.get_backend()}, native conv {dnn.native_conv()}]", Level.INFO)
        nconv.CALLS.clear()
    if getattr(config, "checkpoint", None):
        save_checkpoint(config.checkpoint, model, optimizer, batch_count, ema=ema)
    model.cleanup()
    if hasattr(reducer, "cleanup"):
        reducer.cleanup()
    result = {"losses": values, "rows": rows, "wall_s": wall, "batches": batch_count - start_step,
              "start_step": start_step}
    if eval_set is not None:
        result["evals"] = evals
        if ema is not None:
            result["evals_ema"] = evals_ema
    return result
