"""Command-line configuration, compatible with the reference's positional CLI.

Reference (/root/reference/src/config.py:10-58): nine positionals ``size rank node_dev total_dev
master_addr ifname model_type dataset_root use_gpu`` (``size``/``rank`` may be ``envarg://VAR``)
and ``--job_id --experiment --limit_batches --backend --batch_size --random_input``; hard-coded
``epoch_count=100``, ``grouping_size=25 MiB``, ``lr=0.01``, ``momentum=0.5``, seed 1234.

Kept verbatim (same names, order, meaning), with the hard-coded values promoted to flags and the
MI355X options added (model override, dtype, all-reduce algorithm/channels, native engine,
kernel backend, timer mode). Positionals become optional when launched under ``torchrun`` (the
distributed environment supplies rank/size).
"""
from __future__ import annotations

import argparse
import os
from typing import List, Optional

from .utils.env import eval_arg

GROUPING_SIZE = 25 * 1024 * 1024
FUSION_TEST_SIZES_K = [256, 1024, 4 * 1024, 16 * 1024, 64 * 1024]  # reference main.py:287


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="MI355X distributed learning benchmark tool "
                                            "(reference-compatible CLI)")
    pos = [("size", "n", str, "number of nodes (or envarg://VAR)"),
           ("rank", "r", str, "rank (id) of this node (or envarg://VAR)"),
           ("node_dev", "d", int, "number of devices managed by this node"),
           ("total_dev", "D", int, "total number of devices"),
           ("master_addr", "a", str, "address of the master node"),
           ("ifname", "i", str, "network interface for Gloo (eg. lo, ib0, eth0)"),
           ("model_type", "M", str, "model: mnist | imagenet | resnet18 | resnet18_cifar | resnet50 | resnet152 ..."),
           ("dataset_root", "R", str, "root folder for the datasets"),
           ("use_gpu", "g", int, "whether to use the gpu (1) or just cpu (0)")]
    defaults = {"size": "envarg://WORLD_SIZE", "rank": "envarg://RANK", "node_dev": 1, "total_dev": None,
                "master_addr": "127.0.0.1", "ifname": "lo", "model_type": "mnist", "dataset_root": "../data",
                "use_gpu": None}
    for name, meta, typ, hlp in pos:
        p.add_argument(name, metavar=meta, type=typ, nargs="?", default=defaults[name], help=hlp)
    # reference optionals
    p.add_argument("--job_id", default="job", help="unique string used for the results folder name")
    p.add_argument("--experiment", default="main_ourdist", help="experiment function to run (see experiments.py)")
    p.add_argument("--limit_batches", type=int, default=3, help="number of batches to run")
    p.add_argument("--backend", default=None, help="torch.distributed backend (gloo | nccl); default by device")
    p.add_argument("--batch_size", type=int, default=128, help="per-worker batch size")
    p.add_argument("--random_input", type=int, default=0, help="1 = synthetic data (no dataset needed)")
    # promoted hard-coded values
    p.add_argument("--grouping_size", type=int, default=GROUPING_SIZE, help="fusion bucket size in bytes")
    p.add_argument("--epoch_count", type=int, default=100)
    p.add_argument("--lr", type=float, default=0.01)
    p.add_argument("--momentum", type=float, default=0.5)
    p.add_argument("--weight_decay", type=float, default=0.0)
    p.add_argument("--optimizer", default="sgd", choices=["sgd", "lars", "lamb", "adamw"],
                   help="sgd: fused momentum SGD (the reference's); lars: fused layer-wise adaptive rate scaling "
                        "for large global batches; lamb: fused LAMB (Adam moments, decoupled weight decay, "
                        "layer-wise trust ratio); adamw: fused AdamW")
    p.add_argument("--beta1", type=float, default=0.9, help="lamb / adamw: decay of the first moment, in [0, 1)")
    p.add_argument("--beta2", type=float, default=0.999, help="lamb / adamw: decay of the second moment, in [0, 1)")
    p.add_argument("--opt_eps", type=float, default=1e-6, help="lamb / adamw: epsilon added to sqrt(v), > 0")
    p.add_argument("--lars_eta", type=float, default=1e-3, help="LARS trust coefficient")
    p.add_argument("--max_grad_norm", type=float, default=0.0,
                   help="clip gradients by their global L2 norm (0 = off; --optimizer lars, lamb or adamw)")
    p.add_argument("--warmup_steps", type=int, default=0, help="linear learning-rate warmup from 0 over this many batches")
    p.add_argument("--total_steps", type=int, default=0,
                   help="polynomial learning-rate decay to 0 at this batch (0 = no decay)")
    p.add_argument("--lr_power", type=float, default=2.0, help="power of the polynomial decay")
    p.add_argument("--label_smoothing", type=float, default=0.0,
                   help="label smoothing of the training loss, in [0, 1) (0 = the plain fused cross-entropy)")
    p.add_argument("--eval_batches", type=int, default=0,
                   help="batches per evaluation on held-out data (0 = never evaluate)")
    p.add_argument("--eval_every", type=int, default=0,
                   help="evaluate after every this many batches (0 = once, after the last batch); needs --eval_batches")
    p.add_argument("--topk", type=int, default=5, help="k of the evaluation's top-k accuracy")
    p.add_argument("--augment", default="none", choices=["none", "standard"],
                   help="none: the loaders' fixed normalised tensors; standard: raw uint8 batches transformed on the "
                        "device -- random-resized crop 256 -> 224 + flip (ImageNet models), pad-4 random crop + flip "
                        "(CIFAR models), centre crop for evaluation")
    p.add_argument("--aug_scale_min", type=float, default=0.08,
                   help="smallest area fraction of the random-resized crop, in (0, 1]")
    p.add_argument("--mixup_alpha", type=float, default=0.0,
                   help="Mixup: blend every sample with a partner, weight ~ Beta(alpha, alpha) per batch (0 = off; "
                        "needs --augment standard, whose kernel does the mixing)")
    p.add_argument("--cutmix_alpha", type=float, default=0.0,
                   help="CutMix: paste a box of the partner, area fraction 1 - Beta(alpha, alpha) per batch (0 = off; "
                        "needs --augment standard)")
    p.add_argument("--mix_switch_prob", type=float, default=0.5,
                   help="with both alphas set: the probability that a batch uses CutMix, in [0, 1]")
    p.add_argument("--ema_decay", type=float, default=0.0,
                   help="exponential moving average of the weights, advanced inside the optimizer's update kernels, "
                        "in [0, 1) (0 = off); every evaluation then also reports the averaged model (eval_ema)")
    p.add_argument("--ema_warmup", type=int, default=0, choices=[0, 1],
                   help="1 = the decay of update t is min(ema_decay, (1 + t) / (10 + t))")
    p.add_argument("--staged_dir", default=None,
                   help="ImageNet models: read the uint8 256x256 staging images from the files that "
                        "`python -m distributed_learning_amd.stage` wrote here instead of decoding the JPEG tree "
                        "(needs --augment standard, which takes the raw uint8 form)")
    p.add_argument("--resident", type=int, default=0, choices=[0, 1],
                   help="1 = hold the rank's data shard in device memory for the whole run and let the augmentation "
                        "kernel read each batch in place by index: no decode, collate or image copy per step (needs "
                        "--augment standard); a shard that does not fit beside the step is an error")
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--master_port", type=int, default=29501)
    # MI355X options
    p.add_argument("--model", default=None, help="model override (same names as model_type)")
    p.add_argument("--dtype", default=None, choices=["fp32", "bf16"],
                   help="compute dtype (bf16 on GPU by default, fp32 on CPU); fp32 = the reference's precision")
    p.add_argument("--precision", default=None, choices=["bf16", "autocast", "fp32"],
                   help="bf16: bf16 weights + fp32 master weights in the fused SGD, native kernels (GPU default; "
                        "the bench.py path); autocast: fp32 params under bf16 autocast; fp32: no reduced precision "
                        "(MIOpen / torch kernels, the reference's numerics)")
    p.add_argument("--conv", default="native", choices=["native", "miopen"],
                   help="convolutions / FC heads on the native MFMA kernels (bf16) or MIOpen")
    p.add_argument("--algorithm", default="ring", help="all-reduce algorithm: ring|builtin|central|direct|rsag")
    p.add_argument("--channels", type=int, default=0, help="ring channels (0 = one per xGMI peer)")
    p.add_argument("--native", type=int, default=None, help="1 = C++ RCCL engine (GPU default), 0 = torch.distributed")
    p.add_argument("--kernels", default=None, choices=["native", "torch"], help="model hot-path kernel backend")
    p.add_argument("--comm_dtype", default=None, choices=["fp32", "bf16"], help="gradient wire dtype")
    p.add_argument("--local_size", type=int, default=None, help="devices per (virtual) node for 2-step reducers")
    p.add_argument("--sync_timers", type=int, default=None,
                   help="0 = host timers only; 1 = synchronise the device at every timer; 2 = synchronise once at "
                        "the end of each batch, as the reference's per-batch loss print (.item()) did (GPU default)")
    p.add_argument("--hier_algorithm", default=None,
                   help="native engine algorithm of the 2-step runners (default hier_ring; hier_central for the "
                        "central runner; hier_coll = RCCL collectives on ncclCommSplit sub-communicators)")
    p.add_argument("--find_unused", type=int, default=None, help="graph walk for unused params each forward")
    p.add_argument("--results_root", default="results")
    p.add_argument("--checkpoint", default=None, help="path to save a checkpoint at the end of a run")
    p.add_argument("--resume", default=None, help="checkpoint to resume from")
    p.add_argument("--spawn", type=int, default=None,
                   help="1 = this process spawns node_dev local workers (reference launch style)")
    return p


def parse_args(argv: Optional[List[str]] = None):
    parser = build_parser()
    config = parser.parse_args(argv)
    if config.max_grad_norm < 0:
        parser.error("--max_grad_norm must be >= 0")
    if config.max_grad_norm > 0 and config.optimizer == "sgd":
        parser.error("--max_grad_norm needs --optimizer lars, lamb or adamw (the fused SGD does not clip)")
    if not (0.0 <= config.beta1 < 1.0 and 0.0 <= config.beta2 < 1.0):
        parser.error("--beta1 and --beta2 must be in [0, 1)")
    if not config.opt_eps > 0:
        parser.error("--opt_eps must be > 0")
    if config.warmup_steps < 0 or config.total_steps < 0:
        parser.error("--warmup_steps and --total_steps must be >= 0")
    if not 0.0 <= config.label_smoothing < 1.0:
        parser.error("--label_smoothing must be in [0, 1)")
    if config.eval_batches < 0 or config.eval_every < 0:
        parser.error("--eval_batches and --eval_every must be >= 0")
    if config.topk < 1:
        parser.error("--topk must be >= 1")
    if not 0.0 < config.aug_scale_min <= 1.0:
        parser.error("--aug_scale_min must be in (0, 1]")
    if not (config.mixup_alpha >= 0 and config.cutmix_alpha >= 0):
        parser.error("--mixup_alpha and --cutmix_alpha must be >= 0")
    if not 0.0 <= config.mix_switch_prob <= 1.0:
        parser.error("--mix_switch_prob must be in [0, 1]")
    if not 0.0 <= config.ema_decay < 1.0:
        parser.error("--ema_decay must be in [0, 1)")
    if (config.mixup_alpha > 0 or config.cutmix_alpha > 0) and config.augment == "none":
        parser.error("--mixup_alpha / --cutmix_alpha need --augment standard: the mixing lives in that kernel")
    if config.resident and config.augment == "none":
        parser.error("--resident 1 needs --augment standard: the resident store is read by that kernel")
    if config.staged_dir and config.augment == "none":
        parser.error("--staged_dir needs --augment standard: the staged files hold the raw uint8 form")
    if config.staged_dir:
        from .models import MODELS

        spec = MODELS.get(config.model or config.model_type)
        if spec is not None and spec.dataset != "imagenet":
            parser.error(f"--staged_dir needs an ImageNet model: {spec.dataset} has no staged form")
    if config.augment != "none":
        from .models import MODELS

        spec = MODELS.get(config.model or config.model_type)
        if spec is not None and spec.dataset == "mnist":
            parser.error(f"--augment {config.augment} needs a CIFAR-10 or ImageNet model: MNIST has no raw "
                         f"3-channel form for the device-side transform")
    return finalize(config)


def finalize(config):
    def _int_or(v, default):
        try:
            return int(eval_arg(v))
        except (KeyError, ValueError, TypeError):
            return default

    config.size = _int_or(config.size, 1)
    config.rank = _int_or(config.rank, 0)
    if config.total_dev is None:
        config.total_dev = config.size * config.node_dev
    if config.use_gpu is None:
        import torch

        config.use_gpu = 1 if torch.cuda.is_available() else 0
    model = config.model or config.model_type
    config.model_name = model
    config.epoch_count = int(config.epoch_count)
    if config.dtype is None:
        config.dtype = "fp32" if (not config.use_gpu or config.precision == "fp32") else "bf16"
    if config.precision is None:
        config.precision = "bf16" if config.dtype == "bf16" else "fp32"
    if not config.use_gpu:
        config.precision = "fp32"
    if config.sync_timers is None:
        config.sync_timers = 2 if config.use_gpu else 0
    if config.native is None:
        config.native = 1 if config.use_gpu else 0
    if config.kernels is None:
        config.kernels = "native" if config.use_gpu else "torch"
    if config.backend is None:
        config.backend = "nccl" if config.use_gpu else "gloo"
    if config.find_unused is None:
        config.find_unused = 1 if model in ("imagenet", "googlenet") else 0
    config.devices = [f"cuda:{i}" for i in range(config.node_dev)] if config.use_gpu else ["cpu"] * config.node_dev
    return config
