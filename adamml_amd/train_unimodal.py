"""Restated `train_unimodal` launcher on the HIP backbones: the first step of the reference workflow (README "Training Unimodal
Models"), one network per modality, whose checkpoints `--unimodality_pretrained` of adamml_amd.train reads.

train_unimodal.py:64-404 and the step loops of utils/utils.py:187-317 with the parser, meters, schedules, checkpoint writer and
rank resolution of adamml_amd.train: `build_model` for `--backbone_net resnet | sound_mobilenet_v2`, HipDDP (+ SyncBatchNorm)
around it, one FlatSGD over the backbone's flat buffer, and the reference's checkpoint dictionary (`epoch, arch, state_dict,
best_top1, optimizer, scheduler`; `module.`-prefixed names, torch.optim.SGD's optimizer layout).

The data pipeline is a loader factory as in adamml_amd.train; with --datadir and no factory named it is
`adamml_amd.data:unimodal_loaders`, so the README command lines run as they stand:

    python3 train_unimodal.py --multiprocessing-distributed --backbone_net resnet -d 50 --groups 8 --frames_per_group 4 -b 72 \\
        -j 96 --epochs 60 --modality rgb --datadir /PATH/TO/RGB_DATA --dataset kinetics-sounds --logdir LOGDIR --dense_sampling \\
        --wd 0.0001 --augmentor_ver v2 --lr_scheduler multisteps --lr_steps 20 40 50

A batch is `(input, target)` with ONE input object, not a list: an fp32 tensor in the reference's layout, or what the loader hands
over for the GPU to decode (video.EncodedFrames / video.Frames / audio.Waveforms).  `--synthetic N` runs N synthetic batches per epoch.
"""
import argparse
import os
import shutil
import sys
import time

import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import prefetch, train
from .distributed import HipDDP
from .model_builder import build_model
from .optim import FlatSGD
from .train import (CHANNELS, DATASET_NUM_CLASSES, LRSchedule, Meter, _load_factory, accuracy, arg_parser, enable_launch_plans, init_rank,
                    launch, load_reference_checkpoint, reference_state_dict, save_checkpoint)

DEFAULT_FACTORY = "adamml_amd.data:unimodal_loaders"


def resolve_args(args):
    """The bookkeeping train_unimodal.py:68-94 does on the parsed namespace before building the model."""
    if args.backbone_net == "adamml":
        raise SystemExit("adamml_amd.train_unimodal trains ONE backbone (--backbone_net resnet | sound_mobilenet_v2); "
                         "--backbone_net adamml is adamml_amd.train: python3 train_adamml.py ...")
    if getattr(args, "online", False) or getattr(args, "online_stagger", 0):
        raise SystemExit("--online / --online_stagger step AdaMML's policy one segment at a time; a single backbone has no policy: "
                         "python3 train_adamml.py -e --online ...")
    if args.threed_data:
        raise SystemExit("--threed_data: the registry holds 2-D backbones only (resnet, sound_mobilenet_v2), and their forward takes "
                         "[N, T*C, H, W], not [N, C, T, H, W]")
    if args.num_clips != 1:
        raise SystemExit("--num_clips %d: the 2-D forward views its input as (N * groups, C, H, W) (models/resnet.py:198), which a "
                         "batch of num_clips * groups frames per video does not fit; unimodal training and validation use one clip"
                         % args.num_clips)
    if not isinstance(args.modality, str):
        args.modality = args.modality[0]                                     # train_unimodal.py:68-69
    if args.datadir is not None and not isinstance(args.datadir, str):
        args.datadir = args.datadir[0]
    if args.modality not in CHANNELS:
        raise SystemExit("--modality: invalid choice %r (choose from %s)" % (args.modality, ", ".join(CHANNELS)))
    if args.num_classes is None:
        if args.dataset not in DATASET_NUM_CLASSES:
            raise SystemExit("unknown --dataset %r (known: %s): pass --num_classes" % (args.dataset, ", ".join(DATASET_NUM_CLASSES)))
        args.num_classes = DATASET_NUM_CLASSES[args.dataset]                 # train_unimodal.py:71-72
    args.input_channels = CHANNELS[args.modality]                            # train_unimodal.py:87-94
    # the factories' ImageNet initialisation reads local files only (imagenet_init.py), as in adamml_amd.train.resolve_args
    from . import imagenet_init
    imagenet_init.configure_from_args(getattr(args, "imagenet_weights", None))
    arch = "resnet%d" % args.depth if args.backbone_net == "resnet" else "mobilenet_v2"
    args.imagenet_pretrained = bool(imagenet_init.path_for(arch))
    return args


def mean_std(model, args):
    """train_unimodal.py:97-117: the model's values for the modality unless --mean / --std override them."""
    mean, std = model.mean(args.modality), model.std(args.modality)
    for name, given in (("mean", args.mean), ("std", args.std)):
        if given is None:
            continue
        if args.modality in ("rgb", "rgbdiff") and len(given) != 3:
            raise ValueError("When training with rgb, dim of %s must be three." % name)
        if args.modality == "flow" and len(given) != 1:
            raise ValueError("When training with flow, dim of %s must be three." % name)       # (the reference's wording)
        if name == "mean":
            mean = list(given)
        else:
            std = list(given)
    return mean, std


class SyntheticLoader(train.SyntheticLoader):
    """train.SyntheticLoader's batches for the one modality and one segment: (tensor, target), not (list, target)."""

    def __init__(self, args, n, batch, device, rank):
        super().__init__(argparse.Namespace(**dict(vars(args), modality=[args.modality])), n, batch, device, rank, segments=1)

    def __iter__(self):
        for xs, y in super().__iter__():
            yield xs[0], y


def _reduced_precisions(output, target):
    """prec@1 / prec@5 averaged over the ranks: the reference's two all-reduces (utils/utils.py:228-233) as one packed pair."""
    prec = torch.stack(accuracy(output, target))
    if dist.is_initialized():
        dist.all_reduce(prec)
        prec /= dist.get_world_size()
    return prec


# ------------------------------------------------------------------------------------------------ one epoch
def train_epoch(loader, ddp, opt, epoch, args, rank=0, log=print):
    """utils/utils.py:187-265.  Returns the meters; meters['losses'] lists the local loss of every step."""
    model = ddp.module
    model.train()
    opt.zero_grad()
    device = next(model.parameters()).device
    meters = {k: Meter() for k in ("loss", "top1", "top5", "time", "data")}
    meters["losses"] = []
    late = prefetch.late(loader)
    end = time.time()
    for i, (images, target) in enumerate(loader):
        meters["data"].update(time.time() - end)
        images = images.to(device, non_blocking=True)
        target = target.to(device, non_blocking=True)
        output = ddp(images)
        loss = F.cross_entropy(output, target)
        prec = _reduced_precisions(output.detach(), target)
        loss.backward()
        ddp.reduce_gradients()
        if args.clip_gradient is not None:
            bufs = model.flat_grad_buffers()
            total = torch.sqrt(sum((b.float() ** 2).sum() for b in bufs))
            scale = (args.clip_gradient / (total + 1e-6)).clamp(max=1.0)
            for b in bufs:
                b.mul_(scale)
        opt.step()
        opt.zero_grad()
        local_loss, prec1, prec5 = torch.cat([loss.detach().reshape(1), prec]).tolist()      # one read-back per step
        meters["losses"].append(local_loss)
        meters["loss"].update(local_loss, target.size(0))
        meters["top1"].update(prec1, target.size(0))
        meters["top5"].update(prec5, target.size(0))
        meters["time"].update(time.time() - end)
        end = time.time()
        if i % args.print_freq == 0 and rank == 0:
            log("Epoch: [{}][{}/{}]\tTime {:.3f}\tData {:.3f}\tLoss {:.4f}\tPrec@1 {:.3f}\tPrec@5 {:.3f}".format(
                epoch, i, len(loader), meters["time"].avg, meters["data"].avg, meters["loss"].avg, meters["top1"].avg, meters["top5"].avg))
    line = prefetch.late_line(loader, late, epoch)
    if line and rank == 0:
        log(line)
    return meters


@torch.no_grad()
def validate(loader, ddp):
    """utils/utils.py:268-317: per-batch loss and rank-averaged precisions, weighted by the batch size."""
    model = ddp.module
    model.eval()
    device = next(model.parameters()).device
    meters = {k: Meter() for k in ("loss", "top1", "top5", "time")}
    end = time.time()
    for images, target in loader:
        images = images.to(device, non_blocking=True)
        target = target.to(device, non_blocking=True)
        output = model(images)
        loss = F.cross_entropy(output, target)
        local_loss, prec1, prec5 = torch.cat([loss.reshape(1), _reduced_precisions(output, target)]).tolist()
        meters["loss"].update(local_loss, target.size(0))
        meters["top1"].update(prec1, target.size(0))
        meters["top5"].update(prec5, target.size(0))
        meters["time"].update(time.time() - end)
        end = time.time()
    return meters["top1"].avg, meters["top5"].avg, meters["loss"].avg, meters["time"].avg


def eval_this_epoch(epoch, epochs, lazy_eval):
    """train_unimodal.py:341-346 (epoch counts from 0)."""
    return not lazy_eval or (epoch + 1) % 10 == 0 or (epoch + 1) >= epochs * 0.9


# ------------------------------------------------------------------------------------------------ launcher
def main(argv=None, train_loader=None, val_loader=None, log=print):
    """train_unimodal.py:33-61: the parser and rank placement of adamml_amd.train, `main_worker` below in every rank."""
    args = resolve_args(arg_parser().parse_args(argv))                       # a rejected flag starts no process and needs no GPU
    return launch(args, main_worker, _spawned_worker, train_loader, val_loader, log, "adamml_amd.train_unimodal")


def _spawned_worker(gpu, ngpus_per_node, args):
    main_worker(gpu, ngpus_per_node, args, None, None, print)


def main_worker(gpu, ngpus_per_node, args, train_loader=None, val_loader=None, log=print):
    """train_unimodal.py:64-404 for one rank."""
    resolve_args(args)                                                       # (again in a spawned rank: the ImageNet file table is per process)
    device, rank, world = init_rank(gpu, ngpus_per_node, args)
    per_rank_batch = max(1, int(args.batch_size / world))                    # train_unimodal.py:152
    enable_launch_plans(per_rank_batch)

    model, arch_name = build_model(args)
    mean, std = mean_std(model, args)
    # what the bare backbones need to take the loader's objects (ResNet._forward_frames, sound MobileNetV2.forward)
    model.input_modality, model.input_mean, model.input_std, model.resampling_rate = args.modality, mean, std, args.resampling_rate
    model = model.to(device)
    params = sum(p.numel() for p in model.parameters())
    if args.show_model and rank == 0:                                        # train_unimodal.py:136-139
        log(str(model))
        log("Params: {}".format(params))
        return 0
    if args.pretrained is not None:
        # train_unimodal.py:174-196, the `else` arm (args.transfer is not a flag of opts.py): strict=False, `module.` prefix stripped
        if rank == 0:
            log("=> using pre-trained model '{}'".format(arch_name))
        load_reference_checkpoint(model, args.pretrained, strict=False)
    elif rank == 0:
        log("=> creating model '{}'".format(arch_name))
    ddp = HipDDP(model, sync_bn=(args.sync_bn and world > 1))
    log_folder = os.path.join(args.logdir, arch_name)
    if rank == 0:
        os.makedirs(log_folder, exist_ok=True)

    if (train_loader is None and not args.evaluate) or val_loader is None:   # a loader the caller supplied stays
        factory = args.loader_factory or (DEFAULT_FACTORY if args.datadir and not args.synthetic else None)
        if factory:
            made = _load_factory(factory)(args, rank, world, device)
        elif args.synthetic:
            made = (SyntheticLoader(args, args.synthetic, per_rank_batch, device, rank),
                    SyntheticLoader(args, max(1, args.synthetic // 4), per_rank_batch, device, rank + 7777))
        else:
            raise SystemExit("no dataset was named: pass --datadir DIR (the reference's dataset layout, read by %s), --loader_factory "
                             "MODULE:FUNCTION, train_loader / val_loader to main(), or --synthetic N" % DEFAULT_FACTORY)
        train_loader = made[0] if train_loader is None else train_loader
        val_loader = made[1] if val_loader is None else val_loader
    # --prefetch N: whatever loaders these are, their batches are prepared N ahead on a stream of their own
    train_loader, val_loader = prefetch.wrap(train_loader, args, device), prefetch.wrap(val_loader, args, device)

    if args.evaluate:                                                        # train_unimodal.py:228-241
        top1, top5, loss, speed = validate(val_loader, ddp)
        if rank == 0:
            line = "Val@{}: \tLoss: {:4.4f}\tTop@1: {:.4f}\tTop@5: {:.4f}\tSpeed: {:.2f} ms/batch\tParams: {}".format(
                args.input_size, loss, top1, top5, speed * 1000.0, params)
            log(line)
            with open(os.path.join(log_folder, "evaluate_log.log"), "a") as f:
                print(args.pretrained, file=f)
                print(line, file=f)
        return {"top1": top1, "top5": top5, "loss": loss}

    model.flat_owner.ensure(device)                                          # the flat buffer exists before the optimizer looks at it
    opt = FlatSGD(model.flat_owner, args.lr, args.momentum, args.weight_decay, args.nesterov)      # train_unimodal.py:258-262
    sched = LRSchedule(opt, args.lr_scheduler, args.lr, args.epochs, args.lr_steps)
    best_top1 = 0.0
    if args.auto_resume and os.path.exists(os.path.join(log_folder, "checkpoint.pth.tar")):
        args.resume = os.path.join(log_folder, "checkpoint.pth.tar")
        if rank == 0:
            log("Found the checkpoint in the log folder, will resume from there.")
    logfile = None
    if args.resume:                                                          # train_unimodal.py:281-310
        if not os.path.isfile(args.resume):
            raise ValueError("Checkpoint is not found: {}".format(args.resume))
        if rank == 0:
            log("=> loading checkpoint '{}'".format(args.resume))
            logfile = open(os.path.join(log_folder, "log.log"), "a")
        ck = load_reference_checkpoint(model, args.resume)
        args.start_epoch, best_top1 = ck["epoch"], float(ck["best_top1"])    # (a float, or the tensor older runs stored)
        if isinstance(ck.get("optimizer"), dict) and "param_groups" in ck["optimizer"]:
            opt.load_state_dict(ck["optimizer"])
        try:
            sched.load_state_dict(ck["scheduler"])
        except Exception:                                                    # the reference tolerates a checkpoint without one (:300-303)
            pass
        if rank == 0:
            log("=> loaded checkpoint '{}' (epoch {})".format(args.resume, ck["epoch"]))
    elif rank == 0:
        old = os.path.join(log_folder, "log.log")
        if os.path.exists(old):
            shutil.copyfile(old, old + ".{}".format(int(time.time())))
        logfile = open(old, "w")
    # torch's DistributedDataParallel broadcasts rank 0's parameters and buffers at construction (train_unimodal.py:159)
    ddp.broadcast_parameters()

    def both(line):
        log(line)
        print(line, file=logfile, flush=True)

    if rank == 0:
        print(" ".join(sys.argv), file=logfile, flush=True)
        print(args, file=logfile, flush=True)
        both("Params: {}".format(params))
    history = []
    try:
        for epoch in range(args.start_epoch, args.epochs):                   # train_unimodal.py:331-401
            m = train_epoch(train_loader, ddp, opt, epoch + 1, args, rank, log)
            history.append((epoch + 1, m["losses"]))
            if dist.is_initialized():
                dist.barrier()
            evaluated = eval_this_epoch(epoch, args.epochs, args.lazy_eval)
            top1, top5, vloss, vspeed = validate(val_loader, ddp) if evaluated else (0.0, 0.0, 0.0, 0.0)
            sched.step(epoch + 1, vloss)                                     # plateau: the validation loss; else the epoch (:355-359)
            if rank == 0:
                both("Train: [{:03d}/{:03d}]\tLoss: {:4.4f}\tTop@1: {:.4f}\tTop@5: {:.4f}\tSpeed: {:.2f} ms/batch\tData loading: {:.2f} ms/batch"
                     .format(epoch + 1, args.epochs, m["loss"].avg, m["top1"].avg, m["top5"].avg, m["time"].avg * 1000.0, m["data"].avg * 1000.0))
                if evaluated:
                    both("Val  : [{:03d}/{:03d}]\tLoss: {:4.4f}\tTop@1: {:.4f}\tTop@5: {:.4f}\tSpeed: {:.2f} ms/batch".format(
                        epoch + 1, args.epochs, vloss, top1, top5, vspeed * 1000.0))
                is_best = top1 > best_top1
                best_top1 = max(top1, best_top1)
                save_checkpoint({"epoch": epoch + 1, "arch": arch_name, "state_dict": reference_state_dict(model), "best_top1": best_top1,
                                 "optimizer": opt.state_dict(), "scheduler": sched.state_dict()}, is_best, log_folder)
            if dist.is_initialized():
                dist.barrier()
    finally:
        if logfile is not None:
            logfile.close()
    return {"history": history, "best_top1": best_top1, "log_folder": log_folder, "last_val": (top1, top5, vloss) if history else None,
            "model": model, "ddp_stats": dict(ddp.stats)}


if __name__ == "__main__":
    main()
