#!/usr/bin/env python3
"""Generate tests/golden/unimodal_contract.json and tests/golden/readme_train_unimodal_commands.txt from the REAL reference
(IBM/AdaMML, a checkout at $ADAMML_REF) on the CPU.

Only this script imports the reference, and nothing of its text is copied: the fixture holds what its parser, `build_model`,
torch.optim.SGD and torch's schedulers RETURN for the three `train_unimodal.py` recipes of its README (rgb ResNet-50, flow ResNet-50,
sound_mobilenet_v2; imagenet_pretrained=False, the machine has no network).  train_unimodal.py itself cannot be imported here (it needs
torchsummary), so the few namespace assignments of its main_worker (:68-94) and its two epoch-loop rules (:341-346, :355-359) are driven
from this script around the reference's own objects.

Usage:  ADAMML_REF=/path/to/AdaMML python tools/gen_golden_unimodal.py
"""
import json
import os
import re
import shlex
import sys
import types
import warnings

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("ADAMML_REF")
if not REF or not os.path.isfile(os.path.join(REF, "train_unimodal.py")):
    raise SystemExit("set ADAMML_REF to a checkout of the reference (IBM/AdaMML)")
sys.path.insert(0, REF)

import torch  # noqa: E402
from torch.optim import lr_scheduler  # noqa: E402

# shim: torchvision is absent but utils/utils.py imports it (as in tools/gen_golden.py)
tv, tvt = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
tvt.Compose = lambda ts: None
tvt.CenterCrop = tvt.Resize = lambda *a, **k: None
tv.transforms = tvt
sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt})

from models import build_model  # noqa: E402  (the reference package)
from opts import arg_parser  # noqa: E402
from utils.dataset_config import get_dataset_config  # noqa: E402

CHANNELS = {"rgb": 3, "flow": 10, "rgbdiff": 15, "sound": 1}
GOLDEN = os.path.join(ROOT, "tests", "golden")
EPOCHS = 60


def readme_commands():
    """The `python3 train_unimodal.py ...` command lines of the reference's README, line continuations joined."""
    text = open(os.path.join(REF, "README.md")).read().replace("\\\n", " ")
    return [re.sub(r"\s+", " ", l).strip() for l in text.splitlines() if l.startswith("python3 train_unimodal.py")]


def resolved(line):
    argv = shlex.split(line)[2:]
    argv[argv.index("--dataset") + 1] = "kinetics-sounds"                  # README placeholder DATASET
    args = arg_parser().parse_args(argv)
    args.datadir, args.modality = args.datadir[0], args.modality[0]
    args.num_classes = get_dataset_config(args.dataset)[0]
    args.input_channels = CHANNELS[args.modality]
    args.imagenet_pretrained = False
    return args


def scheduler_for(kind, opt, args):
    if kind == "step":
        return lr_scheduler.StepLR(opt, args.lr_steps[0], gamma=0.1)
    if kind == "multisteps":
        return lr_scheduler.MultiStepLR(opt, args.lr_steps, gamma=0.1)
    if kind == "cosine":
        return lr_scheduler.CosineAnnealingLR(opt, args.epochs, eta_min=0)
    return lr_scheduler.ReduceLROnPlateau(opt, "min")


def recipe(line):
    args = resolved(line)
    torch.manual_seed(0)
    model, arch_train = build_model(args)
    arch_test = build_model(args, test_mode=True)[1]
    out = {"command": line, "modality": args.modality, "datadir": args.datadir, "input_channels": args.input_channels,
           "backbone_net": args.backbone_net, "num_classes": args.num_classes, "arch_name": arch_train, "arch_name_test": arch_test}
    sd = torch.nn.DataParallel(model).state_dict()
    out["state_dict"] = [[k, list(v.shape), str(v.dtype)] for k, v in sd.items()]
    # one SGD step on a tiny input (two videos: the BatchNorms of the last stage see more than one value per channel)
    opt = torch.optim.SGD(model.parameters(), args.lr, momentum=args.momentum, weight_decay=args.weight_decay, nesterov=args.nesterov)
    frames = 1 if args.modality == "sound" else args.groups
    x = torch.randn(2, args.input_channels * frames, 64, 64)
    model.train()
    torch.nn.functional.cross_entropy(model(x), torch.tensor([1, 2])).backward()
    opt.step()
    osd = opt.state_dict()
    groups = [{k: (len(v) if k == "params" else v) for k, v in g.items()} for g in osd["param_groups"]]
    out["optimizer"] = {"keys": sorted(osd.keys()), "param_groups": groups, "num_params": len(osd["param_groups"][0]["params"]),
                        "state_keys": sorted({k for e in osd["state"].values() for k in e}),
                        "momentum_buffer_shapes": [list(osd["state"][i]["momentum_buffer"].shape) for i in sorted(osd["state"])]}
    return out, args, opt


def main():
    os.makedirs(GOLDEN, exist_ok=True)
    lines = readme_commands()
    assert len(lines) == 3, lines
    with open(os.path.join(GOLDEN, "readme_train_unimodal_commands.txt"), "w") as f:
        f.write("# The `python3 train_unimodal.py ...` command lines of the reference's README.md (\"Training Unimodal Models\": rgb, flow,\n"
                "# audio), line continuations joined -- written by tools/gen_golden_unimodal.py; DATA for tests/test_unimodal_cpu.py.\n")
        f.write("\n".join(lines) + "\n")
    doc = {"recipes": []}
    for line in lines:
        rec, args, opt = recipe(line)
        doc["recipes"].append(rec)
    # scheduler state_dict keys of the four kinds (train_unimodal.py:264-271), on the last recipe's optimizer
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        doc["scheduler_keys"] = {k: sorted(scheduler_for(k, opt, args).state_dict().keys()) for k in ("step", "multisteps", "cosine", "plateau")}
        # the learning rate every epoch trains with: `scheduler.step(epoch + 1)` after each epoch (train_unimodal.py:355-359)
        opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], args.lr, momentum=args.momentum)
        sched = scheduler_for("multisteps", opt, args)
        lrs = []
        for epoch in range(EPOCHS):
            lrs.append(opt.param_groups[0]["lr"])
            sched.step(epoch + 1)
    doc["multisteps"] = {"base_lr": args.lr, "lr_steps": args.lr_steps, "epochs": EPOCHS, "lr_per_epoch": lrs}
    # the epochs --lazy_eval validates (train_unimodal.py:341-346; 1-based, as the log lines count them)
    doc["lazy_eval_epochs"] = [e + 1 for e in range(EPOCHS) if (e + 1) % 10 == 0 or (e + 1) >= EPOCHS * 0.9]
    with open(os.path.join(GOLDEN, "unimodal_contract.json"), "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", os.path.getsize(os.path.join(GOLDEN, "unimodal_contract.json")), "bytes")


if __name__ == "__main__":
    main()
