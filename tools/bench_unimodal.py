"""Host cost of the unimodal launcher's loop at the README's size: ms per step of train_unimodal.train_epoch (meters, accuracy, one
loss read-back per step) beside the hand-driven forward + F.cross_entropy + backward + FlatSGD.step + zero_grad of the same model in
the same process, synchronised once per window.  The two alternate; medians over the windows are printed, one JSON line per network.

    python tools/bench_unimodal.py [--batch 72] [--steps 12] [--rounds 3] [rgb flow sound]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adamml_amd import synth, train, train_unimodal as TU  # noqa: E402
from adamml_amd.distributed import HipDDP  # noqa: E402
from adamml_amd.model_builder import build_model  # noqa: E402
from adamml_amd.optim import FlatSGD  # noqa: E402

RECIPE = {"rgb": ["--backbone_net", "resnet", "-d", "50", "--groups", "8", "--modality", "rgb"],
          "flow": ["--backbone_net", "resnet", "-d", "50", "--groups", "8", "--modality", "flow"],
          "sound": ["--backbone_net", "sound_mobilenet_v2", "--modality", "sound"]}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("kinds", nargs="*", default=["rgb", "flow", "sound"])
    p.add_argument("--batch", type=int, default=72)
    p.add_argument("--steps", type=int, default=12)
    p.add_argument("--rounds", type=int, default=3)
    o = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_unimodal.py needs an MI355X")
    dev = torch.device("cuda", 0)
    for kind in o.kinds:
        args = TU.resolve_args(train.arg_parser().parse_args(RECIPE[kind] + ["-b", str(o.batch), "--print-freq", "1000000"]))
        model, _ = build_model(args)
        model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=1234))
        model.to(dev).train()
        model.flat_owner.ensure(dev)
        opt = FlatSGD(model.flat_owner, 1e-4, args.momentum, args.weight_decay)
        ddp = HipDDP(model)
        shape = (o.batch, 1, 256, 256) if kind == "sound" else (o.batch, args.groups * args.input_channels, 224, 224)
        data = [(torch.randn(shape, device=dev), torch.randint(0, args.num_classes, (o.batch,), device=dev)) for _ in range(2)]
        batches = [data[i % 2] for i in range(o.steps)]

        def loop():
            TU.train_epoch(batches, ddp, opt, 1, args, 0, lambda *_: None)

        def by_hand():
            for x, y in batches:
                F.cross_entropy(model(x), y).backward()
                opt.step()
                opt.zero_grad()

        def window(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / o.steps * 1e3

        window(loop), window(by_hand)                      # warm-up of both
        ms = {"loop": [], "by_hand": []}
        for _ in range(o.rounds):
            ms["loop"].append(window(loop))
            ms["by_hand"].append(window(by_hand))
        print(json.dumps({"net": kind, "batch": o.batch, "steps": o.steps, "loop_ms_per_step": round(statistics.median(ms["loop"]), 2),
                          "by_hand_ms_per_step": round(statistics.median(ms["by_hand"]), 2),
                          "loop_windows": [round(v, 2) for v in ms["loop"]], "by_hand_windows": [round(v, 2) for v in ms["by_hand"]]}), flush=True)
        del model, opt, ddp, data, batches
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
