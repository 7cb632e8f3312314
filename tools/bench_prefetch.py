#!/usr/bin/env python3
"""What the input work costs a training step, and how much of it adamml_amd/prefetch.py hides: ms per step of the README's AdaMML
recipe model (rgb + sound, ResNet-50, 5 segments, main-net stage as bench.py runs it) at the benchmark's batch -- 72 videos x 40 rgb
frames of 256 x 340 JPEG as tools/bench_loader.py writes them, plus 5 sound windows per video -- with the input arriving in three ways:

    (a) resident   prepared tensors already on the device (video.Augmented + spectrograms): the floor
    (b) front      a cycled list of pinned, collated loader batches fed as the launchers feed them without --prefetch:
                   .to(device, non_blocking=True), then decode / augment / STFT in the model's data layer, in front of the step
    (c) prefetch   the same list through Prefetcher(depth=1), once with the default and once with the lowest stream priority

The arms run in ONE process and alternate in windows (--windows 3 of --steps 40 each); a step is forward, cross-entropy, backward,
SGD step and the loss read-back that ends a step of train_epoch, timed by the host clock from read-back to read-back.  Per arm: the
median of each window, and min / median / 90th percentile over all its steps.  A cycled list isolates the GPU side from the loader;
`--loader_steps N` adds one run of (b) and of (c) behind the real adamml_amd.data:loaders with --workers 16.  Writes one JSON document
(--out, default profiles/prefetch.json) and prints it.  Needs a GPU.

    python tools/bench_prefetch.py [--batch 72] [--steps 40] [--windows 3] [--distinct 4] [--loader_steps 40] [--workers 16]"""
import argparse
import itertools
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def summary(ms):
    s = sorted(ms)
    return dict(steps=len(s), min=round(s[0], 2), median=round(statistics.median(s), 2), p90=round(s[min(len(s) - 1, int(0.9 * len(s)))], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=72)
    ap.add_argument("--segments", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40, help="steps per window")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=4, help="distinct collated batches in the cycled list")
    ap.add_argument("--loader_steps", type=int, default=40, help="steps of (b) and (c) behind the real loaders (0: skip)")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefetch.json"))
    a = ap.parse_args()

    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("bench_prefetch: needs a GPU (a CPU run says nothing about a step time)")
    import bench_loader
    from adamml_amd import adamml, data, synth, train, video
    from adamml_amd.optim import FlatSGD
    from adamml_amd.prefetch import Prefetcher
    dev = torch.device("cuda", 0)
    mod = ["rgb", "sound"]
    model = adamml(groups=8, modality=mod, input_channels=[3, 1], num_segments=a.segments, rng_policy=False, rng_threshold=0.5,
                   causality_modeling="lstm", num_classes=31, depth=50, without_t_stride=False, dropout=0.5, pooling_method="max",
                   fusion_point="logits", unimodality_pretrained=[], learnable_lf_weights=True)
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=1234))
    model.to(dev)
    model.freeze_policy_net()
    model.train()
    model._flat_main.ensure(dev)
    opt = FlatSGD(model._flat_main, lr=0.001, momentum=0.9, weight_decay=5e-4)

    def step(images, target):
        """train_epoch's step (one rank, main-net stage): its copies, forward, loss, backward, optimizer and the read-back."""
        images = [x.to(dev, non_blocking=True) for x in images]
        target = target.to(dev, non_blocking=True)
        out, _ = model(images)
        loss = F.cross_entropy(out, target)
        loss.backward()
        opt.step()
        opt.zero_grad()
        return loss.item()

    def window(feed, n):
        """ms of each of n steps over `feed`, read-back to read-back (the fetch of a step's batch is inside its time)."""
        torch.cuda.synchronize()
        ms, t0 = [], time.perf_counter()
        for images, target in itertools.islice(feed, n):
            step(images, target)
            t1 = time.perf_counter()
            ms.append((t1 - t0) * 1e3)
            t0 = t1
        torch.cuda.synchronize()
        return ms

    least, greatest = torch.cuda.Stream.priority_range()
    doc = dict(batch=a.batch, segments=a.segments, steps_per_window=a.steps, windows=a.windows, distinct_batches=a.distinct,
               device=torch.cuda.get_device_name(0), hw_queues_env=os.environ.get("GPU_MAX_HW_QUEUES"),
               stream_priority_range=dict(least=least, greatest=greatest))
    with tempfile.TemporaryDirectory() as tmp:
        lines = a.batch * max(a.distinct, a.loader_steps + 8)
        roots, mean_bytes = bench_loader.write_dataset(tmp, 48, lines, 120, 256, 340)
        doc["jpeg_bytes_mean"] = round(mean_bytes)

        def loaders(workers):
            args = train.arg_parser().parse_args(["--modality"] + mod + ["--datadir"] + roots + [
                "--groups", "8", "--num_segments", str(a.segments), "-b", str(a.batch), "--dense_sampling", "-j", str(workers)])
            loader, _ = data.loaders(train.resolve_args(args, log=lambda *_: None), 0, 1, dev)
            loader.log = None
            return loader

        # the cycled list: collated and pinned once, by the loader's own DataLoader in this process
        pinned = list(itertools.islice(iter(loaders(0).loader), a.distinct))
        doc["input_types"] = [type(x).__name__ for x in pinned[0][0]]
        resident = []
        for inputs, target in pinned:
            frames, waves = [x.to(dev) for x in inputs]
            resident.append(([video.Augmented(video.augment(frames), frames.modality, frames.k_out), waves.spectrogram()], target.to(dev)))
        torch.cuda.synchronize()

        # one feed per arm for the whole run: a Prefetcher keeps its stream (and the decoder its per-stream workspace) over the windows
        feeds = {
            "resident": itertools.cycle(resident),
            "front": itertools.cycle(pinned),
            "prefetch": Prefetcher(itertools.cycle(pinned), dev, depth=1),
            "prefetch_low_priority": Prefetcher(itertools.cycle(pinned), dev, depth=1, priority=least),
        }
        doc["stream_priority"] = {name: f.stream.priority for name, f in feeds.items() if isinstance(f, Prefetcher)}
        for feed in feeds.values():                                           # warm every arm's shapes, streams and workspaces
            window(feed, 3)
        late = {name: f.stats.late for name, f in feeds.items() if isinstance(f, Prefetcher)}
        per_arm = {name: [] for name in feeds}
        for w in range(a.windows):
            for name, feed in feeds.items():                                  # (a Prefetcher starts a fresh look-ahead in every window)
                per_arm[name].append(window(feed, a.steps))
        late = {name: feeds[name].stats.late - n for name, n in late.items()}
        del feeds
        doc["arms"] = {}
        for name, wins in per_arm.items():
            doc["arms"][name] = dict(window_medians=[round(statistics.median(w), 2) for w in wins], **summary([t for w in wins for t in w]))
            if name in late:
                doc["arms"][name]["late_hand_overs"] = late[name]
        med = {k: statistics.median(v["window_medians"]) for k, v in doc["arms"].items()}
        spread_front = max(doc["arms"]["front"]["window_medians"]) - min(doc["arms"]["front"]["window_medians"])
        cost = med["front"] - med["resident"]
        doc["cycled_list"] = dict(
            input_cost_ms=round(cost, 2), front_window_spread_ms=round(spread_front, 2),
            **{"recovered_ms_" + k: round(med["front"] - med[k], 2) for k in ("prefetch", "prefetch_low_priority")},
            **{"recovered_share_" + k: (round((med["front"] - med[k]) / cost, 2) if cost > 0 else None) for k in ("prefetch", "prefetch_low_priority")})
        del resident

        if a.loader_steps > 0:
            # behind the real loaders: one epoch prefix per arm, worker start-up and the first steps left out of the summary
            res = {}
            for name in ("front", "prefetch"):
                loader = loaders(a.workers)
                feed = Prefetcher(loader, dev, depth=1) if name == "prefetch" else loader
                ms = window(iter(feed), a.loader_steps + 8)[8:]
                res[name] = dict(workers=loader.loader.num_workers, **summary(ms))
                if name == "prefetch":
                    res[name]["late_hand_overs"] = feed.stats.late
                del feed, loader
            doc["real_loaders"] = res
    text = json.dumps(doc, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
