#!/usr/bin/env python3
"""Batches per second of the dataset loader (adamml_amd.data:loaders) running alone, at the benchmark's batch: 72 videos x 5 clips x 8
frames of 256 x 340 JPEG plus 5 sound windows each, 16 workers.  The dataset is synthetic, written into a temporary directory: a few
distinct videos (noise over gradients, so the files have a realistic size) listed many times over.  Prints one JSON line.

    python tools/bench_loader.py [--workers 16] [--batches 48] [--batch 72] [--device cuda]"""
import argparse
import io
import json
import os
import sys
import tempfile
import time
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_dataset(tmp, videos, lines, frames, height, width):
    from PIL import Image
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:height, 0:width]
    blobs = []
    for k in range(16):
        img = np.stack([128 + 90 * np.sin(xx / 17. + c + k) + 30 * np.cos(yy / 11. * (c + 1)) for c in range(3)], -1)
        buf = io.BytesIO()
        Image.fromarray(np.clip(img + rng.normal(0, 12, img.shape), 0, 255).astype(np.uint8)).save(buf, "JPEG", quality=90)
        blobs.append(buf.getvalue())
    roots = [os.path.join(tmp, "rgb"), os.path.join(tmp, "sound")]
    for r in roots:
        os.makedirs(r)
    for i in range(videos):
        os.makedirs(os.path.join(roots[0], "v%04d" % i))
        for n in range(1, frames + 1):
            with open(os.path.join(roots[0], "v%04d" % i, "%05d.jpg" % n), "wb") as f:
                f.write(blobs[(i + n) % len(blobs)])
        with wave.open(os.path.join(roots[1], "v%04d.wav" % i), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(24000)
            f.writeframes(rng.integers(-20000, 20000, int(24000 * (frames / 29.97 + 1)), dtype=np.int16).tobytes())
    for r, ext in zip(roots, ("", ".wav")):
        for lst in ("train.txt", "val.txt"):
            with open(os.path.join(r, lst), "w") as f:
                for j in range(lines if lst == "train.txt" else 1):
                    f.write("v%04d%s;1;%d;%d\n" % (j % videos, ext, frames, j % 31))
    return roots, sum(len(b) for b in blobs) / len(blobs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--batches", type=int, default=48)
    ap.add_argument("--batch", type=int, default=72)
    ap.add_argument("--videos", type=int, default=48)
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--step_ms", type=float, default=103.6, help="the training step the loader has to keep pace with")
    a = ap.parse_args()
    from adamml_amd import data, train
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.time()
        roots, mean_bytes = write_dataset(tmp, a.videos, a.batch * a.batches, a.frames, 256, 340)
        wrote = time.time() - t0
        args = train.arg_parser().parse_args(["--modality", "rgb", "sound", "--datadir"] + roots + [
            "--groups", "8", "--num_segments", "5", "-b", str(a.batch), "--dense_sampling", "-j", str(a.workers)])
        args = train.resolve_args(args, log=lambda *_: None)
        loader, _ = data.loaders(args, 0, 1, a.device)
        loader.log = None
        stamps, t0 = [], time.time()
        for inputs, target in loader:
            stamps.append(time.time() - t0)
        shapes = [list(x.shape) for x in inputs]
    n = len(stamps)
    half = n // 2                                    # the second half of the epoch: workers started, prefetch queues full
    steady = (n - half) / (stamps[-1] - stamps[half - 1]) if n >= 4 else None
    print(json.dumps(dict(batches=n, batch=a.batch, workers=loader.loader.num_workers, cpus_allowed=len(os.sched_getaffinity(0)),
                          cpus_machine=os.cpu_count(), pin_memory=bool(loader.loader.pin_memory), jpeg_bytes_mean=round(mean_bytes),
                          last_batch_shapes=shapes, dataset_written_s=round(wrote, 1), first_batch_s=round(stamps[0], 2),
                          epoch_s=round(stamps[-1], 2), batches_per_s_epoch=round(n / stamps[-1], 2),
                          batches_per_s_steady=round(steady, 2) if steady else None, step_ms=a.step_ms,
                          needed_batches_per_s=round(1e3 / a.step_ms, 2),
                          keeps_pace=bool(steady and steady >= 1e3 / a.step_ms), pillow_fallbacks=data.pillow_fallbacks)))


if __name__ == "__main__":
    main()
