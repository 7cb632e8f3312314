#!/usr/bin/env python3
"""adamml_video_resample_u8 (adamml_amd.video.augment) at the benchmark step's shapes: 72 videos of 5 segments x 8 frames, sources
alternating 256 x 341 and 256 x 455, cropped to 224^2.  rgb (K = 120) in v1, v2 and val; flow (K = 400) and rgbdiff (K_in = 720 ->
600) in v2.  Device-event time, median over repeats; GB/s over the bytes the source windows hold (what the kernel must read) plus the
bytes written.  PIL's single-core time per RGB frame for the same transforms when Pillow imports.  Prints a table and one JSON line.
Usage: python tools/bench_video_augment.py [--repeats 50]"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from adamml_amd import video as V  # noqa: E402

N = 72
CASES = [("rgb", "v1", True, 120), ("rgb", "v2", True, 120), ("rgb", "val", False, 120), ("flow", "v2", True, 400), ("rgbdiff", "v2", True, 720)]


def gpu_case(modality, version, is_train, k, repeats):
    rng = np.random.default_rng(0)
    base = [rng.integers(0, 256, (256, w, k), dtype=np.uint8) for w in (341, 455)]
    videos = [base[i % 2] for i in range(N)]
    random.seed(1)
    np.random.seed(1)
    aug = V.Augmentor(is_train, 224, version="v1" if version == "v1" else "v2", modality=modality)
    fr = V.Frames(videos, [aug.sample(v.shape[1], v.shape[0]) for v in videos])
    dev = fr.to("cuda")
    y = V.augment(dev)
    for _ in range(3):
        V.augment(dev)
    times = []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        V.augment(dev)
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e))
    ms = float(np.median(times))
    rd, wr = fr.read_bytes, y.numel()
    full = sum(v.nbytes for v in videos)
    return dict(modality=modality, mode=version, k_in=k, k_out=fr.k_out, ms=round(ms, 4), read_gb=round(rd / 1e9, 4),
                write_gb=round(wr / 1e9, 4), full_frames_gb=round(full / 1e9, 4), gbps=round((rd + wr) / ms / 1e6, 1))


def pil_per_frame(version, frames=40):
    """Single-core ms per RGB frame of the reference's PIL work for one video (crop + resize (v1), resize + crop + flip (v2),
    resize + centre crop (val)) on 256 x 341 frames."""
    try:
        from PIL import Image
    except ImportError:
        return None
    rng = np.random.default_rng(0)
    imgs = [Image.fromarray(rng.integers(0, 256, (256, 341, 3), dtype=np.uint8)) for _ in range(frames)]
    t0 = time.perf_counter()
    for _ in range(3):
        for im in imgs:
            if version == "v1":
                im.crop((20, 10, 212, 202)).resize((224, 224), Image.BILINEAR)
            elif version == "v2":
                im.resize((383, 288), Image.BILINEAR).crop((60, 30, 284, 254)).transpose(Image.FLIP_LEFT_RIGHT)
            else:
                im.crop((58, 16, 282, 240))
    return (time.perf_counter() - t0) * 1e3 / (3 * frames)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    a = ap.parse_args()
    torch.cuda.init()
    rows = [gpu_case(*c, a.repeats) for c in CASES]
    print("%-8s %-4s %5s %5s %9s %8s %8s %9s %8s" % ("modality", "mode", "K_in", "K_out", "ms", "read GB", "write GB", "frames GB", "GB/s"))
    for r in rows:
        print("%-8s %-4s %5d %5d %9.4f %8.3f %8.3f %9.3f %8.1f" % (r["modality"], r["mode"], r["k_in"], r["k_out"], r["ms"], r["read_gb"],
                                                            r["write_gb"], r["full_frames_gb"], r["gbps"]))
    pil = {v: pil_per_frame(v) for v in ("v1", "v2", "val")}
    for v, t in pil.items():
        print("PIL %-4s single core: %s" % (v, "not measured (Pillow not installed)" if t is None else "%.3f ms per RGB frame" % t))
    print(json.dumps(dict(tool="bench_video_augment", n=N, rows=rows,
                          pil_ms_per_frame={v: (None if t is None else round(t, 4)) for v, t in pil.items()})))


if __name__ == "__main__":
    main()
