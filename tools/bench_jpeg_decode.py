#!/usr/bin/env python3
"""adamml_jpeg_decode_u8 (adamml_amd.jpeg / video.EncodedFrames) at the benchmark step's load: 72 videos x 5 segments x 8 frames =
2 880 RGB frames, 256 x 341 and 256 x 455 alternating, 4:2:0, synthetic textured content encoded by Pillow at a quality that gives
30-50 KB files -- once as ffmpeg writes them (no restart markers: one entropy-coded segment per frame) and once with one restart
interval per MCU row (16 independent segments per frame).  Per variant: device-event ms of the decode alone and of decode + augment
(median and spread over the repeats), the host ms per frame of parse + Batch (the CPU work that stays in the loader), and Pillow's
single-core decode ms per frame on this host.  The yardstick is what the feature replaces: 16 cores running Pillow,
2880 * pillow_ms / 16 per step, against gpu_ms + 2880 * pack_ms / 16.  Needs Pillow to encode its input (without it: the two
committed full-size 256 x 341 fixtures, and no Pillow timing).  Prints a table and one JSON line.
Usage: python tools/bench_jpeg_decode.py [--repeats 30] [--videos 72]"""
import argparse
import io
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from adamml_amd import jpeg as J, video as V  # noqa: E402

FRAMES_PER_VIDEO = 40
CORES = 16
DISTINCT = 8               # distinct encoded frames per size (the rest of a video repeats them)


def textured(seed, h, w):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([128 + 90 * np.sin(xx / 7. + c + seed) + 30 * np.cos(yy / 5. * (c + 1)) for c in range(3)], -1)
    return np.clip(img + rng.normal(0, 9, img.shape), 0, 255).astype(np.uint8)


def encoded_frames(restart):
    """{width: [DISTINCT files]} for widths 341 and 455, or None without Pillow."""
    try:
        from PIL import Image
    except ImportError:
        return None
    out = {}
    for w in (341, 455):
        out[w] = []
        for s in range(DISTINCT):
            b = io.BytesIO()
            Image.fromarray(textured(s, 256, w)).save(b, "JPEG", quality=93, subsampling=2, **(dict(restart_marker_rows=1) if restart else {}))
            out[w].append(b.getvalue())
    return out


def fixture_frames(restart):
    z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"))
    f = z["full_256x341_rst1.frame" if restart else "full_256x341.frame"].tobytes()
    return {341: [f], 455: [f]}


def pillow_ms(files, rounds=3):
    try:
        from PIL import Image
    except ImportError:
        return None
    best = None
    for _ in range(rounds):
        t0 = time.perf_counter()
        for f in files:
            Image.open(io.BytesIO(f)).copy()
        t = (time.perf_counter() - t0) * 1e3 / len(files)
        best = t if best is None else min(best, t)
    return best


def timed(fn, repeats, min_window_s=1.0):
    """Device-event ms per call: warmed up, repeated at least `repeats` times and for at least min_window_s in total."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times, t0 = [], time.perf_counter()
    while len(times) < repeats or time.perf_counter() - t0 < min_window_s:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e))
        if len(times) >= 50 * repeats:
            break
    t = np.array(times)
    return dict(ms=round(float(np.median(t)), 4), min_ms=round(float(t.min()), 4), p90_ms=round(float(np.percentile(t, 90)), 4), repeats=len(t))


def variant(restart, n_videos, repeats):
    pool = encoded_frames(restart)
    source = "pillow"
    if pool is None:
        pool, source = fixture_frames(restart), "fixtures"
    widths = [(341, 455)[i % 2] if source == "pillow" else 341 for i in range(n_videos)]
    videos = [[pool[w][(i + j) % len(pool[w])] for j in range(FRAMES_PER_VIDEO)] for i, w in enumerate(widths)]
    files = [f for v in videos for f in v]
    random.seed(1)
    np.random.seed(1)
    aug = V.Augmentor(True, 224, version="v2", modality="rgb")
    geos = [aug.sample(w, 256) for w in widths]
    t0 = time.perf_counter()
    ef = V.EncodedFrames(videos, geos, pin_memory=True)
    pack_ms = (time.perf_counter() - t0) * 1e3 / len(files)
    dev = ef.to("cuda")
    y, status = J.decode(dev.batch)
    assert int(status.abs().sum()) == 0, "decode status"
    out = V.augment(dev)
    assert tuple(out.shape) == (n_videos, 224, 224, 3 * FRAMES_PER_VIDEO)
    dec = timed(lambda: J.decode(dev.batch, out=y), repeats)
    both = timed(lambda: V.augment(dev), repeats)
    pil = pillow_ms([f for w in pool for f in pool[w]])
    n = len(files)
    row = dict(restart_intervals=bool(restart), source=source, frames=n, segments_per_frame=len(ef.batch.infos[0].segments),
               file_kb=round(sum(len(f) for f in files) / n / 1024, 1), coded_mb=round(dev.batch.data.numel() / 1e6, 1),
               decode=dec, decode_augment=both, pack_ms_per_frame=round(pack_ms, 4),
               pillow_ms_per_frame=None if pil is None else round(pil, 4))
    row["gpu_path_ms_per_step"] = round(dec["ms"] + n * pack_ms / CORES, 2)
    row["pillow_16_cores_ms_per_step"] = None if pil is None else round(n * pil / CORES, 2)
    row["frames_per_s_gpu_decode"] = round(n / dec["ms"] * 1e3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--videos", type=int, default=72)
    a = ap.parse_args()
    torch.cuda.init()
    rows = [variant(r, a.videos, a.repeats) for r in (False, True)]
    for r in rows:
        print("%-22s %4d frames of %.1f KB, %2d segments each: decode %.3f ms (min %.3f, p90 %.3f, %d repeats), decode + augment %.3f ms, "
              "parse + pack %.3f ms/frame, Pillow %s ms/frame -> GPU path %.1f ms per step, 16 cores of Pillow %s"
              % ("restart per MCU row" if r["restart_intervals"] else "no restart markers", r["frames"], r["file_kb"], r["segments_per_frame"],
                 r["decode"]["ms"], r["decode"]["min_ms"], r["decode"]["p90_ms"], r["decode"]["repeats"], r["decode_augment"]["ms"],
                 r["pack_ms_per_frame"], r["pillow_ms_per_frame"], r["gpu_path_ms_per_step"], r["pillow_16_cores_ms_per_step"]))
    print(json.dumps(dict(tool="bench_jpeg_decode", videos=a.videos, frames_per_video=FRAMES_PER_VIDEO, cores=CORES,
                          device=torch.cuda.get_device_name(0), rows=rows)))


if __name__ == "__main__":
    main()
