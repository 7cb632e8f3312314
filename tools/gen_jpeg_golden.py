#!/usr/bin/env python3
"""Writes tests/golden/jpeg_cases.npz: a dozen small baseline JPEG files (seeded synthetic images encoded by Pillow) with Pillow's
decoded pixels, and more frames with only the SHA-256 of Pillow's pixels (two full-size 256 x 341 frames, the frames of small test
videos): the fixtures of tests/test_jpeg_cpu.py and tests/test_jpeg_gpu.py.  4:2:0 / 4:4:4 / greyscale, odd and sub-MCU sizes,
qualities 3 to 100, saturated noise, optimised Huffman tables, restart intervals, and one file re-muxed the way MJPEG writers lay
theirs out: a single DQT and a single DHT segment holding all tables, a COM segment and no JFIF header.  Needs Pillow.
Usage: python tools/gen_jpeg_golden.py"""
import hashlib
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import jpeg_ref as R  # noqa: E402

# name: (height, width, mode, quality, extra save arguments); mode 420 / 444 / L; content "noise" = saturated black / white
CASES = {
    "c420_q93_48x67": (48, 67, 420, 93, {}),
    "c420_q50_17x33": (17, 33, 420, 50, {}),
    "c420_q3_40x56": (40, 56, 420, 3, {}),
    "c420_q100_33x47": (33, 47, 420, 100, {}),
    "c420_q93_7x5": (7, 5, 420, 93, {}),
    "c420_q93_1x1": (1, 1, 420, 93, {}),
    "c444_q93_16x16": (16, 16, 444, 93, {}),
    "c444_q50_37x53": (37, 53, 444, 50, {}),
    "grey_q93_41x30": (41, 30, "L", 93, {}),
    "grey_q50_8x9_opt": (8, 9, "L", 50, dict(optimize=True)),
    "c420_q93_48x64_opt": (48, 64, 420, 93, dict(optimize=True)),
    "c420_q93_50x70_rst1": (50, 70, 420, 93, dict(restart_marker_rows=1)),
    "c444_q93_30x41_rst2": (30, 41, 444, 93, dict(restart_marker_blocks=2)),
    "c420_q95_32x48_noise": (32, 48, 420, 95, {}),
    "c420_q93_34x50_remux": (34, 50, 420, 93, {}),
}


def encode(name, seed):
    h, w, mode, quality, extra = CASES[name]
    if name.endswith("noise"):
        img = (np.random.default_rng(seed).integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    else:
        img = R.synth_image(seed, h, w, 1 if mode == "L" else 3)
    kw = dict(extra) if mode == "L" else dict(extra, subsampling={420: 2, 444: 0}[mode])
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=quality, **kw)
    return b.getvalue()


def remux(data):
    """The same image with one DQT and one DHT segment carrying all tables, a COM segment and no APPn segments."""
    i, dqt, dht, rest = 2, b"", b"", []
    while True:
        m, length = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        body = data[i + 4:i + 2 + length]
        if m == 0xDB:
            dqt += body
        elif m == 0xC4:
            dht += body
        elif m == 0xDA:
            break
        elif not 0xE0 <= m <= 0xEF:
            rest.append(data[i:i + 2 + length])
        i += 2 + length

    def seg(marker, body):
        return bytes([0xFF, marker, (len(body) + 2) >> 8, (len(body) + 2) & 255]) + body
    return data[:2] + seg(0xFE, b"re-muxed") + seg(0xDB, dqt) + b"".join(rest) + seg(0xC4, dht) + data[i:]


# Frames without their pixels (only Pillow's SHA-256 of them): two full-size 256 x 341 frames as the loader's files are (4:2:0, quality
# 93, with and without one restart interval per MCU row) and the distinct frames of small test videos in two sizes per kind.
FRAMES = {"full_256x341": (256, 341, 420, 93, {}), "full_256x341_rst1": (256, 341, 420, 93, dict(restart_marker_rows=1))}
FRAMES.update({"vid_c_48x67_%d" % j: (48, 67, (420, 444)[j % 2], (93, 80, 97)[j % 3], dict(optimize=j == 2)) for j in range(6)})
FRAMES.update({"vid_c_37x53_%d" % j: (37, 53, 420, 93, dict(restart_marker_rows=j % 2)) for j in range(4)})
FRAMES.update({"vid_g_41x30_%d" % j: (41, 30, "L", (93, 75)[j % 2], {}) for j in range(4)})
FRAMES.update({"vid_g_24x40_%d" % j: (24, 40, "L", 93, dict(optimize=j == 1)) for j in range(3)})


def main():
    out = {}
    for seed, (name, (h, w, mode, quality, extra)) in enumerate(FRAMES.items()):
        img = R.synth_image(1000 + seed, h, w, 1 if mode == "L" else 3, noise=9.0 if name.startswith("full") else 20.0)
        kw = dict(extra) if mode == "L" else dict(extra, subsampling={420: 2, 444: 0}[mode])
        b = io.BytesIO()
        Image.fromarray(img).save(b, "JPEG", quality=quality, **kw)
        out[name + ".frame"] = np.frombuffer(b.getvalue(), np.uint8)
        pixels = np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(b.getvalue()))))
        out[name + ".sha256"] = np.frombuffer(hashlib.sha256(pixels.tobytes()).digest(), np.uint8)
        print("%-24s %6d bytes" % (name, len(b.getvalue())))
    for seed, name in enumerate(CASES):
        data = encode(name, seed)
        if name.endswith("remux"):
            data = remux(data)
        pixels = np.asarray(Image.open(io.BytesIO(data)))
        out[name + ".jpg"] = np.frombuffer(data, np.uint8)
        out[name + ".pixels"] = pixels
        print("%-24s %6d bytes -> %s" % (name, len(data), pixels.shape))
    path = os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
