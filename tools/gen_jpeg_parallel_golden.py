#!/usr/bin/env python3
"""Writes tests/golden/jpeg_parallel_cases.npz: the fixtures of the parallel entropy stage for JPEG scans without restart markers
(csrc/jpeg_decode.hip jpeg_parallel_kernel; tests/test_jpeg_parallel_cpu.py, tests/test_jpeg_parallel_gpu.py).  Needs Pillow, which
encodes seeded synthetic images and decodes them for the expected pixels; per fixture `<name>.jpg` (the file's bytes) and either
`<name>.pixels` (Pillow's pixels) or, for the larger noise images, `<name>.sha256` of them.

The noise images at quality 100 are the long synchronisation chains.  The others are the smallest files found, by searching seeds,
that have one property relative to jpeg.SUBSEQ_BYTES (tests/jpeg_sync_ref.py `properties` names them): a coded length of exactly
k subsequences, of one byte more, a stuffed FF 00 split by a subsequence boundary, a boundary inside magnitude bits that read as a
valid code, a ZRL run across a boundary.  Usage: python tools/gen_jpeg_parallel_golden.py"""
import hashlib
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from adamml_amd import jpeg as J  # noqa: E402
from tests import jpeg_ref as R, jpeg_sync_ref as M  # noqa: E402


def encode(img, quality, subsampling=None):
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=quality, **({} if subsampling is None else dict(subsampling=subsampling)))
    return b.getvalue()


def noise(seed, h, w, channels):
    img = np.random.default_rng(seed).integers(0, 256, (h, w, channels), dtype=np.uint8)
    return img if channels == 3 else img[:, :, 0]


def search(prop, make, seeds=range(4000)):
    """The first seed whose file has the property."""
    for seed in seeds:
        f = make(seed)
        if prop in M.properties(J.Batch([f]), 0):
            return seed, f
    raise SystemExit("no seed gives " + prop)


def main():
    out = {}

    def add(name, f, digest_only=False):
        px = np.asarray(Image.open(io.BytesIO(f)))
        assert np.array_equal(R.decode(f), px), name
        out[name + ".jpg"] = np.frombuffer(f, np.uint8)
        if digest_only:
            out[name + ".sha256"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(px).tobytes()).digest(), np.uint8)
        else:
            out[name + ".pixels"] = px
        print("%-28s %6d bytes  %s" % (name, len(f), sorted(M.properties(J.Batch([f]), 0))))

    add("noise_c420_q100_96x96", encode(noise(1, 96, 96, 3), 100, 2), True)
    add("noise_c444_q100_96x96", encode(noise(2, 96, 96, 3), 100, 0), True)
    add("noise_grey_q100_96x96", encode(noise(3, 96, 96, 1), 100), True)
    small = lambda seed: encode(R.synth_image(500 + seed, 24 + seed % 9, 40 - seed % 7, 3, noise=25.0), 90, 2)      # noqa: E731
    sparse = lambda seed: encode(R.synth_image(900 + seed, 32, 32, 3, noise=60.0), 35 + seed % 30, 0)              # noqa: E731
    for prop, make in (("len_kS", small), ("len_kS1", small), ("ff00_split", small), ("mid_magnitude_valid", small), ("zrl_across", sparse)):
        seed, f = search(prop, make)
        add("%s_seed%d" % (prop, seed), f)
    path = os.path.join(ROOT, "tests", "golden", "jpeg_parallel_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
