#!/usr/bin/env python3
"""Golden digests for the GPU video augmentation (adamml_amd/video.py): runs the REAL reference's augmentor (IBM/AdaMML, read-only at
$ADAMML_REF, default /root/reference) on seeded synthetic frames and records, per video, the RNG draws its transforms made and the
SHA-256 of the array Stack returned -> tests/golden/video_aug_cases.json.  Nothing from the reference is copied; the file holds
outputs only.  Needs Pillow.  Usage: python tools/gen_video_golden.py"""
import hashlib
import json
import os
import random
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = os.environ.get("ADAMML_REF", "/root/reference")
sys.path.insert(1, REF)

from PIL import Image  # noqa: E402

from tests import video_ref as R  # noqa: E402  (synth_video only: the frames the GPU test regenerates)


# shim: torchvision is absent; utils/video_transforms.py wraps two of its transforms (GroupScale, GroupCenterCrop) and
# utils/utils.py composes with it.  Restated by torchvision's rules: Resize(int) scales the short side to `size` and the long one to
# int(size * long / short) (same size: unchanged); CenterCrop offsets are int(round((size - crop) / 2)).
class _Resize:
    def __init__(self, size, interpolation=Image.BILINEAR):
        self.size, self.interpolation = size, interpolation

    def __call__(self, img):
        w, h = img.size
        if min(w, h) == self.size:
            return img
        ow, oh = (self.size, int(self.size * h / w)) if w < h else (int(self.size * w / h), self.size)
        return img.resize((ow, oh), self.interpolation)


class _CenterCrop:
    def __init__(self, size):
        self.size = size

    def __call__(self, img):
        w, h = img.size
        top, left = int(round((h - self.size) / 2.0)), int(round((w - self.size) / 2.0))
        return img.crop((left, top, left + self.size, top + self.size))


class _Compose:
    def __init__(self, transforms):
        self.transforms = transforms


tv, tvt = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
tvt.Resize, tvt.CenterCrop, tvt.Compose = _Resize, _CenterCrop, _Compose
tv.transforms = tvt
sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt})
np.float = float                                     # compute_img_diff (utils/video_dataset.py:33) uses the removed alias

from utils.utils import get_augmentor  # noqa: E402  (the reference)
from utils.video_dataset import compute_img_diff  # noqa: E402
import utils.video_transforms as VT  # noqa: E402

SIZES = [(256, 341), (256, 455), (341, 256), (240, 320), (256, 256), (300, 533)]       # (H, W) of the decoded frames
FRAMES = {"rgb": 2, "flow": 2, "rgbdiff": 2}                                           # frames (rgbdiff: frame groups) per video
DIFFS = 5
MODES = [("v1", True), ("v2", True), ("val", False)]
SEED = {"v1": 11, "v2": 22, "val": 33}


class _Recorder:
    """Records every value the transforms draw from `random` and numpy's global RNG, in order."""

    def __init__(self):
        self.log = []
        self._orig = (random.choice, random.randint, random.random, np.random.randint)

    def __enter__(self):
        c, ri, rr, nri = self._orig

        def choice(seq):
            v = c(seq)
            self.log.append(["random.choice", list(v)])
            return v

        def randint(a, b):
            v = ri(a, b)
            self.log.append(["random.randint", v])
            return v

        def rand():
            v = rr()
            self.log.append(["random.random", v])
            return v

        def np_randint(*a, **k):
            v = nri(*a, **k)
            self.log.append(["np.random.randint", int(v)])
            return v

        random.choice, random.randint, random.random, np.random.randint = choice, randint, rand, np_randint
        return self

    def __exit__(self, *exc):
        random.choice, random.randint, random.random, np.random.randint = self._orig


def _images(video, modality):
    """The PIL images the reference's load_image hands its transform (utils/video_dataset.py:41-90) for one synthetic video."""
    if modality == "flow":
        return [Image.fromarray(np.ascontiguousarray(video[:, :, i]), "L") for i in range(video.shape[2])]
    rgb = [Image.fromarray(np.ascontiguousarray(video[:, :, i:i + 3]), "RGB") for i in range(0, video.shape[2], 3)]
    if modality == "rgb":
        return rgb
    out = []
    for g in range(0, len(rgb), DIFFS + 1):
        out += [compute_img_diff(rgb[g + d + 1], rgb[g + d]) for d in range(DIFFS)]
    return out


def channels(modality):
    return {"rgb": 3, "flow": 2, "rgbdiff": 3 * (DIFFS + 1)}[modality] * FRAMES[modality]


def main():
    cases = []
    for version, is_train in MODES:
        for modality in ("rgb", "flow", "rgbdiff"):
            aug = get_augmentor(is_train, 224, version="v1" if version == "v1" else "v2", scale_range=[256, 320], modality=modality)
            chain = aug.transforms[:-2]                           # up to and including Stack (ToTorchFormatTensor, GroupNormalize dropped)
            assert isinstance(chain[-1], VT.Stack), chain
            random.seed(SEED[version])
            np.random.seed(SEED[version])
            videos = []
            for i, (h, w) in enumerate(SIZES):
                seed = 1000 * SEED[version] + 10 * i + len(modality)
                imgs = _images(R.synth_video(seed, h, w, channels(modality)), modality)
                with _Recorder() as rec:
                    for t in chain:
                        imgs = t(imgs)
                arr = np.ascontiguousarray(imgs)
                videos.append(dict(height=h, width=w, seed=seed, channels=channels(modality), draws=rec.log, shape=list(arr.shape),
                                   dtype=str(arr.dtype), sha256=hashlib.sha256(arr.tobytes()).hexdigest()))
            cases.append(dict(version=version, is_train=is_train, modality=modality, random_seed=SEED[version], np_seed=SEED[version],
                              diffs=DIFFS if modality == "rgbdiff" else 0, videos=videos))
            print(version, modality, [v["draws"] for v in videos][:2])
    doc = dict(
        about=("Reference outputs of the visual augmentor before ToTorchFormatTensor (utils/utils.py:110-150 get_augmentor, "
               "image_size 224, scale_range [256, 320]) on seeded synthetic frames (tests/video_ref.py synth_video(seed, H, W, K)): per "
               "video the values its transforms drew from random / numpy.random (seeded per case with random_seed / np_seed, videos "
               "in order) and the SHA-256 of the uint8 array Stack returned.  GroupMultiScaleCrop (v1), GroupRandomScale, "
               "GroupRandomCrop, GroupRandomHorizontalFlip (with the flow x-image inversion), compute_img_diff (rgbdiff, 5 differences "
               "from 6 consecutive frames per group) and Stack ran the reference's own code with Pillow; the torchvision Resize and "
               "CenterCrop inside GroupScale / GroupCenterCrop (v2 and val) are a shim of torchvision's rules (tools/gen_video_golden.py), "
               "as torchvision is not installed."),
        pillow=Image.__version__, cases=cases)
    path = os.path.join(ROOT, "tests", "golden", "video_aug_cases.json")
    with open(path, "w") as f:                       # one line per video
        cases_txt = ",\n".join('  {"case": %s,\n   "videos": [\n    %s]}'
                                % (json.dumps({k: v for k, v in c.items() if k != "videos"}),
                                   ",\n    ".join(json.dumps(v) for v in c["videos"])) for c in cases)
        f.write('{"about": %s,\n "pillow": %s,\n "cases": [\n%s]}\n' % (json.dumps(doc["about"]), json.dumps(doc["pillow"]), cases_txt))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
