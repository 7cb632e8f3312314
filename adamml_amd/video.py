"""Visual input without the CPU augmentor: the crop / scale / flip of utils/utils.py:110-150 (get_augmentor, everything before
Stack) on the GPU, byte-exact to the reference's PIL transforms.

    aug = augmentor_for(args, 'rgb', is_train=True)                     # loader worker
    geo = aug.sample(width, height)                                     # draws what the reference's transforms would draw
    batch = Frames([frames_of_video_i, ...], [geo_i, ...], pin_memory=True)   # decoded [H, W, K_in] uint8, source windows only
    x = augment(batch.to(device, non_blocking=True))                    # [N, 224, 224, K_out] uint8 = Stack's arrays

`Augmentor.sample` restates GroupMultiScaleCrop (v1), GroupRandomScale + GroupRandomCrop (v2), GroupScale + GroupCenterCrop (val)
and GroupRandomHorizontalFlip, consuming Python's `random` and numpy's global RNG in the reference's order.  The resampling is
Pillow's 8-bit BILINEAR: integer coefficient tables built here in float64 (`coeffs`), applied by the HIP kernel
adamml_video_resample_u8.  AdaMML.forward takes a `Frames` for rgb, flow and rgbdiff.

    batch = EncodedFrames([jpeg_files_of_video_i, ...], [geo_i, ...], pin_memory=True)   # the frames' JPEG files, not decoded

hands over the files instead: `augment` first decodes them on the GPU (adamml_amd/jpeg.py, byte-exact to PIL.Image.open) into each
video's [H, W, K_in] array and then runs the same resampling kernel on full-frame descriptors."""
import copy
import math
import random

import numpy as np
import torch

from . import hip, jpeg, runtime

__all__ = ['Augmented', 'Augmentor', 'EncodedFrames', 'Frames', 'Geometry', 'augment', 'augment_nowait', 'augmentor_for', 'coeffs', 'resized_size', 'check_table', 'KMAX']

PRECISION_BITS = 22      # Pillow's Resample.c, 8 bits per channel
# Taps per table entry (include/adamml_hip.h): the bilinear support of a downscale by s is s on each side, so KMAX = 32 covers every
# scale down to 1/15 per axis (1920 -> 224 needs 19 taps; the augmentor's own scales 2-4).  Larger tables are rejected.
KMAX = 32
DESC = 10                # ints per video descriptor of the kernel
V1_SCALES = (1, .875, .75, .66)
MODALITIES = ('rgb', 'flow', 'rgbdiff')

_coeffs = {}


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def coeffs(in_size, in0, in1, out_size):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for BILINEAR (support 1 scaled by max(scale, 1)), in float64:
    (first [out] int32, taps [out] int32, k [out, ksize] int32).  An axis that keeps its size over the whole image is the identity
    (one tap of 2^22; Pillow skips that pass).  Cached by (in_size, in0, in1, out_size); treat the arrays as read-only."""
    key = (int(in_size), float(in0), float(in1), int(out_size))
    hit = _coeffs.get(key)
    if hit is not None:
        return hit
    if in_size < 1 or out_size < 1 or not (0 <= in0 < in1 <= in_size):
        raise ValueError("coeffs: bad resample of [%g, %g) of %d source pixels to %d" % (in0, in1, in_size, out_size))
    if in_size == out_size and in0 == 0 and in1 == in_size:
        first = np.arange(out_size, dtype=np.int32)
        res = (first, np.ones(out_size, np.int32), np.full((out_size, 1), 1 << PRECISION_BITS, np.int32))
    else:
        f0, f1 = float(np.float32(in0)), float(np.float32(in1))          # the box is float in Resample.c
        scale = float(np.float32(f1 - f0)) / out_size
        filterscale = max(scale, 1.0)
        support = 1.0 * filterscale
        ksize = int(math.ceil(support)) * 2 + 1
        first = np.zeros(out_size, np.int32)
        taps = np.zeros(out_size, np.int32)
        k = np.zeros((out_size, ksize), np.int32)
        ss = 1.0 / filterscale
        for xx in range(out_size):
            center = f0 + (xx + 0.5) * scale
            xmin = max(int(center - support + 0.5), 0)
            xmax = min(int(center + support + 0.5), in_size) - xmin
            w = [_bilinear((x + xmin - center + 0.5) * ss) for x in range(xmax)]
            ww = 0.0
            for v in w:
                ww += v
            if ww != 0.0:
                w = [v / ww for v in w]
            first[xx], taps[xx] = xmin, xmax
            for x, v in enumerate(w):
                k[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        res = (first, taps, k)
    for a in res:
        a.setflags(write=False)
    _coeffs[key] = res
    return res


def check_table(first, taps, k, src_size, what="table"):
    """Reject a table the kernel must not be given: taps in [1, KMAX], taps inside [0, src_size), coefficients in [0, 2^22]."""
    first, taps, k = np.asarray(first), np.asarray(taps), np.asarray(k)
    if first.ndim != 1 or taps.shape != first.shape or k.ndim != 2 or k.shape[0] != first.shape[0] or first.shape[0] < 1:
        raise ValueError("%s: malformed arrays first %s, taps %s, k %s" % (what, first.shape, taps.shape, k.shape))
    if taps.min() < 1 or taps.max() > KMAX or taps.max() > k.shape[1]:
        raise ValueError("%s: tap counts must be in [1, %d] (KMAX), got [%d, %d]" % (what, KMAX, taps.min(), taps.max()))
    if first.min() < 0 or (first.astype(np.int64) + taps).max() > src_size:
        raise ValueError("%s: taps outside the %d source pixels (first %d, last %d)"
                         % (what, src_size, first.min(), (first.astype(np.int64) + taps).max() - 1))
    if k.min() < 0 or k.max() > (1 << PRECISION_BITS):
        raise ValueError("%s: coefficients outside [0, 2^22]" % what)


def resized_size(width, height, size):
    """torchvision Resize(int): the short side becomes `size`, the long side int(size * long / short); same size = identity."""
    if min(width, height) == size:
        return width, height
    if width < height:
        return size, int(size * height / width)
    return int(size * width / height), size


class Geometry:
    """One video's augmentation, in the terms of the resampling tables.  Per axis (in_size, out_size, shift, keep): the output
    positions are entries keep .. keep + crop - 1 of the resize in_size -> out_size, with `shift` added to every source index
    (crop-then-resize: the resize of the crop, shifted by its offset; resize-then-crop: the whole-image resize, crop = kept entries).
    `params` holds what the reference's transforms drew."""

    def __init__(self, width, height, crop, xaxis, yaxis, flip, modality, params):
        self.width, self.height, self.crop = int(width), int(height), int(crop)
        self.xaxis, self.yaxis = tuple(int(v) for v in xaxis), tuple(int(v) for v in yaxis)
        self.flip, self.modality, self.params = bool(flip), modality, params

    def __repr__(self):
        return "Geometry(%dx%d -> %d, %s, flip=%s)" % (self.width, self.height, self.crop, self.params, self.flip)

    def tables(self):
        """(x table over the crop's columns, y table over its rows), each (first, taps, k) on the full frame, flip applied."""
        out = []
        for axis, src, name, flip in ((self.xaxis, self.width, "column table", self.flip), (self.yaxis, self.height, "row table", False)):
            in_size, out_size, shift, keep = axis
            if keep < 0 or keep + self.crop > out_size or shift < 0 or shift + in_size > src:
                raise ValueError("Geometry: %s keeps [%d, %d) of %d outputs of a resize of [%d, %d) on %d pixels"
                                 % (name, keep, keep + self.crop, out_size, shift, shift + in_size, src))
            first, taps, k = coeffs(in_size, 0, in_size, out_size)
            sl = slice(keep, keep + self.crop)
            first, taps, k = first[sl] + shift, taps[sl], k[sl]
            if flip:
                first, taps, k = first[::-1], taps[::-1], k[::-1]
            check_table(first, taps, k, src, name)
            out.append((first, taps, k))
        return out


class Augmentor:
    """The visual part of get_augmentor (utils/utils.py:110-150) before Stack, as geometry: `sample(width, height)` draws one video's
    crop / scale / flip exactly as the reference's transforms would (same RNGs, same order) and needs only the frame size."""

    def __init__(self, is_train, image_size=224, version='v2', scale_range=(256, 320), disable_scaleup=False, modality='rgb'):
        if modality not in MODALITIES:
            raise ValueError("Augmentor: modality %r, expected one of %s" % (modality, MODALITIES))
        if version not in ('v1', 'v2'):
            raise ValueError("Augmentor: version %r, expected 'v1' or 'v2'" % (version,))
        if int(image_size) < 1:
            raise ValueError("Augmentor: image_size %r < 1" % (image_size,))
        scale_range = [int(v) for v in scale_range]
        if len(scale_range) != 2 or not (1 <= scale_range[0] <= scale_range[1]):
            raise ValueError("Augmentor: scale_range %r, expected (lo, hi) with 1 <= lo <= hi" % (scale_range,))
        self.is_train, self.image_size, self.version = bool(is_train), int(image_size), version
        self.scale_range, self.disable_scaleup, self.modality = tuple(scale_range), bool(disable_scaleup), modality

    def sample(self, width, height):
        width, height, size = int(width), int(height), self.image_size
        if width < 1 or height < 1:
            raise ValueError("Augmentor.sample: frame size %d x %d" % (width, height))
        if self.is_train and self.version == 'v1':
            cw, ch, ow, oh = self._multiscale_crop(width, height)
            geo = dict(crop=size, xaxis=(cw, size, ow, 0), yaxis=(ch, size, oh, 0), params=dict(crop_w=cw, crop_h=ch, offset_w=ow, offset_h=oh))
        elif self.is_train:
            s = int(np.random.randint(low=self.scale_range[0], high=self.scale_range[1] + 1, dtype=int))     # GroupRandomScale
            rw, rh = resized_size(width, height, s)
            if rw < size or rh < size:
                raise ValueError("Augmentor.sample: %d x %d scaled to %d x %d is smaller than the %d crop" % (width, height, rw, rh, size))
            x1 = random.randint(0, rw - size)                                                              # GroupRandomCrop
            y1 = random.randint(0, rh - size)
            geo = dict(crop=size, xaxis=(width, rw, 0, x1), yaxis=(height, rh, 0, y1), params=dict(scale=s, x1=x1, y1=y1))
        else:
            s = size if self.disable_scaleup else int(size / 0.875 + 0.5)                                  # GroupScale
            rw, rh = resized_size(width, height, s)
            if rw < size or rh < size:
                raise ValueError("Augmentor.sample: %d x %d scaled to %d x %d is smaller than the %d crop" % (width, height, rw, rh, size))
            left, top = int(round((rw - size) / 2.0)), int(round((rh - size) / 2.0))                        # GroupCenterCrop
            geo = dict(crop=size, xaxis=(width, rw, 0, left), yaxis=(height, rh, 0, top), params=dict(scale=s, x1=left, y1=top))
        flip = self.is_train and random.random() < 0.5                                                    # GroupRandomHorizontalFlip
        geo['params']['flip'] = flip
        return Geometry(width, height, flip=flip, modality=self.modality, **geo)

    def _multiscale_crop(self, image_w, image_h):
        """GroupMultiScaleCrop._sample_crop_size with max_distort 1, fix_crop and more_fix_crop (video_transforms.py:196-250)."""
        size = self.image_size
        base = min(image_w, image_h)
        crop_sizes = [int(base * x) for x in V1_SCALES]
        crop_h = [size if abs(x - size) < 3 else x for x in crop_sizes]
        crop_w = [size if abs(x - size) < 3 else x for x in crop_sizes]
        pairs = [(w, h) for i, h in enumerate(crop_h) for j, w in enumerate(crop_w) if abs(i - j) <= 1]
        cw, ch = random.choice(pairs)
        ws, hs = (image_w - cw) // 4, (image_h - ch) // 4
        offsets = [(0, 0), (4 * ws, 0), (0, 4 * hs), (4 * ws, 4 * hs), (2 * ws, 2 * hs),
                   (0, 2 * hs), (4 * ws, 2 * hs), (2 * ws, 4 * hs), (2 * ws, 0),
                   (ws, hs), (3 * ws, hs), (ws, 3 * hs), (3 * ws, 3 * hs)]
        ow, oh = random.choice(offsets)
        return cw, ch, ow, oh


def augmentor_for(args, modality, is_train):
    """The Augmentor get_augmentor would build from the launcher's namespace (--input_size, --augmentor_ver, --scale_range,
    --disable_scaleup)."""
    return Augmentor(is_train, image_size=getattr(args, 'input_size', 224), version=getattr(args, 'augmentor_ver', 'v2'),
                     scale_range=tuple(getattr(args, 'scale_range', (256, 320))), disable_scaleup=getattr(args, 'disable_scaleup', False),
                     modality=modality)


def _align(n, a=16):
    return (n + a - 1) // a * a


def split_offset(offset):
    """A byte offset as the descriptor's two int32 words (low 32 bits, high 32 bits), each the bit pattern of the unsigned word."""
    if not 0 <= offset < 1 << 62:
        raise ValueError("Frames: byte offset %d out of range" % offset)
    lo, hi = offset & 0xffffffff, offset >> 32
    return lo - (1 << 32) if lo >= 1 << 31 else lo, hi


class Frames:
    """A batch of N decoded videos for `augment`, as a loader hands it over: one flat uint8 buffer holding only each video's
    source window (the rows and columns its tables read) and one int32 tensor of descriptors + tables shifted to the window.

    videos: N uint8 arrays [H_i, W_i, K_in] (all frames of a video concatenated along the channel axis: flow x / y images
    alternate, rgbdiff holds diffs + 1 consecutive RGB frames per frame group); geometries: `Augmentor.sample` of each video.
    A plain class on purpose: DistributedDataParallel's input scatter passes it through as it is."""

    def __init__(self, videos, geometries, diffs=5, pin_memory=False):
        videos, geometries = list(videos), list(geometries)
        if len(videos) != len(geometries):
            raise ValueError("Frames: %d videos but %d geometries" % (len(videos), len(geometries)))
        if not videos:
            raise ValueError("Frames: empty batch")
        for i, g in enumerate(geometries):
            if not isinstance(g, Geometry):
                raise TypeError("Frames: geometry %d is a %s, expected Augmentor.sample's Geometry" % (i, type(g).__name__))
        g0 = geometries[0]
        self.n, self.out_h, self.out_w, self.modality = len(videos), g0.crop, g0.crop, g0.modality
        k_in = None
        for i, (v, g) in enumerate(zip(videos, geometries)):
            if not isinstance(v, np.ndarray) or v.dtype != np.uint8 or v.ndim != 3:
                raise ValueError("Frames: video %d must be a uint8 numpy array [H, W, K], got %s" % (i, getattr(v, 'dtype', type(v))))
            if v.shape[:2] != (g.height, g.width):
                raise ValueError("Frames: video %d is %d x %d but its geometry was sampled for %d x %d" % (i, v.shape[1], v.shape[0], g.width, g.height))
            if (g.crop, g.modality) != (g0.crop, g0.modality):
                raise ValueError("Frames: video %d has crop %d / modality %s, video 0 %d / %s" % (i, g.crop, g.modality, g0.crop, g0.modality))
            k_in = v.shape[2] if k_in is None else k_in
            if v.shape[2] != k_in:
                raise ValueError("Frames: video %d has %d channels, video 0 %d" % (i, v.shape[2], k_in))
        self.k_in = k_in
        self.diffs = int(diffs) if self.modality == 'rgbdiff' else 0
        if self.modality == 'rgbdiff':
            if self.diffs < 1 or k_in % (3 * (self.diffs + 1)):
                raise ValueError("Frames: rgbdiff needs (diffs + 1) = %d RGB frames per frame group, got %d channels" % (self.diffs + 1, k_in))
            self.k_out = k_in // (self.diffs + 1) * self.diffs
        else:
            self.k_out = k_in

        # tables on the full frame -> source windows -> descriptors + deduplicated tables
        meta = [np.zeros(self.n * DESC, np.int32)]
        nmeta, tab_at, windows = self.n * DESC, {}, []
        offset = 0
        for i, g in enumerate(geometries):
            desc = meta[0][i * DESC:(i + 1) * DESC]
            lo_hi = []
            for j, (first, taps, k) in enumerate(g.tables()):
                lo, hi = int(first.min()), int((first + taps).max())
                lo_hi.append((lo, hi))
                stride = 2 + int(taps.max())
                ent = np.zeros((first.shape[0], stride), np.int32)
                ent[:, 0], ent[:, 1], ent[:, 2:] = first - lo, taps, k[:, :stride - 2]
                key = ent.tobytes()
                if key not in tab_at:
                    tab_at[key] = nmeta
                    meta.append(ent.reshape(-1))
                    nmeta += ent.size
                desc[5 + 2 * j], desc[6 + 2 * j] = tab_at[key], stride
            (x0, x1), (y0, y1) = lo_hi
            h, w = y1 - y0, x1 - x0
            desc[0], desc[1] = split_offset(offset)
            desc[2], desc[3], desc[4] = h, w, w * k_in
            desc[9] = 1 if (g.flip and self.modality == 'flow') else 0
            windows.append((offset, y0, y1, x0, x1))
            offset += _align(h * w * k_in)
        self.read_bytes = sum((y1 - y0) * (x1 - x0) * k_in for _, y0, y1, x0, x1 in windows)
        self.data = torch.empty(max(offset, 16), dtype=torch.uint8, pin_memory=pin_memory)
        buf = self.data.numpy()
        for v, (off, y0, y1, x0, x1) in zip(videos, windows):
            n = (y1 - y0) * (x1 - x0) * k_in
            buf[off:off + n].reshape(y1 - y0, x1 - x0, k_in)[...] = v[y0:y1, x0:x1]
        self.meta = torch.from_numpy(np.concatenate(meta))
        if pin_memory:
            self.meta = self.meta.pin_memory()
        self.geometries = geometries

    @property
    def device(self):
        return self.data.device

    @property
    def shape(self):
        """Shape of `augment`'s output: [N, OH, OW, K_out]."""
        return torch.Size((self.n, self.out_h, self.out_w, self.k_out))

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def to(self, device, non_blocking=False):
        """A Frames whose buffers live on `device` (the copies are asynchronous from pinned memory with non_blocking=True)."""
        out = copy.copy(self)
        out.data = self.data.to(device, non_blocking=non_blocking)
        out.meta = self.meta.to(device, non_blocking=non_blocking)
        return out

    def pin_memory(self):
        out = copy.copy(self)
        out.data, out.meta = self.data.pin_memory(), self.meta.pin_memory()
        return out

    def __repr__(self):
        return "Frames(%s, N=%d, %dx%d, K %d -> %d, %s)" % (self.modality, self.n, self.out_h, self.out_w, self.k_in, self.k_out, self.device)


class EncodedFrames:
    """A batch of N videos for `augment` as their JPEG files: the decoding happens on the GPU too (adamml_amd/jpeg.py), byte-exact
    to PIL.Image.open, straight into each video's interleaved [H_i, W_i, K_in] array.

    videos: per video the list of its frames' JPEG byte strings in Stack's channel order (rgb: one colour file per frame; flow: the
    greyscale x and y files alternating; rgbdiff: the diffs + 1 consecutive colour frames of every frame group); geometries:
    `Augmentor.sample` of each video.  Every file of a video must have the size its Geometry was sampled for.  A file the GPU
    decoder does not handle raises jpeg.Unsupported naming the video and file: decode that batch with Pillow into a `Frames`."""

    def __init__(self, videos, geometries, diffs=5, pin_memory=False):
        videos, geometries = [list(v) for v in videos], list(geometries)
        if len(videos) != len(geometries):
            raise ValueError("EncodedFrames: %d videos but %d geometries" % (len(videos), len(geometries)))
        if not videos:
            raise ValueError("EncodedFrames: empty batch")
        for i, g in enumerate(geometries):
            if not isinstance(g, Geometry):
                raise TypeError("EncodedFrames: geometry %d is a %s, expected Augmentor.sample's Geometry" % (i, type(g).__name__))
        g0 = geometries[0]
        self.n, self.out_h, self.out_w, self.modality = len(videos), g0.crop, g0.crop, g0.modality
        ch = 1 if self.modality == 'flow' else 3
        files, infos, places, self.file_of, k_in, offset = [], [], [], [], None, 0
        meta = [np.zeros(self.n * DESC, np.int32)]
        nmeta, tab_at = self.n * DESC, {}
        for i, (v, g) in enumerate(zip(videos, geometries)):
            if (g.crop, g.modality) != (g0.crop, g0.modality):
                raise ValueError("EncodedFrames: video %d has crop %d / modality %s, video 0 %d / %s" % (i, g.crop, g.modality, g0.crop, g0.modality))
            k_in = len(v) * ch if k_in is None else k_in
            if not v or len(v) * ch != k_in:
                raise ValueError("EncodedFrames: video %d has %d files, video 0 %d" % (i, len(v), k_in // ch))
            for j, f in enumerate(v):
                try:
                    inf = jpeg.parse(f)
                except jpeg.Unsupported as e:
                    raise jpeg.Unsupported("EncodedFrames: video %d, file %d: %s" % (i, j, e)) from None
                if (inf.height, inf.width) != (g.height, g.width):
                    raise ValueError("EncodedFrames: video %d, file %d is %d x %d but the geometry was sampled for %d x %d"
                                     % (i, j, inf.width, inf.height, g.width, g.height))
                if inf.channels != ch:
                    raise ValueError("EncodedFrames: video %d, file %d has %d components, the %s modality stacks files of %d"
                                     % (i, j, inf.channels, self.modality, ch))
                files.append(f)
                infos.append(inf)
                places.append(jpeg.Placement(offset, g.width * k_in, k_in, j * ch))
                self.file_of.append((i, j))
            desc = meta[0][i * DESC:(i + 1) * DESC]
            for j, (first, taps, k) in enumerate(g.tables()):           # the tables on the full frame, as they are
                stride = 2 + int(taps.max())
                ent = np.zeros((first.shape[0], stride), np.int32)
                ent[:, 0], ent[:, 1], ent[:, 2:] = first, taps, k[:, :stride - 2]
                key = ent.tobytes()
                if key not in tab_at:
                    tab_at[key] = nmeta
                    meta.append(ent.reshape(-1))
                    nmeta += ent.size
                desc[5 + 2 * j], desc[6 + 2 * j] = tab_at[key], stride
            desc[0], desc[1] = split_offset(offset)
            desc[2], desc[3], desc[4] = g.height, g.width, g.width * k_in
            desc[9] = 1 if (g.flip and self.modality == 'flow') else 0
            offset += _align(g.height * g.width * k_in)
        self.k_in = k_in
        self.diffs = int(diffs) if self.modality == 'rgbdiff' else 0
        if self.modality == 'rgbdiff':
            if self.diffs < 1 or k_in % (3 * (self.diffs + 1)):
                raise ValueError("EncodedFrames: rgbdiff needs (diffs + 1) = %d RGB frames per frame group, got %d files" % (self.diffs + 1, k_in // 3))
            self.k_out = k_in // (self.diffs + 1) * self.diffs
        else:
            self.k_out = k_in
        self.batch = jpeg.Batch(files, places, offset, pin_memory=pin_memory, infos=infos)
        self.meta = torch.from_numpy(np.concatenate(meta))
        if pin_memory:
            self.meta = self.meta.pin_memory()
        self.geometries = geometries

    @property
    def device(self):
        return self.meta.device

    @property
    def shape(self):
        """Shape of `augment`'s output: [N, OH, OW, K_out]."""
        return torch.Size((self.n, self.out_h, self.out_w, self.k_out))

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def to(self, device, non_blocking=False):
        out = copy.copy(self)
        out.batch = self.batch.to(device, non_blocking=non_blocking)
        out.meta = self.meta.to(device, non_blocking=non_blocking)
        return out

    def pin_memory(self):
        out = copy.copy(self)
        out.batch, out.meta = self.batch.pin_memory(), self.meta.pin_memory()
        return out

    def decode_nowait(self):
        """(y, status): the decoded videos as one flat uint8 buffer on the GPU (video i is [H_i, W_i, K_in] at the offset of its
        descriptor) and the int32 decode status of every file, both on the device and on the current stream: no host read.  The
        caller brings `status` to the host when it suits it and hands it to `check_status`."""
        return jpeg.decode(self.batch)

    def check_status(self, status_host):
        """Raise if a file's stream was damaged: status_host is `decode_nowait`'s status as a host tensor."""
        bad = torch.nonzero(status_host).flatten().tolist()
        if bad:
            i, j = self.file_of[bad[0]]
            raise RuntimeError("EncodedFrames: video %d, file %d has a damaged JPEG stream (decode status %d; %d files of the batch affected)"
                               % (i, j, int(status_host[bad[0]]), len(bad)))

    def decode(self):
        """`decode_nowait`'s buffer.  Waits for the decode status (one small device-to-host copy) and raises if a file's stream was
        damaged."""
        y, status = self.decode_nowait()
        self.check_status(status.cpu())
        return y

    def __repr__(self):
        return "EncodedFrames(%s, N=%d, %dx%d, K %d -> %d, %s)" % (self.modality, self.n, self.out_h, self.out_w, self.k_in, self.k_out,
                                                                   self.device)


class Augmented:
    """A batch of N videos that `augment` has already been through, the prepared input of adamml_amd/prefetch.py: u8 is
    [N, OH, OW, K_out] uint8 on the device, modality and k_out say what it holds.  AdaMML.forward and ResNet.forward take it where
    they take a `Frames` and skip the decode and the resampling.  A plain class, like `Frames`: DistributedDataParallel's input
    scatter passes it through as it is."""

    def __init__(self, u8, modality, k_out):
        if not torch.is_tensor(u8) or u8.dtype != torch.uint8 or u8.dim() != 4:
            raise ValueError("Augmented: expected a uint8 tensor [N, OH, OW, K_out], got %s %s"
                             % (getattr(u8, 'dtype', type(u8).__name__), tuple(getattr(u8, 'shape', ()))))
        if modality not in MODALITIES:
            raise ValueError("Augmented: modality %r, expected one of %s" % (modality, MODALITIES))
        if int(k_out) != u8.size(3):
            raise ValueError("Augmented: k_out %d but the tensor holds %d channels" % (k_out, u8.size(3)))
        self.u8, self.modality, self.k_out = u8, modality, int(k_out)

    @property
    def device(self):
        return self.u8.device

    @property
    def shape(self):
        return self.u8.shape

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def to(self, device, non_blocking=False):
        """`self` when the tensor is on `device` already, else an Augmented whose tensor lives there."""
        u8 = self.u8.to(device, non_blocking=non_blocking)
        return self if u8 is self.u8 else Augmented(u8, self.modality, self.k_out)

    def __repr__(self):
        return "Augmented(%s, %s, %s)" % (self.modality, tuple(self.u8.shape), self.device)


def augment_nowait(frames):
    """(u8, status): `augment`'s [N, OH, OW, K_out] uint8 tensor without its host synchronisation, and the per-file int32 decode
    status on the device for `EncodedFrames.check_status` -- None for a `Frames`, which has none.  Runs on the current stream.  Where
    the status is not 0 the pixels of that video are not to be used."""
    if isinstance(frames, EncodedFrames):
        y, status = frames.decode_nowait()
        return runtime.video_resample_u8(y, frames.meta, frames.n, frames.out_h, frames.out_w, frames.k_in, frames.k_out, frames.diffs), status
    if not isinstance(frames, Frames):
        raise TypeError("augment: expected a video.Frames, got %s" % type(frames).__name__)
    return runtime.video_resample_u8(frames.data, frames.meta, frames.n, frames.out_h, frames.out_w, frames.k_in, frames.k_out, frames.diffs), None


def augment(frames):
    """[N, OH, OW, K_out] uint8 on the GPU: exactly the arrays the reference's augmentor + Stack produce for these videos and
    geometries.  Runs on the current stream; a `Frames` needs no host synchronisation, an `EncodedFrames` one (its decode status)."""
    if isinstance(frames, EncodedFrames):
        return runtime.video_resample_u8(frames.decode(), frames.meta, frames.n, frames.out_h, frames.out_w, frames.k_in, frames.k_out,
                                         frames.diffs)
    return augment_nowait(frames)[0]
