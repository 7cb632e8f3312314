"""Integer numpy restatement of the reference's visual augmentation before and including Stack (utils/video_transforms.py,
utils/video_dataset.py:32-38), written independently of adamml_amd/video.py: Pillow's 8-bit BILINEAR resize (Resample.c:
precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal / Vertical_8bpc with PRECISION_BITS = 22), crop, horizontal
flip, the flow x-image inversion, compute_img_diff and Stack.  Also the seeded synthetic frames the golden digests were made from."""
import math

import numpy as np

PREC = 22


def pil_coeffs(in_size, out_size, in0=0.0, in1=None):
    """(xmin [out], n [out], k [out, ksize]) as Resample.c computes them for BILINEAR: float64 weights normalised by their sum,
    then int(+-0.5 + w * 2^22)."""
    in1 = float(in_size) if in1 is None else in1
    in0, in1 = np.float32(in0), np.float32(in1)
    scale = float(np.float32(in1 - in0)) / out_size
    fs = scale if scale > 1.0 else 1.0
    support = fs
    ksize = int(math.ceil(support)) * 2 + 1
    xmin = np.zeros(out_size, np.int64)
    n = np.zeros(out_size, np.int64)
    kk = np.zeros((out_size, ksize), np.int64)
    for xx in range(out_size):
        center = float(in0) + (xx + 0.5) * scale
        lo = int(center - support + 0.5)
        lo = 0 if lo < 0 else lo
        hi = int(center + support + 0.5)
        hi = in_size if hi > in_size else hi
        cnt = hi - lo
        w = np.zeros(cnt)
        for x in range(cnt):
            t = abs((x + lo - center + 0.5) * (1.0 / fs))
            w[x] = 1.0 - t if t < 1.0 else 0.0
        tot = 0.0
        for v in w:
            tot += v
        if tot != 0.0:
            w = w / tot
        xmin[xx], n[xx] = lo, cnt
        for x in range(cnt):
            kk[xx, x] = int(0.5 + w[x] * (1 << PREC)) if w[x] >= 0 else int(-0.5 + w[x] * (1 << PREC))
    return xmin, n, kk


def apply_axis(img, xmin, n, kk, axis):
    """One 8-bit pass along `axis` (1 = columns, 0 = rows) of img [H, W, C] uint8: clip8((2^21 + sum k * px) >> 22)."""
    a = np.moveaxis(img.astype(np.int64), axis, 0)                  # [in, other, C]
    out = np.full((len(xmin),) + a.shape[1:], 1 << (PREC - 1), np.int64)
    for t in range(kk.shape[1]):
        live = t < n
        idx = np.where(live, xmin + t, 0)
        out += np.where(live, kk[:, t], 0)[:, None, None] * a[idx]
    out = np.clip(out >> PREC, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def pil_resize(img, width, height):
    """PIL.Image.resize((width, height), BILINEAR) of an 8-bit image [H, W, C]: horizontal pass first over the rows the vertical pass
    reads, each pass skipped when its axis keeps its size; a resize to the same size is a copy."""
    h, w = img.shape[:2]
    if (w, h) == (width, height):
        return img.copy()
    ymin, yn, yk = pil_coeffs(h, height)
    if w != width:
        y0, y1 = int(ymin[0]), int(ymin[-1] + yn[-1])
        img = apply_axis(img[y0:y1], *pil_coeffs(w, width), axis=1)
        ymin = ymin - y0
    if h != height:
        img = apply_axis(img, ymin, yn, yk, axis=0)
    return img


def crop(img, x, y, w, h):
    return img[y:y + h, x:x + w].copy()


def hflip(img):
    return img[:, ::-1].copy()


def tv_resize_size(w, h, s):
    """torchvision.transforms.Resize(s) on a (w, h) image."""
    if min(w, h) == s:
        return w, h
    return (s, int(s * h / w)) if w < h else (int(s * w / h), s)


def img_diff(nxt, cur):
    """compute_img_diff(next, cur): float64 (next - cur + 255) * 0.5, truncated to uint8."""
    d = (nxt.astype(np.float64) - cur.astype(np.float64) + 255.0) * (255.0 / 510.0)
    return d.astype(np.uint8)


def images_of(video, modality, diffs=5):
    """A Frames-style video [H, W, K_in] -> the list of images the reference's transforms see ([H, W, 3] RGB or [H, W, 1] L)."""
    if modality == 'flow':
        return [video[:, :, i:i + 1] for i in range(video.shape[2])]
    imgs = [video[:, :, i:i + 3] for i in range(0, video.shape[2], 3)]
    if modality == 'rgb':
        return imgs
    out = []
    for g in range(0, len(imgs), diffs + 1):
        grp = imgs[g:g + diffs + 1]
        out += [img_diff(grp[d + 1], grp[d]) for d in range(diffs)]
    return out


def transform(images, version, is_train, params, modality, size=224):
    """The augmentor chain with given draws (params as adamml_amd.video.Geometry.params / the golden file), then Stack."""
    out = []
    for im in images:
        h, w = im.shape[:2]
        if is_train and version == 'v1':
            im = crop(im, params['offset_w'], params['offset_h'], params['crop_w'], params['crop_h'])
            im = pil_resize(im, size, size)
        else:
            rw, rh = tv_resize_size(w, h, params['scale'])
            im = pil_resize(im, rw, rh)
            im = crop(im, params['x1'], params['y1'], size, size)
        out.append(im)
    if params.get('flip'):
        out = [hflip(im) for im in out]
        if modality == 'flow':
            out = [255 - im if i % 2 == 0 else im for i, im in enumerate(out)]
    return np.concatenate(out, axis=2)


def synth_video(seed, height, width, channels):
    """Seeded synthetic decoded frames [H, W, K] uint8: noise over a smooth gradient (so resampling has edges and slopes to get right)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    base = (xx * 255 // max(width - 1, 1) + yy * 127 // max(height - 1, 1))[:, :, None] + np.arange(channels)[None, None, :] * 37
    noise = rng.integers(-40, 41, size=(height, width, channels))
    return np.clip((base % 256) + noise, 0, 255).astype(np.uint8)


def run_packed(data, meta, n, oh, ow, k_in, k_out, diffs=0):
    """CPU model of adamml_video_resample_u8 on a packed batch (flat uint8 buffer + int32 descriptors and tables, the layout of
    include/adamml_hip.h): what the kernel must compute, for checking the packing on the host."""
    data, meta = np.asarray(data, np.uint8), np.asarray(meta, np.int64)
    out = np.empty((n, oh, ow, k_out), np.uint8)

    def table(at, stride, count):
        e = meta[at:at + stride * count].reshape(count, stride)
        return e[:, 0], e[:, 1], e[:, 2:]

    for i in range(n):
        d = meta[i * 10:(i + 1) * 10]
        off = int(d[0] & 0xffffffff) | (int(d[1]) << 32)
        h, w, rs = int(d[2]), int(d[3]), int(d[4])
        img = data[off:off + h * rs].reshape(h, rs)[:, :w * k_in].reshape(h, w, k_in)
        if diffs:
            c = np.arange(k_out)
            cur = (c // (3 * diffs)) * 3 * (diffs + 1) + c % (3 * diffs)
            img = ((img[:, :, cur + 3].astype(np.int64) - img[:, :, cur] + 255) >> 1).astype(np.uint8)
        img = apply_axis(img, *table(int(d[5]), int(d[6]), ow), axis=1)
        img = apply_axis(img, *table(int(d[7]), int(d[8]), oh), axis=0)
        if d[9] & 1:
            img[:, :, 0::2] = 255 - img[:, :, 0::2]
        out[i] = img
    return out
