"""Baseline JPEG decoding restated in numpy: test infrastructure for adamml_amd/jpeg.py and csrc/jpeg_decode.hip, byte-exact to
Pillow / libjpeg(-turbo) (tests/test_jpeg_cpu.py checks that against committed Pillow pixels and against Pillow itself).

`decode_packed` is a CPU model of adamml_jpeg_decode_u8: it reads the same packed bytes, descriptors, segment records and tables
(`jpeg.Batch`) and applies the same stated rules to damaged streams -- the bit reader supplies zero bits from a segment's end or a
marker on; a code no table entry matches (or a DC category above 11) and an AC run past coefficient 63 end the segment; a block
after which more bits were consumed than the segment holds ends it too; from there the segment's blocks have zero coefficients;
a segment with 8 or more data bits left after its last MCU is flagged."""
import numpy as np

from adamml_amd import jpeg as J

_luts = {}


def _lut(words):
    """16-bit peek -> (length, symbol) of one packed Huffman table (80 words); length 0 = no code matches."""
    key = words.tobytes()
    t = _luts.get(key)
    if t is None:
        bits, vals = [int(b) for b in words[:16]], np.ascontiguousarray(words[16:80]).view(np.uint8)
        t = np.zeros((65536, 2), np.int32)
        code = k = 0
        for l in range(1, 17):
            for _ in range(bits[l - 1]):
                lo = code << (16 - l)
                t[lo:lo + (1 << (16 - l))] = (l, vals[min(k, 255)])
                code += 1
                k += 1
            code <<= 1
        t = _luts[key] = (t[:, 0].tolist(), t[:, 1].tolist())
    return t


class _Bits:
    """MSB-first reader of one segment: FF 00 is the data byte FF, any other FF xx (or a final FF) ends the data; zero bits after."""

    def __init__(self, seg):
        seg = np.asarray(seg, np.uint8)
        ff = np.flatnonzero(seg == 0xFF)
        nxt = np.append(seg, 1)[ff + 1]                       # a final FF counts as a marker
        stop = ff[nxt != 0]
        seg = seg[:int(stop[0])] if len(stop) else seg
        ff = np.flatnonzero(seg == 0xFF)
        self.b = np.delete(seg, ff + 1).tobytes()
        self.real = 8 * len(self.b)
        self.p = self.acc = self.n = self.used = 0

    def _fill(self):
        while self.n <= 32:
            v = self.b[self.p] if self.p < len(self.b) else 0
            self.p += 1
            self.acc = ((self.acc << 8) | v) & 0xFFFFFFFFFFFFFFFF
            self.n += 8

    def peek16(self):
        self._fill()
        return (self.acc >> (self.n - 16)) & 0xFFFF

    def skip(self, k):
        self.n -= k
        self.used += k

    def get(self, k):
        if k == 0:
            return 0
        self._fill()
        v = (self.acc >> (self.n - k)) & ((1 << k) - 1)
        self.skip(k)
        return v

    @property
    def overrun(self):
        return self.used > self.real


def _extend(v, s):
    return v if s == 0 or v >= (1 << (s - 1)) else v - (1 << s) + 1


def _idct1d(x, shift):
    """jidctint's 1-D pass along the last axis of x [..., 8] int64, descaled by `shift`."""
    z2, z3 = x[..., 2], x[..., 6]
    z1 = (z2 + z3) * 4433
    t2, t3 = z1 - z3 * 15137, z1 + z2 * 6270
    t0, t1 = (x[..., 0] + x[..., 4]) << 13, (x[..., 0] - x[..., 4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a, b, c, d = x[..., 7], x[..., 5], x[..., 3], x[..., 1]
    z1, z2, z3, z4 = a + d, b + c, a + c, b + d
    z5 = (z3 + z4) * 9633
    a, b, c, d = a * 2446, b * 16819, c * 25172, d * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a, b, c, d = a + z1 + z3, b + z2 + z4, c + z2 + z3, d + z1 + z4
    out = np.stack([t10 + d, t11 + c, t12 + b, t13 + a, t13 - a, t12 - b, t11 - c, t10 - d], -1)
    return (out + (1 << (shift - 1))) >> shift


def idct_plane(coef, q):
    """coef [bh, bw, 64] (natural order) x q [64] -> the uint8-valued plane [8 bh, 8 bw] (int32)."""
    x = (coef.astype(np.int64) * q.astype(np.int64)).reshape(coef.shape[0], coef.shape[1], 8, 8)
    w = _idct1d(x.swapaxes(2, 3), 11).swapaxes(2, 3)
    o = np.clip(_idct1d(w, 18) + 128, 0, 255)
    return o.transpose(0, 2, 1, 3).reshape(coef.shape[0] * 8, coef.shape[1] * 8).astype(np.int32)


def upsample_h2v2(c, oh, ow):
    """libjpeg's fancy h2v2 upsampling of the true chroma plane c [ceil(oh/2), ceil(ow/2)] to [oh, ow]."""
    up, dn = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
    out = np.zeros((2 * c.shape[0], 2 * c.shape[1]), np.int32)
    for v, nb in ((0, up), (1, dn)):
        s = 3 * c + nb
        l, r = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
        ev, od = (3 * s + l + 8) >> 4, (3 * s + r + 7) >> 4
        ev[:, 0], od[:, -1] = (4 * s[:, 0] + 8) >> 4, (4 * s[:, -1] + 7) >> 4
        out[v::2, 0::2], out[v::2, 1::2] = ev, od
    return out[:oh, :ow]


def _entropy(data, meta, desc):
    """Coefficients per component [bh, bw, 64] int32 and the status bits of one image of a packed batch."""
    H, W, nc, hs = (int(v) for v in desc[:4])
    mw, mh = -(-W // (8 * hs)), -(-H // (8 * hs))
    per = [hs, 1, 1][:nc]
    coef = [np.zeros((mh * h, mw * h, 64), np.int32) for h in per]
    dc = [_lut(meta[desc[9 + c]:desc[9 + c] + J.HUFF]) for c in range(nc)]
    ac = [_lut(meta[desc[12 + c]:desc[12 + c] + J.HUFF]) for c in range(nc)]
    zz = J.ZIGZAG.tolist()
    status = 0
    for s in range(int(desc[5])):
        off, length, first, count = (int(v) for v in meta[desc[4] + 4 * s:desc[4] + 4 * s + 4])
        br, pred, err = _Bits(data[off:off + length]), [0] * nc, 0
        for mcu in range(first, first + count):
            my, mx = divmod(mcu, mw)
            for c in range(nc):
                h = per[c]
                for b in range(h * h):
                    blk = coef[c][my * h + b // h, mx * h + b % h]
                    look = br.peek16()
                    l, t = dc[c][0][look], dc[c][1][look]
                    if l == 0 or t > 11:
                        err |= J.STATUS_BAD_CODE
                        break
                    br.skip(l)
                    pred[c] = max(-32768, min(32767, pred[c] + _extend(br.get(t), t)))
                    blk[0] = pred[c]
                    k = 1
                    while k <= 63:
                        look = br.peek16()
                        l, rs = ac[c][0][look], ac[c][1][look]
                        if l == 0:
                            err |= J.STATUS_BAD_CODE
                            break
                        br.skip(l)
                        r, sz = rs >> 4, rs & 15
                        if sz == 0:
                            if r != 15:
                                break
                            k += 16
                            continue
                        k += r
                        if k > 63:
                            err |= J.STATUS_BAD_INDEX
                            break
                        blk[zz[k]] = _extend(br.get(sz), sz)
                        k += 1
                    if err == 0 and br.overrun:
                        err |= J.STATUS_OVERRUN
                    if err:
                        break
                if err:
                    break
            if err:
                break
        if err == 0 and br.real - br.used >= 8:
            err = J.STATUS_LEFTOVER
        status |= err
    return coef, status


def decode_image(data, meta, i):
    """(pixels [H, W, 3] or [H, W] uint8, status) of image i of a packed batch."""
    desc = meta[i * J.DESC:(i + 1) * J.DESC]
    H, W, nc, hs = (int(v) for v in desc[:4])
    coef, status = _entropy(data, meta, desc)
    planes = [idct_plane(coef[c], meta[desc[6 + c]:desc[6 + c] + 64]) for c in range(nc)]
    if nc == 1:
        return planes[0][:H, :W].astype(np.uint8), status
    y = planes[0][:H, :W]
    if hs == 2:
        ch, cw = -(-H // 2), -(-W // 2)
        cb, cr = (upsample_h2v2(p[:ch, :cw], H, W) for p in planes[1:])
    else:
        cb, cr = planes[1][:H, :W], planes[2][:H, :W]
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8), status


def decode_packed(data, meta, n, out_bytes, out=None):
    """The CPU model of adamml_jpeg_decode_u8 on a `jpeg.Batch`'s arrays: (flat uint8 output buffer, int32 status [n])."""
    data, meta = np.asarray(data, np.uint8), np.asarray(meta, np.int32)
    y = np.zeros(out_bytes, np.uint8) if out is None else out
    status = np.zeros(n, np.int32)
    for i in range(n):
        d = meta[i * J.DESC:(i + 1) * J.DESC]
        px, status[i] = decode_image(data, meta, i)
        H, W = px.shape[:2]
        px = px.reshape(H, W, -1)
        off = (int(d[15]) & 0xffffffff) | (int(d[16]) << 32)
        at = off + int(d[19]) + np.arange(H)[:, None, None] * int(d[17]) + np.arange(W)[None, :, None] * int(d[18]) + np.arange(px.shape[2])
        y[at] = px
    return y, status


def decode(file_bytes):
    """One JPEG file -> its pixels, through jpeg.parse + jpeg.Batch + the packed-batch model."""
    b = J.Batch([file_bytes])
    y, status = decode_packed(b.data.numpy(), b.meta.numpy(), 1, b.out_bytes)
    assert status[0] == 0, status
    return b.image(y, 0)


def synth_image(seed, h, w, channels=3, noise=20.0):
    """Seeded textured test image [h, w, channels] (or [h, w]) uint8: smooth waves plus noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([128 + 90 * np.sin(xx / 7. + c + seed) + 30 * np.cos(yy / 5. * (c + 1)) for c in range(channels)], -1)
    img = np.clip(img + rng.normal(0, noise, img.shape), 0, 255).astype(np.uint8)
    return img if channels == 3 else img[:, :, 0]


def damage(batch, image, kind):
    """(data, meta) of `batch` as numpy copies with the entropy-coded bytes of `image`'s LAST segment damaged: 'cut' halves its
    stated length, 'ff' / 'zero' overwrite its second quarter with FF / 00 bytes, 'tail0' everything from its middle on with 00."""
    data, meta = batch.data.cpu().numpy().copy(), batch.meta.cpu().numpy().copy()
    d = meta[image * J.DESC:(image + 1) * J.DESC]
    rec = int(d[4]) + 4 * (int(d[5]) - 1)
    off, length = int(meta[rec]), int(meta[rec + 1])
    if kind == "cut":
        meta[rec + 1] = length // 2
    elif kind in ("ff", "zero"):
        data[off + length // 4:off + length // 2] = 0xFF if kind == "ff" else 0
    elif kind == "tail0":
        data[off + length // 2:off + length] = 0
    else:
        raise ValueError(kind)
    return data, meta
