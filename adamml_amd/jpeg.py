"""Baseline JPEG frames decoded on the GPU, byte-exact to Pillow / libjpeg(-turbo): the host half.

    info = parse(data)                                   # markers up to SOS; raises Unsupported for what the kernel does not do
    batch = Batch([bytes_of_frame_0, ...], pin_memory=True)
    y, status = decode(batch.to(device, non_blocking=True))     # flat uint8 buffer of the frames' pixels, int32 status per image

numpy only (no Pillow).  `parse` reads DQT, SOF0, DHT, DRI and SOS and splits the scan at its restart markers; `Batch` packs the
entropy-coded bytes of N files (byte stuffing left in place) and one int32 `meta` tensor for the HIP kernels of
csrc/jpeg_decode.hip (adamml_jpeg_decode_u8; the layout of every word is in include/adamml_hip.h).  Supported: SOF0, 8 bits, one
scan, greyscale or YCbCr 4:2:0 / 4:4:4.  `video.EncodedFrames` builds on this to feed `video.augment`."""
import copy

import numpy as np
import torch

from . import hip, runtime

__all__ = ['Batch', 'Info', 'Unsupported', 'decode', 'parse', 'Placement', 'ZIGZAG', 'DESC', 'STATUS_OVERRUN', 'STATUS_BAD_CODE',
           'STATUS_BAD_INDEX', 'STATUS_BAD_DESC', 'STATUS_LEFTOVER', 'MAX_PIXELS', 'SUBSEQ_BYTES']

DESC = 22                  # ints per image descriptor (include/adamml_hip.h)
SEG = 4                    # ints per segment record
HUFF = 80                  # ints per Huffman table: BITS[16], then HUFFVAL[256] as 64 little-endian words
MAX_PIXELS = 1 << 24       # default pixel cap of parse(): 4096 x 4096
SUBSEQ_BYTES = 128         # a scan without restart markers is decoded in subsequences of this many bytes, one lane each
#                            (ADAMML_JPEG_SUBSEQ_BYTES in include/adamml_hip.h; why 128: csrc/jpeg_decode.hip)
STATUS_OVERRUN, STATUS_BAD_CODE, STATUS_BAD_INDEX, STATUS_BAD_DESC, STATUS_LEFTOVER = 1, 2, 4, 8, 16

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63],
                  np.int32)
ZIGZAG.setflags(write=False)

_SOF_NAMES = {0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless", 0xC5: "differential sequential",
              0xC6: "differential progressive", 0xC7: "differential lossless", 0xC9: "arithmetic sequential",
              0xCA: "arithmetic progressive", 0xCB: "arithmetic lossless", 0xCD: "arithmetic differential sequential",
              0xCE: "arithmetic differential progressive", 0xCF: "arithmetic differential lossless"}


class Unsupported(ValueError):
    """A JPEG file the GPU decoder does not handle (the message names the reason): decode that file with Pillow instead."""


class Info:
    """What `parse` found.  components: [(id, h, v, quantisation table, DC table, AC table)] in scan order = frame order;
    huffman: {(class, id): (BITS [16] uint8, HUFFVAL uint8)}, class 0 = DC, 1 = AC; quant: {id: [64] int32 in natural order};
    segments: [(start, end)] byte ranges of `data` holding entropy-coded bytes (split at RSTn, the trailing EOI excluded)."""

    def __init__(self, height, width, components, huffman, quant, restart_interval, segments):
        self.height, self.width, self.components = height, width, components
        self.huffman, self.quant, self.restart_interval, self.segments = huffman, quant, restart_interval, segments

    @property
    def channels(self):
        return len(self.components)

    @property
    def sampling(self):
        """1 (greyscale and 4:4:4) or 2 (4:2:0): the luma sampling factor on both axes."""
        return self.components[0][1] if len(self.components) == 3 else 1

    @property
    def mcus(self):
        """(MCUs per row, MCU rows); a greyscale scan is not interleaved: its MCU is one block."""
        s = 8 * self.sampling
        return -(-self.width // s), -(-self.height // s)

    @property
    def blocks(self):
        """8 x 8 blocks of all components (the image's share of the decoder's workspace)."""
        mw, mh = self.mcus
        return mw * mh * (self.sampling ** 2 + 2 if self.channels == 3 else 1)

    def __repr__(self):
        return "Info(%d x %d, %d components, sampling %d, %d segments)" % (self.width, self.height, self.channels, self.sampling,
                                                                          len(self.segments))


_dqt_cache, _dht_cache = {}, {}


def _cached(cache, seg, fn):
    """fn(seg) remembered by the segment's bytes: the frames of a dataset share a handful of DQT / DHT segments."""
    key = seg.tobytes()
    hit = cache.get(key)
    if hit is None:
        if len(cache) >= 1024:
            cache.clear()
        hit = cache[key] = fn(seg)
    return hit


def _parse_dqt(seg):
    out, p = {}, 0
    while p < len(seg):
        pq, tq = int(seg[p]) >> 4, int(seg[p]) & 15
        if pq != 0:
            raise Unsupported("16-bit quantisation table")
        if tq > 3 or p + 65 > len(seg):
            raise Unsupported("damaged DQT segment")
        t = np.zeros(64, np.int32)
        t[ZIGZAG] = seg[p + 1:p + 65]
        t.setflags(write=False)
        out[tq] = t
        p += 65
    return out


def _parse_dht(seg):
    out, p = {}, 0
    while p < len(seg):
        tc, th = int(seg[p]) >> 4, int(seg[p]) & 15
        if tc > 1 or th > 3 or p + 17 > len(seg):
            raise Unsupported("damaged DHT segment")
        bits = np.array(seg[p + 1:p + 17], np.uint8)
        cnt = int(bits.sum())
        code, ok = 0, cnt <= 256 and p + 17 + cnt <= len(seg)
        for k, b in enumerate(bits):                 # canonical codes of length k + 1 must fit in k + 1 bits
            code += int(b)
            ok = ok and code <= 1 << (k + 1)
            code <<= 1
        if not ok:
            raise Unsupported("damaged DHT segment (code lengths do not form a prefix code)")
        out[(tc, th)] = (bits, np.array(seg[p + 17:p + 17 + cnt], np.uint8))
        p += 17 + cnt
    return out


def parse(data, max_pixels=MAX_PIXELS):
    """Read the markers of a JPEG file up to SOS -> Info.  Raises Unsupported (a ValueError) naming the reason for everything
    outside baseline sequential Huffman 8-bit, one scan, greyscale / YCbCr 4:2:0 / 4:4:4."""
    d = np.frombuffer(data, np.uint8)
    n = d.shape[0]
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise Unsupported("not a JPEG file (no SOI marker)")
    i, quant, huff, ri, frame, jfif, adobe = 2, {}, {}, 0, None, False, False
    while True:
        if i + 4 > n:
            raise Unsupported("truncated header (no SOS marker)")
        if d[i] != 0xFF:
            raise Unsupported("truncated or damaged header (byte %d is not a marker)" % i)
        m = int(d[i + 1])
        if m == 0xFF:                       # fill byte
            i += 1
            continue
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            i += 2
            continue
        if m == 0xD9:
            raise Unsupported("truncated header (EOI before SOS)")
        length = (int(d[i + 2]) << 8) | int(d[i + 3])
        if length < 2 or i + 2 + length > n:
            raise Unsupported("truncated header (marker %02X runs past the end of the file)" % m)
        seg = d[i + 4:i + 2 + length]
        if m == 0xDB:
            quant.update(_cached(_dqt_cache, seg, _parse_dqt))
        elif m == 0xC0:
            if frame is not None:
                raise Unsupported("more than one frame header")
            if len(seg) < 6 or len(seg) < 6 + 3 * int(seg[5]):
                raise Unsupported("truncated header (SOF0)")
            if seg[0] != 8:
                raise Unsupported("%d-bit samples" % seg[0])
            h, w, nc = (int(seg[1]) << 8) | int(seg[2]), (int(seg[3]) << 8) | int(seg[4]), int(seg[5])
            frame = (h, w, [(int(seg[6 + 3 * c]), int(seg[7 + 3 * c]) >> 4, int(seg[7 + 3 * c]) & 15, int(seg[8 + 3 * c])) for c in range(nc)])
        elif m in _SOF_NAMES:
            raise Unsupported("%s JPEG (SOF%d)" % (_SOF_NAMES[m], m - 0xC0))
        elif m == 0xC4:
            huff.update(_cached(_dht_cache, seg, _parse_dht))
        elif m == 0xDD:
            if len(seg) < 2:
                raise Unsupported("truncated header (DRI)")
            ri = (int(seg[0]) << 8) | int(seg[1])
        elif m == 0xE0 and len(seg) >= 5 and bytes(seg[:5]) == b"JFIF\0":
            jfif = True
        elif m == 0xEE and len(seg) >= 5 and bytes(seg[:5]) == b"Adobe":
            adobe = True
        elif m == 0xDA:
            break
        i += 2 + length
    if frame is None:
        raise Unsupported("no frame header before the scan")
    height, width, comps = frame
    if height < 1 or width < 1:
        raise Unsupported("size %d x %d" % (width, height))
    if height * width > max_pixels:
        raise Unsupported("%d x %d is above the cap of %d pixels" % (width, height, max_pixels))
    if len(comps) not in (1, 3):
        raise Unsupported("%d components" % len(comps))
    if adobe:
        raise Unsupported("Adobe APP14 marker (another colour transform)")
    if len(comps) == 3 and not jfif and [c[0] for c in comps] == [ord('R'), ord('G'), ord('B')]:
        raise Unsupported("component ids 'R', 'G', 'B' without a JFIF header (stored as RGB)")
    samp = [(c[1], c[2]) for c in comps]
    if len(comps) == 3 and samp not in ([(1, 1)] * 3, [(2, 2), (1, 1), (1, 1)]):
        raise Unsupported("chroma sampling %s (only 4:2:0 and 4:4:4)" % "/".join("%dx%d" % s for s in samp))
    if len(comps) == 1:
        comps = [(comps[0][0], 1, 1, comps[0][3])]          # a single-component scan is not interleaved: factors do not matter
    ns = int(seg[0]) if len(seg) else 0
    if ns != len(comps) or len(seg) < 1 + 2 * ns + 3:
        raise Unsupported("multiple scans (the first scan holds %d of %d components)" % (ns, len(comps)))
    if (int(seg[1 + 2 * ns]), int(seg[2 + 2 * ns]), int(seg[3 + 2 * ns])) != (0, 63, 0):
        raise Unsupported("a scan that is not sequential (spectral selection / successive approximation)")
    components = []
    for k, c in enumerate(comps):
        if int(seg[1 + 2 * k]) != c[0]:
            raise Unsupported("scan components out of frame order")
        td, ta = int(seg[2 + 2 * k]) >> 4, int(seg[2 + 2 * k]) & 15
        if c[3] not in quant:
            raise Unsupported("missing quantisation table %d" % c[3])
        if (0, td) not in huff or (1, ta) not in huff:
            raise Unsupported("missing Huffman table (DC %d / AC %d)" % (td, ta))
        components.append((c[0], c[1], c[2], c[3], td, ta))
    s0 = i + 2 + length
    scan = d[s0:]
    ff = np.flatnonzero(scan[:-1] == 0xFF) if len(scan) > 1 else np.zeros(0, np.int64)
    nxt = scan[ff + 1]
    rst = ff[(nxt >= 0xD0) & (nxt <= 0xD7)]
    other = ff[(nxt != 0) & (nxt != 0xFF) & ((nxt < 0xD0) | (nxt > 0xD7))]
    end = int(other[0]) if len(other) else len(scan)
    if len(other) and any(int(scan[o + 1]) == 0xDA for o in other):
        raise Unsupported("multiple scans")
    rst = rst[rst < end]
    starts = [0] + [int(r) + 2 for r in rst]
    ends = [int(r) for r in rst] + [end]
    info = Info(height, width, components, huff, quant, ri, [(s0 + a, s0 + b) for a, b in zip(starts, ends)])
    mw, mh = info.mcus
    want = -(-(mw * mh) // ri) if ri else 1
    if len(info.segments) != want:
        raise Unsupported("%d entropy-coded segments where the restart interval %d asks for %d (truncated or damaged scan)"
                          % (len(info.segments), ri, want))
    return info


class Placement:
    """Where an image's pixels go in the output buffer: byte offset, row stride, pixel stride and channel offset (all in bytes)."""

    def __init__(self, offset, row_stride, pixel_stride, channel=0):
        self.offset, self.row_stride, self.pixel_stride, self.channel = int(offset), int(row_stride), int(pixel_stride), int(channel)


def _align(n, a=16):
    return (n + a - 1) // a * a


def _split(offset):
    lo, hi = offset & 0xffffffff, offset >> 32
    return lo - (1 << 32) if lo >= 1 << 31 else lo, hi


class Batch:
    """N JPEG files packed for one adamml_jpeg_decode_u8 launch.

    data: flat uint8 buffer with the entropy-coded bytes of every segment (each 16-byte aligned, byte stuffing left in place).
    meta: int32: N image descriptors of DESC words, then per image its segment records (byte offset, length, first MCU, MCU
    count), then the quantisation tables (64 words, natural order) and Huffman tables (BITS, HUFFVAL) -- identical tables stored
    once.  placements: per image a Placement; by default image i is a dense [H, W, C] array at `offsets[i]` (16-byte aligned).
    infos may carry the files' `parse` results when the caller has them already.
    parallel: per image whether its entropy decoding takes the parallel stage for scans without restart markers
    (adamml_jpeg_decode_parallel_supported) -- a label: the pixels are the same either way."""

    def __init__(self, files, placements=None, out_bytes=None, pin_memory=False, infos=None):
        files = list(files)
        if not files:
            raise ValueError("jpeg.Batch: empty batch")
        infos = [parse(f) for f in files] if infos is None else list(infos)
        if placements is None:
            placements, off = [], 0
            for inf in infos:
                placements.append(Placement(off, inf.width * inf.channels, inf.channels, 0))
                off += _align(inf.height * inf.width * inf.channels)
            out_bytes = off
        placements = list(placements)
        if len(placements) != len(files) or len(infos) != len(files) or out_bytes is None:
            raise ValueError("jpeg.Batch: %d files, %d placements, %d infos, out_bytes %r" % (len(files), len(placements), len(infos), out_bytes))
        self.n, self.infos, self.placements, self.out_bytes = len(files), infos, placements, max(int(out_bytes), 16)
        self.offsets = [p.offset for p in placements]
        for i, (inf, p) in enumerate(zip(infos, placements)):
            last = p.offset + (inf.height - 1) * p.row_stride + (inf.width - 1) * p.pixel_stride + p.channel + inf.channels
            if min(p.offset, p.row_stride, p.pixel_stride, p.channel) < 0 or last > self.out_bytes:
                raise ValueError("jpeg.Batch: image %d placed outside the %d output bytes" % (i, self.out_bytes))

        nseg = sum(len(inf.segments) for inf in infos)
        head = np.zeros(self.n * DESC + nseg * SEG, np.int32)
        parts, nmeta, tab_at = [head], head.size, {}

        def table(words):
            nonlocal nmeta
            key = words.tobytes()
            if key not in tab_at:
                tab_at[key] = nmeta
                parts.append(words)
                nmeta += words.size
            return tab_at[key]

        chunks, src_off, seg_at, blk = [], 0, self.n * DESC, 0
        for i, (f, inf, p) in enumerate(zip(files, infos, placements)):
            raw = np.frombuffer(f, np.uint8)
            desc = head[i * DESC:(i + 1) * DESC]
            mw, mh = inf.mcus
            nmcu, ri = mw * mh, inf.restart_interval or mw * mh
            desc[0], desc[1], desc[2], desc[3] = inf.height, inf.width, inf.channels, inf.sampling
            desc[4], desc[5] = seg_at, len(inf.segments)
            for c, comp in enumerate(inf.components):
                bits, vals = inf.huffman[(0, comp[4])], inf.huffman[(1, comp[5])]
                desc[6 + c] = table(np.ascontiguousarray(inf.quant[comp[3]], np.int32))
                for slot, (b, v) in ((9, bits), (12, vals)):
                    hv = np.zeros(256, np.uint8)
                    hv[:len(v)] = v
                    desc[slot + c] = table(np.concatenate([b.astype(np.int32), hv.view('<i4')]))
            desc[15], desc[16] = _split(p.offset)
            desc[17], desc[18], desc[19] = p.row_stride, p.pixel_stride, p.channel
            desc[20], desc[21] = _split(blk)
            blk += inf.blocks
            for s, (a, b) in enumerate(inf.segments):
                head[seg_at:seg_at + SEG] = (src_off, b - a, s * ri, min(ri, nmcu - s * ri))
                chunks.append((src_off, raw[a:b]))
                src_off += _align(b - a)
                seg_at += SEG
        if src_off >= 1 << 31:
            raise ValueError("jpeg.Batch: %d entropy-coded bytes in one batch (limit 2^31 - 1)" % src_off)
        self.total_blocks = blk
        self.data = torch.zeros(max(src_off, 16), dtype=torch.uint8, pin_memory=pin_memory)
        buf = self.data.numpy()
        for off, c in chunks:
            buf[off:off + len(c)] = c
        self.meta = torch.from_numpy(np.concatenate(parts))
        if pin_memory:
            self.meta = self.meta.pin_memory()

    @property
    def device(self):
        return self.data.device

    @property
    def parallel(self):
        probe = hip.load().adamml_jpeg_decode_parallel_supported
        return [bool(probe(inf.height, inf.width, inf.channels, inf.sampling, len(inf.segments), inf.segments[0][1] - inf.segments[0][0]))
                for inf in self.infos]

    def to(self, device, non_blocking=False):
        """A Batch whose buffers live on `device` (asynchronous copies from pinned memory with non_blocking=True)."""
        out = copy.copy(self)
        out.data = self.data.to(device, non_blocking=non_blocking)
        out.meta = self.meta.to(device, non_blocking=non_blocking)
        return out

    def pin_memory(self):
        out = copy.copy(self)
        out.data, out.meta = self.data.pin_memory(), self.meta.pin_memory()
        return out

    def image(self, y, i):
        """Image i of a default-placed batch as an [H, W, C] (or [H, W]) view of the decoded buffer `y`."""
        inf, p = self.infos[i], self.placements[i]
        v = y[p.offset:p.offset + inf.height * inf.width * inf.channels]
        return v.reshape(inf.height, inf.width, inf.channels) if inf.channels == 3 else v.reshape(inf.height, inf.width)

    def __repr__(self):
        return "jpeg.Batch(N=%d, %d coded bytes, %d meta words, %s)" % (self.n, self.data.numel(), self.meta.numel(), self.device)


def decode(batch, out=None):
    """(y, status): the flat uint8 output buffer of `batch.out_bytes` bytes (bytes no image covers are left as they are: zero
    when `out` is not given) and an int32 status per image (0 = decoded cleanly; STATUS_* bits otherwise: include/adamml_hip.h).  Runs on the current
    stream; no host synchronisation."""
    if not isinstance(batch, Batch):
        raise TypeError("jpeg.decode: expected a jpeg.Batch, got %s" % type(batch).__name__)
    return runtime.jpeg_decode_u8(batch.data, batch.meta, batch.n, batch.out_bytes, batch.total_blocks, out)
