"""The parallel entropy stage of csrc/jpeg_decode.hip (jpeg_parallel_kernel) restated in Python on a packed `jpeg.Batch`: test
infrastructure.  A scan without restart markers is cut into subsequences of `jpeg.SUBSEQ_BYTES` raw bytes (byte stuffing in place);

  1. every subsequence is decoded from a guessed state (its first byte, block 0 of an MCU, DC next) to its end, recording the exit
     state and the blocks completed;
  2. Jacobi rounds: a subsequence whose predecessor's exit state differs from the state it was last decoded from is decoded again from
     it, until a round changes nothing (a decode that met a bad code has no exit state and tells its successor nothing);
  3. the prefix sum of the block counts places every subsequence; one more decode from the true states stores the coefficients, DC
     as its difference;
  4. per component the prefix sum of the DC differences in scan order.

A state is (raw bit position, block in MCU, next zigzag index); a position names a data byte, never the 00 of a stuffed FF 00; a
subsequence owns the symbols that begin in its bytes.  `entropy` returns the coefficients in tests/jpeg_ref.py's layout and what
happened on the way (rounds, decodes, whether the stage gave the image up to the sequential decoder, and with trace=True the true
symbols: the fixtures' properties are read off them)."""
import numpy as np

from adamml_amd import jpeg as J
from tests import jpeg_ref as R

MAXSUB = 2048


class _Segment:
    """The segment's data bytes (stuffed 00s removed, zero bytes after the end) and the two maps between raw and data positions."""

    def __init__(self, raw):
        raw = np.asarray(raw, np.uint8)
        self.raw, self.len = raw, len(raw)
        ff = raw == 0xFF
        stuffed = np.zeros(len(raw), bool)
        stuffed[1:] = ff[:-1] & (raw[1:] == 0)
        self.stuffed = stuffed
        self.marker = bool((ff & ~np.append(stuffed[1:], False)).any())           # an FF that no 00 follows
        self.raw_of = np.flatnonzero(~stuffed).tolist()
        self.nd = len(self.raw_of)
        self.below = np.concatenate([[0], np.cumsum(~stuffed)]).tolist()          # data bytes with a raw index < i
        self.b = raw[~stuffed].tobytes() + bytes(16)

    def to_data(self, pos):
        i = pos >> 3
        return ((self.below[i] if i < self.len else self.nd + i - self.len) << 3) | (pos & 7)

    def to_raw(self, dpos):
        j = dpos >> 3
        return ((self.raw_of[j] if j < self.nd else self.len + j - self.nd) << 3) | (dpos & 7)

    def peek(self, dpos, k):
        """k <= 16 bits from data bit position dpos."""
        j = min(dpos >> 3, len(self.b) - 4)
        return (int.from_bytes(self.b[j:j + 4], "big") >> (32 - k - (dpos & 7))) & ((1 << k) - 1) if k else 0


def _decode(seg, st, end, geo, dc, ac, store=None, trace=None):
    """The symbols that begin in [st's position, end) from state st -> (exit state or None, blocks completed, failed).  store:
    (coef per component, first block, is the last subsequence): the placing decode, which stops at the image's last block."""
    if st is None:
        return None, 0, True
    nc, hs, mw, nblk, bpm = geo
    pos, rr, k = st
    dpos, dend = seg.to_data(pos), seg.to_data(end) if end < seg.len * 8 else seg.nd * 8
    count, bad, fail, g = 0, False, False, 0
    if store is not None:
        coef, g, last = store
        fail = g % bpm != rr
    zz = J.ZIGZAG.tolist()

    def block(g, rr):
        m = g // bpm
        c = 0 if nc == 1 or rr < hs * hs else rr - hs * hs + 1
        hv, b = (hs, rr) if c == 0 else (1, 0)
        return coef[c][(m // mw) * hv + b // hv, (m % mw) * hv + b % hv]
    blk = block(g, rr) if store is not None and g < nblk else None
    while dpos < dend:
        if store is not None and g >= nblk:
            break
        c = 0 if nc == 1 or rr < hs * hs else rr - hs * hs + 1
        look = seg.peek(dpos, 16)
        at = dpos
        if k == 0:
            l, t = dc[c][0][look], dc[c][1][look]
            if l == 0 or t > 11:
                bad = True
                break
            v = R._extend(seg.peek(dpos + l, t), t)
            dpos += l + t
            if trace is not None:
                trace.append((seg.to_raw(at), seg.to_raw(at + l), seg.to_raw(dpos), "dc", t))
            if blk is not None:
                blk[0] = v
            k = 1
        else:
            l, rs = ac[c][0][look], ac[c][1][look]
            if l == 0:
                bad = True
                break
            run, size = rs >> 4, rs & 15
            if size == 0:
                dpos += l
                k = k + 16 if run == 15 else 64
                if trace is not None:
                    trace.append((seg.to_raw(at), seg.to_raw(dpos), seg.to_raw(dpos), "zrl" if run == 15 else "eob", rs))
            else:
                k += run
                if k > 63:
                    bad = True
                    break
                v = R._extend(seg.peek(dpos + l, size), size)
                dpos += l + size
                if trace is not None:
                    trace.append((seg.to_raw(at), seg.to_raw(at + l), seg.to_raw(dpos), "ac", rs))
                if blk is not None:
                    blk[zz[k]] = v
                k += 1
        if k >= 64:
            k, rr, count = 0, (rr + 1) % bpm, count + 1
            if store is not None:
                g += 1
                blk = block(g, rr) if g < nblk else None
    if store is not None:
        if bad or seg.marker or dpos > seg.nd * 8:
            fail = True
        if dpos < dend and (g < nblk or (dpos + 7) >> 3 < seg.nd):         # stopped at the last block with a whole byte left
            fail = True
        if last and g != nblk:
            fail = True
    return (None if bad else (seg.to_raw(dpos), rr, k)), count, fail


def entropy(data, meta, desc, subseq=None, trace=False):
    """(coefficients per component [bh, bw, 64] int32 -- None when the image is not the parallel stage's or the stage gave it up --,
    info) of one image of a packed batch.  info: eligible, gave_up, nsub, rounds (decode passes of step 1 + 2), decodes (subsequence
    decodes in them), unknown (guessed starts that met a bad code in round 0), symbols (trace=True: per symbol of the true decode the raw bit
    positions of its code, of its magnitude bits and of its end, its kind 'dc' / 'ac' / 'zrl' / 'eob' and the symbol), guesses (the
    guessed start positions), seg, dc0 (the table a guessed start reads first)."""
    S = J.SUBSEQ_BYTES if subseq is None else subseq
    data, meta = np.asarray(data, np.uint8), np.asarray(meta, np.int32)
    H, W, nc, hs = (int(v) for v in desc[:4])
    info = dict(eligible=False, gave_up=False, nsub=0, rounds=0, decodes=0, unknown=0, symbols=None)
    if int(desc[5]) != 1:
        return None, info
    off, length, first, count = (int(v) for v in meta[desc[4]:desc[4] + 4])
    mw, mh = -(-W // (8 * hs)), -(-H // (8 * hs))
    if length < 1 or length > MAXSUB * S or first != 0 or count != mw * mh:
        return None, info
    info["eligible"] = True
    per = [hs, 1, 1][:nc]
    bpm = hs * hs + 2 if nc == 3 else 1
    nblk = mw * mh * bpm
    geo = (nc, hs, mw, nblk, bpm)
    dc = [R._lut(meta[desc[9 + c]:desc[9 + c] + J.HUFF]) for c in range(nc)]
    ac = [R._lut(meta[desc[12 + c]:desc[12 + c] + J.HUFF]) for c in range(nc)]
    seg = _Segment(data[off:off + length])
    nsub = -(-length // S)
    ends = [min((i + 1) * S, length) * 8 for i in range(nsub)]
    # 1. guessed starts
    entry = [((i * S + (1 if i and seg.stuffed[i * S] else 0)) * 8, 0, 0) for i in range(nsub)]
    exit_, cnt, need = [None] * nsub, [0] * nsub, list(range(nsub))
    rounds = 0
    # 2. rounds
    while need and rounds < nsub:
        for i in need:
            exit_[i], cnt[i], _ = _decode(seg, entry[i], ends[i], geo, dc, ac)
        if rounds == 0:
            info["unknown"] = sum(e is None for e in exit_[:-1])
        rounds += 1
        info["decodes"] += len(need)
        need = [i for i in range(1, nsub) if exit_[i - 1] is not None and exit_[i - 1] != entry[i]]      # unknown tells nothing
        for i in need:
            entry[i] = exit_[i - 1]
    info.update(nsub=nsub, rounds=rounds, entry=list(entry), guesses=[(i * S + (1 if i and seg.stuffed[i * S] else 0)) * 8 for i in range(nsub)],
                seg=seg, dc0=dc[0])
    fail = bool(need) or any(e is None for e in entry)
    # 3. placement
    coef = [np.zeros((mh * h, mw * h, 64), np.int32) for h in per]
    firsts = np.concatenate([[0], np.cumsum(cnt)[:-1]]).tolist()
    symbols = [] if trace else None
    if not fail:
        for i in range(nsub):
            _, _, f = _decode(seg, entry[i], ends[i], geo, dc, ac, store=(coef, firsts[i], i == nsub - 1), trace=symbols)
            fail = fail or f
    # 4. DC
    if not fail:
        for c in range(nc):
            h = per[c]
            d = coef[c][:, :, 0]
            scan = d.reshape(mh, h, mw, h).transpose(0, 2, 1, 3).reshape(-1)            # MCU by MCU, its blocks in raster order
            pred = np.cumsum(scan.astype(np.int64))
            if pred.min(initial=0) < -32768 or pred.max(initial=0) > 32767:
                fail = True
            d[...] = pred.reshape(mh, mw, h, h).transpose(0, 2, 1, 3).reshape(mh * h, mw * h)
    info.update(gave_up=fail, symbols=symbols)
    return (None if fail else coef), info


def batch_entropy(batch, i, **kw):
    meta = batch.meta.numpy()
    return entropy(batch.data.numpy(), meta, meta[i * J.DESC:(i + 1) * J.DESC], **kw)


def properties(batch, i):
    """What image i of the batch exercises in the parallel stage, as a set of names:
    len_kS / len_kS1   the coded length is a multiple of SUBSEQ_BYTES / one byte more;
    short              shorter than one subsequence;
    ff00_split         a subsequence begins on the 00 of a stuffed FF 00;
    mid_code           a subsequence begins inside a Huffman code;
    mid_magnitude_valid  a subsequence begins inside magnitude bits, and what it reads there is a valid code of the guessed table;
    zrl_across         a ZRL symbol is the last of its subsequence: its run of zeros continues in the next;
    long_chain         32 rounds or more (a full-size video frame of 340 subsequences settles in 18)."""
    S = J.SUBSEQ_BYTES
    coef, info = batch_entropy(batch, i, trace=True)
    assert info["eligible"] and not info["gave_up"]
    seg, out = info["seg"], set()
    if seg.len % S == 0:
        out.add("len_kS")
    if seg.len % S == 1 and seg.len > S:
        out.add("len_kS1")
    if seg.len < S:
        out.add("short")
    if any(seg.stuffed[k] for k in range(S, seg.len, S)):
        out.add("ff00_split")
    if info["rounds"] >= 32:
        out.add("long_chain")
    sym = info["symbols"]
    starts = [s[0] for s in sym]
    for g in info["guesses"][1:]:
        u = int(np.searchsorted(starts, g, side="right")) - 1          # the symbol that holds bit g
        a, m, e, kind, _ = sym[u]
        if a < g < m:
            out.add("mid_code")
        if m < g < e:
            look = seg.peek(seg.to_data(g), 16)
            if info["dc0"][0][look] and info["dc0"][1][look] <= 11:
                out.add("mid_magnitude_valid")
    for u in range(len(sym) - 1):
        if sym[u][3] == "zrl" and (sym[u][0] >> 3) // S != (sym[u + 1][0] >> 3) // S:
            out.add("zrl_across")
    return out
