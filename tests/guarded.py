"""Guard-banded allocations for the float64 conformance modules: every buffer a row hands to a kernel comes from one Scope.

    out(shape, dtype)     an output: a view into a larger allocation, the interior pre-filled with NaN (floating types) or the byte
                          INTERIOR_BYTE (integer types), a band of BAND_BYTE on both sides
    inout(base)           the same layout, the interior initialised from `base` (accumulating outputs, dw, statistic accumulators,
                          optimizer state: every non-const pointer that is read as well as written)
    workspace(nbytes)     exactly nbytes bytes of 0xFF inside the same kind of band (fill() re-fills the interior)
    frozen(tensor)        a read-only operand: uploaded, and a second copy kept to compare with
    check(what)           every band still holds its sentinel, every NaN-filled interior is fully written (unless the row said
                          written=False), every frozen operand is bit for bit what was uploaded
    untouched(t)          the whole allocation behind t is as it was handed out (an unsupported or refused call must not write)

Band size (band_bytes): the largest of 128 rows of the buffer's innermost row, STORE_TILE_BYTES and 4096 bytes, rounded up to a multiple
of 256 bytes, on both sides; the interior starts `band` bytes into a fresh allocation (so as aligned as one) and ends at exactly its own
byte size.  128 rows is one pixel tile of conv_gemm_kernel (BP = 128) and four of the streaming kernels: a ragged last pixel tile stored
unpredicated, or a per-group stride off by one row block, lands in the band.  STORE_TILE_BYTES covers the cases where one workgroup's
store step is larger than 128 innermost rows (narrow rows: a [C][3][3] depthwise dw, a [G][C] vector, a workspace):

    conv_gemm_kernel (conv_gemm.hip)                  BP x BC = 128 pixels x at most 128 channels, bf16                     32 KiB
    conv_wgrad_glds_kernel<256,128> / <128,256>       one 256 x 128 float32 tile of a partial (conv_wgrad.hip)              128 KiB
    conv3x3_c64_wgrad_kernel (conv3x3_c64.hip)        one [64][9][64] float32 quadrant of a partial per workgroup           144 KiB
    gram_colsum_kernel<256> (gram.hip)                one partial of C * C + C float32 per workgroup                        257 KiB
    res_prod_stream_kernel, tpool_bwd_prod_kernel     one [256][64] float32 partial per workgroup                            64 KiB
    conv_gemm_kernel<128,RES,EID,PF>                  one [128][64] float32 partial per workgroup                            32 KiB
    dwconv weight-gradient kernels                    one [9][C] float32 partial per workgroup, C <= 2048                    72 KiB
    conv_stem_wgrad_kernel (conv_stem.hip)            one [64][KTOT = 224] float32 partial per workgroup                     56 KiB
    streaming 1x1 kernels (TPX = 32 pixels)           32 pixels x at most 512 channels, bf16                                 32 KiB
    row walkers, pools, optimizers, packs             256 threads x 16 bytes per step                                         4 KiB

so STORE_TILE_BYTES = (256 * 256 + 256) * 4, the largest of them (a statistic accumulator row, [2C] float64, is bounded by the 128-row
term: 128 rows are four groups' worth of STAT_SLOTS = 32 slots).  Nothing here depends on the device: tests/test_guarded_cpu.py plants
each defect on the CPU."""
import torch

BAND_ROWS = 128
STORE_TILE_BYTES = (256 * 256 + 256) * 4
MIN_BAND_BYTES = 4096
BAND_BYTE = 0xA5          # sentinel of the bands
INTERIOR_BYTE = 0x5A      # pre-fill of an integer output
WS_BYTE = 0xFF            # pre-fill of a workspace (a NaN in every float32 / float64 / bf16 lane)


def band_bytes(row_bytes):
    b = max(BAND_ROWS * row_bytes, STORE_TILE_BYTES, MIN_BAND_BYTES)
    return (b + 255) // 256 * 256


def _bytes(t):
    """the bytes of a contiguous tensor, 1-D"""
    return t.reshape(-1).view(torch.uint8)


class _Buf:
    def __init__(self, name, kind):
        self.name, self.kind = name, kind
        self.full = self.t = self.init = self.ref = None
        self.band = self.nbytes = 0
        self.nan_filled = self.must_write = False
        self.fill = None

    def sides(self):
        return (("front", self.full[:self.band]), ("back", self.full[self.band + self.nbytes:]))

    def interior(self):
        return self.full[self.band:self.band + self.nbytes]

    def bands(self):
        """both bands as one [2, band] view (one comparison covers them)"""
        return self.full.as_strided((2, self.band), (self.band + self.nbytes, 1))


class Scope:
    def __init__(self, device):
        self.device = device
        self.bufs = []

    def reset(self):
        self.bufs = []

    # ---------------------------------------------------------------------------------------------------------------- allocation
    def _alloc(self, name, kind, shape, dtype):
        shape = tuple(int(s) for s in shape)
        item = torch.empty(0, dtype=dtype).element_size()
        n = 1
        for s in shape:
            n *= s
        b = _Buf(name or "%s#%d %s%s" % (kind, len(self.bufs), str(dtype).replace("torch.", ""), list(shape)), kind)
        b.nbytes = n * item
        b.band = band_bytes((shape[-1] if shape else 1) * item)
        b.full = torch.full((2 * b.band + b.nbytes,), BAND_BYTE, dtype=torch.uint8, device=self.device)
        b.t = b.interior().view(dtype).view(shape)
        self.bufs.append(b)
        return b

    def out(self, shape, dtype, name=None, written=True):
        b = self._alloc(name, "out", shape, dtype)
        if dtype.is_floating_point:
            b.t.fill_(float("nan"))
            b.nan_filled, b.must_write = True, written
        else:
            b.interior().fill_(INTERIOR_BYTE)
        return b.t

    def inout(self, base, name=None):
        b = self._alloc(name, "inout", base.shape, base.dtype)
        b.t.copy_(base)
        b.init = b.interior().clone()
        return b.t

    def zeros(self, shape, dtype, name=None):
        """an in/out buffer that starts at zero (a statistic accumulator), filled on the device"""
        b = self._alloc(name, "inout", shape, dtype)
        b.interior().zero_()
        b.init = b.interior().clone()
        return b.t

    def workspace(self, nbytes, name=None, fill=WS_BYTE):
        b = self._alloc(name or "workspace#%d [%d bytes]" % (len(self.bufs), nbytes), "workspace", (nbytes,), torch.uint8)
        b.fill = fill
        b.interior().fill_(fill)
        return b.t

    def fill(self, ws, byte):
        """re-fill the interior of a workspace"""
        b = self.buf(ws)
        assert b.kind == "workspace"
        b.fill = byte
        b.interior().fill_(byte)

    def frozen(self, tensor, name=None):
        """upload a read-only operand (a tensor already on the device is taken as it is)"""
        if tensor is None:
            return None
        b = _Buf(name or "frozen#%d %s%s" % (len(self.bufs), str(tensor.dtype).replace("torch.", ""), list(tensor.shape)), "frozen")
        b.t = tensor.contiguous().to(self.device)
        if b.t.device.type == "cpu" and b.t.data_ptr() == tensor.data_ptr():
            b.t = b.t.clone()                    # (on the CPU: never the caller's own tensor, which its reference still reads)
        b.ref = b.t.clone()
        self.bufs.append(b)
        return b.t

    def buf(self, t):
        for b in self.bufs:
            if b.t is t or (b.t.data_ptr() == t.data_ptr() and b.t.numel() == t.numel() and b.t.dtype == t.dtype):
                return b
        raise KeyError("not a tensor of this scope")

    def unwritten_ok(self, *tensors):
        """the row says that these NaN-filled outputs need not be fully written (a refused call, a NaN that propagates)"""
        for t in tensors:
            self.buf(t).must_write = False

    def written_required(self, *tensors):
        for t in tensors:
            b = self.buf(t)
            b.must_write = b.nan_filled

    # --------------------------------------------------------------------------------------------------------------------- checks
    def _flags(self, b, good, bad):
        """device flags: every entry of `good` must be true, every entry of `bad` false"""
        if b.kind == "frozen":
            good.append((_bytes(b.t) == _bytes(b.ref)).all())
            return
        good.append((b.bands() == BAND_BYTE).all())
        if b.must_write:
            bad.append(torch.isnan(b.t).any())

    def _describe(self, b):
        """the slow path: what is wrong with b, or None"""
        if b.kind == "frozen":
            bad = (_bytes(b.t) != _bytes(b.ref)).nonzero()
            if bad.numel():
                return "read-only operand %s modified: %d bytes differ, the first at byte offset %d" % (b.name, bad.numel(), int(bad[0]))
            return None
        for side, s in b.sides():
            bad = (s != BAND_BYTE).nonzero()
            if bad.numel():
                off = int(bad[0]) if side == "back" else int(bad[0]) - b.band
                where = "%d bytes past its end" % off if side == "back" else "%d bytes before its start" % -off
                return "guard band of %s written: %s band, %d bytes, the first %s" % (b.name, side, bad.numel(), where)
        if b.must_write:
            n = int(torch.isnan(b.t).sum())
            if n:
                return "%s: %d of %d elements never written, the first at flat index %d" % (
                    b.name, n, b.t.numel(), int(torch.isnan(b.t).reshape(-1).nonzero()[0]))
        return None

    def check(self, what=""):
        """one device reduction when everything holds; the messages come from a second, slow pass"""
        good, bad = [], []
        for b in self.bufs:
            self._flags(b, good, bad)
        ok = torch.stack(good).all() if good else None
        if bad:
            nb = ~torch.stack(bad).any()
            ok = nb if ok is None else ok & nb
        if ok is None or bool(ok):
            return
        msgs = [m for m in (self._describe(b) for b in self.bufs) if m]
        raise AssertionError((what + ": " if what else "") + "; ".join(msgs))

    def untouched(self, t):
        b = self.buf(t)
        if b.kind == "frozen":
            return bool((_bytes(b.t) == _bytes(b.ref)).all())
        if not all(bool((s == BAND_BYTE).all()) for _, s in b.sides()):
            return False
        if b.kind == "inout":
            return bool((b.interior() == b.init).all())
        if b.kind == "workspace":
            return bool((b.interior() == b.fill).all())
        return bool(torch.isnan(b.t).all()) if b.nan_filled else bool((b.interior() == INTERIOR_BYTE).all())


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((_bytes(a.contiguous()) == _bytes(b.contiguous())).all())


def workspace_launches(scope, q, make, launch, short, what, sync=None):
    """The three launches of a workspace-taking row.  make() -> a tuple of fresh guarded outputs; launch(outs, ws, nbytes) calls the entry
    point (ws: the uint8 workspace tensor).  exact: workspace(q), workspace_bytes = q; dirty: the same launch on a workspace of 0x00
    instead of 0xFF, outputs bit-identical; short: workspace_bytes = q - 4 with the same buffer: short == "refuse": RuntimeError, outputs
    and workspace untouched; short == "fallback": the launch runs without the workspace, which stays untouched.  Each launch gets its own
    check.  Returns (outputs of the exact launch, outputs of the short launch or None)."""
    assert q > 0, what + ": the workspace query answers 0: the row would not test the workspace path"
    assert short in ("refuse", "fallback")
    ws = scope.workspace(q, name=what + " workspace")
    first = make()
    launch(first, ws, q)
    scope.check(what + " exact")
    scope.fill(ws, 0x00)
    second = make()
    launch(second, ws, q)
    scope.check(what + " dirty")
    for i, (a, b) in enumerate(zip(first, second)):
        assert same_bits(a, b), "%s: output %d depends on what the workspace held before" % (what, i)
    scope.fill(ws, WS_BYTE)
    third = make()
    if short == "fallback":
        launch(third, ws, q - 4)
        scope.check(what + " short")
        assert scope.untouched(ws), what + ": workspace_bytes one float short, and the workspace was written"
        return first, third
    try:
        launch(third, ws, q - 4)
    except RuntimeError:
        pass
    else:
        raise AssertionError(what + ": workspace_bytes one float short was not refused")
    if sync is not None:
        sync()
    for i, t in enumerate(third):
        assert scope.untouched(t), "%s: refused, but output %d was written" % (what, i)
    assert scope.untouched(ws), what + ": refused, but the workspace was written"
    scope.unwritten_ok(*[t for t in third if scope.buf(t).nan_filled])
    scope.check(what + " short")
    return first, None
