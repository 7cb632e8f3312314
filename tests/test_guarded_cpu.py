"""tests/guarded.py catches planted defects (on the CPU: the helper takes the device as an argument).  Every "kernel" here is a plain
tensor write through the address arithmetic a kernel would use: an index relative to the interior's first element."""
import pytest
import torch

from tests import guarded as Gd

DTYPES = [torch.bfloat16, torch.float32, torch.float64, torch.uint8, torch.int16, torch.int32]


def raw(scope, t):
    """the whole allocation behind t as elements of t's dtype, and the index of t's first element in it"""
    b = scope.buf(t)
    return b.full.view(t.dtype), b.band // t.element_size()


def write_all(t):
    t.copy_(torch.arange(t.numel()).reshape(t.shape) % 7)


def test_band_is_the_largest_term_rounded_to_256_bytes():
    assert Gd.band_bytes(2) == Gd.STORE_TILE_BYTES                       # a narrow row: the store tile decides
    assert Gd.band_bytes(4096 * 8) == 128 * 4096 * 8                     # a statistic accumulator row: 128 rows decide
    assert Gd.band_bytes(2 * 3001) == (128 * 2 * 3001 + 255) // 256 * 256 and Gd.band_bytes(2 * 3001) % 256 == 0
    assert Gd.STORE_TILE_BYTES >= Gd.MIN_BAND_BYTES == 4096


@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).replace("torch.", "") for d in DTYPES])
def test_layout_and_clean_run(dtype):
    s = Gd.Scope("cpu")
    t = s.out((37, 24), dtype, name="y")
    b = s.buf(t)
    assert t.shape == (37, 24) and t.dtype == dtype and t.is_contiguous()
    assert b.band % 256 == 0 and b.band == Gd.band_bytes(24 * t.element_size())
    assert b.full.numel() == 2 * b.band + 37 * 24 * t.element_size()      # the interior ends at exactly its own byte size
    assert t.data_ptr() == b.full.data_ptr() + b.band
    assert s.untouched(t)
    if dtype.is_floating_point:
        assert torch.isnan(t).all()
    else:
        assert (b.interior() == Gd.INTERIOR_BYTE).all()
    write_all(t)
    s.check("clean")
    assert not s.untouched(t)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float64, torch.int16], ids=["bfloat16", "float64", "int16"])
@pytest.mark.parametrize("where", ["one-before", "one-after", "one-band-after"])
def test_write_outside_the_interior_fails_by_name(dtype, where):
    s = Gd.Scope("cpu")
    other = s.out((5, 8), torch.float32, name="neighbour")
    t = s.out((33, 16), dtype, name="dx")
    write_all(other)
    write_all(t)
    full, first = raw(s, t)
    band = s.buf(t).band // t.element_size()
    i = {"one-before": first - 1, "one-after": first + t.numel(), "one-band-after": first + t.numel() + band - 1}[where]
    full[i] = 1
    side = "front" if where == "one-before" else "back"
    with pytest.raises(AssertionError, match=r"row 7: guard band of dx written: %s band" % side) as e:
        s.check("row 7")
    assert "neighbour" not in str(e.value)
    off = {"one-before": "%d bytes before its start" % t.element_size(), "one-after": "the first 0 bytes past its end",
           "one-band-after": "the first %d bytes past its end" % ((band - 1) * t.element_size())}[where]
    assert off in str(e.value), str(e.value)
    assert not s.untouched(t) and s.untouched(s.workspace(16))


def test_write_into_a_frozen_operand_fails_by_name():
    s = Gd.Scope("cpu")
    x = torch.randn(9, 8).to(torch.bfloat16)
    x[3, 3] = float("nan")                                               # (bit for bit: a NaN operand compares equal to itself)
    xd = s.frozen(x.clone(), name="bn_vec")
    m = s.frozen(torch.arange(12, dtype=torch.uint8), name="mask")
    s.check("clean")
    assert s.untouched(xd)
    xd[8, 7] = xd[8, 7] + 1
    with pytest.raises(AssertionError, match=r"read-only operand bn_vec modified: .* the first at byte offset %d" % ((8 * 8 + 7) * 2)):
        s.check()
    xd.copy_(x)
    s.check()
    m[11] ^= 1
    with pytest.raises(AssertionError, match="read-only operand mask modified"):
        s.check()
    assert s.frozen(None) is None


def test_frozen_minus_zero_is_a_change():
    s = Gd.Scope("cpu")
    z = s.frozen(torch.zeros(4), name="z")
    z[2] = -0.0
    with pytest.raises(AssertionError, match="operand z modified"):
        s.check()


def test_write_into_the_last_byte_of_a_workspace_rear_band_fails():
    s = Gd.Scope("cpu")
    ws = s.workspace(1000, name="wgrad workspace")
    b = s.buf(ws)
    assert ws.numel() == 1000 and ws.dtype == torch.uint8 and (ws == 0xFF).all() and b.full.numel() == 1000 + 2 * b.band
    ws.fill_(3)                                                          # the interior is the kernel's
    s.check()
    b.full[-1] = 0
    with pytest.raises(AssertionError, match=r"guard band of wgrad workspace written: back band, 1 bytes, the first %d bytes past" % (b.band - 1)):
        s.check()


def test_workspace_fill_and_untouched():
    s = Gd.Scope("cpu")
    ws = s.workspace(64)
    assert s.untouched(ws)
    s.fill(ws, 0x00)
    assert (ws == 0).all() and s.untouched(ws)
    ws[63] = 1
    assert not s.untouched(ws)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.float64], ids=["bfloat16", "float32", "float64"])
def test_interior_element_left_unwritten_fails(dtype):
    s = Gd.Scope("cpu")
    t = s.out((10, 8), dtype, name="y")
    write_all(t)
    t[9, 7] = float("nan")
    with pytest.raises(AssertionError, match=r"y: 1 of 80 elements never written, the first at flat index 79"):
        s.check()
    s.unwritten_ok(t)                                                    # unless the row says otherwise
    s.check()
    u = s.out((3,), dtype, name="u", written=False)
    s.check()
    assert s.untouched(u)


def test_inout_interior_may_be_overwritten_but_not_its_bands():
    s = Gd.Scope("cpu")
    base = torch.randn(6, 5)
    dw = s.inout(base, name="dw")
    assert torch.equal(dw, base) and s.untouched(dw)
    dw += 1.0
    s.check()
    assert not s.untouched(dw)
    nanbase = torch.full((4, 4), float("nan"))
    c = s.inout(nanbase, name="strided c")                               # an in/out buffer may hold NaN: nothing says it is written
    s.check()
    assert s.untouched(c)
    full, first = raw(s, dw)
    full[first + dw.numel()] = 0.0
    with pytest.raises(AssertionError, match="guard band of dw written: back band"):
        s.check()


def test_zeros_is_an_inout_buffer_filled_on_the_device():
    s = Gd.Scope("cpu")
    z = s.zeros((3, 32, 16), torch.float64, name="sums")
    assert z.shape == (3, 32, 16) and not z.any() and s.untouched(z)
    z[2, 31, 15] = 1.0
    s.check()
    assert not s.untouched(z)
    full, first = raw(s, z)
    full[first - 1] = 1.0
    with pytest.raises(AssertionError, match="guard band of sums written: front band"):
        s.check()


def test_several_defects_are_all_named():
    s = Gd.Scope("cpu")
    a, b = s.out((4, 4), torch.float32, name="a"), s.out((4, 4), torch.uint8, name="b")
    f = s.frozen(torch.ones(3), name="f")
    full, first = raw(s, b)
    full[first - 1] = 0
    f[0] = 2
    with pytest.raises(AssertionError) as e:
        s.check("row")
    msg = str(e.value)
    assert "a: 16 of 16 elements never written" in msg and "guard band of b written: front band" in msg and "operand f modified" in msg
    s.reset()
    s.check()


def test_workspace_launches_exact_dirty_short():
    """the three launches against toy entry points: a good one, one that reads its workspace before writing it, one that does not refuse
    an undersized workspace, one that writes before refusing"""
    q = 64

    def entry(reads_dirty=False, refuses=True, writes_first=False):
        def launch(outs, ws, nbytes):
            if writes_first:
                ws[0] = 1
            if nbytes < q:
                if refuses:
                    raise RuntimeError("workspace too small")
                outs[0].fill_(5.0)                                       # the fallback: no workspace
                return
            before = float(ws[5]) if reads_dirty else 0.0
            ws.fill_(2)
            outs[0].fill_(before + float(ws[0]) + 3.0)
        return launch

    def run(launch, short):
        s = Gd.Scope("cpu")
        return Gd.workspace_launches(s, q, lambda: (s.out((4,), torch.float32, name="y"),), launch, short, "toy")

    first, third = run(entry(), "refuse")
    assert (first[0] == 5.0).all() and third is None
    first, third = run(entry(refuses=False), "fallback")
    assert (third[0] == 5.0).all()
    with pytest.raises(AssertionError, match="depends on what the workspace held before"):
        run(entry(reads_dirty=True), "refuse")
    with pytest.raises(AssertionError, match="one float short was not refused"):
        run(entry(refuses=False), "refuse")
    with pytest.raises(AssertionError, match="refused, but the workspace was written"):
        run(entry(writes_first=True), "refuse")
    with pytest.raises(AssertionError, match="query answers 0"):
        s = Gd.Scope("cpu")
        Gd.workspace_launches(s, 0, lambda: (), entry(), "refuse", "toy")
