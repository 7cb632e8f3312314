"""The host half of the GPU JPEG decoder (adamml_amd/jpeg.py) and its numpy restatement (tests/jpeg_ref.py), no GPU needed: the
restatement equals Pillow's pixels byte for byte on every committed fixture and on a generated sweep when Pillow imports; `parse`
rejects what the kernel does not decode, naming the reason; the packed batch is aligned, complete and stores identical tables once;
damaged streams terminate in the CPU model with a status; EncodedFrames checks its files; the C ABI declares and exports the entry."""
import hashlib
import io
import os

import numpy as np
import pytest

from adamml_amd import abi, hip, jpeg as J, video as V
from tests import jpeg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"))
    return {k[:-4]: (z[k].tobytes(), z[k[:-4] + ".pixels"]) for k in z.files if k.endswith(".jpg")}


CASES = _cases()


def test_fixture_set_is_what_the_issue_lists():
    assert len(CASES) >= 12
    infos = {k: J.parse(f) for k, (f, _) in CASES.items()}
    assert {(i.channels, i.sampling) for i in infos.values()} == {(3, 2), (3, 1), (1, 1)}
    assert any(i.restart_interval for i in infos.values()) and any(len(i.segments) > 4 for i in infos.values())
    assert {(17, 33), (7, 5), (16, 16), (1, 1)} <= {(i.height, i.width) for i in infos.values()}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz")) < 300 * 1024


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_pillow_pixels_on_fixture(name):
    data, want = CASES[name]
    got = R.decode(data)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), "%d differing bytes" % int((got != want).sum())


def test_restatement_has_pillows_digest_on_the_frames_kept_without_pixels():
    """The full-size 256 x 341 frames and the frames of the small test videos: SHA-256 of Pillow's pixels, recorded with the files."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"))
    names = [k[:-6] for k in z.files if k.endswith(".frame")]
    assert len(names) >= 19 and {"full_256x341", "full_256x341_rst1"} <= set(names)
    for k in names:
        data = z[k + ".frame"].tobytes()
        if k.startswith("full"):
            inf = J.parse(data)
            assert (inf.height, inf.width, inf.sampling) == (256, 341, 2) and 30000 <= len(data) <= 50000
            assert len(inf.segments) == (16 if k.endswith("rst1") else 1)
        assert hashlib.sha256(np.ascontiguousarray(R.decode(data)).tobytes()).digest() == z[k + ".sha256"].tobytes(), k


def test_restatement_equals_pillow_on_a_generated_sweep():
    Image = pytest.importorskip("PIL.Image")
    n = 0
    for seed, (h, w, sub, quality, extra) in enumerate([
            (64, 80, 2, 90, {}), (37, 53, 2, 93, {}), (37, 53, 0, 75, {}), (41, 30, None, 95, {}), (48, 67, 2, 93, dict(restart_marker_rows=1)),
            (33, 47, 2, 100, dict(restart_marker_rows=2)), (16, 16, 0, 98, {}), (5, 7, 2, 60, {}), (1, 1, None, 80, {}), (9, 8, 0, 3, {}),
            (100, 100, 2, 93, dict(optimize=True)), (70, 90, 0, 93, dict(optimize=True, restart_marker_blocks=3)),
            (60, 75, None, 30, dict(optimize=True)), (256, 340, 2, 93, {})]):
        img = R.synth_image(100 + seed, h, w, 1 if sub is None else 3)
        b = io.BytesIO()
        Image.fromarray(img).save(b, "JPEG", quality=quality, **(dict(extra) if sub is None else dict(extra, subsampling=sub)))
        want = np.asarray(Image.open(io.BytesIO(b.getvalue())))
        got = R.decode(b.getvalue())
        assert np.array_equal(got, want), ((h, w, sub, quality, extra), int((got != want).sum()))
        n += 1
    # saturated black / white noise: every clamp of the IDCT and of the colour conversion is reached
    img = (np.random.default_rng(5).integers(0, 2, (40, 56, 3)) * 255).astype(np.uint8)
    for sub in (0, 2):
        b = io.BytesIO()
        Image.fromarray(img).save(b, "JPEG", quality=97, subsampling=sub)
        assert np.array_equal(R.decode(b.getvalue()), np.asarray(Image.open(io.BytesIO(b.getvalue()))))


# ---- parse ------------------------------------------------------------------------------------------------------------------------------

def _find(data, marker):
    """Offset of the first `FF marker` segment of the header."""
    i = 2
    while True:
        m, length = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        if m == marker:
            return i
        assert m != 0xDA, "marker %02X not found" % marker
        i += 2 + length


def _edit(data, marker, at, value):
    b = bytearray(data)
    b[_find(data, marker) + at] = value
    return bytes(b)


def _insert(data, segment_marker, body):
    seg = bytes([0xFF, segment_marker, (len(body) + 2) >> 8, (len(body) + 2) & 255]) + body
    return data[:2] + seg + data[2:]


def test_parse_reads_the_header():
    data, px = CASES["c420_q93_50x70_rst1"]
    inf = J.parse(data)
    assert (inf.height, inf.width, inf.channels, inf.sampling) == (50, 70, 3, 2)
    assert inf.mcus == (5, 4) and inf.restart_interval == 5 and len(inf.segments) == 4
    assert [c[1:3] for c in inf.components] == [(2, 2), (1, 1), (1, 1)]
    assert set(inf.huffman) == {(0, 0), (0, 1), (1, 0), (1, 1)} and set(inf.quant) == {0, 1}
    for (a, b), (a2, _) in zip(inf.segments, inf.segments[1:] + [(len(data), 0)]):
        assert data[b] == 0xFF and (0xD0 <= data[b + 1] <= 0xD7 or data[b + 1] == 0xD9) and a2 == b + 2
    grey = J.parse(CASES["grey_q93_41x30"][0])
    assert (grey.channels, grey.sampling, grey.mcus, grey.blocks) == (1, 1, (4, 6), 24)
    remux = J.parse(CASES["c420_q93_34x50_remux"][0])
    assert len(remux.huffman) == 4 and len(remux.quant) == 2
    assert b"JFIF" not in CASES["c420_q93_34x50_remux"][0][:64]


def test_parse_rejects_what_the_kernel_does_not_decode():
    data = CASES["c420_q93_48x67"][0]
    sof = 0xC0
    for what, bad in [
            ("progressive", _edit(data, sof, 1, 0xC2)), ("extended sequential", _edit(data, sof, 1, 0xC1)),
            ("arithmetic", _edit(data, sof, 1, 0xC9)), ("12-bit samples", _edit(data, sof, 4, 12)),
            ("16-bit quantisation", _edit(data, 0xDB, 4, 0x10)), ("chroma sampling 2x1", _edit(data, sof, 11, 0x21)),
            ("chroma sampling", _edit(data, sof, 14, 0x22)), ("size 67 x 0", _edit(_edit(data, sof, 5, 0), sof, 6, 0)),
            ("Adobe", _insert(data, 0xEE, b"Adobe\0d\0\0\0\0\0\1")), ("multiple scans", _edit(data, 0xDA, 4, 1)),
            ("missing Huffman table", _edit(data, 0xC4, 1, 0xFE)), ("missing quantisation table", _edit(data, sof, 12, 3)),
            ("not sequential", _edit(data, 0xDA, 12, 5)), ("truncated header", data[:40]), ("truncated header", data[:_find(data, 0xDA) + 3]),
            ("not a JPEG", b"\x89PNG" + data[4:]), ("entropy-coded segments", CASES["c420_q93_50x70_rst1"][0][:-600])]:
        with pytest.raises(J.Unsupported, match=what):
            J.parse(bad)
    with pytest.raises(J.Unsupported, match="above the cap of 1000 pixels"):
        J.parse(data, max_pixels=1000)
    # four components: the frame header of a CMYK file
    at = _find(data, sof)
    four = data[:at] + bytes([0xFF, sof, 0, 20, 8, 0, 48, 0, 67, 4, 1, 0x11, 0, 2, 0x11, 0, 3, 0x11, 0, 4, 0x11, 0]) + data[at + 19:]
    with pytest.raises(J.Unsupported, match="4 components"):
        J.parse(four)
    # RGB component ids without a JFIF header: libjpeg then does no colour transform
    rgb = bytearray(CASES["c420_q93_34x50_remux"][0])
    for marker, first, step in ((sof, 10, 3), (0xDA, 5, 2)):
        at = _find(bytes(rgb), marker)
        for k, ch in enumerate(b"RGB"):
            rgb[at + first + step * k] = ch
    with pytest.raises(J.Unsupported, match="'R', 'G', 'B'"):
        J.parse(bytes(rgb))
    assert issubclass(J.Unsupported, ValueError)


def test_parse_rejects_pillow_progressive_and_422():
    Image = pytest.importorskip("PIL.Image")
    img = Image.fromarray(R.synth_image(1, 40, 40))
    for kw, what in ((dict(progressive=True), "progressive"), (dict(subsampling=1), "chroma sampling 2x1"), (dict(), "4 components")):
        b = io.BytesIO()
        (img.convert("CMYK") if not kw else img).save(b, "JPEG", **kw)
        with pytest.raises(J.Unsupported, match=what):
            J.parse(b.getvalue())


# ---- Batch ------------------------------------------------------------------------------------------------------------------------------

def test_batch_layout_alignment_and_table_deduplication():
    names = sorted(CASES)
    files = [CASES[k][0] for k in names]
    b = J.Batch(files)
    meta, data = b.meta.numpy(), b.data.numpy()
    assert meta.dtype == np.int32 and data.dtype == np.uint8 and len(data) % 16 == 0
    nseg, blocks = 0, 0
    for i, f in enumerate(files):
        inf, d = b.infos[i], meta[i * J.DESC:(i + 1) * J.DESC]
        assert tuple(d[:4]) == (inf.height, inf.width, inf.channels, inf.sampling)
        assert d[4] == b.n * J.DESC + 4 * nseg and d[5] == len(inf.segments)
        assert (int(d[20]) | (int(d[21]) << 32)) == blocks
        assert d[15] % 16 == 0 and d[17] == inf.width * inf.channels and d[18] == inf.channels and d[19] == 0
        mcu = 0
        for s, (a, e) in enumerate(inf.segments):
            off, length, first, count = meta[d[4] + 4 * s:d[4] + 4 * s + 4]
            assert off % 16 == 0 and length == e - a and first == mcu and count >= 1
            assert data[off:off + length].tobytes() == f[a:e]                     # byte stuffing left in place
            mcu += count
        assert mcu == inf.mcus[0] * inf.mcus[1]
        for c, comp in enumerate(inf.components):
            assert np.array_equal(meta[d[6 + c]:d[6 + c] + 64], inf.quant[comp[3]])
            bits, vals = inf.huffman[(1, comp[5])]
            t = meta[d[12 + c]:d[12 + c] + J.HUFF]
            assert np.array_equal(t[:16], bits) and np.array_equal(t[16:].view(np.uint8)[:len(vals)], vals)
        nseg += len(inf.segments)
        blocks += inf.blocks
    assert b.total_blocks == blocks
    # identical tables once: the same file 20 times adds descriptors and segment records only
    one, many = J.Batch(files[:1]), J.Batch(files[:1] * 20)
    per_image = J.DESC + 4 * len(one.infos[0].segments)
    assert many.meta.numel() - one.meta.numel() == 19 * per_image
    std = [k for k in names if "opt" not in k and k.startswith("c420_q93")]
    b2 = J.Batch([CASES[k][0] for k in std])
    d = b2.meta.numpy()[:b2.n * J.DESC].reshape(b2.n, J.DESC)
    assert (d[:, 6:15] == d[0, 6:15]).all()                                      # one copy of the standard tables and of quality 93
    with pytest.raises(ValueError, match="empty batch"):
        J.Batch([])
    with pytest.raises(ValueError, match="outside the"):
        J.Batch(files[:1], [J.Placement(0, 67 * 3, 3, 0)], 100)
    assert repr(b).startswith("jpeg.Batch(N=%d" % len(files))


def test_interleaved_placement_in_the_cpu_model():
    """Three 4:2:0 frames of one size as channels 0-2, 3-5, 6-8 of one [H, W, 9] array, and greyscale files as single channels."""
    Image = pytest.importorskip("PIL.Image")
    files = []
    for s in range(3):
        b = io.BytesIO()
        Image.fromarray(R.synth_image(30 + s, 24, 40)).save(b, "JPEG", quality=90)
        files.append(b.getvalue())
    batch = J.Batch(files, [J.Placement(0, 40 * 9, 9, 3 * j) for j in range(3)], 24 * 40 * 9)
    y, status = R.decode_packed(batch.data.numpy(), batch.meta.numpy(), 3, batch.out_bytes)
    assert not status.any()
    y = y.reshape(24, 40, 9)
    for j, f in enumerate(files):
        assert np.array_equal(y[:, :, 3 * j:3 * j + 3], np.asarray(Image.open(io.BytesIO(f))))


@pytest.mark.parametrize("kind", ["cut", "ff", "zero", "tail0"])
def test_damaged_streams_end_with_a_status_in_the_cpu_model(kind):
    names = sorted(CASES)
    b = J.Batch([CASES[k][0] for k in names])
    clean, st = R.decode_packed(b.data.numpy(), b.meta.numpy(), b.n, b.out_bytes)
    assert not st.any()
    for i in (names.index("c420_q93_48x67"), names.index("grey_q93_41x30"), names.index("c420_q93_50x70_rst1"), names.index("c444_q93_30x41_rst2")):
        data, meta = R.damage(b, i, kind)
        y, st = R.decode_packed(data, meta, b.n, b.out_bytes)
        assert st[i] != 0 and not np.delete(st, i).any(), (kind, names[i], st)
        for j in range(b.n):
            assert np.array_equal(b.image(y, j), b.image(clean, j)) == (j != i), (kind, names[i], j)


# ---- EncodedFrames ----------------------------------------------------------------------------------------------------------------------

def test_encoded_frames_checks_its_files():
    colour, grey = CASES["c420_q93_48x67"][0], CASES["grey_q93_41x30"][0]
    g = V.Augmentor(False, 32, disable_scaleup=True).sample(67, 48)
    ef = V.EncodedFrames([[colour, colour], [colour, colour]], [g, g])
    assert ef.shape == (2, 32, 32, 6) and (ef.k_in, ef.k_out, ef.modality) == (6, 6, "rgb") and ef.batch.n == 4
    d = ef.meta.numpy()[:20].reshape(2, 10)
    assert (d[:, 2:5] == (48, 67, 67 * 6)).all() and d[1, 0] == (48 * 67 * 6 + 15) // 16 * 16
    assert [(p.offset, p.row_stride, p.pixel_stride, p.channel) for p in ef.batch.placements[2:]] == [(d[1, 0], 67 * 6, 6, 0), (d[1, 0], 67 * 6, 6, 3)]
    with pytest.raises(ValueError, match="video 0, file 1 is 50 x 34 but the geometry was sampled for 67 x 48"):
        V.EncodedFrames([[colour, CASES["c420_q93_34x50_remux"][0]]], [g])
    with pytest.raises(ValueError, match="has 1 components, the rgb modality"):
        V.EncodedFrames([[grey]], [V.Augmentor(False, 24, disable_scaleup=True).sample(30, 41)])
    gf = V.Augmentor(False, 24, disable_scaleup=True, modality="flow").sample(30, 41)
    assert V.EncodedFrames([[grey] * 4], [gf]).k_in == 4
    with pytest.raises(ValueError, match="has 3 components, the flow modality"):
        V.EncodedFrames([[colour]], [V.Augmentor(False, 32, disable_scaleup=True, modality="flow").sample(67, 48)])
    with pytest.raises(ValueError, match="video 1 has 1 files, video 0 2"):
        V.EncodedFrames([[colour, colour], [colour]], [g, g])
    with pytest.raises(J.Unsupported, match="video 0, file 1: progressive"):
        V.EncodedFrames([[colour, _edit(colour, 0xC0, 1, 0xC2)]], [g])
    with pytest.raises(ValueError, match="rgbdiff needs"):
        V.EncodedFrames([[colour] * 5], [V.Augmentor(False, 32, disable_scaleup=True, modality="rgbdiff").sample(67, 48)])
    with pytest.raises(ValueError, match="1 videos but 2 geometries"):
        V.EncodedFrames([[colour]], [g, g])
    with pytest.raises(TypeError, match="expected Augmentor.sample's Geometry"):
        V.EncodedFrames([[colour]], [dict(g.params)])


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_jpeg_decode():
    declared = abi.FUNCTIONS
    assert str(declared["adamml_jpeg_decode_u8"]) == (
        "int adamml_jpeg_decode_u8(const uint8_t* src, int64_t src_bytes, const int32_t* meta, int meta_len, "
        "uint8_t* y, int64_t y_bytes, int32_t* status, void* workspace, int64_t workspace_bytes, int N, hipStream_t stream)")
    assert str(declared["adamml_jpeg_decode_workspace"]) == "size_t adamml_jpeg_decode_workspace(int64_t total_blocks)"
    lib = hip.load()
    assert hasattr(lib, "adamml_jpeg_decode_u8") and hasattr(lib, "adamml_jpeg_decode_workspace")
    assert lib.adamml_jpeg_decode_workspace(10) == 1920 and lib.adamml_jpeg_decode_workspace(0) == 0
    assert "adamml_jpeg_decode_u8" in hip.SIGNATURES and len(hip.SIGNATURES["adamml_jpeg_decode_u8"]) == 11
