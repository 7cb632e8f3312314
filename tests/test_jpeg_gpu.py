"""The JPEG decoder on the GPU (adamml_jpeg_decode_u8, adamml_amd.jpeg / video.EncodedFrames) against the numpy restatement
(tests/jpeg_ref.py, itself byte-exact to Pillow: tests/test_jpeg_cpu.py), zero differing bytes everywhere: every fixture in ONE
batch, full-size frames, interleaved placement, augment(EncodedFrames) == augment(Frames) in every mode and modality, AdaMML fed
either, argument checks, and damaged streams (status + exactly the CPU model's pixels, the other images untouched).  Needs no Pillow:
the encoded inputs are the committed fixtures."""
import hashlib
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from adamml_amd import adamml, hip, jpeg as J, runtime, synth, video as V  # noqa: E402
from tests import jpeg_ref as R  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"))
NAMES = sorted(k[:-4] for k in Z.files if k.endswith(".jpg"))
FILES = {k: Z[k + ".jpg"].tobytes() for k in NAMES}
FRAMES = {k[:-6]: Z[k].tobytes() for k in Z.files if k.endswith(".frame")}          # full-size frames and the frames of test videos


def _gpu(batch, data=None, meta=None):
    dev = batch.to(DEV)
    if data is not None:
        dev.data, dev.meta = torch.from_numpy(data).to(DEV), torch.from_numpy(meta).to(DEV)
    y, status = J.decode(dev)
    torch.cuda.synchronize()
    return y.cpu().numpy(), status.cpu().numpy()


def test_every_fixture_in_one_batch_equals_the_restatement_and_pillow():
    b = J.Batch([FILES[k] for k in NAMES], pin_memory=True)
    want, wst = R.decode_packed(b.data.numpy(), b.meta.numpy(), b.n, b.out_bytes)
    got, st = _gpu(b)
    assert not wst.any() and not st.any(), st
    for i, k in enumerate(NAMES):
        diff = int((b.image(got, i) != b.image(want, i)).sum())
        print("  %-24s %d differing bytes" % (k, diff))
        assert diff == 0, k
        assert np.array_equal(b.image(got, i), Z[k + ".pixels"]), k                # Pillow's own pixels
    assert np.array_equal(got, want)                                               # the alignment gaps stay zero


def _grow(data, height):
    """The restart-per-MCU-row fixture with its MCU rows repeated up to `height` (width unchanged): each row restarts the DC
    prediction, so the result is a valid baseline stream of any height."""
    inf = J.parse(data)
    rows = -(-height // 16)
    sof = data.index(b"\xff\xc0")
    head = bytearray(data[:inf.segments[0][0]])
    head[sof + 5], head[sof + 6] = height >> 8, height & 255
    body = b"".join(data[a:b] + bytes([0xFF, 0xD0 + (r % 8)])
                    for r, (a, b) in ((r, inf.segments[r % len(inf.segments)]) for r in range(rows)))
    return bytes(head) + body[:-2] + b"\xff\xd9"


def test_full_size_frames_equal_the_restatement():
    files = [FRAMES["full_256x341"], FRAMES["full_256x341_rst1"]] * 2 + [_grow(FILES["c420_q93_50x70_rst1"], 1100), FRAMES["full_256x341"]]
    b = J.Batch(files)
    assert [(i.height, i.width) for i in b.infos[:2]] == [(256, 341)] * 2 and [len(i.segments) for i in b.infos[:2]] == [1, 16]
    want, wst = R.decode_packed(b.data.numpy(), b.meta.numpy(), b.n, b.out_bytes)
    got, st = _gpu(b)
    assert not wst.any() and not st.any(), st
    for i in range(b.n):
        diff = int((b.image(got, i) != b.image(want, i)).sum())
        print("  %s: %d differing bytes" % (b.infos[i], diff))
        assert diff == 0
    for i, k in enumerate(("full_256x341", "full_256x341_rst1")):                   # Pillow's pixels, by their recorded digest
        assert hashlib.sha256(np.ascontiguousarray(b.image(got, i)).tobytes()).digest() == Z[k + ".sha256"].tobytes()


def test_interleaved_output_equals_the_per_frame_decode():
    """The frames of a video at channel offsets 0, 3, 6, ... of one [H, W, K] array (greyscale files at 0, 1, 2, ...)."""
    for name, ch, count in (("c420_q93_48x67", 3, 4), ("c444_q50_37x53", 3, 3), ("grey_q93_41x30", 1, 5)):
        inf = J.parse(FILES[name])
        single, st = _gpu(J.Batch([FILES[name]]))
        assert not st.any()
        px = single[:inf.height * inf.width * ch].reshape(inf.height, inf.width, ch)
        k = ch * count
        places = [J.Placement(32, inf.width * k, k, ch * j) for j in range(count)]
        got, st = _gpu(J.Batch([FILES[name]] * count, places, 32 + inf.height * inf.width * k))
        assert not st.any() and not got[:32].any()
        got = got[32:].reshape(inf.height, inf.width, k)
        for j in range(count):
            assert np.array_equal(got[:, :, ch * j:ch * (j + 1)], px), (name, j)


@pytest.mark.parametrize("kind", ["cut", "ff", "zero", "tail0"])
def test_damaged_streams_return_a_status_and_the_cpu_models_pixels(kind):
    b = J.Batch([FILES[k] for k in NAMES])
    clean, _ = R.decode_packed(b.data.numpy(), b.meta.numpy(), b.n, b.out_bytes)
    for name in ("c420_q93_48x67", "grey_q93_41x30", "c420_q93_50x70_rst1", "c444_q93_30x41_rst2"):
        i = NAMES.index(name)
        data, meta = R.damage(b, i, kind)
        want, wst = R.decode_packed(data, meta, b.n, b.out_bytes)        # the CPU model first: it ends with a status
        assert wst[i] != 0
        got, st = _gpu(b, data, meta)
        print("  %-5s %-24s status %d (model %d)" % (kind, name, st[i], wst[i]))
        assert np.array_equal(st, wst), (kind, name, st, wst)
        assert np.array_equal(got, want), (kind, name, int((got != want).sum()))
        for j in range(b.n):
            if j != i:
                assert np.array_equal(b.image(got, j), b.image(clean, j)), (kind, name, j)


def test_two_runs_are_identical_and_out_buffer_is_reused():
    b = J.Batch([FILES[k] for k in NAMES]).to(DEV)
    y1, s1 = J.decode(b)
    out = torch.full_like(y1, 7)
    y2, s2 = J.decode(b, out=out)
    assert y2 is out and torch.equal(s1, s2)
    for i in range(b.n):
        assert torch.equal(b.image(y1, i), b.image(y2, i))
    assert (y2 == 7).any() and not (y1 == 7).all()                                   # bytes no image covers are not written


def test_argument_errors_name_what_is_wrong_and_n0_is_a_noop():
    call = hip.call
    a = ("adamml_jpeg_decode_u8",)
    with pytest.raises(RuntimeError, match="N = -1 outside"):
        call(*a, None, 16, None, 200, None, 16, None, None, 192, -1)
    with pytest.raises(RuntimeError, match="meta_len = 50 < N"):
        call(*a, None, 16, None, 50, None, 16, None, None, 192, 1)
    with pytest.raises(RuntimeError, match="src_bytes = 17 must be a multiple of 16"):
        call(*a, None, 17, None, 200, None, 16, None, None, 192, 1)
    with pytest.raises(RuntimeError, match="y_bytes = 0 < 1"):
        call(*a, None, 16, None, 200, None, 0, None, None, 192, 1)
    with pytest.raises(RuntimeError, match="workspace_bytes = 100 < 192"):
        call(*a, None, 16, None, 200, None, 16, None, None, 100, 1)
    with pytest.raises(RuntimeError, match="null argument"):
        call(*a, None, 16, None, 200, None, 16, None, None, 192, 1)
    call(*a, None, 0, None, 0, None, 0, None, None, 0, 0)                             # N == 0: a no-op
    y, st = runtime.jpeg_decode_u8(torch.zeros(0, dtype=torch.uint8, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), 0, 0, 0)
    assert st.shape == (0,)
    b = J.Batch([FILES[NAMES[0]]])
    with pytest.raises(RuntimeError, match="no CPU path"):
        J.decode(b)
    with pytest.raises(RuntimeError, match="meta must be"):
        runtime.jpeg_decode_u8(b.data.to(DEV), b.meta.to(DEV).long(), 1, b.out_bytes, b.total_blocks)
    with pytest.raises(TypeError, match="expected a jpeg.Batch"):
        J.decode(b.data)


# ---- EncodedFrames -> augment -> AdaMML --------------------------------------------------------------------------------------------------

_decoded = {}


def _videos(modality, sizes, frames):
    """Per video its list of files (the distinct fixture frames of that size, cycled from a different start per video) and the
    restatement's decoded [H, W, K_in] array."""
    vids, arrays = [], []
    for v, size in enumerate(sizes):
        pool = sorted(k for k in FRAMES if k.startswith("vid_%s_%dx%d_" % ("g" if modality == "flow" else "c", size[0], size[1])))
        assert len(pool) >= 3
        names = [pool[(j + v) % len(pool)] for j in range(frames)]
        for k in names:
            if k not in _decoded:
                _decoded[k] = R.decode(FRAMES[k]).reshape(size[0], size[1], -1)
        vids.append([FRAMES[k] for k in names])
        arrays.append(np.concatenate([_decoded[k] for k in names], 2))
    return vids, arrays


MODES = [("v1", True), ("v2", True), ("val", False)]


@pytest.mark.parametrize("version,is_train", MODES)
@pytest.mark.parametrize("modality,frames", [("rgb", 4), ("flow", 6), ("rgbdiff", 12)])
def test_augment_encoded_frames_equals_augment_frames(version, is_train, modality, frames):
    sizes = [(41, 30), (24, 40), (41, 30)] if modality == "flow" else [(48, 67), (37, 53), (48, 67), (37, 53)]
    random.seed(3)
    np.random.seed(3)
    aug = V.Augmentor(is_train, 20, version="v1" if version == "v1" else "v2", scale_range=(24, 34), modality=modality)
    vids, arrays = _videos(modality, sizes, frames)
    geos = [aug.sample(a.shape[1], a.shape[0]) for a in arrays]
    if is_train:
        for g, f in zip(geos, (True, False, True)):
            g.flip = g.params["flip"] = f
    want = V.augment(V.Frames(arrays, geos).to(DEV))
    ef = V.EncodedFrames(vids, geos, pin_memory=True).to(DEV, non_blocking=True)
    got = V.augment(ef)
    assert got.shape == want.shape == ef.shape and got.dtype == torch.uint8
    assert torch.equal(got, want), int((got != want).sum())
    flat = ef.decode().cpu().numpy()                    # and the decoded scratch holds exactly Stack's interleaved arrays
    for i, a in enumerate(arrays):
        off = int(ef.meta[i * V.DESC])
        assert np.array_equal(flat[off:off + a.size].reshape(a.shape), a), i


def test_augment_raises_on_a_damaged_file_naming_it():
    g = V.Augmentor(False, 24, disable_scaleup=True).sample(67, 48)
    f = FILES["c420_q93_48x67"]
    inf = J.parse(f)
    a, b = inf.segments[-1]
    bad = f[:a + (b - a) // 2] + f[b:]                   # half of the scan is missing: the header still parses
    ef = V.EncodedFrames([[f, f], [f, bad]], [g, g]).to(DEV)
    with pytest.raises(RuntimeError, match="video 1, file 1 has a damaged JPEG stream"):
        V.augment(ef)


CH = {"rgb": 3, "flow": 10, "rgbdiff": 15}
PER_FRAME = {"rgb": 1, "flow": 10, "rgbdiff": 6}            # files per frame of the model's input


def test_adamml_forward_is_bitwise_the_same_for_encoded_frames_and_frames():
    modality, B, S = ["rgb", "flow", "rgbdiff"], 2, 2
    model = adamml(groups=8, modality=modality, input_channels=[CH[m] for m in modality], num_segments=S, rng_policy=False,
                   rng_threshold=0.5, causality_modeling="lstm", num_classes=31, depth=50, without_t_stride=False, dropout=0.0,
                   pooling_method="max", fusion_point="logits", unimodality_pretrained=[], learnable_lf_weights=True)
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=1234))
    model = model.to(DEV).eval()
    random.seed(5)
    np.random.seed(5)
    ins = []
    for m in modality:
        sizes = [(41, 30), (24, 40)] if m == "flow" else [(48, 67), (37, 53)]
        aug = V.Augmentor(False, 64, modality=m)
        vids, arrays = _videos(m, sizes, S * 8 * PER_FRAME[m])
        geos = [aug.sample(a.shape[1], a.shape[0]) for a in arrays]
        ins.append((V.EncodedFrames(vids, geos).to(DEV), V.Frames(arrays, geos).to(DEV)))
    expo = synth.synth_gumbel_exponential(S, 2, B, seed=11).to(DEV)
    with torch.no_grad():
        a, da = model([x[0] for x in ins], gumbel_exponential=expo)
        b, db = model([x[1] for x in ins], gumbel_exponential=expo)
    assert torch.equal(a, b) and torch.equal(da, db)
    with torch.no_grad(), pytest.raises(ValueError, match="flow Frames given for the rgbdiff modality"):
        model([ins[0][0], ins[1][0], ins[1][0]], gumbel_exponential=expo)
