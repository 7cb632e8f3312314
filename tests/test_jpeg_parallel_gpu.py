"""The parallel entropy stage for JPEG scans without restart markers on the GPU (jpeg_parallel_kernel behind adamml_jpeg_decode_u8),
zero differing bytes everywhere against the sequential restatement (tests/jpeg_ref.py decode_packed) and the recorded Pillow pixels:
every marker-less fixture with restart-marker files beside them in one batch, full-size frames, damaged streams (status and pixels of
the CPU model, the other images untouched: the stage hands those images to the sequential kernel inside the call), interleaved
placement, augment(EncodedFrames) == augment(Frames), two runs identical."""
import hashlib
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from adamml_amd import jpeg as J, video as V  # noqa: E402
from tests import jpeg_ref as R  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"))
NEW = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_parallel_cases.npz"))
FILES = {k[:-4]: OLD[k].tobytes() for k in OLD.files if k.endswith(".jpg")}
PIXELS = {k[:-4]: OLD[k[:-4] + ".pixels"] for k in OLD.files if k.endswith(".jpg")}
NEW_NAMES = sorted(k[:-4] for k in NEW.files if k.endswith(".jpg"))
FILES.update({k: NEW[k + ".jpg"].tobytes() for k in NEW_NAMES})
PIXELS.update({k: NEW[k + ".pixels"] for k in NEW_NAMES if k + ".pixels" in NEW.files})
DIGEST = {k: NEW[k + ".sha256"].tobytes() for k in NEW_NAMES if k + ".sha256" in NEW.files}
FULL, FULL_RST = OLD["full_256x341.frame"].tobytes(), OLD["full_256x341_rst1.frame"].tobytes()
MARKERLESS = sorted(k for k, f in FILES.items() if len(J.parse(f).segments) == 1)
RESTART = ["c420_q93_50x70_rst1", "c444_q93_30x41_rst2"]
MIXED = MARKERLESS[:len(MARKERLESS) // 2] + RESTART[:1] + MARKERLESS[len(MARKERLESS) // 2:] + RESTART[1:]

_reference = {}


def _mixed():
    """The mixed batch and the CPU model's output for it, computed once and never written to."""
    if not _reference:
        b = J.Batch([FILES[k] for k in MIXED])
        want, wst = R.decode_packed(b.data.numpy(), b.meta.numpy(), b.n, b.out_bytes)
        want.setflags(write=False)
        _reference.update(batch=b, want=want, status=wst)
    return _reference["batch"], _reference["want"], _reference["status"]


def _gpu(batch, data=None, meta=None):
    dev = batch.to(DEV)
    if data is not None:
        dev.data, dev.meta = torch.from_numpy(data).to(DEV), torch.from_numpy(meta).to(DEV)
    y, status = J.decode(dev)
    torch.cuda.synchronize()
    return y.cpu().numpy(), status.cpu().numpy()


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()


def test_mixed_batch_equals_the_restatement_and_pillow():
    b, want, wst = _mixed()
    assert b.parallel == [k not in RESTART for k in MIXED] and sum(b.parallel) >= 20
    got, st = _gpu(b)
    assert not wst.any() and not st.any(), st
    for i, k in enumerate(MIXED):
        diff = int((b.image(got, i) != b.image(want, i)).sum())
        print("  %-28s %s %d differing bytes" % (k, "parallel  " if b.parallel[i] else "sequential", diff))
        assert diff == 0, k
        if k in PIXELS:
            assert np.array_equal(b.image(got, i), PIXELS[k]), k
        else:
            assert _digest(b.image(got, i)) == DIGEST[k], k
    assert np.array_equal(got, want)


def test_full_size_frames_have_pillows_digest():
    b = J.Batch([FULL] * 3 + [FULL_RST] + [FULL] * 3)
    assert b.parallel == [True] * 3 + [False] + [True] * 3
    a, e = b.infos[0].segments[0]
    assert 330 <= -(-(e - a) // J.SUBSEQ_BYTES) <= 350
    got, st = _gpu(b)
    assert not st.any(), st
    for i in range(b.n):
        assert _digest(b.image(got, i)) == OLD["full_256x341_rst1.sha256" if i == 3 else "full_256x341.sha256"].tobytes(), i


@pytest.mark.parametrize("kind", ["cut", "ff", "zero", "tail0"])
def test_damaged_streams_fall_back_to_the_sequential_answer(kind):
    names = ["c420_q93_48x67", "full_256x341", "c420_q93_50x70_rst1", "noise_c420_q100_96x96", "grey_q93_41x30"]
    key = "damage_batch"
    if key not in _reference:
        b = J.Batch([FULL if k == "full_256x341" else FILES[k] for k in names])
        clean, cst = R.decode_packed(b.data.numpy(), b.meta.numpy(), b.n, b.out_bytes)
        assert not cst.any()
        clean.setflags(write=False)
        _reference[key] = (b, clean)
    b, clean = _reference[key]
    for name in ("full_256x341", "noise_c420_q100_96x96"):
        i = names.index(name)
        data, meta = R.damage(b, i, kind)
        px, wst = R.decode_image(data, meta, i)                         # the CPU model of the damaged image alone
        assert wst != 0
        want = clean.copy()
        b.image(want, i)[...] = px
        got, st = _gpu(b, data, meta)
        print("  %-5s %-24s status %d (model %d)" % (kind, name, st[i], wst))
        assert st[i] == wst and not np.delete(st, i).any(), (kind, name, st, wst)
        assert np.array_equal(got, want), (kind, name, int((got != want).sum()))
        for j in range(b.n):
            if j != i:
                assert np.array_equal(b.image(got, j), b.image(clean, j)), (kind, name, j)


def test_interleaved_marker_less_video_augment_and_repeatability():
    names = ["noise_c420_q100_96x96", "noise_c444_q100_96x96", "noise_c420_q100_96x96"]
    b, want, _ = _mixed()
    frames = [b.image(want, MIXED.index(k)) for k in names]             # the CPU model's pixels, from the shared reference
    k = 3 * len(names)
    places = [J.Placement(32, 96 * k, k, 3 * j) for j in range(len(names))]
    vb = J.Batch([FILES[n] for n in names], places, 32 + 96 * 96 * k)
    assert vb.parallel == [True] * 3
    got, st = _gpu(vb)
    assert not st.any() and not got[:32].any()
    array = np.concatenate(frames, 2)
    assert np.array_equal(got[32:].reshape(96, 96, k), array)
    again, st2 = _gpu(vb)
    assert np.array_equal(again, got) and np.array_equal(st2, st)       # two runs are identical
    random.seed(7)
    np.random.seed(7)
    aug = V.Augmentor(True, 20, version="v2", scale_range=(24, 34), modality="rgb")
    geo = aug.sample(96, 96)
    wanted = V.augment(V.Frames([array], [geo]).to(DEV))
    ef = V.EncodedFrames([[FILES[n] for n in names]], [geo], pin_memory=True).to(DEV, non_blocking=True)
    out = V.augment(ef)
    assert out.shape == wanted.shape and torch.equal(out, wanted), int((out != wanted).sum())
    assert torch.equal(V.augment(ef), out)
