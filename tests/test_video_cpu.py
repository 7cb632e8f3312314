"""CPU checks of the GPU video augmentation (no GPU): the integer restatement (tests/video_ref.py) is PIL.Image.resize bit for bit,
adamml_amd.video's coefficient tables are the restatement's, Augmentor.sample draws what the reference's transforms drew
(tests/golden/video_aug_cases.json), packing only each video's source window computes the same bytes as the full frame, malformed
geometry and tables are rejected on the host, and the C ABI declares and exports adamml_video_resample_u8."""
import ctypes
import json
import os
import random
import types

import numpy as np
import pytest

import __graft_entry__ as ge
from adamml_amd import abi, video as V
from tests import video_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "video_aug_cases.json")


def _pil_cases():
    """(image [H, W, C], crop box or None, (out_w, out_h)): random RGB / L sizes 100..500 up and down, crop then resize, same-size and
    single-axis resizes, and 1080 x 1920 -> 224^2."""
    rng = np.random.default_rng(7)
    cases = []
    for i in range(40):
        h, w = (int(v) for v in rng.integers(100, 501, 2))
        img = rng.integers(0, 256, (h, w, 3 if i % 2 else 1), dtype=np.uint8)
        oh, ow = (int(v) for v in rng.integers(100, 501, 2))
        cases.append((img, None, (ow, oh)))
        if i % 4 == 0:
            cases.append((img, None, (w, oh)))                                     # columns keep their size
            cases.append((img, None, (ow, h)))                                     # rows keep their size
            cases.append((img, None, (w, h)))                                      # a copy
        if i % 3 == 0:
            cw, ch = int(rng.integers(50, w + 1)), int(rng.integers(50, h + 1))
            x, y = int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - ch + 1))
            cases.append((img, (x, y, cw, ch), (224, 224)))                       # GroupMultiScaleCrop's crop then resize
    big = rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)
    cases.append((big, None, (224, 224)))
    return cases


def test_restatement_is_pil_resize_bit_for_bit():
    Image = pytest.importorskip("PIL.Image")
    cases = _pil_cases()
    assert len(cases) >= 70
    for img, box, (ow, oh) in cases:
        src = img if box is None else R.crop(img, *box)
        pil = Image.fromarray(src if src.shape[2] == 3 else src[:, :, 0], "RGB" if src.shape[2] == 3 else "L")
        if box is not None:
            pil = Image.fromarray(img if img.shape[2] == 3 else img[:, :, 0]).crop((box[0], box[1], box[0] + box[2], box[1] + box[3]))
        want = np.asarray(pil.resize((ow, oh), Image.BILINEAR)).reshape(oh, ow, src.shape[2])
        got = R.pil_resize(src, ow, oh)
        assert np.array_equal(got, want), (src.shape, box, ow, oh)
    print("  %d resizes equal PIL (Pillow %s)" % (len(cases), Image.__version__ if hasattr(Image, "__version__") else "?"))


@pytest.mark.parametrize("in_size,out_size", [(256, 224), (341, 224), (455, 298), (341, 426), (256, 320), (168, 224), (192, 224),
                                              (1920, 224), (1080, 224), (101, 499), (499, 101), (7, 3), (3, 7), (1, 5)])
def test_product_tables_are_the_restatement(in_size, out_size):
    first, taps, k = V.coeffs(in_size, 0, in_size, out_size)
    xmin, n, kk = R.pil_coeffs(in_size, out_size)
    assert np.array_equal(first, xmin) and np.array_equal(taps, n)
    assert np.array_equal(k, kk[:, :k.shape[1]]) and not kk[:, k.shape[1]:].any()
    V.check_table(first, taps, k, in_size)


def test_an_unchanged_axis_is_the_identity():
    first, taps, k = V.coeffs(341, 0, 341, 341)
    assert np.array_equal(first, np.arange(341)) and (taps == 1).all() and (k == 1 << 22).all()
    # Pillow's own table for that axis (applied when the other axis changes nothing is skipped) is the identity too
    xmin, n, kk = R.pil_coeffs(341, 341)
    img = R.synth_video(0, 5, 341, 3)
    assert np.array_equal(R.apply_axis(img, xmin, n, kk, axis=1), img)


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _augmentor(case):
    version, is_train = case["version"], case["is_train"]
    return V.Augmentor(is_train, 224, version="v1" if version == "v1" else "v2", scale_range=(256, 320), modality=case["modality"])


def _expected_params(case, draws):
    """The parameters the reference's transforms drew, from the recorded draw values."""
    vals = [d[1] for d in draws]
    if case["version"] == "v1":
        return dict(crop_w=vals[0][0], crop_h=vals[0][1], offset_w=vals[1][0], offset_h=vals[1][1], flip=vals[2] < 0.5)
    if case["version"] == "v2":
        return dict(scale=vals[0], x1=vals[1], y1=vals[2], flip=vals[3] < 0.5)
    return None


def test_sample_draws_what_the_reference_drew():
    doc = _golden()
    flips = set()
    for entry in doc["cases"]:
        case = entry["case"]
        aug = _augmentor(case)
        random.seed(case["random_seed"])
        np.random.seed(case["np_seed"])
        for v in entry["videos"]:
            before = (random.getstate(), np.random.get_state()[1].copy())
            geo = aug.sample(v["width"], v["height"])
            want = _expected_params(case, v["draws"])
            if want is None:                                       # val: no draws at all
                assert v["draws"] == [] and random.getstate() == before[0] and np.array_equal(np.random.get_state()[1], before[1])
                assert geo.params["flip"] is False
            else:
                assert geo.params == want, (case, v["width"], v["height"])
                flips.add(geo.params["flip"])
    assert flips == {True, False}


def test_val_geometry_is_torchvision_center_crop():
    g = V.Augmentor(False).sample(341, 256)
    assert g.params == dict(scale=256, x1=58, y1=16, flip=False)               # (341 - 224) / 2 = 58.5 rounds to 58
    assert V.resized_size(341, 256, 256) == (341, 256) and V.resized_size(256, 341, 288) == (288, 383)
    assert V.resized_size(455, 256, 300) == (533, 300)
    g = V.Augmentor(False, disable_scaleup=True).sample(300, 240)
    assert g.params["scale"] == 224 and g.xaxis == (300, 280, 0, 28)


def _full_reference(video, geo, modality, version, is_train):
    return R.transform(R.images_of(video, modality), version, is_train, geo.params, modality)


@pytest.mark.parametrize("version,is_train", [("v1", True), ("v2", True), ("val", False)])
@pytest.mark.parametrize("modality,k", [("rgb", 6), ("flow", 4), ("rgbdiff", 36)])
def test_packed_windows_compute_the_full_frame_bytes(version, is_train, modality, k):
    random.seed(5)
    np.random.seed(5)
    aug = V.Augmentor(is_train, 224, version="v1" if version == "v1" else "v2", modality=modality)
    sizes = [(256, 341), (256, 455), (320, 256), (240, 300), (256, 256)]
    videos = [R.synth_video(100 + i, h, w, k) for i, (h, w) in enumerate(sizes)]
    geos = [aug.sample(v.shape[1], v.shape[0]) for v in videos]
    if is_train:
        for g, flip in zip(geos[:2], (True, False)):                               # both flip states in every training case
            g.flip = g.params["flip"] = flip
    fr = V.Frames(videos, geos)
    got = R.run_packed(fr.data.numpy(), fr.meta.numpy(), fr.n, fr.out_h, fr.out_w, fr.k_in, fr.k_out, fr.diffs)
    for i, (v, g) in enumerate(zip(videos, geos)):
        want = _full_reference(v, g, modality, version, is_train)
        assert got[i].shape == want.shape and np.array_equal(got[i], want), (i, g)
    full = sum(v.nbytes for v in videos)
    print("  %s %s: window bytes %d of %d" % (version, modality, fr.read_bytes, full))
    assert fr.read_bytes < full
    assert fr.shape == (5, 224, 224, fr.k_out) and fr.size(0) == 5 and fr.k_out == (30 if modality == "rgbdiff" else k)


def test_offsets_beyond_2_gib_are_encoded_as_two_unsigned_words():
    for off in (0, 16, (1 << 31) - 16, 1 << 31, 2155505040, (1 << 32) + 48, 5 << 32):
        lo, hi = V.split_offset(off)
        meta = np.array([lo, hi], np.int32)                                # what the descriptor holds
        assert (int(meta[0]) & 0xffffffff) | (int(meta[1]) << 32) == off     # how the kernel reads it back
    with pytest.raises(ValueError):
        V.split_offset(-16)


def test_frames_is_a_plain_object_that_stock_ddp_passes_through():
    from torch.distributed.utils import _recursive_to
    v = R.synth_video(1, 256, 341, 3)
    fr = V.Frames([v], [V.Augmentor(False).sample(341, 256)])
    assert not isinstance(fr, (tuple, list, dict))
    out = _recursive_to([fr], None, False)
    assert out[0][0] is fr


def test_malformed_geometry_and_tables_are_rejected_on_the_host():
    first, taps, k = (np.array(a) for a in V.coeffs(341, 0, 341, 224))
    V.check_table(first, taps, k, 341)
    bad = [(first - 1, taps, k, "outside"), (first + 1, taps, k, "outside"), (first, taps * 0, k, "tap counts"),
           (first, np.full_like(taps, V.KMAX + 1), np.zeros((224, V.KMAX + 1), np.int32), "tap counts"), (first, taps, -k, "coefficients"),
           (first, taps, k * 2, "coefficients"), (first[:5], taps, k, "malformed")]
    for f, t, kk, msg in bad:
        with pytest.raises(ValueError, match=msg):
            V.check_table(f, t, kk, 341)
    with pytest.raises(ValueError, match="tap counts"):                           # a downscale beyond KMAX taps
        V.check_table(*V.coeffs(4000, 0, 4000, 100), 4000)
    v = R.synth_video(2, 256, 341, 6)
    g = V.Augmentor(False).sample(341, 256)
    with pytest.raises(ValueError, match="geometry was sampled"):
        V.Frames([v[:, :300]], [g])
    g2 = V.Geometry(341, 256, 224, (341, 341, 0, 200), (256, 256, 0, 16), False, "rgb", {})
    with pytest.raises(ValueError, match="keeps"):                               # a crop past the resized frame
        V.Frames([v], [g2])
    g3 = V.Geometry(341, 256, 224, (300, 224, 60, 0), (256, 224, 0, 0), False, "rgb", {})
    with pytest.raises(ValueError, match="keeps"):                               # a crop window past the frame
        V.Frames([v], [g3])
    with pytest.raises(ValueError, match="channels"):
        V.Frames([v, v[:, :, :3]], [g, g])
    with pytest.raises(ValueError, match="rgbdiff"):
        V.Frames([v], [V.Augmentor(False, modality="rgbdiff").sample(341, 256)])
    with pytest.raises(ValueError, match="uint8"):
        V.Frames([v.astype(np.int16)], [g])
    with pytest.raises(TypeError):
        V.Frames([v], [dict(g.params)])
    with pytest.raises(ValueError, match="empty"):
        V.Frames([], [])
    for kw in (dict(version="v3"), dict(modality="sound"), dict(scale_range=(320, 256)), dict(image_size=0)):
        with pytest.raises(ValueError):
            V.Augmentor(True, **kw)
    with pytest.raises(ValueError, match="smaller than the 224 crop"):
        V.Augmentor(True, scale_range=(128, 160)).sample(341, 256)
    with pytest.raises(TypeError):
        V.augment(v)


def test_augmentor_for_reads_the_launcher_flags():
    from adamml_amd import train
    args = train.arg_parser().parse_args([])
    aug = V.augmentor_for(args, "flow", is_train=True)
    assert (aug.image_size, aug.version, aug.scale_range, aug.disable_scaleup, aug.modality) == (224, "v2", (256, 320), False, "flow")
    ns = types.SimpleNamespace(input_size=112, augmentor_ver="v1", scale_range=[128, 160], disable_scaleup=True)
    aug = V.augmentor_for(ns, "rgb", is_train=False)
    assert (aug.image_size, aug.version, aug.scale_range, aug.disable_scaleup, aug.is_train) == (112, "v1", (128, 160), True, False)


def test_header_declares_and_library_exports_video_resample():
    assert str(abi.FUNCTIONS["adamml_video_resample_u8"]) == (
        "int adamml_video_resample_u8(const uint8_t* src, int64_t src_bytes, const int32_t* meta, int meta_len, "
        "uint8_t* y, int N, int OH, int OW, int K_in, int K_out, int diffs, hipStream_t stream)")
    ge.build()
    lib = ctypes.CDLL(ge.LIB)
    assert hasattr(lib, "adamml_video_resample_u8")
    assert lib.adamml_version() >= 103
    from adamml_amd import hip
    assert "adamml_video_resample_u8" in hip.SIGNATURES
