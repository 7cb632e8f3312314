"""The dataset loaders (adamml_amd/data.py) on the host: frame indices and RNG consumption equal the reference's own
(tests/golden/dataset_index_cases.json, tools/gen_golden_dataset.py); list parsing, file naming, the WAV reader, the sound windows,
the per-item random-number order, the batches `Collate` builds (with the Pillow fallback) and the loader factory."""
import hashlib
import json
import os
import random
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from adamml_amd import audio, data as D, jpeg, video as V
from tests import data_ref as R, jpeg_ref, spectrogram_ref, video_ref


def _state():
    _, key, pos, _, _ = np.random.get_state()
    return hashlib.sha256(np.asarray(key, '<u4').tobytes() + int(pos).to_bytes(4, 'little')).hexdigest()[:12]


# ---- indices ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.filterwarnings("ignore::DeprecationWarning")
def test_indices_and_rng_state_equal_the_reference_rows():
    rows = R.golden_rows()
    assert len(rows["train"]) == 7 * 2 * 2 * 2 * 2 and len(rows["val"]) == 7 * 2 * 2 * 2 * 2 * 4
    for name, fn in (("train", D.sample_train_clip), ("val", D.sample_val_test_clip)):
        for args, seed, state, want in rows[name]:
            np.random.seed(seed)
            got = fn(*args)
            assert np.asarray(got).tolist() == want, (name, args)
            assert _state() == state, (name, args, "numpy's global RNG is not where the reference leaves it")


def test_spot_values_computed_from_the_reference():
    """Guards the fixture itself: three results stated in the feature request, present in the fixture and reproduced."""
    rows = R.golden_rows()
    np.random.seed(3)
    a = D.sample_train_clip(120, 1, 8, 2, True, 5).tolist()
    assert a[:10] == [11, 13, 15, 17, 19, 21, 23, 25, 24, 26] and a[-4:] == [108, 110, 112, 114] and len(a) == 40
    b = D.sample_val_test_clip(120, 5, 8, 1, True, True, 5).tolist()
    assert b == [s + i for s in (1, 28, 55, 82, 109) for i in range(8)]
    c = D.sample_val_test_clip(12, 1, 8, 1, False, True, 3).tolist()
    assert c == [1, 2, 4, 5, 7, 8, 10, 11, 1, 3, 4, 6, 7, 9, 10, 12, 2, 3, 5, 6, 8, 9, 11, 12]
    assert [r[3] for r in rows["val"] if r[0] == [120, 5, 8, 1, True, True, 5]] == [b]
    assert [r[3] for r in rows["val"] if r[0] == [120, 1, 8, 1, False, True, 3]]


def test_random_clip_draws():
    np.random.seed(0)
    fresh = _state()
    assert D.random_clip(5, 1, 8) == [0, 1, 2, 3, 4, 0, 1, 2]                    # nothing fits: offset 0, wrapped, no draw
    assert D.random_clip(20, 2, 4, fixed_offset=True) == [6, 8, 10, 12]
    assert _state() == fresh
    np.random.seed(5)
    want = int(np.random.RandomState(5).randint(3, 7, 1)[0])
    assert D.random_clip(20, 1, 4, False, 3, 7) == [want + i for i in range(4)]


# ---- lists ------------------------------------------------------------------------------------------------------------------------
def _list(tmp_path, text, name="list.txt"):
    (tmp_path / name).write_text(text)
    return str(tmp_path), name


def test_list_parsing(tmp_path):
    root, name = _list(tmp_path, "a/v1 1 30 4\nb/v2 5 12 7\nv3 1 100 0\n")
    ds = D.VideoDataSet(root, name, separator=" ", filter_video=10)
    assert ds.list_file == os.path.join(root, name)
    assert [(r.path, r.video_id, r.start_frame, r.end_frame, r.label, r.num_frames, r.line) for r in ds.video_list] == [
        ("a/v1", "v1", 1, 30, 4.0, 30, 1), ("v3", "v3", 1, 100, 0.0, 100, 3)]                 # b/v2 has 8 frames < filter_video
    assert not ds.multi_label and ds.get_label(ds.video_list[0]) == 4 and ds.num_consecutive_frames == 1
    assert len(D.VideoDataSet(root, name, separator=" ", filter_video=0)) == 3
    # test_mode keeps short videos and has no labels: the video id stands in
    ts = D.VideoDataSet(root, name, separator=" ", filter_video=10, test_mode=True)
    assert len(ts) == 3 and ts.video_list[1].label == -1 and ts.get_label(ts.video_list[1]) == "v2"
    # another separator; rgbdiff lists one frame fewer; flow and rgbdiff read 5 consecutive frames per index
    root, name = _list(tmp_path, "v1;1;30;4\nv2;3;12;7\n", "semi.txt")
    rd = D.VideoDataSet(root, name, separator=";", modality="rgbdiff")
    assert [(r.end_frame, r.num_frames) for r in rd.video_list] == [(29, 29), (11, 9)] and rd.num_consecutive_frames == 5
    assert D.VideoDataSet(root, name, separator=";", modality="flow").num_consecutive_frames == 5
    assert D.VideoDataSet(root, name, separator=";", modality="flow").video_list[0].end_frame == 30
    with pytest.raises(ValueError, match="modality"):
        D.VideoDataSet(root, name, modality="depth")
    with pytest.raises(ValueError, match="line 1"):
        D.VideoDataSet(root, name, separator=" ")


def test_multi_label_lists(tmp_path):
    root, name = _list(tmp_path, "v1;1;30;4;2\nv2;1;30;7\nv3;1;30;0;1;5\n")               # mean row length 5 > 4
    ds = D.VideoDataSet(root, name, separator=";", num_classes=8)
    assert ds.multi_label and [r.label for r in ds.video_list] == [[4.0, 2.0], [7.0], [0.0, 1.0, 5.0]]
    hot = ds.get_label(ds.video_list[2])
    assert hot.dtype == torch.float32 and hot.tolist() == [1, 1, 0, 0, 0, 1, 0, 0]
    root, name = _list(tmp_path, "v1;1;30;4;2\nv2;1;30;7\nv3;1;30;0\n", "single.txt")       # mean row length 4 1/3 > 4 as well
    assert D.VideoDataSet(root, name, separator=";").multi_label
    root, name = _list(tmp_path, "v1;1;30;4\nv2;1;30;7\n", "plain.txt")
    assert not D.VideoDataSet(root, name, separator=";").multi_label


# ---- file names -------------------------------------------------------------------------------------------------------------------
def test_file_names_and_the_reference_clipping(tmp_path):
    root, name = _list(tmp_path, "v1;1;30;4\nsub/v2;10;30;7\n")
    rgb = D.VideoDataSet(root, name, separator=";", modality="rgb")
    late = rgb.video_list[1]                                       # start_frame 10, 21 frames: numbers are clipped at 21, not at 30
    assert rgb.file_names(late, [1, 5, 12, 15]) == ["sub/v2/%05d.jpg" % n for n in (10, 14, 21, 21)]
    flow = D.VideoDataSet(root, name, separator=";", modality="flow", image_tmpl="f{:04d}.jpg")
    assert flow.file_names(flow.video_list[0], [3]) == ["v1/%s_f%04d.jpg" % (p, n) for n in range(3, 8) for p in "xy"]
    assert flow.file_names(flow.video_list[0], [28]) == ["v1/%s_f%04d.jpg" % (p, n) for n in (28, 29, 30, 30, 30) for p in "xy"]
    assert flow.file_names(flow.video_list[1], [2])[::2] == ["sub/v2/x_f%04d.jpg" % n for n in range(11, 16)]
    diff = D.VideoDataSet(root, name, separator=";", modality="rgbdiff")
    assert diff.file_names(diff.video_list[0], [3, 25]) == ["v1/%05d.jpg" % n for n in list(range(3, 9)) + list(range(25, 31))]
    with pytest.raises(ValueError) as e:
        diff.file_names(diff.video_list[0], [3, 27])               # 27 28 29 29 29: not five consecutive frames
    msg = str(e.value)
    assert "v1" in msg and name in msg and "line 1" in msg and "[3, 27]" in msg and "[27, 28, 29, 29, 29]" in msg
    with pytest.raises(ValueError, match=r"sub/v2.*line 2"):
        diff.file_names(diff.video_list[1], [12])                  # 21 frames -> 20 for rgbdiff: 21 22 ... clipped at 20


# ---- WAV --------------------------------------------------------------------------------------------------------------------------
def _wav_header(fmt_body, data):
    chunks = b"fmt " + struct.pack("<I", len(fmt_body)) + fmt_body + b"LIST" + struct.pack("<I", 3) + b"abc\0" + \
        b"data" + struct.pack("<I", len(data)) + data
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


def test_wav_reader(tmp_path):
    mono, stereo = R.track(1, 0.05, 1), R.track(2, 0.05, 2)
    R.write_wav(str(tmp_path / "m.wav"), mono, rate=16000)          # the rate is not looked at
    R.write_wav(str(tmp_path / "s.wav"), stereo)
    got = D.read_wav(str(tmp_path / "m.wav"))
    assert got.dtype == np.float32 and got.shape == (mono.shape[0],)
    assert np.array_equal(got, mono[:, 0].astype(np.float32) / np.float32(32768))
    got = D.read_wav(str(tmp_path / "s.wav"))
    x = stereo.astype(np.float32) / np.float32(32768)
    assert got.dtype == np.float32 and np.array_equal(got, ((x[:, 0] + x[:, 1]) / np.float32(2)).astype(np.float32))
    # WAVE_FORMAT_EXTENSIBLE with the PCM subformat, an odd-sized chunk before the data
    ext = struct.pack("<HHIIHH", 0xFFFE, 2, 24000, 96000, 4, 16) + struct.pack("<HHI", 22, 16, 3) + D.PCM_SUBFORMAT
    (tmp_path / "e.wav").write_bytes(_wav_header(ext, stereo.tobytes()))
    assert np.array_equal(D.read_wav(str(tmp_path / "e.wav")), got)
    # rejected, naming the file and the format
    R.write_wav(str(tmp_path / "u8.wav"), (mono >> 8).astype(np.uint8) + 128, width=1)
    with pytest.raises(ValueError, match=r"u8\.wav.*8 bits"):
        D.read_wav(str(tmp_path / "u8.wav"))
    flt = struct.pack("<HHIIHH", 3, 1, 24000, 96000, 4, 32)
    (tmp_path / "f32.wav").write_bytes(_wav_header(flt, np.zeros(64, np.float32).tobytes()))
    with pytest.raises(ValueError, match=r"f32\.wav.*format 3"):
        D.read_wav(str(tmp_path / "f32.wav"))
    ieee = ext[:24] + b"\x03" + D.PCM_SUBFORMAT[1:]
    (tmp_path / "xf.wav").write_bytes(_wav_header(ieee, stereo.tobytes()))
    with pytest.raises(ValueError, match=r"xf\.wav.*subformat"):
        D.read_wav(str(tmp_path / "xf.wav"))
    (tmp_path / "no.wav").write_bytes(b"RIFX" + b"\0" * 40)
    with pytest.raises(ValueError, match=r"no\.wav"):
        D.read_wav(str(tmp_path / "no.wav"))


# ---- sound windows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [8, 5])
def test_sound_windows_follow_the_centre_index_rule(tmp_path, groups):
    root = str(tmp_path)
    samples = R.track(3, 2.0, 2)
    R.write_wav(os.path.join(root, "a.wav"), samples)
    (tmp_path / "l.txt").write_text("a.wav;3;60;1\nb.wav;1;60;2\n")
    clips = 3
    ds = D.VideoDataSet(root, "l.txt", num_groups=groups, num_clips=clips, modality="sound", separator=";", dense_sampling=True)
    rec = ds.video_list[0]
    indices = np.concatenate([np.arange(groups) + 1, np.arange(groups) * 2 + 14, np.arange(groups) + 56])     # start, middle, past the end
    wave, missing = ds.get_data(rec, indices)
    mono = D.read_wav(os.path.join(root, "a.wav"))
    need = 30720
    assert wave.shape == (clips, need) and wave.dtype == np.float32 and missing.tolist() == [False] * clips
    centres = []
    for c in range(clips):
        clip = indices[c * groups:(c + 1) * groups].tolist()
        centre = (clip[groups // 2 - 1] + clip[groups // 2]) // 2 if groups % 2 == 0 else clip[groups // 2]
        centres.append(min(rec.num_frames, centre))
        assert np.array_equal(wave[c], spectrogram_ref.load_sound_slice(mono, centres[-1], rec.start_frame)[:need]), (c, centres)
    assert ds.sound_centres(rec, indices) == centres and centres[-1] <= rec.num_frames
    assert not np.array_equal(wave[0], wave[1]) and not np.array_equal(wave[1], wave[2])
    # no track: zero windows, every flag set
    wave, missing = ds.get_data(ds.video_list[1], indices)
    assert wave.shape == (clips, need) and not wave.any() and missing.tolist() == [True] * clips


def test_waveforms_class():
    w = audio.Waveforms(np.ones((2, 3, 16), np.float32), np.array([[True, False, False], [False, False, True]]))
    assert w.shape == (2, 3, 16) and w.size(2) == 16 and w.size() == w.shape and w.device.type == "cpu" and w.num_missing == 2
    assert audio.Waveforms(torch.zeros(1, 2, 4)).missing.tolist() == [[False, False]]
    assert w.to("cpu").wave is not None and "2 missing" in repr(w)
    with pytest.raises(ValueError):
        audio.Waveforms(np.ones((2, 16), np.float32))
    with pytest.raises(ValueError):
        audio.Waveforms(np.ones((2, 3, 16), np.float32), np.zeros((2, 2), bool))
    with pytest.raises(RuntimeError, match="MI355X"):
        w.spectrogram()                                             # no CPU path


# ---- items ------------------------------------------------------------------------------------------------------------------------
def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


@pytest.mark.parametrize("is_train", [True, False])
def test_item_draws_indices_first_then_each_modality_in_order(tmp_path, is_train):
    modality = ["rgb", "sound", "flow"]
    roots = R.make_dataset(tmp_path, modality, videos=2)
    args = R.launcher_args(modality, roots)
    augs = [None if m == "sound" else V.augmentor_for(args, m, is_train) for m in modality]
    ds = D.MultiVideoDataSet(roots, "train.txt", 8, 1, num_clips=2, modality=modality, dense_sampling=True, augmentor=augs,
                             is_train=is_train, separator=";", num_classes=31)
    assert ds.num_consecutive_frames == 5
    _seed(7)
    item = ds[1]
    # the restatement: indices from the first modality's record with the largest num_consecutive_frames, then rgb's draws, then flow's
    _seed(7)
    rec = ds.video_list[1]
    want = (D.sample_train_clip(rec.num_frames, 5, 8, 1, True, 2) if is_train else D.sample_val_test_clip(rec.num_frames, 5, 8, 1, True, True, 2))
    geos = [V.augmentor_for(args, m, is_train).sample(R.W, R.H) for m in ("rgb", "flow")]
    assert item["indices"].tolist() == want.tolist() and len(want) == 16 and item["label"] == 1 and item["index"] == 1
    rgb, sound, flow = item["data"]
    assert rgb["geometry"].params == geos[0].params and flow["geometry"].params == geos[1].params
    assert (rgb["geometry"].modality, flow["geometry"].modality) == ("rgb", "flow")
    assert len(rgb["files"]) == 16 and len(flow["files"]) == 160 and all(isinstance(b, bytes) for b in rgb["files"])
    assert rgb["names"][0] == "vid01/%05d.jpg" % want[0] and flow["names"][1] == "vid01/y_%05d.jpg" % want[0]
    with open(os.path.join(roots[0], rgb["names"][3]), "rb") as f:
        assert f.read() == rgb["files"][3]
    assert sound["wave"].shape == (2, 30720) and sound["missing"].tolist() == [False, False]
    # two seeded reads are identical; the item pickles
    import pickle
    _seed(7)
    again = pickle.loads(pickle.dumps(ds[1]))
    assert again["indices"].tolist() == item["indices"].tolist() and again["data"][0]["files"] == rgb["files"]
    assert again["data"][0]["geometry"].params == rgb["geometry"].params and again["data"][2]["geometry"].params == flow["geometry"].params
    assert np.array_equal(again["data"][1]["wave"], sound["wave"])
    if is_train:
        _seed(8)
        assert ds[1]["data"][0]["geometry"].params != rgb["geometry"].params or ds[1]["indices"].tolist() != want.tolist()


def test_frame_size_comes_from_the_first_files_header(tmp_path):
    roots = R.make_dataset(tmp_path, ["rgb"], videos=1, frames=12)
    with open(os.path.join(roots[0], "vid00", "00001.jpg"), "wb") as f:
        f.write(R.jpeg_bytes(1, progressive=True, h=56, w=80))
    with pytest.raises(jpeg.Unsupported):
        jpeg.parse(R.jpeg_bytes(1, progressive=True))
    ds = D.VideoDataSet(roots[0], "train.txt", 8, 1, modality="rgb", dense_sampling=True, fixed_offset=True, is_train=False, separator=";",
                        augmentor=V.Augmentor(False, 64, modality="rgb"))
    item = ds[0]
    assert item["indices"][0] == 1 and (item["data"][0]["geometry"].width, item["data"][0]["geometry"].height) == (80, 56)


# ---- collate ----------------------------------------------------------------------------------------------------------------------
def _items(roots, modality, is_train, seed, num_clips=1, groups=2, which=(0, 1)):
    args = R.launcher_args(modality, roots)
    augs = [None if m == "sound" else V.augmentor_for(args, m, is_train) for m in modality]
    ds = D.MultiVideoDataSet(roots, "train.txt", groups, 1, num_clips=num_clips, modality=modality, dense_sampling=True, augmentor=augs,
                             is_train=is_train, separator=";", num_classes=31)
    _seed(seed)
    return [ds[i] for i in which]


def _model_bytes(x):
    """The CPU models of the decode and resample kernels on a packed batch."""
    if isinstance(x, V.EncodedFrames):
        b = x.batch
        y, status = jpeg_ref.decode_packed(b.data.numpy(), b.meta.numpy(), b.n, b.out_bytes)
        assert not status.any()
    else:
        y = x.data.numpy()
    return video_ref.run_packed(y, x.meta.numpy(), x.n, x.out_h, x.out_w, x.k_in, x.k_out, x.diffs)


def test_collate_builds_the_kernel_inputs_and_both_decode_routes_agree(tmp_path):
    order = ["rgbdiff", "rgb", "flow", "sound"]              # rgbdiff first: the shared indices then leave it its sixth frame
    roots = R.make_dataset(tmp_path, order, videos=2, frames=12, missing_sound=(1,))
    items = _items(roots, order, True, 11)
    inputs, target = D.Collate(order, 1, 2)(items)
    assert target.dtype == torch.long and target.tolist() == [0, 1]
    diff, rgb, flow, sound = inputs
    for x, m, k_in, k_out in ((rgb, "rgb", 6, 6), (flow, "flow", 20, 20), (diff, "rgbdiff", 36, 30)):
        assert isinstance(x, V.EncodedFrames) and x.modality == m and (x.k_in, x.k_out) == (k_in, k_out)
        assert x.shape == (2, 64, 64, k_out) and x.device.type == "cpu" and not x.meta.is_pinned()
        assert [g.params for g in x.geometries] == [it["data"][order.index(m)]["geometry"].params for it in items]
    assert isinstance(sound, audio.Waveforms) and sound.shape == (2, 1, 30720) and sound.missing.tolist() == [[False], [True]]
    assert not sound.wave[1].any() and sound.wave[0].any()
    # the same items decoded with Pillow on the host: the same bytes out of the CPU models of the kernels
    before = D.pillow_fallbacks
    host, _ = D.Collate(order, 1, 2, pillow=True)(items)
    assert D.pillow_fallbacks == before
    for a, b in zip(inputs[:3], host[:3]):
        assert isinstance(b, V.Frames) and (b.k_in, b.k_out, b.modality) == (a.k_in, a.k_out, a.modality)
        assert np.array_equal(_model_bytes(a), _model_bytes(b)), a.modality
    # ... and those bytes are the transform of Pillow's pixels
    it = items[0]["data"][1]
    px = np.concatenate([R.pil_pixels(b) for b in it["files"]], axis=2)
    want = video_ref.transform(video_ref.images_of(px, "rgb"), "v2", True, it["geometry"].params, "rgb", 64)
    assert np.array_equal(_model_bytes(rgb)[0], want)


def test_one_progressive_file_switches_its_modality_to_pillow(tmp_path):
    modality = ["rgb", "flow"]
    roots = R.make_dataset(tmp_path, modality, videos=2, frames=12)
    plain = _items(roots, modality, True, 5)
    name = os.path.join(roots[0], plain[1]["data"][0]["names"][1])
    with open(name, "wb") as f:
        f.write(R.jpeg_bytes(77, progressive=True))
    items = _items(roots, modality, True, 5)
    assert items[1]["data"][0]["names"] == plain[1]["data"][0]["names"]
    before = D.pillow_fallbacks
    inputs, _ = D.Collate(modality, 1, 2)(items)
    assert D.pillow_fallbacks == before + 1
    rgb, flow = inputs
    assert isinstance(rgb, V.Frames) and isinstance(flow, V.EncodedFrames) and rgb.shape == (2, 64, 64, 6)
    assert [g.params for g in rgb.geometries] == [it["data"][0]["geometry"].params for it in plain]
    px = np.concatenate([R.pil_pixels(b) for b in items[1]["data"][0]["files"]], axis=2)
    want = video_ref.transform(video_ref.images_of(px, "rgb"), "v2", True, rgb.geometries[1].params, "rgb", 64)
    assert np.array_equal(_model_bytes(rgb)[1], want)


def test_collate_targets_and_the_uniform_sampling_error(tmp_path):
    roots = R.make_dataset(tmp_path, ["rgb"], videos=2, frames=20)
    with open(os.path.join(roots[0], "train.txt"), "w") as f:
        f.write("vid00;1;20;3;5\nvid01;1;20;4\nvid01;1;20;0;1;2\n")
    args = R.launcher_args(["rgb"], roots)
    ds = D.MultiVideoDataSet(roots, "train.txt", 2, 1, num_clips=1, modality=["rgb"], dense_sampling=True, is_train=True, separator=";",
                             augmentor=[V.augmentor_for(args, "rgb", True)], num_classes=6)
    _, target = D.Collate(["rgb"], 1, 2)([ds[0], ds[2]])
    assert target.dtype == torch.float32 and target.tolist() == [[0, 0, 0, 1, 0, 1], [1, 1, 1, 0, 0, 0]]
    # uniform sampling draws groups x frames_per_group frames whatever num_clips says
    uni = D.MultiVideoDataSet(roots, "val.txt", 2, 1, num_clips=2, modality=["rgb"], dense_sampling=False, is_train=True, separator=";",
                              augmentor=[V.augmentor_for(args, "rgb", True)], num_classes=6)
    item = uni[0]
    assert len(item["indices"]) == 2
    with pytest.raises(ValueError, match=r"uniform sampling ignores num_clips.*--dense_sampling"):
        D.Collate(["rgb"], 2, 2)([item])


# ---- factory ----------------------------------------------------------------------------------------------------------------------
def test_dataset_table_is_the_reference_entry():
    assert D.DATASETS == {"kinetics-sounds": dict(train_list="train.txt", val_list="val.txt", separator=";", image_tmpl="{:05d}.jpg",
                                                  filter_video=0)}


def test_factory_two_ranks_share_the_list(tmp_path):
    modality = ["rgb", "sound"]
    roots = R.make_dataset(tmp_path, modality, videos=6, frames=16, val_videos=4)
    epochs = {}
    for rank in (0, 1):
        many = D.loaders(R.launcher_args(modality, roots, ["-j", "10000"]), rank, 2, "cpu")[0]
        assert many.loader.num_workers == len(os.sched_getaffinity(0))
        train, val = D.loaders(R.launcher_args(modality, roots), rank, 2, "cpu")
        assert len(train) == 3 and len(val) == 2 and train.loader.batch_size == 1 and val.loader.batch_size == 1          # -b 2 over 2 ranks
        assert train.loader.num_workers == 0 and not train.loader.pin_memory
        assert train.sampler.num_replicas == 2 and train.sampler.rank == rank and train.dataset.num_clips == 2
        assert val.dataset.num_clips == 2 and not val.dataset.is_train and train.dataset.is_train
        epochs[rank] = []
        lines = []
        train.log = lines.append if rank == 0 else None
        for _ in range(2):
            seen = []
            for inputs, target in train:
                assert isinstance(inputs[0], V.EncodedFrames) and isinstance(inputs[1], audio.Waveforms) and target.shape == (1,)
                assert inputs[0].shape == (1, 64, 64, 48) and inputs[1].shape == (1, 2, 30720)
                seen.append(int(target[0]))
            epochs[rank].append(seen)
        assert train.epoch == 2 and len(lines) == (2 if rank == 0 else 0)
        vals = [int(t[0]) for _, t in val]
        assert len(vals) == 2
        epochs[rank].append(vals)
    for e in (0, 1):
        assert sorted(epochs[0][e] + epochs[1][e]) == list(range(6)), epochs                      # disjoint, and together the whole list
    assert sorted(epochs[0][2] + epochs[1][2]) == list(range(4))
    assert epochs[0][0] + epochs[1][0] != epochs[0][1] + epochs[1][1], "the second epoch was not reshuffled"


def test_factory_single_rank_shuffles_only_training(tmp_path):
    roots = R.make_dataset(tmp_path, ["rgb"], videos=3, frames=16)
    args = R.launcher_args(["rgb"], roots)
    train, val = D.loaders(args, 0, 1, torch.device("cpu"))
    assert train.sampler is None and isinstance(train.loader.sampler, torch.utils.data.RandomSampler)
    assert isinstance(val.loader.sampler, torch.utils.data.SequentialSampler) and train.loader.batch_size == 2 and len(train) == 2
    assert [t.tolist() for _, t in val] == [[0, 1], [2]]


CHILD = r"""
import json, sys
import torch
from adamml_amd import audio, data, video
from tests import data_ref
roots = sys.argv[1:]
args = data_ref.launcher_args(["rgb", "sound"], roots, ["-j", "2"])
train, val = data.loaders(args, 0, 1, "cpu")
out = {"workers": train.loader.num_workers, "labels": [], "types": []}
for inputs, target in train:
    out["labels"] += target.tolist()
    out["types"].append([type(x).__name__ for x in inputs] + [str(target.dtype), list(inputs[0].shape), list(inputs[1].shape)])
out["cuda"] = torch.cuda.is_initialized()
print("RESULT " + json.dumps(out))
"""


def test_one_epoch_through_worker_processes(tmp_path):
    roots = R.make_dataset(tmp_path, ["rgb", "sound"], videos=5, frames=16)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([R.ROOT] + os.environ.get("PYTHONPATH", "").split(os.pathsep)).rstrip(os.pathsep))
    p = subprocess.run([sys.executable, "-c", CHILD] + roots, cwd=R.ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    assert out["workers"] == min(2, len(os.sched_getaffinity(0))) and not out["cuda"]
    assert sorted(out["labels"]) == list(range(5))                                                # every video exactly once
    assert [t[:3] for t in out["types"]] == [["EncodedFrames", "Waveforms", "torch.int64"]] * 3
    assert [t[3] for t in out["types"]] == [[2, 64, 64, 48], [2, 64, 64, 48], [1, 64, 64, 48]]
    assert [t[4] for t in out["types"]] == [[2, 2, 30720], [2, 2, 30720], [1, 2, 30720]]
