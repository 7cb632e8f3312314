"""The video augmentation on the GPU (adamml_video_resample_u8, adamml_amd.video): byte for byte the integer restatement of the
reference's PIL transforms (tests/video_ref.py) in every mode and modality, with and without flips, mixed source sizes in one batch and
at the benchmark step's shapes; the SHA-256 of its output equals the reference's own Stack output (tests/golden/video_aug_cases.json);
reproducible; argument-checked; and AdaMML fed Frames gives bit for bit what it gives for the restatement's uint8 arrays."""
import hashlib
import json
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from adamml_amd import adamml, hip, runtime, synth, video as V  # noqa: E402
from tests import video_ref as R  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [("v1", True), ("v2", True), ("val", False)]


def _augmentor(version, is_train, modality, size=224, scale_range=(256, 320)):
    return V.Augmentor(is_train, size, version="v1" if version == "v1" else "v2", scale_range=scale_range, modality=modality)


def _batch(version, is_train, modality, k, sizes, seed, size=224, scale_range=(256, 320), flips=(True, False)):
    """Videos, geometries (the first ones forced to the given flip states in training) and the restatement's Stack arrays."""
    random.seed(seed)
    np.random.seed(seed)
    aug = _augmentor(version, is_train, modality, size, scale_range)
    videos = [R.synth_video(seed * 100 + i, h, w, k) for i, (h, w) in enumerate(sizes)]
    geos = [aug.sample(v.shape[1], v.shape[0]) for v in videos]
    if is_train:
        for g, f in zip(geos, flips):
            g.flip = g.params["flip"] = f
    want = [R.transform(R.images_of(v, modality), version, is_train, g.params, modality, size) for v, g in zip(videos, geos)]
    return videos, geos, want


def _gpu(videos, geos, pin=False):
    fr = V.Frames(videos, geos, pin_memory=pin)
    return V.augment(fr.to(DEV, non_blocking=pin)).cpu().numpy(), fr


MIXED = [(256, 341), (256, 455), (341, 256), (240, 320), (256, 256), (300, 533), (480, 640)]


@pytest.mark.parametrize("version,is_train", MODES)
@pytest.mark.parametrize("modality,k", [("rgb", 12), ("rgb", 3), ("flow", 10), ("rgbdiff", 36), ("rgbdiff", 18)])
def test_byte_exact_every_mode_and_modality(version, is_train, modality, k):
    videos, geos, want = _batch(version, is_train, modality, k, MIXED, seed=3)
    got, fr = _gpu(videos, geos, pin=(k == 12))
    assert got.shape == (len(videos), 224, 224, fr.k_out) and got.dtype == np.uint8
    for i in range(len(videos)):
        assert np.array_equal(got[i], want[i]), (i, geos[i])


def test_odd_channel_counts_and_large_downscale():
    """Byte-wise loads (K = 5: no vector width divides it) and a 1080 x 1920 frame to 224^2 (19 taps per axis)."""
    for sizes, k in (([(256, 341), (260, 347)], 5), ([(1080, 1920)], 3)):
        aug = V.Augmentor(False, 224, disable_scaleup=True)
        videos = [R.synth_video(40 + i, h, w, k) for i, (h, w) in enumerate(sizes)]
        geos = [aug.sample(v.shape[1], v.shape[0]) for v in videos]
        got, _ = _gpu(videos, geos)
        for i, (v, g) in enumerate(zip(videos, geos)):
            assert np.array_equal(got[i], R.transform(R.images_of(v, "rgb"), "val", False, g.params, "rgb")), (sizes[i], k)
    # a whole-frame resize 1080 x 1920 -> 224 x 224 (GroupMultiScaleCrop-style crop of the full frame)
    v = R.synth_video(50, 1080, 1920, 3)
    g = V.Geometry(1920, 1080, 224, (1920, 224, 0, 0), (1080, 224, 0, 0), False, "rgb", {})
    got, _ = _gpu([v], [g])
    assert np.array_equal(got[0], R.pil_resize(v, 224, 224))


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "video_aug_cases.json")) as f:
        return json.load(f)


def test_sha256_equals_the_reference_stack_outputs():
    doc = _golden()
    n = 0
    for entry in doc["cases"]:
        case = entry["case"]
        random.seed(case["random_seed"])
        np.random.seed(case["np_seed"])
        aug = _augmentor(case["version"], case["is_train"], case["modality"])
        vids = entry["videos"]
        videos = [R.synth_video(v["seed"], v["height"], v["width"], v["channels"]) for v in vids]
        geos = [aug.sample(v["width"], v["height"]) for v in vids]
        fr = V.Frames(videos, geos, diffs=case["diffs"] or 5)
        got = V.augment(fr.to(DEV)).cpu().numpy()
        for i, v in enumerate(vids):
            assert list(got[i].shape) == v["shape"]
            assert hashlib.sha256(np.ascontiguousarray(got[i]).tobytes()).hexdigest() == v["sha256"], (case, i, geos[i])
            n += 1
    print("  %d videos match the reference's digests" % n)
    assert n == 54


def _step_videos(k, n=72):
    """The benchmark step's sources: N videos alternating 256 x 341 and 256 x 455 (two distinct synthetic frame stacks)."""
    base = [R.synth_video(7, 256, 341, k), R.synth_video(8, 256, 455, k)]
    return [base[i % 2] for i in range(n)]


@pytest.mark.parametrize("version,is_train", MODES)
def test_bench_step_shapes_rgb(version, is_train):
    videos = _step_videos(120)
    random.seed(9)
    np.random.seed(9)
    aug = _augmentor(version, is_train, "rgb")
    geos = [aug.sample(v.shape[1], v.shape[0]) for v in videos]
    got, fr = _gpu(videos, geos, pin=True)
    assert got.shape == (72, 224, 224, 120)
    for i in list(range(0, 72, 9)) + [71]:
        want = R.transform(R.images_of(videos[i], "rgb"), version, is_train, geos[i].params, "rgb")
        assert np.array_equal(got[i], want), (i, geos[i])


@pytest.mark.parametrize("modality,k", [("flow", 400), ("rgbdiff", 720)])
def test_bench_step_shapes_flow_rgbdiff(modality, k):
    videos = _step_videos(k, n=8)
    random.seed(10)
    np.random.seed(10)
    aug = _augmentor("v2", True, modality)
    geos = [aug.sample(v.shape[1], v.shape[0]) for v in videos]
    geos[0].flip = geos[0].params["flip"] = True
    geos[1].flip = geos[1].params["flip"] = False
    got, fr = _gpu(videos, geos)
    assert got.shape == (8, 224, 224, 600 if modality == "rgbdiff" else 400)
    for i in range(8):
        want = R.transform(R.images_of(videos[i], modality), "v2", True, geos[i].params, modality)
        assert np.array_equal(got[i], want), (i, geos[i])


def test_two_runs_are_identical():
    videos, geos, _ = _batch("v1", True, "flow", 20, MIXED, seed=4)
    fr = V.Frames(videos, geos).to(DEV)
    a, b = V.augment(fr), V.augment(fr)
    assert torch.equal(a, b)


def test_argument_errors_name_what_is_wrong_and_n0_is_a_noop():
    call = hip.call
    with pytest.raises(RuntimeError, match="N = -1 outside"):
        call("adamml_video_resample_u8", None, 16, None, 10, None, -1, 224, 224, 3, 3, 0)
    with pytest.raises(RuntimeError, match="bad output size"):
        call("adamml_video_resample_u8", None, 16, None, 10, None, 1, 0, 224, 3, 3, 0)
    with pytest.raises(RuntimeError, match="K_out = 4 != K_in = 3"):
        call("adamml_video_resample_u8", None, 16, None, 10, None, 1, 224, 224, 3, 4, 0)
    with pytest.raises(RuntimeError, match="rgbdiff needs"):
        call("adamml_video_resample_u8", None, 16, None, 10, None, 1, 224, 224, 36, 31, 5)
    with pytest.raises(RuntimeError, match="meta_len = 5"):
        call("adamml_video_resample_u8", None, 16, None, 5, None, 1, 224, 224, 3, 3, 0)
    with pytest.raises(RuntimeError, match="null argument"):
        call("adamml_video_resample_u8", None, 16, None, 10, None, 1, 224, 224, 3, 3, 0)
    call("adamml_video_resample_u8", None, 0, None, 0, None, 0, 224, 224, 3, 3, 0)          # N == 0: a no-op
    y = runtime.video_resample_u8(torch.zeros(0, dtype=torch.uint8, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV),
                                  0, 224, 224, 3, 3)
    assert y.shape == (0, 224, 224, 3)
    videos, geos, _ = _batch("val", False, "rgb", 3, MIXED[:2], seed=5)
    fr = V.Frames(videos, geos)
    with pytest.raises(RuntimeError, match="no CPU path"):
        V.augment(fr)
    with pytest.raises(RuntimeError, match="meta must be"):
        runtime.video_resample_u8(fr.data.to(DEV), fr.meta.to(DEV).long(), fr.n, 224, 224, 3, 3)


# ---- AdaMML fed Frames ------------------------------------------------------------------------------------------------------------

CH = {"rgb": 3, "flow": 10, "rgbdiff": 15, "sound": 1}
KIN = {"rgb": 3, "flow": 10, "rgbdiff": 18}


def _model(modality, S, sd=None):
    model = adamml(groups=8, modality=modality, input_channels=[CH[m] for m in modality], num_segments=S, rng_policy=False,
                   rng_threshold=0.5, causality_modeling="lstm", num_classes=31, depth=50, without_t_stride=False, dropout=0.0,
                   pooling_method="max", fusion_point="logits", unimodality_pretrained=[], learnable_lf_weights=True)
    sd = sd or synth.synth_state_dict(model.state_dict(), seed=1234)
    model.load_state_dict(sd)
    return model.to(DEV), sd


def _inputs(modality, B, S, is_train):
    """Per modality: (Frames on the GPU, the restatement's uint8 [B, 64, 64, K] on the GPU); sound: its spectrogram twice."""
    out = []
    for j, m in enumerate(modality):
        if m == "sound":
            s = synth.synth_inputs(["sound"], B, S, 8, 64, sound_size=64, seed=5)[0].to(DEV)
            out.append((s, s))
            continue
        videos, geos, want = _batch("v2" if is_train else "val", is_train, m, S * 8 * KIN[m], [(72, 96), (80, 72)][:B], seed=20 + j,
                                    size=64, scale_range=(72, 90))
        fr = V.Frames(videos, geos, pin_memory=True).to(DEV, non_blocking=True)
        out.append((fr, torch.from_numpy(np.stack(want)).to(DEV)))
    num_mod = len(modality) - 1 if ("flow" in modality and "rgbdiff" in modality) else len(modality)
    return out, synth.synth_gumbel_exponential(S, num_mod, B, seed=11).to(DEV)


@pytest.mark.parametrize("modality", [["rgb", "sound"], ["rgb", "flow", "rgbdiff"]])
def test_adamml_frames_input_train_is_bitwise_the_uint8_input(modality):
    B, S = 2, 2
    ins, expo = _inputs(modality, B, S, True)
    res, sd = [], None
    for pick in (0, 1):
        model, sd = _model(modality, S, sd)
        model.freeze_policy_net()
        model.train()
        logits, sel = model([x[pick] for x in ins], gumbel_exponential=expo)
        logits.sum().backward()
        torch.cuda.synchronize()
        grads = [p.grad.detach().clone() for p in model.parameters() if p.grad is not None]
        res.append((logits.detach().clone(), sel.detach().clone(), grads))
    (la, da, ga), (lb, db, gb) = res
    assert torch.equal(la, lb) and torch.equal(da, db)
    assert len(ga) == len(gb) > 0 and all(torch.equal(a, b) for a, b in zip(ga, gb))


@pytest.mark.parametrize("modality", [["rgb", "sound"], ["rgb", "flow", "rgbdiff"]])
def test_adamml_frames_input_eval_skipping(modality):
    B, S = 2, 2
    ins, expo = _inputs(modality, B, S, False)
    model, _ = _model(modality, S)
    model.eval()
    assert model.skip_unselected
    with torch.no_grad():
        a, da = model([x[0] for x in ins], gumbel_exponential=expo)
        b, db = model([x[1] for x in ins], gumbel_exponential=expo)
    assert model.last_skip_stats is not None
    assert torch.equal(a, b) and torch.equal(da, db)


def test_adamml_rejects_frames_of_another_modality():
    ins, expo = _inputs(["rgb", "flow", "rgbdiff"], 2, 2, False)
    model, _ = _model(["rgb", "flow", "rgbdiff"], 2)
    model.eval()
    with torch.no_grad(), pytest.raises(ValueError, match="flow Frames given for the rgbdiff modality"):
        model([ins[0][0], ins[1][0], ins[1][0]], gumbel_exponential=expo)
