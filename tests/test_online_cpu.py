"""adamml_amd/online.py on the host: `split_segments` for every input form (shapes, which frames and files land in which piece, the
shared geometry, the `missing` flags, the refusals) -- the pieces run through the CPU models of the resampling and JPEG kernels
(tests/video_ref.py, tests/jpeg_ref.py) give exactly the channel slices of the whole -- and the refusals of `Session` and of the
launcher's --online flag, none of which launches anything."""
import io

import numpy as np
import pytest
import torch
import torch.nn as nn

from adamml_amd import audio, online, video
from tests import jpeg_ref as JR
from tests import video_ref as VR

S, GROUPS, H, W = 2, 2, 40, 56


def geometries(modality, n=2, train=True):
    import random
    random.seed(3)
    np.random.seed(3)
    aug = video.Augmentor(train, image_size=24, scale_range=(26, 32), modality=modality)
    return [aug.sample(W, H) for _ in range(n)]


def jpeg_file(seed, gray=False):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(JR.synth_image(seed, H, W, 1 if gray else 3), "L" if gray else "RGB").save(buf, "JPEG", quality=90)
    return buf.getvalue()


def packed_augment(fr):
    """`video.augment` of a Frames / EncodedFrames through the CPU models of the two kernels."""
    if isinstance(fr, video.EncodedFrames):
        y, status = JR.decode_packed(fr.batch.data.numpy(), fr.batch.meta.numpy(), fr.batch.n, fr.batch.out_bytes)
        assert not status.any()
    else:
        y = fr.data.numpy()
    return VR.run_packed(y, fr.meta.numpy(), fr.n, fr.out_h, fr.out_w, fr.k_in, fr.k_out, fr.diffs)


# ---- tensors, Waveforms, Augmented ------------------------------------------------------------------------------------------------------

def test_tensors_are_sliced_along_the_segment_major_channel_axis():
    rgb = torch.arange(2 * 3 * 4 * 3 * 5 * 5, dtype=torch.float32).reshape(2, 3 * 4 * 3, 5, 5)      # S = 3, F = 4, C = 3
    sound = torch.arange(2 * 3 * 6 * 6, dtype=torch.float32).reshape(2, 3, 6, 6)
    wave = torch.arange(2 * 3 * 7, dtype=torch.float32).reshape(2, 3, 7)
    u8 = torch.arange(2 * 4 * 4 * 18, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(2, 4, 4, 18)
    steps = online.split_segments([rgb, sound, wave, u8], 3)
    assert len(steps) == 3 and all(len(s) == 4 for s in steps)
    for t, (a, b, c, d) in enumerate(steps):
        assert a.shape == (2, 12, 5, 5) and torch.equal(a, rgb[:, 12 * t:12 * (t + 1)])
        assert b.shape == (2, 1, 6, 6) and torch.equal(b, sound[:, t:t + 1])
        assert c.shape == (2, 1, 7) and torch.equal(c, wave[:, t:t + 1])
        assert d.shape == (2, 4, 4, 6) and torch.equal(d, u8[..., 6 * t:6 * (t + 1)])
    with pytest.raises(ValueError, match=r"36 channels.*num_segments = 5"):
        online.split_segments([rgb], 5)
    with pytest.raises(TypeError, match="split_segments"):
        online.split_segments([object()], 2)


def test_waveforms_keep_their_missing_flags():
    wave = torch.arange(3 * 2 * 5, dtype=torch.float32).reshape(3, 2, 5)
    missing = torch.tensor([[False, True], [False, False], [True, True]])
    pieces = [s[0] for s in online.split_segments([audio.Waveforms(wave, missing)], 2)]
    for t, p in enumerate(pieces):
        assert isinstance(p, audio.Waveforms) and p.shape == (3, 1, 5)
        assert torch.equal(p.wave, wave[:, t:t + 1]) and torch.equal(p.missing, missing[:, t:t + 1])
    assert [p.num_missing for p in pieces] == [1, 2]
    with pytest.raises(ValueError, match=r"2 segments.*num_segments = 3"):
        online.split_segments([audio.Waveforms(wave, missing)], 3)


def test_augmented_is_sliced_along_its_channel_axis():
    u8 = torch.arange(2 * 3 * 3 * 12, dtype=torch.int64).remainder(253).to(torch.uint8).reshape(2, 3, 3, 12)
    pieces = [s[0] for s in online.split_segments([video.Augmented(u8, 'rgb', 12)], 2)]
    for t, p in enumerate(pieces):
        assert isinstance(p, video.Augmented) and (p.modality, p.k_out) == ('rgb', 6) and torch.equal(p.u8, u8[..., 6 * t:6 * (t + 1)])
    with pytest.raises(ValueError, match=r"12 channels.*num_segments = 5"):
        online.split_segments([video.Augmented(u8, 'rgb', 12)], 5)


# ---- Frames -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("modality,per_group", [("rgb", 3), ("flow", 10), ("rgbdiff", 18)])
def test_frames_pieces_hold_their_segments_frames_and_the_videos_geometry(modality, per_group):
    k = S * GROUPS * per_group
    geos = geometries(modality)
    whole = video.Frames([VR.synth_video(10 + i, H, W, k) for i in range(2)], geos)
    pieces = [s[0] for s in online.split_segments([whole], S)]
    want = packed_augment(whole)
    assert len(pieces) == S
    for t, p in enumerate(pieces):
        assert isinstance(p, video.Frames) and (p.n, p.modality, p.k_in, p.diffs) == (2, modality, k // S, whole.diffs)
        assert p.shape == (2, 24, 24, whole.k_out // S)
        assert p.geometries is whole.geometries                                # one augmentation per video, shared by its segments
        got = packed_augment(p)
        assert np.array_equal(got, want[..., t * p.k_out:(t + 1) * p.k_out]), (modality, t)
    assert sum(p.read_bytes for p in pieces) == whole.read_bytes
    assert whole.k_in == k and np.array_equal(packed_augment(whole), want)         # the whole is left as it was
    with pytest.raises(ValueError, match=r"%d channels.*num_segments = 7" % k):
        online.split_segments([whole], 7)


def test_rgbdiff_frames_are_cut_at_frame_groups_only():
    geos = geometries("rgbdiff", 1)
    whole = video.Frames([VR.synth_video(1, H, W, 3 * 18)], geos)                  # 3 frame groups of 6 RGB frames
    with pytest.raises(ValueError, match="54 channels.*num_segments = 4"):
        online.split_segments([whole], 4)
    for pieces in (2, 6):                                                          # 27 / 9 channels per piece: frame groups cut in two
        with pytest.raises(ValueError, match="frame groups"):
            online.split_segments([whole], pieces)
    assert [s[0].k_out for s in online.split_segments([whole], 3)] == [15, 15, 15]


def test_frames_pieces_stay_pinned_and_movable():
    whole = video.Frames([VR.synth_video(2, H, W, S * GROUPS * 3)], geometries("rgb", 1))
    p = online.split_segments([whole], S)[1][0]
    q = p.to("cpu")
    assert isinstance(q, video.Frames) and torch.equal(q.data, p.data) and torch.equal(q.meta, p.meta)
    assert p.data.numel() % 16 == 0 and p.meta.dtype == torch.int32


# ---- EncodedFrames ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("modality,files_per_group", [("rgb", 1), ("flow", 10), ("rgbdiff", 6)])
def test_encoded_pieces_hold_their_segments_files(modality, files_per_group):
    nf = S * GROUPS * files_per_group
    gray = modality == "flow"
    files = [[jpeg_file(100 * i + j, gray) for j in range(nf)] for i in range(2)]
    geos = geometries(modality, train=(modality != "rgb"))
    whole = video.EncodedFrames(files, geos)
    pieces = [s[0] for s in online.split_segments([whole], S)]
    want = packed_augment(whole)
    per = nf // S
    for t, p in enumerate(pieces):
        assert isinstance(p, video.EncodedFrames) and (p.n, p.modality, p.batch.n) == (2, modality, 2 * per)
        assert p.file_of == [(i, j) for i in range(2) for j in range(per)]
        assert p.geometries is whole.geometries
        # the files of the piece are files t * per .. of each video: the same pixels as decoding them alone
        fresh = video.EncodedFrames([v[t * per:(t + 1) * per] for v in files], geos)
        assert p.k_in == fresh.k_in and p.k_out == fresh.k_out and p.batch.out_bytes == fresh.batch.out_bytes
        assert torch.equal(p.meta, fresh.meta) and torch.equal(p.batch.meta, fresh.batch.meta) and torch.equal(p.batch.data, fresh.batch.data)
        assert np.array_equal(packed_augment(p), want[..., t * p.k_out:(t + 1) * p.k_out]), (modality, t)
        assert p.to("cpu").batch.n == p.batch.n
        p.check_status(torch.zeros(p.batch.n, dtype=torch.int32))
        with pytest.raises(RuntimeError, match="video 1, file 0"):
            p.check_status(torch.tensor([0] * per + [2] + [0] * (per - 1), dtype=torch.int32))
    with pytest.raises(ValueError, match="%d channels.*num_segments = 7" % whole.k_in):
        online.split_segments([whole], 7)


def test_flow_files_are_cut_at_x_y_pairs_only():
    files = [[jpeg_file(j, True) for j in range(6)]]
    whole = video.EncodedFrames(files, geometries("flow", 1))
    with pytest.raises(ValueError, match="2-channel units"):
        online.split_segments([whole], 2)                                          # 3 files per piece: an x image without its y
    assert [s[0].k_in for s in online.split_segments([whole], 3)] == [2, 2, 2]


# ---- the session's refusals: a stub model, nothing is launched --------------------------------------------------------------------------

class Stub(nn.Module):
    """What Session reads of an AdaMML before it launches anything."""

    def __init__(self, modality=("rgb", "sound"), rng_policy=True):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(1))
        self.modality, self.num_modality, self.rng_policy, self.rng_threshold = list(modality), len(modality), rng_policy, 0.5
        self.policy_net = nn.Module()
        self.policy_net.causality_modeling = "lstm"

    def data_layer(self, *a):
        raise AssertionError("a refused step must not reach the data layer")


def inputs(n):
    return [torch.zeros(n, 24, 8, 8), torch.zeros(n, 1, 16, 16)]


def test_session_refuses_training_mode_and_enabled_grad():
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="training mode"):
            online.Session(Stub().train(), 3, 2)
    with pytest.raises(RuntimeError, match="gradients are enabled"):
        online.Session(Stub().eval(), 3, 2)


@pytest.mark.parametrize("rng_policy", [True, False])
def test_session_draws_its_noise_as_forward_does(rng_policy):
    with torch.no_grad():
        torch.manual_seed(9)
        s = online.Session(Stub(rng_policy=rng_policy).eval(), 3, 4)
        torch.manual_seed(9)
        if rng_policy:
            assert torch.equal(s._rand, torch.rand((3, 2, 4)))
        else:
            assert torch.equal(s._expo, torch.empty(3 * 2 * 4, 2).exponential_().reshape(3, 2, 4, 2))
        given = torch.rand(3, 2 * 4, 2)
        assert torch.equal(online.Session(Stub(rng_policy=False).eval(), 3, 4, given)._expo, given.reshape(3, 2, 4, 2))
        with pytest.raises(ValueError, match=r"holds 40 values.*needs 48"):
            online.Session(Stub(rng_policy=False).eval(), 3, 4, torch.rand(20, 2))


def test_session_refuses_a_step_too_many_another_batch_and_another_modality_count():
    with torch.no_grad():
        s = online.Session(Stub().eval(), 3, 2)
        s.t = 3                                                                    # three segments served
        with pytest.raises(RuntimeError, match=r"step 4 .*num_segments = 3"):
            s.step(inputs(2))
        s.t = 0
        with pytest.raises(ValueError, match=r"sound input holds 5 videos.*batch_size = 2"):
            s.step([inputs(2)[0], inputs(5)[1]])
        with pytest.raises(ValueError, match=r"1 inputs for the model's 2 modalities"):
            s.step(inputs(2)[:1])
        with pytest.raises(ValueError, match=r"forced decisions of shape \(2, 3\).*\[2, 2\]"):
            s.step(inputs(2), decisions=torch.zeros(2, 3))
        with pytest.raises(RuntimeError, match="before the first step"):
            s.result()
        assert s.t == 0


# ---- the gated-clip runner of forward, Session and Pool: a stand-in net, nothing is launched -------------------------------------------

class LinearNet:
    """A main net whose `forward_nhwc` is a fixed linear map of each clip and which records the shapes it was called with.  Weights
    and inputs are small integers: every sum is exact in fp32, whichever clips share a call."""

    def __init__(self, clip_numel, frames_per_clip, classes=5):
        g = torch.Generator().manual_seed(1)
        self.fc = nn.Linear(clip_numel, classes)
        self.fc.weight.data = torch.randint(-3, 4, (classes, clip_numel), generator=g).float()
        self.fc.bias.data = torch.randint(-3, 4, (classes,), generator=g).float()
        self.fpc, self.calls = frames_per_clip, []

    def forward_nhwc(self, frames, groups):
        self.calls.append((tuple(frames.shape), groups))
        if frames.dtype == torch.float32 and groups > 1:                           # the whole [B, S, H, W]: segment = group
            frames = frames.transpose(0, 1).reshape(-1, 1, *frames.shape[2:])
        with torch.no_grad():
            return self.fc(frames.reshape(frames.shape[0] // self.fpc, -1).float())


@pytest.mark.parametrize("form", ["bf16", "raw32"])
def test_run_selected_runs_exactly_the_selected_clips(form):
    from adamml_amd.adamml import run_selected
    S, B, F, H, W, C = 2, 3, 2, 3, 4, 2
    g = torch.Generator().manual_seed(7)
    if form == "bf16":
        m_x = torch.randint(-4, 5, (S, B * F, H, W, C), generator=g).to(torch.bfloat16)      # [S, B*F, H, W, C]
        net, whole, clip = LinearNet(F * H * W * C, F), ((S * B * F, H, W, C), 1), lambda k: (k * F, H, W, C)
    else:
        m_x = torch.randint(-4, 5, (B, S, H, W), generator=g).float()                         # [B, S, H, W]
        net, whole, clip = LinearNet(H * W, 1), ((B, S, H, W), S), lambda k: (k, 1, H, W)
    everything = net.forward_nhwc(m_x if form == "raw32" else m_x.flatten(0, 1), whole[1])    # [S*B, classes], row s*B + b
    assert everything.shape == (S * B, 5) and len({tuple(r.tolist()) for r in everything}) == S * B     # every clip's row is its own
    # (segment 0, video 1), (segment 1, video 0), (segment 1, video 2): read as b*S + s these rows would name three other clips
    patterns = {"none": [0, 0, 0, 0, 0, 0], "all": [1, 1, 1, 1, 1, 1], "partial": [0, 1, 0, 1, 0, 1]}
    for name, rows in patterns.items():
        selected = torch.tensor(rows, dtype=torch.float32)
        want = torch.where(selected[:, None] > 0.5, everything, torch.zeros(()))
        for nsel in (None, sum(rows)):                                             # counted by the runner, or known to the caller
            for pad_to in (0, 8):
                net.calls = []
                out, ran = run_selected(net, m_x, selected, S, B, nsel=nsel, pad_to=pad_to)
                assert ran == sum(rows) and out.dtype == torch.float32
                assert torch.equal(out, want), (form, name, nsel, pad_to)         # also: the padded call gives the same result
                if name == "none":
                    assert net.calls == []                                         # nothing runs on the net
                elif name == "all":
                    assert net.calls == [whole]                                    # the whole input, as it is, padded or not
                else:
                    assert net.calls == [(clip(8 if pad_to else sum(rows)), 1)], (form, nsel, pad_to, net.calls)


# ---- the launcher's flag ----------------------------------------------------------------------------------------------------------------

def test_online_without_evaluate_exits_with_the_reason():
    from adamml_amd import train, train_unimodal
    with pytest.raises(SystemExit, match="--online is valid only with -e"):
        train.main(["--online", "--synthetic", "1"])
    args = train.arg_parser().parse_args(["-e", "--online"])
    assert args.online and args.evaluate
    train.check_online(args)                                                       # accepted
    assert not train.arg_parser().parse_args(["-e"]).online
    with pytest.raises(SystemExit, match="--online"):
        train_unimodal.main(["--backbone_net", "resnet", "--modality", "rgb", "-e", "--online"])
