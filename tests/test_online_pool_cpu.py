"""The host side of serving staggered streams (adamml_amd/online.py): `stagger_schedule`, `gather_videos` for every supported form,
the noise a `Pool` stream draws or is handed against the `Session`'s, the pool's refusals on a stub model, and the launcher's
--online_stagger flag; and the pool's bookkeeping against the lock-step `Session` on a torch stand-in for the model.  Nothing here
launches anything."""
import os
import re
import shlex

import pytest
import torch
import torch.nn as nn

from adamml_amd import audio, online, video

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- stagger_schedule -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,S,k", [(1, 1, 0), (4, 3, 0), (4, 3, 1), (4, 3, 2), (3, 2, 2), (3, 2, 5), (8, 10, 1)])
def test_stagger_schedule_serves_every_segment_once_and_in_order(n, S, k):
    ticks = online.stagger_schedule(n, S, k)
    flat = [e for tick in ticks for e in tick]
    assert sorted(flat) == [(j, t) for j in range(n) for t in range(S)]        # every (stream, t) exactly once
    assert all(tick and len({j for j, _ in tick}) == len(tick) for tick in ticks)                  # no empty tick, a stream once per tick
    for j in range(n):
        seen = [(i, t) for i, tick in enumerate(ticks) for s, t in tick if s == j]
        assert [t for _, t in seen] == list(range(S))                          # t ascends by tick ...
        assert [i for i, _ in seen] == list(range(seen[0][0], seen[0][0] + S))  # ... in consecutive ticks
    firsts = [next(i for i, tick in enumerate(ticks) if (j, 0) in tick) for j in range(n)]
    if k <= S:
        assert firsts == [j * k for j in range(n)]                             # stream j opens at tick j * k
    if k == 0:
        assert ticks == [[(j, t) for j in range(n)] for t in range(S)]         # lock-step
    if k >= S:
        assert all(len(tick) == 1 for tick in ticks) and len(ticks) == n * S   # never overlaps


def test_stagger_schedule_of_the_issue_and_its_refusals():
    assert online.stagger_schedule(4, 3, 1) == [[(0, 0)], [(0, 1), (1, 0)], [(0, 2), (1, 1), (2, 0)], [(1, 2), (2, 1), (3, 0)],
                                                [(2, 2), (3, 1)], [(3, 2)]]
    for bad in ((0, 3, 1), (2, 0, 1), (2, 3, -1)):
        with pytest.raises(ValueError, match="stagger_schedule"):
            online.stagger_schedule(*bad)


# ---- gather_videos ----------------------------------------------------------------------------------------------------------------------

def batch(n=3, S=2):
    """A loader's batch of n videos in four forms: fp32 rgb, uint8 frames, Waveforms with missing flags, Augmented."""
    rgb = torch.arange(n * S * 6 * 4 * 4, dtype=torch.float32).reshape(n, S * 6, 4, 4)
    u8 = torch.arange(n * 4 * 4 * S * 6, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(n, 4, 4, S * 6)
    wave = torch.arange(n * S * 7, dtype=torch.float32).reshape(n, S, 7)
    missing = torch.zeros(n, S, dtype=torch.bool)
    missing[1, 0] = missing[2, 1] = True
    return rgb, u8, audio.Waveforms(wave, missing), video.Augmented(u8.flip(0).contiguous(), "rgb", S * 6)


def test_gather_videos_takes_the_named_rows_of_every_form():
    n, S = 3, 2
    rgb, u8, wf, aug = batch(n, S)
    pieces = online.split_segments([rgb, u8, wf, aug], S)
    parts = [(pieces[1], 2), (pieces[0], 0), (pieces[1], 1)]                  # rows of two different segments, out of order
    a, b, c, d = online.gather_videos(parts)
    want = [(1, 2), (0, 0), (1, 1)]
    assert a.dtype == torch.float32 and a.shape == (3, 6, 4, 4)
    assert b.dtype == torch.uint8 and b.shape == (3, 4, 4, 6)
    assert isinstance(c, audio.Waveforms) and c.wave.shape == (3, 1, 7) and c.missing.shape == (3, 1) and c.missing.dtype == torch.bool
    assert isinstance(d, video.Augmented) and d.modality == "rgb" and d.k_out == 6 and d.u8.shape == (3, 4, 4, 6) and d.u8.dtype == torch.uint8
    for i, (t, r) in enumerate(want):
        assert torch.equal(a[i], rgb[r, 6 * t:6 * (t + 1)])
        assert torch.equal(b[i], u8[r, :, :, 6 * t:6 * (t + 1)])
        assert torch.equal(c.wave[i], wf.wave[r, t:t + 1]) and c.missing[i, 0].item() == wf.missing[r, t].item()
        assert torch.equal(d.u8[i], aug.u8[r, :, :, 6 * t:6 * (t + 1)])
    assert c.missing[:, 0].tolist() == [True, False, False] and c.num_missing == 1
    # all rows of one piece, in order, is that piece
    whole = online.gather_videos([(pieces[0], r) for r in range(n)])
    assert torch.equal(whole[0], pieces[0][0]) and torch.equal(whole[2].missing, pieces[0][2].missing)


def test_gather_videos_turns_frames_into_augmented_once_per_piece(monkeypatch):
    """A video.Frames piece goes through `video.augment` (stubbed here: the kernel needs a GPU) once per distinct piece and call;
    `online.augmented` is that conversion, for the caller that caches it."""
    import random
    import numpy as np
    random.seed(3)
    np.random.seed(3)
    aug = video.Augmentor(False, image_size=24, scale_range=(26, 32), modality="rgb")
    rng = np.random.RandomState(0)
    frames = video.Frames([rng.randint(0, 255, (40, 56, 12), dtype=np.uint8) for _ in range(2)], [aug.sample(56, 40) for _ in range(2)])
    calls = []

    def fake_augment(fr):
        calls.append(fr)
        return torch.full((fr.n, fr.out_h, fr.out_w, fr.k_out), len(calls), dtype=torch.uint8) + torch.arange(fr.n, dtype=torch.uint8)[:, None, None, None]

    monkeypatch.setattr(video, "augment", fake_augment)
    pieces = online.split_segments([frames], 2)
    (got,) = online.gather_videos([(pieces[0], 1), (pieces[1], 0), (pieces[0], 0)])
    assert len(calls) == 2 and calls[0] is pieces[0][0] and calls[1] is pieces[1][0]
    assert isinstance(got, video.Augmented) and got.modality == "rgb" and got.k_out == 6 and got.u8.shape == (3, 24, 24, 6)
    assert got.u8[:, 0, 0, 0].tolist() == [2, 2, 1]                           # piece 0 row 1, piece 1 row 0, piece 0 row 0
    cached = online.augmented(pieces[0])
    assert len(calls) == 3 and isinstance(cached[0], video.Augmented)
    online.gather_videos([(cached, 0), (cached, 1)])
    assert len(calls) == 3                                                     # the cached result is not decoded again


def test_gather_videos_names_the_form_it_refuses():
    good = torch.zeros(2, 6, 4, 4)
    with pytest.raises(TypeError, match=r"gather_videos: .*got a int64 tensor"):
        online.gather_videos([([torch.zeros(2, 3, dtype=torch.int64)], 0)])
    with pytest.raises(TypeError, match=r"gather_videos: .*got a dict"):
        online.gather_videos([([good, {}], 0)])
    with pytest.raises(TypeError, match=r"differ in form: float32 tensor and uint8 tensor"):
        online.gather_videos([([good], 0), ([good.to(torch.uint8)], 0)])
    with pytest.raises(ValueError, match="no \\(piece, row\\)"):
        online.gather_videos([])
    with pytest.raises(ValueError, match="different numbers of modalities"):
        online.gather_videos([([good], 0), ([good, good], 0)])


# ---- the pool's noise and refusals: a stub model, nothing is launched ---------------------------------------------------------------------

class Stub(nn.Module):
    """What Pool reads of an AdaMML before it launches anything."""

    def __init__(self, rng_policy=False, causality="lstm"):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(1))
        self.modality, self.num_modality, self.rng_policy, self.rng_threshold = ["rgb", "sound"], 2, rng_policy, 0.5
        self.policy_net = nn.Module()
        self.policy_net.causality_modeling = causality

    def online_pool(self, S, capacity=8):
        return online.Pool(self, S, capacity)

    def data_layer(self, *a):
        raise AssertionError("a refused step must not reach the data layer")


def inputs(n):
    return [torch.zeros(n, 24, 8, 8), torch.zeros(n, 1, 16, 16)]


def test_pool_refuses_training_mode_and_enabled_grad():
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="training mode"):
            online.Pool(Stub().train(), 3)
        with pytest.raises(ValueError, match="capacity 0"):
            online.Pool(Stub().eval(), 3, 0)
    with pytest.raises(RuntimeError, match="gradients are enabled"):
        online.Pool(Stub().eval(), 3)


@pytest.mark.parametrize("rng_policy,causality", [(False, "lstm"), (False, None), (True, "lstm")])
def test_a_stream_draws_its_noise_as_a_one_video_session_does(rng_policy, causality):
    S, M = 3, 2
    with torch.no_grad():
        model = Stub(rng_policy, causality).eval()
        torch.manual_seed(9)
        session = online.Session(model, S, 1)
        torch.manual_seed(9)
        pool = online.Pool(model, S, capacity=2)
        pool.open()                                                            # slot 0 ...
        after_one = torch.get_rng_state()
        torch.manual_seed(9)
        b = pool.open()                                                        # ... and slot 1 from the same state
        assert torch.equal(torch.get_rng_state(), after_one)                   # the same amount drawn
        assert pool._stream(b).slot == 1 and torch.equal(pool._noise[:, 0], pool._noise[:, 1])
        if rng_policy:
            assert torch.equal(pool._noise[:, 1], session._rand[:, :, 0])      # [S, M]
        else:
            assert torch.equal(pool._noise[:, 1], session._expo[:, :, 0])      # [S, M, 2], segment-major in both, for both heads


@pytest.mark.parametrize("rng_policy,causality", [(False, "lstm"), (False, None), (True, "lstm")])
def test_batch_noise_is_the_sessions_draw_cut_into_columns(rng_policy, causality):
    S, N, M = 3, 4, 2
    with torch.no_grad():
        model = Stub(rng_policy, causality).eval()
        torch.manual_seed(5)
        session = online.Session(model, S, N)
        after = torch.get_rng_state()
        torch.manual_seed(5)
        noise = online.batch_noise(model, S, N)
        assert torch.equal(torch.get_rng_state(), after) and len(noise) == N
        pool = online.Pool(model, S, capacity=N)
        for j in range(N):
            pool.open(**noise[j])
            want = session._rand[:, :, j] if rng_policy else session._expo[:, :, j]
            assert torch.equal(pool._noise[:, j], want), j
        assert torch.equal(torch.get_rng_state(), after)                       # a given noise draws nothing
        if not rng_policy:
            given = torch.rand(S, M * N, 2) + 0.1
            cut = online.batch_noise(model, S, N, given)
            ref = online.Session(model, S, N, given)._expo
            for j in range(N):
                assert torch.equal(cut[j]["gumbel_exponential"], ref[:, :, j])
            with pytest.raises(ValueError, match=r"holds 40 values.*needs 48"):
                online.batch_noise(model, S, N, torch.rand(20, 2))


def test_pool_open_close_and_refusals():
    with torch.no_grad():
        pool = Stub().eval().online_pool(3, capacity=2)
        a, b = pool.open(), pool.open(gumbel_exponential=torch.ones(3, 2, 2))
        assert a != b and pool.position(a) == pool.position(b) == 0
        with pytest.raises(RuntimeError, match=r"all 2 slots are in use \(capacity = 2\)"):
            pool.open()
        with pytest.raises(ValueError, match=r"gumbel_exponential of shape \(3, 4, 2\), expected \[S, M, 2\] = \[3, 2, 2\]"):
            online.Pool(Stub().eval(), 3).open(gumbel_exponential=torch.ones(3, 4, 2))
        with pytest.raises(ValueError, match="takes gumbel_exponential, not rand"):
            online.Pool(Stub().eval(), 3).open(rand=torch.ones(3, 2))
        with pytest.raises(ValueError, match=r"rand of shape \(2, 3\), expected \[S, M\] = \[3, 2\]"):
            online.Pool(Stub(rng_policy=True).eval(), 3).open(rand=torch.ones(2, 3))
        with pytest.raises(KeyError, match="no open stream with id 7"):
            pool.step([a, 7], inputs(2))
        with pytest.raises(ValueError, match="more than once"):
            pool.step([a, a], inputs(2))
        with pytest.raises(ValueError, match=r"sound input holds 3 videos, the step names 2 streams"):
            pool.step([a, b], [inputs(2)[0], inputs(3)[1]])
        with pytest.raises(ValueError, match=r"1 inputs for the model's 2 modalities"):
            pool.step([a], inputs(1)[:1])
        with pytest.raises(ValueError, match=r"forced decisions of shape \(2, 3\).*\[2, 2\]"):
            pool.step([a, b], inputs(2), decisions=torch.zeros(2, 3))
        with pytest.raises(ValueError, match="at least one stream"):
            pool.step([], inputs(0))
        with pytest.raises(RuntimeError, match="before its first step"):
            pool.result(a)
        pool._stream(b).t = 3                                                  # three segments served
        with pytest.raises(RuntimeError, match=r"step 4 of stream 1 .*num_segments = 3"):
            pool.step([a, b], inputs(2))
        assert pool.position(a) == 0 and pool.position(b) == 3 and pool.ticks == 0
        slot = pool._stream(a).slot
        pool.close(a)
        for call in (pool.close, pool.position, pool.result, pool.executed, lambda s: pool.step([s], inputs(1))):
            with pytest.raises(KeyError, match="no open stream with id 0"):
                call(a)
        c = pool.open()
        assert c not in (a, b) and pool._stream(c).slot == slot                # the slot is reused, the id is not
        with pytest.raises(RuntimeError, match="capacity = 2"):
            pool.open()


# ---- the pool's bookkeeping on a torch stand-in for the model ---------------------------------------------------------------------------
# What Session and Pool call of an AdaMML, in plain torch on the host: a joint feature net, a causal recurrent head (or FC heads) with
# the Gumbel comparison, two linear "main nets" and a decision-gated sum.  Not the model: it checks which rows, slots, positions and
# noise columns the pool hands on, for every schedule, without a GPU.

class Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = nn.Linear(8, 5)

    def forward_nhwc(self, frames, groups):
        return self.fc(frames.reshape(frames.shape[0], -1))


class Joint(nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(16, 6)
        self.last_channels = 6

    def features(self, xs, groups=1):
        return torch.relu(self.lin(torch.cat([x.reshape(x.shape[0], -1) for x in xs], 1)))


class Pol(nn.Module):
    def __init__(self, caus):
        super().__init__()
        self.joint_net = Joint()
        self.causality_modeling = caus
        self.W = nn.Linear(6 + 4, 7)
        self.U = nn.Linear(7, 7)
        self.fcs = nn.ModuleList([nn.Linear(7 if caus else 6, 2) for _ in range(2)])

    def decide(self, feats, expo):
        S, B, F = feats.shape
        M = 2
        if self.causality_modeling is None:
            expo = expo.reshape(M, S, B, 2)
            logits = torch.stack([fc(feats) for fc in self.fcs], 0)          # [M, S, B, 2]
            g = logits - expo.log()
            return (g[..., 1] > g[..., 0]).float().transpose(0, 1), logits.transpose(0, 1)
        expo = expo.reshape(S, M, B, 2)
        h, prev = torch.zeros(B, 7), torch.zeros(B, 4)
        decs, logs = [], []
        for t in range(S):
            h = torch.tanh(self.W(torch.cat([feats[t], prev], 1)) + self.U(h))
            l = torch.stack([fc(h) for fc in self.fcs], 0)                # [M, B, 2]
            g = l - expo[t].log()
            d = (g[..., 1] > g[..., 0]).float()                   # [M, B]
            prev = torch.cat([torch.stack([1 - d[m], d[m]], 1) for m in range(M)], 1)
            decs.append(d)
            logs.append(l)
        return torch.stack(decs), torch.stack(logs)


class Main(nn.Module):
    def __init__(self):
        super().__init__()
        self.nets = nn.ModuleList([Net(), Net()])

    def fuse_segments(self, stacked, dec, S):
        return sum(x * dec[0, m][:, None] for m, x in enumerate(stacked))


class Flat:

    def ensure(self, device):
        pass


class TorchModel(nn.Module):
    def __init__(self, caus="lstm", rng=False):
        super().__init__()
        self.modality, self.num_modality, self.rng_policy, self.rng_threshold = ["rgb", "sound"], 2, rng, 0.5
        self.policy_net, self.main_net = Pol(caus), Main()
        self._flat_policy = self._flat_main = Flat()

    def data_layer(self, x, S):
        return list(x), list(x), S


@pytest.mark.parametrize("causality,rng_policy", [("lstm", False), (None, False), ("lstm", True)])
@pytest.mark.parametrize("k", [0, 1, 2, 5])
def test_pool_on_a_torch_model_equals_the_lockstep_session(causality, rng_policy, k):
    """5 streams of S = 4, stream j opening at tick j * k, each tick's rows reversed, finished streams closed; k = 2 runs in 3 slots,
    so slots are reused with another stream's features still in them unless `open` clears them."""
    S, B = 4, 5
    torch.manual_seed(0)
    model = TorchModel(causality, rng_policy).eval()
    xs = [torch.randn(B, S, 2, 4), torch.randn(B, S, 2, 4)]
    with torch.no_grad():
        torch.manual_seed(3)
        session = online.Session(model, S, B)
        torch.manual_seed(3)
        noise = online.batch_noise(model, S, B)
        pieces = online.split_segments(xs, S)
        steps = [session.step(p) for p in pieces]
        ref_logits, ref_dec = session.result()
        assert 0 < ref_dec.sum().item() < ref_dec.numel()
        pool, sids = online.Pool(model, S, capacity=3 if k == 2 else B), {}
        for tick in online.stagger_schedule(B, S, k):
            tick = tick[::-1]
            for j, t in tick:
                if t == 0:
                    sids[j] = pool.open(**noise[j])
            st = pool.step([sids[j] for j, _ in tick], online.gather_videos([(pieces[t], j) for j, t in tick]))
            assert st.executed == [int(v) for v in st.decisions.sum(0).tolist()]
            for i, (j, t) in enumerate(tick):
                assert pool.position(sids[j]) == t + 1
                assert torch.equal(st.decisions[i], steps[t].decisions[j]), (tick, i)
                assert torch.allclose(st.logits[i], steps[t].logits[j], rtol=1e-5, atol=1e-6)
                if rng_policy:
                    assert st.policy_logits is None
                else:
                    assert torch.allclose(st.policy_logits[:, i], steps[t].policy_logits[:, j], rtol=1e-5, atol=1e-6)
                if t == S - 1:
                    logits, dec = pool.result(sids[j])
                    assert torch.equal(dec, ref_dec[j]) and torch.allclose(logits, ref_logits[j], rtol=1e-5, atol=1e-6)
                    assert pool.executed(sids[j]) == [int(v) for v in dec.sum(0).tolist()]
                    pool.close(sids[j])
        assert model.last_skip_stats == {"clips": S * B, "executed_per_modality": [int(v) for v in ref_dec.sum((0, 1)).tolist()]}


# ---- the launcher's flag ----------------------------------------------------------------------------------------------------------------

def test_online_stagger_without_online_exits_with_the_reason():
    from adamml_amd import train
    with pytest.raises(SystemExit, match="--online_stagger is valid only with -e --online"):
        train.main(["-e", "--online_stagger", "1", "--synthetic", "1"])
    with pytest.raises(SystemExit, match="--online is valid only with -e"):
        train.main(["--online", "--online_stagger", "1", "--synthetic", "1"])
    with pytest.raises(SystemExit, match="--online_stagger is valid only with -e --online"):
        train.main(["--online_stagger", "2", "--synthetic", "1"])
    with pytest.raises(SystemExit, match="--online_stagger -1.*cannot be negative"):
        train.check_online(train.arg_parser().parse_args(["-e", "--online", "--online_stagger", "-1"]))
    args = train.arg_parser().parse_args(["-e", "--online", "--online_stagger", "2"])
    assert args.online_stagger == 2
    train.check_online(args)                                                   # accepted
    assert train.arg_parser().parse_args(["-e", "--online"]).online_stagger == 0
    train.check_online(train.arg_parser().parse_args(["-e", "--online"]))
    from adamml_amd import train_unimodal
    with pytest.raises(SystemExit, match="--online_stagger"):
        train_unimodal.main(["--backbone_net", "resnet", "--modality", "rgb", "-e", "--online_stagger", "1"])


def test_the_readme_command_with_online_stagger_parses():
    from adamml_amd import train
    with open(os.path.join(ROOT, "README.md")) as f:
        text = f.read().replace("\\\n", " ")
    lines = [l for l in text.splitlines() if re.match(r"^python3 train_adamml\.py .*--online_stagger", l)]
    assert len(lines) == 1, lines
    argv = shlex.split(lines[0].split("#")[0])[2:]
    args = train.arg_parser().parse_args(argv)
    assert args.evaluate and args.online and args.online_stagger == 1 and args.backbone_net == "adamml"
    train.check_online(args)
