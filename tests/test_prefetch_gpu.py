"""adamml_amd/prefetch.py on the GPU: what the Prefetcher hands over is bit for bit what `video.augment` / `Waveforms.spectrogram` make
of the same loader batch on the caller's stream; SGD steps fed through it equal the steps fed with the loader's objects (AdaMML, the
bare ResNet over the video.Augmented route, the bare sound net); a handed-over batch is never written again; a damaged JPEG file
raises at the hand-over of ITS batch; both launchers train with --prefetch 1; an iterator dropped mid-epoch leaves nothing behind.
Nothing here asserts on a time or an overlap.

The shapes of tests/data_ref.py (test_data_gpu.py): 48 x 64 frames, 64-pixel crops, 8 frames per clip, 2 clips, batch 2, no worker
processes -- the smallest at which all three input kernels run.  Every batch list is collated once, so no RNG is involved in a
comparison."""
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from adamml_amd import audio, data as D, jpeg as J, prefetch, synth, train, train_unimodal as TU, video as V  # noqa: E402
from adamml_amd.model_builder import build_model  # noqa: E402
from adamml_amd.optim import FlatSGD  # noqa: E402
from adamml_amd.prefetch import Prefetcher  # noqa: E402
from tests import data_ref as R  # noqa: E402
from tests.test_data_gpu import _model  # noqa: E402
from tests.test_train_gpu import ARGS  # noqa: E402

DEV = "cuda"
UNI = ["--groups", "8", "-b", "2", "--input_size", "64", "--scale_range", "72", "88", "--dense_sampling", "-j", "0", "--dropout", "0",
       "--print-freq", "1000"]
NET = {"rgb": ["--backbone_net", "resnet", "-d", "18", "--modality", "rgb"], "sound": ["--backbone_net", "sound_mobilenet_v2", "--modality", "sound"]}


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def _pinned(batch):
    """The batch as a DataLoader with pin_memory=True yields it."""
    inputs, target = batch
    return ([x.pin_memory() for x in inputs] if isinstance(inputs, list) else inputs.pin_memory()), target.pin_memory()


def _collated(loader, videos, flips=None, collate=None, seed=3):
    """The loader's own dataset and collate function over videos 0 .. videos - 1, two per batch: a list of pinned batches."""
    _seed(seed)
    items = [loader.dataset[i] for i in range(videos)]
    if flips is not None:
        for it, f in zip(items, flips):
            for part in it["data"]:
                part["geometry"].flip = part["geometry"].params["flip"] = f
    collate = collate or loader.loader.collate_fn
    return [_pinned(collate(items[i:i + 2])) for i in range(0, videos, 2)]


def _direct(x):
    """What the model's data layer makes of a loader object today, on the current stream."""
    x = x.to(DEV)
    return x.spectrogram() if isinstance(x, audio.Waveforms) else V.augment(x)


def _tensor(x):
    return x.u8 if isinstance(x, V.Augmented) else x


@pytest.fixture(scope="module")
def rgb_sound(tmp_path_factory):
    """Four batches of ["rgb", "sound"] (8 videos, video 1 without a sound track), the last one decoded with Pillow into a Frames."""
    modality = ["rgb", "sound"]
    roots = R.make_dataset(tmp_path_factory.mktemp("rgb_sound"), modality, videos=8, missing_sound=(1,))
    args = R.launcher_args(modality, roots)
    loader, _ = D.loaders(args, 0, 1, torch.device(DEV))
    batches = _collated(loader, 6)
    batches += _collated(loader, 8, collate=D.Collate(modality, args.num_segments, args.groups, pillow=True))[3:]
    assert [type(b[0][0]) for b in batches] == [V.EncodedFrames] * 3 + [V.Frames] and all(isinstance(b[0][1], audio.Waveforms) for b in batches)
    assert batches[0][0][1].num_missing == 2
    return batches


@pytest.fixture(scope="module")
def flow_rgbdiff(tmp_path_factory):
    """Two batches of ["flow", "rgbdiff"] (4 videos) of the train augmentor, flips forced on for videos 0 and 3."""
    modality = ["flow", "rgbdiff"]
    roots = R.make_dataset(tmp_path_factory.mktemp("flow_rgbdiff"), modality, videos=4)
    loader, _ = D.loaders(R.launcher_args(modality, roots), 0, 1, torch.device(DEV))
    batches = _collated(loader, 4, flips=(True, False, False, True))
    assert [g.flip for g in batches[0][0][0].geometries] == [True, False] and [g.flip for g in batches[1][0][1].geometries] == [False, True]
    return batches


# ---- 1. batches ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("which", ["rgb_sound", "flow_rgbdiff"])
def test_prepared_batches_are_the_direct_results_bit_for_bit(request, which, depth):
    batches = request.getfixturevalue(which)
    want = [[_direct(x) for x in inputs] for inputs, _ in batches]
    pf = Prefetcher(batches, DEV, depth=depth)
    got = list(pf)
    assert len(got) == len(batches) == len(pf)
    for k, ((inputs, target), (src, src_target)) in enumerate(zip(got, batches)):
        assert isinstance(inputs, list) and len(inputs) == 2 and target.is_cuda and torch.equal(target.cpu(), src_target)
        for x, s, w in zip(inputs, src, want[k]):
            if isinstance(s, audio.Waveforms):
                assert torch.is_tensor(x) and x.dtype == torch.float32 and x.shape == (2, 2, 256, 256)
            else:
                assert isinstance(x, V.Augmented) and (x.modality, x.k_out) == (s.modality, s.k_out) and x.shape == s.shape
            assert _tensor(x).is_cuda and torch.equal(_tensor(x), w), (which, depth, k, s)
    assert pf.stats.batches == len(batches) and pf.stats.prepared == 2 * len(batches)
    if which == "rgb_sound":
        assert not got[0][0][1][1].view(torch.int32).any() and got[0][0][1][0].abs().max() > 0      # the missing track: exactly 0
    # what is prepared already passes through: tensors and Augmented, nothing converted
    again = Prefetcher(got[:2], DEV, depth=depth)
    for (inputs, target), (a, t) in zip(again, got):
        assert all(x is y for x, y in zip(inputs, a)) and target is t
    assert again.stats.prepared == 0 and again.stats.batches == 2


# ---- 2. steps ------------------------------------------------------------------------------------------------------------------------
def _steps(model, flat, feed, forward):
    """Three SGD steps over `feed`: [(logits, extras, loss)] and the state_dict afterwards."""
    model.train()
    flat.ensure(torch.device(DEV, torch.cuda.current_device()))
    opt = FlatSGD(flat, 0.01, 0.9, 1e-4, False)
    out = []
    for inputs, target in feed:
        logits, extra = forward(model, inputs)
        loss = F.cross_entropy(logits, target.to(DEV))
        loss.backward()
        opt.step()
        opt.zero_grad()
        out.append((logits.detach().clone(), extra, loss.detach().clone()))
    return out, {k: v.detach().clone() for k, v in model.state_dict().items()}


def _assert_same_steps(a, b):
    (steps_a, sd_a), (steps_b, sd_b) = a, b
    assert len(steps_a) == len(steps_b) == 3
    for k, ((la, ea, lossa), (lb, eb, lossb)) in enumerate(zip(steps_a, steps_b)):
        assert torch.isfinite(la).all() and torch.equal(la, lb) and torch.equal(lossa, lossb), k
        assert (ea is None and eb is None) or torch.equal(ea, eb), k
    assert not torch.equal(steps_a[0][0], steps_a[1][0])
    assert list(sd_a) == list(sd_b)
    for k in sd_a:
        assert torch.equal(sd_a[k], sd_b[k]), k


def _objects(batches):
    """The batches fed as today: the loader's objects, copied to the device in front of the step."""
    for inputs, target in batches:
        yield ([x.to(DEV, non_blocking=True) for x in inputs] if isinstance(inputs, list) else inputs.to(DEV, non_blocking=True)), target


def test_adamml_steps_through_the_prefetcher_are_the_steps_on_the_loader_objects(rgb_sound):
    batches = rgb_sound[:3]
    expo = synth.synth_gumbel_exponential(2, 2, 2, seed=11).to(DEV)

    def forward(model, inputs):
        logits, decisions = model(inputs, gumbel_exponential=expo)
        return logits, decisions.detach().clone()

    runs = []
    for feed in (_objects, lambda b: Prefetcher(b, DEV, depth=1)):
        model = _model(["rgb", "sound"], 2)
        model.freeze_policy_net()
        runs.append(_steps(model, model._flat_main, feed(batches), forward))
    _assert_same_steps(*runs)


def _unimodal(tmp_path, kind, videos=6):
    """(args, three one-object batches of the unimodal loader's dataset and collate function) for the bare backbone of `kind`."""
    root = R.make_dataset(tmp_path, [kind], videos=videos)[0]
    args = TU.resolve_args(train.arg_parser().parse_args(NET[kind] + UNI + ["--datadir", root]))
    loader, _ = D.unimodal_loaders(args, 0, 1, torch.device(DEV))
    return args, _collated(loader, videos)


@pytest.mark.parametrize("kind", ["rgb", "sound"])
def test_bare_backbone_steps_through_the_prefetcher(tmp_path, kind):
    args, batches = _unimodal(tmp_path, kind)
    assert isinstance(batches[0][0], V.EncodedFrames if kind == "rgb" else audio.Waveforms)
    runs, seen = [], []

    def forward(model, x):
        seen.append(type(x))
        return model(x), None

    for feed in (_objects, lambda b: Prefetcher(b, DEV, depth=2)):
        model, _ = build_model(args)
        model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=1234))
        model.input_modality = args.modality
        model = model.to(DEV)
        runs.append(_steps(model, model.flat_owner, feed(batches), forward))
    _assert_same_steps(*runs)
    assert seen == [type(batches[0][0])] * 3 + [V.Augmented if kind == "rgb" else torch.Tensor] * 3
    if kind == "rgb":
        wrong = V.Augmented(torch.zeros(2, 64, 64, 12, dtype=torch.uint8, device=DEV), "rgb", 12)
        with pytest.raises(ValueError, match="Frames with 12 channels"):
            model(wrong)


def test_adamml_refuses_an_augmented_of_another_modality(flow_rgbdiff):
    (inputs, _), = list(Prefetcher(flow_rgbdiff[:1], DEV))
    model = _model(["flow", "rgbdiff"], 2)
    with torch.no_grad(), pytest.raises(ValueError, match="AdaMML: rgbdiff Frames given for the flow modality"):
        model([inputs[1], inputs[0]])


# ---- 3. lifetimes --------------------------------------------------------------------------------------------------------------------
def test_a_handed_over_batch_stays_intact(rgb_sound):
    want = [_direct(x) for x in rgb_sound[0][0]]
    it = iter(Prefetcher(rgb_sound, DEV, depth=2))
    first, _ = next(it)                                                       # batches 0, 1 and 2 are prepared by now
    held = [_tensor(x) for x in first]                                        # kept, not cloned
    later = [next(it), next(it)]                                              # batch 3 prepared, 1 and 2 handed over
    torch.cuda.synchronize()
    assert all(torch.equal(h, w) for h, w in zip(held, want))
    assert all(_tensor(x).data_ptr() != h.data_ptr() for inputs, _ in later for x in inputs for h in held)


def test_abandoning_the_iterator_mid_epoch(rgb_sound):
    want = [[_direct(x) for x in inputs] for inputs, _ in rgb_sound]
    for inputs, _ in Prefetcher(rgb_sound, DEV, depth=2):
        assert all(torch.equal(_tensor(x), w) for x, w in zip(inputs, want[0]))
        break                                                                 # batches 1 and 2 are queued on the prefetch stream
    torch.cuda.synchronize()
    got = list(Prefetcher(rgb_sound, DEV, depth=1))
    assert len(got) == 4
    for (inputs, _), w in zip(got, want):
        assert all(torch.equal(_tensor(x), y) for x, y in zip(inputs, w))


# ---- 4. a damaged file ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2])
def test_a_damaged_file_raises_at_the_hand_over_of_its_batch(depth):
    """The damage of test_jpeg_gpu.py::test_augment_raises_on_a_damaged_file_naming_it -- half of the scan removed, so that the header
    still parses and the decoder reports it in its status -- in the second of three batches."""
    g = V.Augmentor(False, 24, disable_scaleup=True).sample(R.W, R.H)
    f = R.jpeg_bytes(7)
    a, b = J.parse(f).segments[-1]
    bad = f[:a + (b - a) // 2] + f[b:]
    good = [[f, f], [f, f]]
    batches = [(V.EncodedFrames(v, [g, g], pin_memory=True), torch.tensor([0, 1])) for v in (good, [[f, f], [f, bad]], good)]
    pf = Prefetcher(batches, DEV, depth=depth)
    it = iter(pf)
    x, target = next(it)                                                      # batch 1 is decoded by now, on the prefetch stream: no error yet
    assert isinstance(x, V.Augmented) and torch.equal(x.u8, V.augment(batches[0][0].to(DEV))) and target.tolist() == [0, 1]
    with pytest.raises(RuntimeError, match="video 1, file 1 has a damaged JPEG stream") as e:
        next(it)
    assert "1 files of the batch affected" in str(e.value)
    with pytest.raises(StopIteration):                                        # the iterator is dead afterwards
        next(it)
    assert pf.stats.batches == 1
    with pytest.raises(RuntimeError, match="video 1, file 1 has a damaged JPEG stream"):      # `augment` itself is as it was
        V.augment(batches[1][0].to(DEV))


# ---- 5. launchers --------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def made(monkeypatch):
    """How many Prefetchers the launchers construct, and with what."""
    calls = []

    class Counting(Prefetcher):
        def __init__(self, loader, device, **kw):
            calls.append(kw)
            super().__init__(loader, device, **kw)

    monkeypatch.setattr(prefetch, "Prefetcher", Counting)
    return calls


def test_launcher_trains_on_a_tiny_dataset_with_prefetch(tmp_path, made):
    roots = R.make_dataset(tmp_path / "data", ["rgb", "sound"], videos=3)
    at = ARGS.index("--synthetic")
    argv = ARGS[:at] + ARGS[at + 2:]                                          # "--synthetic 2" removed
    lines = []
    res = train.main(argv + ["--dense_sampling", "--datadir", roots[0], roots[1], "--loader_factory", "adamml_amd.data:loaders", "-j", "0",
                             "--logdir", str(tmp_path / "log"), "--prefetch", "1"], log=lines.append)
    assert made == [dict(depth=1, resampling_rate=24000)] * 2                # the train and the validation loader
    assert [h[0] for h in res["history"]] == ["warmup", "main", "policy", "finetune"]
    assert all(np.isfinite(h[2]) for h in res["history"])
    for f in ("checkpoint.pth.tar", "checkpoint_warmup_01.pth.tar", "checkpoint_main_01.pth.tar", "checkpoint_finetune_01.pth.tar"):
        assert os.path.exists(os.path.join(res["log_folder"], f)), f
    assert any(ln.startswith("Val:") for ln in lines) and any("Epoch: [1][1/2]" in ln for ln in lines)


def test_unimodal_launcher_with_and_without_prefetch(tmp_path, made):
    """train_unimodal on a tiny rgb dataset: --prefetch 1 wraps both loaders and the run is the run of --prefetch 0, loss for loss (the
    loaders draw from the same seeded RNGs in the same order; dropout is off); with 0 no Prefetcher is constructed."""
    root = R.make_dataset(tmp_path / "data", ["rgb"], videos=4)[0]
    argv = NET["rgb"] + UNI + ["--datadir", root, "--num_classes", "4", "--epochs", "1", "--lr_scheduler", "step", "--lr_steps", "100"]
    runs = {}
    for n in (0, 1):
        _seed(21)
        lines = []
        runs[n] = TU.main(argv + ["--prefetch", str(n), "--logdir", str(tmp_path / ("log%d" % n))], log=lines.append)
        assert len(made) == 2 * n
        assert {"checkpoint.pth.tar", "log.log"} <= set(os.listdir(runs[n]["log_folder"]))
        assert any(ln.startswith("Val  : [001/001]") for ln in lines) and not any(ln.startswith("prefetch:") for ln in lines if n == 0)
    assert made == [dict(depth=1, resampling_rate=24000)] * 2
    (epoch, losses), = runs[1]["history"]
    assert epoch == 1 and len(losses) == 2 and all(np.isfinite(losses))
    assert runs[1]["history"] == runs[0]["history"] and runs[1]["last_val"] == runs[0]["last_val"]
