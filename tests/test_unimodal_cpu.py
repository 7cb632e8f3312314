"""The unimodal launcher (adamml_amd/train_unimodal.py) on the host: the reference's three README commands resolve to what its own
parser and `build_model` give (tests/golden/unimodal_contract.json, tools/gen_golden_unimodal.py), the bare models carry the
reference's DataParallel state_dict, the schedule and the --lazy_eval rule equal the reference's, `data.unimodal_loaders` yields what
iterating the VideoDataSet directly yields, and the unsupported flags are rejected with their reason."""
import json
import os
import random
import shlex

import numpy as np
import pytest
import torch

from adamml_amd import audio, data as D, train, train_unimodal as TU, video as V
from adamml_amd.model_builder import build_model
from tests import data_ref as R

GOLDEN = os.path.join(R.ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def contract():
    with open(os.path.join(GOLDEN, "unimodal_contract.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def readme():
    """The three command lines, parsed verbatim and resolved: [(line, args, model, arch_name, arch_name_test)]."""
    with open(os.path.join(GOLDEN, "readme_train_unimodal_commands.txt")) as f:
        lines = [l for l in f.read().splitlines() if l and not l.startswith("#")]
    out = []
    for l in lines:
        argv = shlex.split(l)
        assert argv[:2] == ["python3", "train_unimodal.py"]
        args = train.arg_parser().parse_args(argv[2:])
        args.dataset = "kinetics-sounds"                      # (README placeholder DATASET)
        TU.resolve_args(args)
        model, arch = build_model(args)
        out.append((l, args, model, arch, build_model(args, test_mode=True)[1]))
    return out


def test_readme_commands_resolve_as_the_reference_resolves_them(contract, readme):
    assert len(readme) == 3 and len(contract["recipes"]) == 3
    for (line, args, _, arch, arch_test), want in zip(readme, contract["recipes"]):
        assert line == want["command"]
        assert (args.modality, args.datadir, args.input_channels, args.backbone_net, args.num_classes) == \
            (want["modality"], want["datadir"], want["input_channels"], want["backbone_net"], want["num_classes"])
        assert arch == want["arch_name"] and arch_test == want["arch_name_test"]
        assert args.multiprocessing_distributed and args.batch_size == 72 and args.workers == 96 and args.epochs == 60
        assert args.lr_scheduler == "multisteps" and args.lr_steps == [20, 40, 50] and args.weight_decay == 1e-4
    assert [r[1].modality for r in readme] == ["rgb", "flow", "sound"]


def test_bare_models_carry_the_reference_dataparallel_state_dict(contract, readme):
    for (_, args, model, _, _), want in zip(readme, contract["recipes"]):
        got = [["module." + k, list(v.shape), str(v.dtype)] for k, v in model.state_dict().items()]
        assert got == want["state_dict"], args.modality
        assert list(train.reference_state_dict(model)) == [k for k, _, _ in want["state_dict"]]
        # the parameters the optimizer would hold, in order: one momentum buffer each
        assert [list(p.shape) for p in model.parameters()] == want["optimizer"]["momentum_buffer_shapes"]
        assert len(list(model.parameters())) == want["optimizer"]["num_params"]
        # the surface HipDDP queries on the module it wraps
        assert model.backbones() == [model] and model.flat_grad_buffers() == []


def test_schedule_and_lazy_eval_equal_the_reference(contract):
    ms = contract["multisteps"]

    class Opt:
        lr = ms["base_lr"]
    sched = train.LRSchedule(Opt, "multisteps", ms["base_lr"], ms["epochs"], ms["lr_steps"])
    lrs = []
    for epoch in range(ms["epochs"]):
        lrs.append(Opt.lr)
        sched.step(epoch + 1, 0.0)                            # as the launcher steps it (train_unimodal.py:355-359)
    assert lrs == ms["lr_per_epoch"]
    assert [e + 1 for e in range(ms["epochs"]) if TU.eval_this_epoch(e, ms["epochs"], True)] == contract["lazy_eval_epochs"]
    assert all(TU.eval_this_epoch(e, ms["epochs"], False) for e in range(ms["epochs"]))
    # the state the launcher saves is restored by torch's schedulers (`__dict__.update`): no key they do not know
    for kind, keys in contract["scheduler_keys"].items():
        assert set(train.LRSchedule(Opt, kind, 0.01, 60, [20, 40, 50]).state_dict()) <= set(keys), kind


# ---- loader -----------------------------------------------------------------------------------------------------------------------
H, W, FRAMES, VIDEOS = 24, 32, 12, 3


def _dataset(tmp, modality):
    """One root in the reference's layout: 32 x 24 JPEG frames written with Pillow (flow: grey x_ / y_ files), or short WAV tracks
    (video 1 has none); train.txt / val.txt list `name;1;frames;label`."""
    root = os.path.join(str(tmp), modality)
    os.makedirs(root)
    names = []
    for i in range(VIDEOS):
        name = "vid%02d.wav" % i if modality == "sound" else "vid%02d" % i
        names.append(name)
        if modality == "sound":
            if i != 1:
                R.write_wav(os.path.join(root, name), R.track(i, 0.6, 1 + i % 2))
            continue
        os.makedirs(os.path.join(root, name))
        for n in range(1, FRAMES + 1):
            for k, prefix in enumerate(("x_", "y_") if modality == "flow" else ("",)):
                with open(os.path.join(root, name, "%s%05d.jpg" % (prefix, n)), "wb") as f:
                    f.write(R.jpeg_bytes(100 * i + n + 50 * k, gray=modality == "flow", h=H, w=W))
    for lst in ("train.txt", "val.txt"):
        with open(os.path.join(root, lst), "w") as f:
            f.writelines("%s;1;%d;%d\n" % (names[i], FRAMES, i) for i in range(VIDEOS))
    return root


def _args(modality, root, extra=()):
    argv = ["--backbone_net", "sound_mobilenet_v2" if modality == "sound" else "resnet", "-d", "18", "--modality", modality, "--datadir", root,
            "--groups", "4", "-b", "2", "-j", "0", "--input_size", "16", "--scale_range", "20", "24", "--dense_sampling"] + list(extra)
    return TU.resolve_args(train.arg_parser().parse_args(argv))


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


@pytest.mark.parametrize("modality", ["rgb", "flow", "rgbdiff", "sound"])
def test_unimodal_loaders_yield_what_the_dataset_yields(tmp_path, modality):
    root = _dataset(tmp_path, modality)
    args = _args(modality, root)
    loaders = D.unimodal_loaders(args, 0, 1, "cpu")
    assert len(loaders) == 2
    for is_train, loader in zip((True, False), loaders):
        assert loader.loader.batch_size == 2 and len(loader) == 2 and loader.sampler is None and loader.dataset.num_clips == 1
        assert loader.dataset.is_train == is_train and isinstance(loader.dataset, D.VideoDataSet) and loader.dataset.modality == modality
        _seed(7)
        batches = list(loader)
        order = [int(v) for _, t in batches for v in t]                        # label == video index
        assert sorted(order) == list(range(VIDEOS)) and (is_train or order == list(range(VIDEOS)))
        # the same videos read from the VideoDataSet itself, in that order, from the same seed
        ds = D.VideoDataSet(root, "train.txt" if is_train else "val.txt", 4, 1, num_clips=1, modality=modality, dense_sampling=True,
                            augmentor=None if modality == "sound" else V.augmentor_for(args, modality, is_train), is_train=is_train,
                            separator=";", num_classes=31)
        _seed(7)
        items = [ds[i] for i in order]
        at = 0
        for x, target in batches:
            part = items[at:at + len(target)]
            at += len(target)
            assert not isinstance(x, (list, tuple)) and target.dtype == torch.long and target.tolist() == [it["label"] for it in part]
            if modality == "sound":
                assert isinstance(x, audio.Waveforms) and x.shape == (len(part), 1, 30720)
                assert np.array_equal(x.wave.numpy(), np.stack([it["data"][0]["wave"] for it in part]))
                assert x.missing.tolist() == [[it["index"] == 1] for it in part]
                continue
            geos = [it["data"][0]["geometry"] for it in part]
            want = V.EncodedFrames([it["data"][0]["files"] for it in part], geos)
            assert isinstance(x, V.EncodedFrames) and x.modality == modality and x.shape == want.shape == (len(part), 16, 16, 4 * args.input_channels)
            assert [g.params for g in x.geometries] == [g.params for g in geos]
            assert torch.equal(x.meta, want.meta) and torch.equal(x.batch.data, want.batch.data) and torch.equal(x.batch.meta, want.batch.meta)
    # `loaders` and `Collate` keep their form: a list per batch
    inputs, target = D.Collate([modality], 1, 4)([ds[0]])
    assert isinstance(inputs, list) and len(inputs) == 1 and target.tolist() == [0]


def test_a_progressive_file_switches_the_batch_to_pillow(tmp_path):
    root = _dataset(tmp_path, "rgb")
    with open(os.path.join(root, "vid00", "00003.jpg"), "wb") as f:
        f.write(R.jpeg_bytes(9, progressive=True, h=H, w=W))
    _, val = D.unimodal_loaders(_args("rgb", root), 0, 1, "cpu")
    kinds = [type(x).__name__ for x, _ in val]
    assert kinds == ["Frames", "EncodedFrames"]


def test_two_ranks_split_the_list(tmp_path):
    root = _dataset(tmp_path, "rgb")
    seen = []
    for rank in (0, 1):
        train_l, val_l = D.unimodal_loaders(_args("rgb", root), rank, 2, "cpu")
        assert train_l.loader.batch_size == 1 and train_l.sampler.num_replicas == 2 and train_l.sampler.rank == rank
        seen.append([int(t[0]) for _, t in val_l])
    assert seen[0] == [0, 2] and seen[1][0] == 1


# ---- rejections -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra, message", [(["--num_clips", "2"], r"--num_clips 2.*models/resnet\.py:198"),
                                            (["--threed_data"], r"--threed_data.*2-D"),
                                            (["--backbone_net", "adamml"], r"--backbone_net adamml is adamml_amd\.train")])
def test_unsupported_flags_exit_with_their_reason(extra, message):
    with pytest.raises(SystemExit, match=message):
        TU.main(["--backbone_net", "resnet", "--modality", "rgb", "--synthetic", "1"] + extra)


def test_mean_std_override_and_its_length_checks():
    from adamml_amd.common import MeanStdMixin
    ms = MeanStdMixin()
    args = _args("rgb", "/nowhere")
    assert TU.mean_std(ms, args) == (ms.mean("rgb"), ms.std("rgb"))
    args.std = [0.5, 0.25, 0.125]
    assert TU.mean_std(ms, args) == (ms.mean("rgb"), [0.5, 0.25, 0.125])
    args.mean = [0.5]
    with pytest.raises(ValueError, match="dim of mean must be three"):
        TU.mean_std(ms, args)
    flow = _args("flow", "/nowhere")
    flow.std = [0.2, 0.2, 0.2]
    with pytest.raises(ValueError, match="training with flow"):
        TU.mean_std(ms, flow)
    assert _args("sound", "/nowhere").input_channels == 1 and flow.input_channels == 10 and _args("rgbdiff", "/nowhere").input_channels == 15
