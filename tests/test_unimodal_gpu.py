"""The unimodal launcher (adamml_amd/train_unimodal.py) on the GPU: its train loop equals the hand-driven sequence bit for bit, the bare
backbones take the loader's objects (video.Frames / EncodedFrames, audio.Waveforms) with the result of the tensor path, the launcher
writes reference-format checkpoints, resumes and evaluates from them, AdaMML's --unimodality_pretrained reads them, and two ranks
end with the same parameters.

Shapes: ResNet-18, 8 frames (all three temporal pools 8 -> 4 -> 2 -> 1) of 64 x 64, two videos per rank (the smallest batch whose
BatchNorm statistics span more than one video); the sound net at its only size, 256 x 256, two videos."""
import gzip
import io
import json
import os
import random
import socket

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from adamml_amd import audio, synth, train, train_unimodal as TU, video as V  # noqa: E402
from adamml_amd.distributed import HipDDP  # noqa: E402
from adamml_amd.model_builder import build_model  # noqa: E402
from adamml_amd.optim import FlatSGD  # noqa: E402
from tests import data_ref as R  # noqa: E402

DEV = "cuda"
GOLDEN = os.path.join(R.ROOT, "tests", "golden")
NET = {"rgb": ["--backbone_net", "resnet", "-d", "18", "--modality", "rgb"],
       "flow": ["--backbone_net", "resnet", "-d", "18", "--modality", "flow"],
       "rgbdiff": ["--backbone_net", "resnet", "-d", "18", "--modality", "rgbdiff"],
       "sound": ["--backbone_net", "sound_mobilenet_v2", "--modality", "sound"]}
COMMON = ["--groups", "8", "--input_size", "64", "-b", "2", "--print-freq", "1000"]


def _quiet(*_):
    pass


def _args(kind, extra=()):
    return TU.resolve_args(train.arg_parser().parse_args(NET[kind] + COMMON + list(extra)))


def _model(kind, extra=(), seed=1234):
    args = _args(kind, extra)
    model, _ = build_model(args)
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=seed))
    return args, model.to(DEV)


def _batches(args, n=2):
    return [(synth.synth_inputs([args.modality], 2, 1, 8, 64, seed=50 + i)[0].to(DEV), synth.synth_labels(2, args.num_classes, seed=50 + i).to(DEV))
            for i in range(n)]


def _contract():
    with open(os.path.join(GOLDEN, "unimodal_contract.json")) as f:
        return json.load(f)


# ---- 1. the loop equals its parts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rgb", "flow", "sound"])
def test_train_loop_equals_the_hand_driven_steps(kind):
    """Two steps of train_epoch against forward, F.cross_entropy, backward, FlatSGD.step, zero_grad from the same synthetic state and the
    same dropout draws: weights, BatchNorm running statistics, momentum buffers and losses are identical (the project's sums are
    order-fixed; no tolerance)."""
    args, a = _model(kind, ["--nesterov"])
    batches = _batches(args)
    assert batches[0][0].shape[1] == {"rgb": 24, "flow": 80, "sound": 1}[kind]
    a.flat_owner.ensure(torch.device(DEV, torch.cuda.current_device()))
    opt_a = FlatSGD(a.flat_owner, args.lr, args.momentum, args.weight_decay, args.nesterov)
    torch.manual_seed(5)
    meters = TU.train_epoch(batches, HipDDP(a), opt_a, 1, args, 0, _quiet)

    _, b = _model(kind, ["--nesterov"])
    b.train()
    b.flat_owner.ensure(torch.device(DEV, torch.cuda.current_device()))
    opt_b = FlatSGD(b.flat_owner, args.lr, args.momentum, args.weight_decay, args.nesterov)
    torch.manual_seed(5)
    losses = []
    for x, y in batches:
        loss = F.cross_entropy(b(x), y)
        loss.backward()
        opt_b.step()
        opt_b.zero_grad()
        losses.append(loss.item())
    print("  %s losses: loop %s, by hand %s" % (kind, meters["losses"], losses))
    assert meters["losses"] == losses and len(losses) == 2 and all(np.isfinite(losses)) and losses[0] != losses[1]
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    first = next(k for k in sa if k.endswith("num_batches_tracked"))
    assert int(sa[first]) == 2
    assert opt_a.steps == 2 and torch.equal(opt_a.mom, opt_b.mom) and float(opt_a.mom.abs().max()) > 0
    assert meters["loss"].n == 4 and abs(meters["loss"].avg - sum(losses) / 2) < 1e-12


# ---- 2. device-side inputs ------------------------------------------------------------------------------------------------------------
W0, H0 = 80, 60
FILES = {"rgb": 8, "flow": 80, "rgbdiff": 48}


def _videos(modality, n=2):
    """Per video the JPEG files (80 x 60) of 8 frame groups in Stack's order, and their Pillow pixels [H, W, K_in]."""
    files = [[R.jpeg_bytes(1000 * i + j, gray=modality == "flow", h=H0, w=W0) for j in range(FILES[modality])] for i in range(n)]
    pixels = [np.ascontiguousarray(np.concatenate([R.pil_pixels(b) for b in v], axis=2)) for v in files]
    return files, pixels


def _host_normalised(u8, mean, std):
    """ToTorchFormatTensor + GroupNormalize on the host (tests/test_options_gpu.py builds x the same way): [N, K, H, W] fp32."""
    x = u8.cpu().permute(0, 3, 1, 2).float().div(255)
    rep = x.shape[1] // len(mean)
    return (x - torch.tensor(list(mean) * rep).view(1, -1, 1, 1)) / torch.tensor(list(std) * rep).view(1, -1, 1, 1)


def _forward(net, x, training):
    """Eval mode without autograd, or one train-mode call with its backward (every recorded tape is run)."""
    net.train(training)
    if not training:
        with torch.no_grad():
            return net(x)
    out = net(x)
    out.sum().backward()
    return out.detach()


@pytest.mark.parametrize("modality", ["rgb", "flow", "rgbdiff"])
def test_resnet_takes_frames_and_encoded_frames(modality):
    """net(Frames) == net(EncodedFrames) == net(x32), bit for bit, x32 the host's normalisation of the same augmented uint8 pixels:
    train and val geometry, eval and train mode."""
    args, net = _model(modality, ["--dropout", "0", "--scale_range", "72", "80"])
    net.input_modality = args.modality
    files, pixels = _videos(modality)
    mean, std = net.mean(modality), net.std(modality)
    for is_train in (True, False):
        random.seed(3)
        np.random.seed(3)
        aug = V.augmentor_for(args, modality, is_train)
        geos = [aug.sample(W0, H0) for _ in files]
        enc, dec = V.EncodedFrames(files, geos).to(DEV), V.Frames(pixels, geos).to(DEV)
        u8 = V.augment(enc)
        assert u8.shape == (2, 64, 64, 8 * args.input_channels) and torch.equal(u8, V.augment(dec))
        x32 = _host_normalised(u8, mean, std).to(DEV)
        for training in (False, True):
            want, got_dec, got_enc = _forward(net, x32, training), _forward(net, dec, training), _forward(net, enc, training)
            assert want.shape == (2, args.num_classes) and torch.isfinite(want).all()
            assert torch.equal(got_dec, want) and torch.equal(got_enc, want), (modality, is_train, training)
    # an override (--std) changes the result, and the result is the tensor path's with the same override
    plain = _forward(net, dec, False)
    over = [0.5, 0.25, 0.125] if modality != "flow" else [0.5]
    net.input_std = over
    got, base = _forward(net, dec, False), _forward(net, _host_normalised(u8, mean, over).to(DEV), False)
    assert torch.equal(got, base) and not torch.equal(got, plain)
    # a clip of another modality or frame count is refused
    other = "flow" if modality != "flow" else "rgb"
    o_files, _ = _videos(other, 1)
    bad = V.EncodedFrames(o_files, [V.augmentor_for(args, other, False).sample(W0, H0)]).to(DEV)
    with pytest.raises(ValueError, match="Frames"):
        net(bad)
    short = V.Frames([p[:, :, :p.shape[2] // 2] for p in pixels], geos).to(DEV)
    with pytest.raises(ValueError, match="Frames"):
        net(short)


def test_launcher_sets_the_normalisation_on_the_model(tmp_path):
    """--std reaches the model through the launcher: evaluating Frames batches equals evaluating their host-normalised tensors."""
    files, pixels = _videos("rgb")
    geos = [V.Augmentor(False, 64, modality="rgb").sample(W0, H0) for _ in files]
    y = torch.tensor([0, 1])
    argv = NET["rgb"] + COMMON + ["--num_classes", "2", "-e", "--std", "0.5", "0.25", "0.125", "--logdir", str(tmp_path)]
    torch.manual_seed(11)
    a = TU.main(argv, val_loader=[(V.Frames(pixels, geos), y)], log=_quiet)
    u8 = V.augment(V.Frames(pixels, geos).to(DEV))
    torch.manual_seed(11)
    b = TU.main(argv, val_loader=[(_host_normalised(u8, [0.485, 0.456, 0.406], [0.5, 0.25, 0.125]), y)], log=_quiet)
    torch.manual_seed(11)
    c = TU.main(argv[:-6] + argv[-2:], val_loader=[(V.Frames(pixels, geos), y)], log=_quiet)
    assert a == b and a["loss"] != c["loss"]


def test_sound_net_takes_waveforms():
    args, net = _model("sound", ["--dropout", "0"])
    rng = np.random.default_rng(2)
    wave = (rng.standard_normal((2, 1, 30720)) * 0.1).astype(np.float32)
    wf = audio.Waveforms(wave, np.array([[False], [True]])).to(DEV)
    spec = wf.spectrogram(sample_rate=args.resampling_rate)
    assert spec.shape == (2, 1, 256, 256) and not spec[1].any() and spec[0].abs().max() > 0
    for training in (False, True):
        want, got = _forward(net, spec, training), _forward(net, wf, training)
        assert want.shape == (2, args.num_classes) and torch.equal(got, want)
    with pytest.raises(ValueError, match="one"):
        net(audio.Waveforms(np.zeros((2, 2, 30720), np.float32)).to(DEV))


# ---- 3. launcher end to end -----------------------------------------------------------------------------------------------------------
RUN = ["--num_classes", "2", "--synthetic", "2", "--dropout", "0", "--lr_scheduler", "step", "--lr_steps", "100"]


def _val_loader(kind):
    """One batch: the same clip twice with the labels 0 and 1.  Eval-mode logits depend on the sample alone, so exactly one of the two is
    right whatever the weights: top-1 is 50 in every validation, and the first one is the best model."""
    x = synth.synth_inputs([kind], 1, 1, 8, 64, seed=9)[0]
    return [(x.repeat(2, 1, 1, 1), torch.tensor([0, 1]))]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Two epochs of two synthetic batches for the rgb ResNet-18 and the sound net, through main()."""
    out = {}
    for kind in ("rgb", "sound"):
        logdir = str(tmp_path_factory.mktemp(kind))
        lines = []
        torch.manual_seed(21)                                                   # the initial weights (test_resume_... starts from the same)
        res = TU.main(NET[kind] + COMMON + RUN + ["--epochs", "2", "--logdir", logdir], val_loader=_val_loader(kind), log=lines.append)
        res["final"] = {k: v.detach().cpu().clone() for k, v in res["model"].state_dict().items()}
        out[kind] = dict(res=res, logdir=logdir, lines=lines)
    return out


@pytest.mark.parametrize("kind", ["rgb", "sound"])
def test_launcher_writes_reference_format_checkpoints(runs, kind):
    run = runs[kind]
    res, folder = run["res"], run["res"]["log_folder"]
    assert os.path.basename(folder) == "kinetics-sounds-%s-%s-f8-step-bs2-e2" % (kind, "resnet" if kind == "rgb" else "sound_mobilenet_v2")
    assert sorted(os.listdir(folder)) == ["checkpoint.pth.tar", "log.log", "model_best.pth.tar"]
    assert [e for e, _ in res["history"]] == [1, 2] and all(len(l) == 2 and all(np.isfinite(l)) for _, l in res["history"])
    assert res["last_val"][0] == 50.0 and res["best_top1"] == 50.0
    ck = torch.load(os.path.join(folder, "checkpoint.pth.tar"), map_location="cpu")
    best = torch.load(os.path.join(folder, "model_best.pth.tar"), map_location="cpu")
    assert set(ck) == set(best) == {"epoch", "arch", "state_dict", "best_top1", "optimizer", "scheduler"}
    assert (ck["epoch"], best["epoch"], ck["arch"], ck["best_top1"]) == (2, 1, os.path.basename(folder), 50.0)
    # names, shapes and dtypes of the reference's DataParallel state_dict (the head has this run's two classes)
    if kind == "sound":
        manifest = [(k, s, d) for k, s, d in _contract()["recipes"][2]["state_dict"]]
    else:
        with gzip.open(os.path.join(GOLDEN, "state_manifest_basic.json.gz")) as f:
            manifest = [("module." + k, s, d) for k, (s, d) in json.load(f)["resnet18:rgb"].items()]
    assert list(ck["state_dict"]) == [k for k, _, _ in manifest]
    for k, shape, dtype in manifest:
        t = ck["state_dict"][k]
        assert str(t.dtype) == dtype and list(t.shape) == ([2] + shape[1:] if shape[:1] == [31] else shape), k
        assert torch.equal(t, res["final"][k[7:]]), k
    steps = [int(v) for k, v in ck["state_dict"].items() if k.endswith("num_batches_tracked")]
    assert steps and set(steps) == {4}                                          # 2 epochs x 2 batches, one train-mode call each
    # the optimizer is torch.optim.SGD's: the reference's group keys and values, one momentum buffer per parameter
    want = _contract()["recipes"][0 if kind == "rgb" else 2]["optimizer"]
    osd = ck["optimizer"]
    shapes = [list(p.shape) for p in res["model"].parameters()]
    assert sorted(osd) == want["keys"] and len(osd["param_groups"]) == 1
    group = dict(osd["param_groups"][0])
    assert group.pop("params") == list(range(len(shapes))) and group == {k: v for k, v in want["param_groups"][0].items() if k != "params"}
    assert sorted(osd["state"]) == list(range(len(shapes))) and all(sorted(e) == want["state_keys"] for e in osd["state"].values())
    assert [list(osd["state"][i]["momentum_buffer"].shape) for i in range(len(shapes))] == shapes
    if kind == "sound":
        assert shapes[:-2] == want["momentum_buffer_shapes"][:-2] and len(shapes) == want["num_params"]
    sgd = torch.optim.SGD([torch.nn.Parameter(torch.zeros(s)) for s in shapes], lr=0.5, momentum=0.1)
    sgd.load_state_dict(osd)
    assert sgd.param_groups[0]["lr"] == 0.01 and torch.equal(sgd.state[sgd.param_groups[0]["params"][0]]["momentum_buffer"], osd["state"][0]["momentum_buffer"])
    assert set(ck["scheduler"]) <= set(_contract()["scheduler_keys"]["step"]) and ck["scheduler"]["last_epoch"] == 2
    # the log holds the reference's lines
    log = open(os.path.join(folder, "log.log")).read()
    assert log.count("Train: [") == 2 and "Val  : [002/002]\tLoss: " in log and "Train: [001/002]\tLoss: " in "\n".join(run["lines"])


def test_evaluate_reports_the_last_validation(runs):
    run = runs["rgb"]
    lines = []
    ck = os.path.join(run["res"]["log_folder"], "checkpoint.pth.tar")
    res = TU.main(NET["rgb"] + COMMON + ["--num_classes", "2", "--dropout", "0", "-e", "--pretrained", ck, "--logdir", run["logdir"]],
                  val_loader=_val_loader("rgb"), log=lines.append)
    top1, top5, loss = run["res"]["last_val"]
    assert (res["top1"], res["top5"], res["loss"]) == (top1, top5, loss)
    val = [l for l in lines if l.startswith("Val@64: \tLoss: ")]
    assert len(val) == 1 and "Top@1: 50.0000" in val[0] and "Params: " in val[0]


def test_resume_continues_bit_identically(runs, tmp_path):
    """One epoch, then --resume for the second: the weights, statistics and momentum of the straight two-epoch run."""
    torch.manual_seed(21)
    one = TU.main(NET["rgb"] + COMMON + RUN + ["--epochs", "1", "--logdir", str(tmp_path)], val_loader=_val_loader("rgb"), log=_quiet)
    ck = os.path.join(one["log_folder"], "checkpoint.pth.tar")
    two = TU.main(NET["rgb"] + COMMON + RUN + ["--epochs", "2", "--resume", ck, "--logdir", str(tmp_path)], val_loader=_val_loader("rgb"), log=_quiet)
    straight = runs["rgb"]["res"]
    assert [e for e, _ in two["history"]] == [2] and two["history"][0][1] == straight["history"][1][1]
    for k, v in two["model"].state_dict().items():
        assert torch.equal(v.cpu(), straight["final"][k]), k
    a = torch.load(os.path.join(two["log_folder"], "checkpoint.pth.tar"), map_location="cpu")
    b = torch.load(os.path.join(straight["log_folder"], "checkpoint.pth.tar"), map_location="cpu")
    assert a["epoch"] == 2 and all(torch.equal(a["optimizer"]["state"][i]["momentum_buffer"], b["optimizer"]["state"][i]["momentum_buffer"])
                                   for i in b["optimizer"]["state"])


def test_a_reference_format_checkpoint_resumes(tmp_path):
    """What the reference's train_unimodal.py saves, rebuilt from the manifest of its ResNet-18 with synthetic values: DataParallel names,
    torch.optim.SGD and MultiStepLR state, best_top1 as a tensor."""
    with gzip.open(os.path.join(GOLDEN, "state_manifest_basic.json.gz")) as f:
        manifest = json.load(f)["resnet18:rgb"]
    sd = synth.synth_state_dict({k: torch.zeros(s, dtype=getattr(torch, d.split(".")[1])) for k, (s, d) in manifest.items()}, seed=77)
    params = [torch.nn.Parameter(v.clone()) for k, v in sd.items() if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]
    sgd = torch.optim.SGD(params, 0.01, momentum=0.9, weight_decay=1e-4)
    for p in params:
        p.grad = torch.full_like(p, 0.25)
    sgd.step()
    sched = torch.optim.lr_scheduler.MultiStepLR(sgd, [20, 40, 50], gamma=0.1)
    path = str(tmp_path / "reference.pth.tar")
    torch.save({"epoch": 1, "arch": "reference", "state_dict": {"module." + k: v for k, v in sd.items()}, "best_top1": torch.tensor(12.5),
                "optimizer": sgd.state_dict(), "scheduler": sched.state_dict()}, path)
    buf = io.StringIO()
    res = TU.main(NET["rgb"] + COMMON + ["--synthetic", "1", "--dropout", "0", "--lr_scheduler", "multisteps", "--lr_steps", "20", "40", "50",
                                         "--epochs", "2", "--resume", path, "--logdir", str(tmp_path)], log=lambda s: buf.write(s + "\n"))
    assert "=> loaded checkpoint '%s' (epoch 1)" % path in buf.getvalue()
    assert [e for e, _ in res["history"]] == [2] and np.isfinite(res["history"][0][1]).all() and res["best_top1"] >= 12.5
    ck = torch.load(os.path.join(res["log_folder"], "checkpoint.pth.tar"), map_location="cpu")
    assert ck["epoch"] == 2 and int(ck["state_dict"]["module.bn1.num_batches_tracked"]) == 1
    # the restored momentum took part in the step: 0.9 x the saved buffer + the new gradient
    assert not torch.equal(ck["optimizer"]["state"][0]["momentum_buffer"], sgd.state_dict()["state"][0]["momentum_buffer"])
    assert not torch.equal(ck["state_dict"]["module.conv1.weight"], sd["conv1.weight"])


# ---- 4. hand-off ----------------------------------------------------------------------------------------------------------------------
def test_adamml_reads_the_unimodal_checkpoints(runs):
    paths = [os.path.join(runs[k]["res"]["log_folder"], "checkpoint.pth.tar") for k in ("rgb", "sound")]
    args = train.arg_parser().parse_args(["--backbone_net", "adamml", "-d", "18", "--groups", "8", "--modality", "rgb", "sound", "--num_classes", "2",
                                          "--causality_modeling", "lstm", "--unimodality_pretrained"] + paths)
    train.resolve_args(args, log=_quiet)
    model, _ = build_model(args)
    for i, kind in enumerate(("rgb", "sound")):
        got, want = model.main_net.nets[i].state_dict(), runs[kind]["res"]["final"]
        assert list(got) == list(want)
        for k in want:
            assert torch.equal(got[k].cpu(), want[k]), (kind, k)
        assert int(got[next(k for k in got if k.endswith("num_batches_tracked"))]) == 4


# ---- 5. two ranks ---------------------------------------------------------------------------------------------------------------------
def test_two_ranks_end_with_the_same_parameters(tmp_path, monkeypatch):
    """Two ranks share the one GPU over gloo (as tests/test_train_gpu.py sets its two ranks up), SyncBatchNorm on, one epoch of one batch of
    the sound net: every rank ends with the same parameters and statistics, the gradients went through at least one all-reduce, rank 0
    alone wrote a checkpoint."""
    import torch.multiprocessing as mp
    from tests import unimodal_ranks
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    argv = ["--multiprocessing-distributed"] + NET["sound"] + ["-b", "4", "--synthetic", "1", "--epochs", "1", "--sync-bn", "--dropout", "0",
                                                               "--dist-backend", "gloo", "--dist-url", "tcp://127.0.0.1:%d" % port, "--logdir", str(tmp_path / "log")]
    out = tmp_path / "out"
    out.mkdir()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=unimodal_ranks.rank_main, args=(r, 2, argv, str(out))) for r in (0, 1)]
    for p in procs:
        p.start()
    try:
        for p in procs:
            p.join(timeout=240)
            assert p.exitcode == 0, "rank process ended with %r" % (p.exitcode,)      # nothing more is started after an abnormal end
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    ranks = [json.load(open(str(out / ("rank%d.json" % r)))) for r in (0, 1)]
    assert [r["rank"] for r in ranks] == [0, 1] and all(r["sync"] for r in ranks)
    assert ranks[0]["digest"] == ranks[1]["digest"]
    assert all(r["stats"]["bucket_all_reduces"] + r["stats"]["gap_all_reduces"] >= 1 for r in ranks)
    assert ranks[0]["losses"] != ranks[1]["losses"] and all(np.isfinite(r["losses"]).all() for r in ranks)      # each rank its own half
    folders = os.listdir(str(tmp_path / "log"))
    assert folders == ["kinetics-sounds-sound-sound_mobilenet_v2-f8-cosine-syncbn-bs4-e1"]
    saved = sorted(f for f in os.listdir(str(tmp_path / "log" / folders[0])) if f.endswith(".pth.tar"))
    assert saved in (["checkpoint.pth.tar"], ["checkpoint.pth.tar", "model_best.pth.tar"])
    ck = torch.load(str(tmp_path / "log" / folders[0] / "checkpoint.pth.tar"), map_location="cpu")
    assert ck["epoch"] == 1 and unimodal_ranks.state_digest(_Bag({k[7:]: v for k, v in ck["state_dict"].items()})) == ranks[0]["digest"]


def test_multiprocessing_distributed_spawns_the_ranks(tmp_path, monkeypatch):
    """The flag itself (train_unimodal.py:52-61), as tests/test_train_gpu.py runs it for train_adamml: main() starts the two ranks with
    torch.multiprocessing.spawn, which ends them all when one fails; rank 0 leaves the checkpoint of the one epoch."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    monkeypatch.setenv("ADAMML_SPAWN_RANKS", "2")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    assert TU.main(["--multiprocessing-distributed"] + NET["sound"] + ["-b", "4", "--synthetic", "1", "--epochs", "1", "--sync-bn", "--dist-backend", "gloo",
                                                                      "--dist-url", "tcp://127.0.0.1:%d" % port, "--logdir", str(tmp_path)]) is None
    folder = tmp_path / "kinetics-sounds-sound-sound_mobilenet_v2-f8-cosine-syncbn-bs4-e1"
    ck = torch.load(str(folder / "checkpoint.pth.tar"), map_location="cpu")
    assert ck["epoch"] == 1 and int(ck["state_dict"]["module.features.0.1.num_batches_tracked"]) == 1
    assert all(torch.isfinite(v).all() for v in ck["state_dict"].values() if v.is_floating_point())
    assert "Train: [001/001]" in (folder / "log.log").read_text()


class _Bag:
    def __init__(self, sd):
        self._sd = sd

    def state_dict(self):
        return self._sd
