"""`train.validate_report` and what the launcher makes of it (the reference's validation line, all_selection*.npz, the logits dump) on
the GPU: mAP against a brute-force reference on the dumped logits, the selection meter as the mean of batch means, the FLOPs
estimate on those ratios, and "what is reported as selected is what ran" (the clips the skipping forward executed)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# as tests/test_train_gpu.py::ARGS
ARGS = ["--backbone_net", "adamml", "-d", "50", "--groups", "8", "--num_segments", "2", "--modality", "rgb", "sound",
        "--causality_modeling", "lstm", "--learnable_lf_weights", "-b", "2", "--input_size", "64", "--epochs", "1",
        "--warmup_epochs", "1", "--finetune_epochs", "1", "--val_num_clips", "2", "--cost_weights", "1.0", "0.05",
        "--synthetic", "2", "--print-freq", "1", "--lr", "0.001", "--p_lr", "0.0001"]
SEED = 2
LABELS = [[3, 17], [3]]
NUM = r"(-?\d+\.\d+)"
REPORT = (r": \tLoss: " + NUM + r"\tTop@1: " + NUM + r"\tTop@5: " + NUM + r"\tmAP: " + NUM + r"\tSpeed: " + NUM + r" ms/batch\tflops: " + NUM
          + r"\tSelection: rgb:" + NUM + r" sound:" + NUM + r" $")


def brute_force_map(probs, targets):
    """100 * mean over classes of AP; AP = mean over the positives i of posrank / rank, with rank = 1 + #{j ahead} and
    posrank = 1 + #{positive j ahead}, j ahead of i when s_j > s_i, or s_j == s_i and j < i.  float64."""
    s, t = np.asarray(probs, dtype=np.float64), np.asarray(targets) != 0
    n, k = s.shape
    ap = np.zeros(k)
    for c in range(k):
        terms = []
        for i in range(n):
            if t[i, c]:
                ahead = [j for j in range(n) if s[j, c] > s[i, c] or (s[j, c] == s[i, c] and j < i)]
                terms.append((1 + sum(1 for j in ahead if t[j, c])) / (1 + len(ahead)))
        ap[c] = np.mean(terms) if terms else 0.0
    return 100.0 * ap.mean()


def val_loader():
    """Two batches of UNEQUAL size (2 videos, then 1) with known labels, on the host."""
    from adamml_amd import synth
    return [(synth.synth_inputs(["rgb", "sound"], len(y), 2, 8, 64, seed=300 + i), torch.tensor(y)) for i, y in enumerate(LABELS)]


def test_evaluate_reports_map_flops_selection_and_what_ran(tmp_path):
    import torch.nn.functional as F
    from adamml_amd import metrics, train
    from adamml_amd.distributed import HipDDP
    argv = ARGS + ["-e", "--logdir", str(tmp_path)]
    loader, lines = val_loader(), []
    torch.manual_seed(SEED)
    res = train.main(argv, val_loader=loader, log=lines.append)
    labels = torch.tensor(sum(LABELS, []))
    folder = os.path.join(str(tmp_path), os.listdir(str(tmp_path))[0])

    # 1. the existing line, with the returned numbers
    old = "Val: Loss {:.4f}\tTop@1 {:.4f}\tTop@5 {:.4f}".format(res["loss"], res["top1"], res["top5"])
    assert old in lines, lines
    # 2. the new line follows it and parses
    new = lines[lines.index(old) + 1]
    m = re.match(r"^Val@64@2" + REPORT, new)
    assert m, repr(new)
    loss, top1, top5, m_ap, speed, flops, pct_rgb, pct_sound = m.groups()
    assert (loss, top1, top5) == ("%.4f" % res["loss"], "%.4f" % res["top1"], "%.4f" % res["top5"])
    assert (m_ap, flops, speed) == ("%.4f" % res["mAP"], "%.2f" % res["flops"], "%.2f" % res["speed_ms"])

    # 3. the logits dump, and mAP on it
    logits = np.load(os.path.join(folder, "val_1crops_2clips_64_details_.npy"))
    assert logits.shape == (3, 31) and logits.dtype == np.float32
    acc, want = metrics.actnet_acc(torch.from_numpy(logits), labels)
    one_hot = np.zeros((3, 31))
    one_hot[np.arange(3), labels.numpy()] = 1
    brute = brute_force_map(torch.softmax(torch.from_numpy(logits), dim=1).numpy(), one_hot)
    print("mAP reported %.12f, actnet_acc %.12f, brute force %.12f" % (res["mAP"], want, brute))
    assert abs(res["mAP"] - want) <= 1e-9 and abs(res["mAP"] - brute) <= 1e-9
    assert abs(acc[0] - res["top1"]) < 1e-4 and abs(acc[1] - res["top5"]) < 1e-4

    # 4. the selections dump
    z = np.load(os.path.join(folder, "all_selection.npz"))
    sel = z["selections"]
    assert sel.shape == (3, 2, 2) and sel.dtype == np.bool_ and str(z["modality"]) == "rgb_sound"

    # 5. the selection meter is the mean of the two batch means -- which, for this seed, is not the mean over the three videos
    batch_means = (sel[:2].mean(axis=(0, 1)) + sel[2:].mean(axis=(0, 1))) / 2.0
    video_means = sel.mean(axis=(0, 1))
    print("selections", sel.astype(int).tolist(), "batch means", batch_means, "video means", video_means)
    assert np.abs(batch_means - video_means).max() > 1e-3, "pick another SEED: both means coincide"
    assert list(res["selection"]) == ["rgb", "sound"]
    assert np.abs(np.array([res["selection"]["rgb"], res["selection"]["sound"]]) - batch_means).max() < 1e-6
    assert (pct_rgb, pct_sound) == ("%.2f" % (100 * res["selection"]["rgb"]), "%.2f" % (100 * res["selection"]["sound"]))
    assert abs(float(pct_rgb) - 100 * batch_means[0]) <= 0.01 and abs(float(pct_sound) - 100 * batch_means[1]) <= 0.01

    # 6. the FLOPs estimate on those ratios
    assert res["flops"] == metrics.flops_computation(["rgb", "sound"], res["selection"], 2)
    assert abs(res["flops"] - metrics.flops_computation(["rgb", "sound"], dict(zip(["rgb", "sound"], batch_means.tolist())), 2)) < 1e-5

    # 7. what is reported as selected is what ran
    assert list(res["executed"]) == ["rgb", "sound"]
    for i, name in enumerate(["rgb", "sound"]):
        assert res["executed"][name] == (int(sel[:, :, i].sum()), 3 * 2), (name, res["executed"])

    # 8. `validate` on the same loader and seed: its four values, unchanged -- equal to the report's, and to top-k / cross entropy
    #    computed from the dumped logits
    torch.manual_seed(SEED)
    args = train.arg_parser().parse_args(argv)
    train.resolve_args(args, log=lambda *_: None)
    model = train.build_model(args)[0].to("cuda")
    out = train.validate(loader, HipDDP(model), args, 2)
    assert len(out) == 4
    v1, v5, vloss, vsel = out
    assert (v1, v5, vloss) == (res["top1"], res["top5"], res["loss"])
    assert vsel.shape == (3, 2, 2) and np.array_equal(vsel.cpu().numpy().astype(bool), sel)
    t1, t5 = train.accuracy(torch.from_numpy(logits), labels)
    ce = (2 * F.cross_entropy(torch.from_numpy(logits[:2]), labels[:2]) + F.cross_entropy(torch.from_numpy(logits[2:]), labels[2:])) / 3
    assert abs(v1 - t1.item()) < 1e-4 and abs(v5 - t5.item()) < 1e-4 and abs(vloss - ce.item()) < 1e-5 * max(1.0, abs(vloss))


def test_training_writes_per_epoch_selections_and_report_lines(tmp_path):
    from adamml_amd import train
    argv = ARGS + ["--logdir", str(tmp_path)]
    argv[argv.index("--warmup_epochs") + 1] = "0"
    lines = []
    torch.manual_seed(SEED)
    res = train.main(argv, log=lines.append)
    for name in ("all_selection_main_1.npz", "all_selection_finetune_1.npz"):
        z = np.load(os.path.join(res["log_folder"], name))
        assert str(z["modality"]) == "rgb_sound"                             # (the reference writes a bare '_' here)
        assert z["selections"].shape == (2, 2, 2) and z["selections"].dtype == np.bool_
    old = [i for i, l in enumerate(lines) if isinstance(l, str) and l.startswith("Val: [001/001]\tLoss ")]
    assert len(old) == 2, lines
    for i in old:
        m = re.match(r"^Val: \[001/001\]" + REPORT, lines[i + 1])
        assert m, repr(lines[i + 1])
        loss, top1, top5 = re.match(r"^Val: \[001/001\]\tLoss " + NUM + r"\tTop@1 " + NUM + r"\tTop@5 " + NUM + "$", lines[i]).groups()
        assert m.groups()[:3] == (loss, top1, top5)


def test_two_ranks_gather_rows_and_average_the_selection(tmp_path):
    """Two ranks on one GPU over gloo (ADAMML_SPAWN_RANKS, as tests/test_train_gpu.py), -e on one synthetic batch of 2 videos per rank:
    the dumps hold both ranks' rows, rank-major, and -- the batches being equal-sized -- the logged selection is their mean."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, ADAMML_SPAWN_RANKS="2", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    argv = ["--multiprocessing-distributed", "--backbone_net", "adamml", "-d", "50", "--groups", "8", "--num_segments", "2", "--modality", "rgb",
            "sound", "--causality_modeling", "lstm", "--learnable_lf_weights", "-b", "4", "-j", "4", "--input_size", "64", "--val_num_clips", "2",
            "--synthetic", "1", "-e", "--dist-backend", "gloo", "--dist-url", "tcp://127.0.0.1:%d" % port, "--logdir", str(tmp_path)]
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "adamml_amd.train"] + argv, cwd=ROOT, env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-4000:]
    folder = os.path.join(str(tmp_path), os.listdir(str(tmp_path))[0])
    sel = np.load(os.path.join(folder, "all_selection.npz"))["selections"]
    logits = np.load(os.path.join(folder, "val_1crops_2clips_64_details_.npy"))
    per_rank = 4 // 2                                                       # one batch of (global batch / ranks) videos on each rank
    assert sel.shape == (2 * per_rank, 2, 2) and logits.shape == (2 * per_rank, 31) and logits.dtype == np.float32
    report = [l for l in run.stdout.splitlines() if l.startswith("Val@64@2")]
    assert len(report) == 1, run.stdout[-4000:]                              # rank 0 only
    m = re.match(r"^Val@64@2" + REPORT, report[0])
    assert m, repr(report[0])
    want = 100.0 * sel.mean(axis=(0, 1))
    assert abs(float(m.group(7)) - want[0]) <= 0.01 and abs(float(m.group(8)) - want[1]) <= 0.01, (report[0], want)
