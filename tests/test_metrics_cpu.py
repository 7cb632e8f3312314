"""adamml_amd.metrics on the host: average precision / mAP (torchnet's APMeter restated, ties in input order), `actnet_acc` and the
GFLOPs estimate.

mAP has no golden from the reference (its `actnet_acc` needs torchnet: tools/gen_golden_metrics.py), so it is pinned by three
independent references: a brute-force float64 rank count written here, a float32 restatement of APMeter in torch, and sklearn where it
imports.  `flops_computation` is checked against what the reference's own function returned (tests/golden/flops_cases.json)."""
import json
import os
import time

import numpy as np
import pytest
import torch

from adamml_amd import metrics

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def brute_force_ap(scores, targets):
    """float64 [K].  For each positive i: rank = 1 + #{j ahead}, posrank = 1 + #{positive j ahead}, where j is ahead of i when
    s_j > s_i, or s_j == s_i and j < i; AP = mean over the positives of posrank / rank (0 without a positive)."""
    s, t = np.asarray(scores, dtype=np.float64), np.asarray(targets) != 0
    n, k = s.shape
    idx = np.arange(n)
    ap = np.zeros(k, dtype=np.float64)
    for c in range(k):
        ahead = (s[None, :, c] > s[:, None, c]) | ((s[None, :, c] == s[:, None, c]) & (idx[None, :] < idx[:, None]))   # [i, j]
        rank = 1 + ahead.sum(1)
        posrank = 1 + (ahead & t[None, :, c]).sum(1)
        if t[:, c].any():
            ap[c] = (posrank[t[:, c]] / rank[t[:, c]]).mean()
    return ap


def apmeter_float32(scores, targets):
    """torchnet's APMeter.value() in its own precision: (stable) sort, float cumsum, div, float32 sum.  float32 [K]."""
    scores, targets = torch.as_tensor(scores, dtype=torch.float32), torch.as_tensor(targets)
    n, k = scores.shape
    rg = torch.arange(1, n + 1).float()
    ap = torch.zeros(k)
    for c in range(k):
        order = torch.sort(scores[:, c], dim=0, descending=True, stable=True)[1]
        truth = targets[:, c][order]
        precision = truth.float().cumsum(0).div(rg)
        ap[c] = precision[truth.bool()].sum() / max(float(truth.sum()), 1)
    return ap


def one_hot(labels, k):
    t = np.zeros((len(labels), k), dtype=np.int64)
    t[np.arange(len(labels)), labels] = 1
    return t


@pytest.fixture(scope="module")
def tied():
    """N = 257, K = 7: logits 3 * randn, every fifth row overwritten by its neighbour (exact ties in every class), class 6 without
    a positive.  -> (probabilities float32 [N, K], labels [N], one-hot targets, brute-force AP)."""
    g = torch.Generator().manual_seed(20240607)
    n, k = 257, 7
    logits = 3.0 * torch.randn(n, k, generator=g)
    logits[4::5] = logits[3::5][:logits[4::5].shape[0]]
    labels = torch.randint(0, k - 1, (n,), generator=g)
    probs = torch.softmax(logits, dim=1)
    targets = one_hot(labels.numpy(), k)
    assert len(np.unique(probs[:, 0].numpy())) < n and targets[:, 6].sum() == 0
    return logits, probs, labels, targets, brute_force_ap(probs.numpy(), targets)


# ------------------------------------------------------------------------------------------------ hand cases
def test_hand_case():
    ap = metrics.average_precision(np.array([[.9], [.8], [.7], [.6]]), np.array([[1], [0], [1], [0]]))
    assert ap.dtype == np.float64 and ap.shape == (1,)
    assert abs(ap[0] - 5.0 / 6.0) < 1e-15                                    # (1/1 + 2/3) / 2


def test_ties_keep_input_order():
    s = np.array([[.5], [.5]])
    assert metrics.average_precision(s, np.array([[0], [1]]))[0] == 0.5
    assert metrics.average_precision(s, np.array([[1], [0]]))[0] == 1.0


def test_class_without_a_positive_is_zero_and_counts_in_the_mean():
    s = np.array([[.9, .1], [.8, .2], [.7, .3], [.6, .4]])
    t = np.array([[1, 0], [0, 0], [1, 0], [0, 0]])
    ap = metrics.average_precision(s, t)
    assert ap[1] == 0.0 and abs(ap[0] - 5.0 / 6.0) < 1e-15
    assert abs(metrics.mean_average_precision(s, t) - 100.0 * (5.0 / 6.0) / 2.0) < 1e-12
    assert isinstance(metrics.mean_average_precision(s, t), float)


# ------------------------------------------------------------------------------------------------ random data with ties
def test_against_brute_force_with_ties(tied):
    _, probs, _, targets, want = tied
    got = metrics.average_precision(probs, torch.from_numpy(targets))
    err = np.abs(got - want).max()
    print("max |AP - brute force| =", err)
    assert got.dtype == np.float64 and got[6] == 0.0
    assert err <= 1e-12
    assert abs(metrics.mean_average_precision(probs, targets) - 100.0 * want.mean()) <= 1e-10


def test_against_float32_apmeter_restatement(tied):
    _, probs, _, targets, _ = tied
    got = metrics.average_precision(probs, targets)
    ref = apmeter_float32(probs, targets).double().numpy()
    for c in range(probs.shape[1]):
        p = int(targets[:, c].sum())
        bound = (p + 1) * 2.0 ** -24                                        # one rounding per term + the float32 sum, relative
        err = abs(got[c] - ref[c]) / max(abs(got[c]), 1e-300) if got[c] else abs(ref[c])
        print("class %d: P = %d, relative difference %.3g (bound %.3g)" % (c, p, err, bound))
        assert err <= bound, (c, err, bound)


def test_against_sklearn_without_ties():
    skm = pytest.importorskip("sklearn.metrics")
    g = torch.Generator().manual_seed(7)
    n, k = 257, 7
    probs = torch.softmax(3.0 * torch.randn(n, k, generator=g), dim=1).numpy()
    assert all(len(np.unique(probs[:, c])) == n for c in range(k))          # no ties
    targets = one_hot(torch.randint(0, k - 1, (n,), generator=g).numpy(), k)
    got = metrics.average_precision(probs, targets)
    for c in range(k):
        if targets[:, c].any():
            want = skm.average_precision_score(targets[:, c], probs[:, c].astype(np.float64))
            assert abs(got[c] - want) <= 1e-9, (c, got[c], want)


def test_multi_hot_targets(tied):
    _, probs, _, _, _ = tied
    g = torch.Generator().manual_seed(11)
    targets = (torch.rand(probs.shape, generator=g) < 0.3).long()
    targets[:, 2] = 0
    targets[:, 2][5] = 3                                                    # non-zero means positive
    got = metrics.average_precision(probs, targets)
    assert np.abs(got - brute_force_ap(probs.numpy(), targets.numpy())).max() <= 1e-12


# ------------------------------------------------------------------------------------------------ actnet_acc
def test_actnet_acc_matches_train_accuracy_and_the_brute_force(tied):
    from adamml_amd import train
    logits, probs, labels, targets, want = tied
    acc, m_ap = metrics.actnet_acc(logits, labels)
    top1, top5 = train.accuracy(logits, labels)
    assert acc == [top1.item(), top5.item()]
    assert all(isinstance(v, float) for v in acc) and isinstance(m_ap, float)
    assert abs(m_ap - 100.0 * want.mean()) <= 1e-10                          # softmax in float32 on the host, as the fixture's
    # multi-hot targets: no accuracies (the reference returns [0, 0]); the mAP of the same one-hot matrix is unchanged
    acc_mh, m_ap_mh = metrics.actnet_acc(logits, torch.from_numpy(targets))
    assert acc_mh == [0, 0] and m_ap_mh == m_ap


def test_actnet_acc_three_classes_and_explicit_topk():
    g = torch.Generator().manual_seed(3)
    logits, labels = torch.randn(20, 3, generator=g), torch.randint(0, 3, (20,), generator=g)
    acc, _ = metrics.actnet_acc(logits, labels)                              # topk = [1, min(5, 3)]
    assert len(acc) == 2 and acc[1] == 100.0
    assert abs(acc[0] - int((logits.argmax(1) == labels).sum()) * 100.0 / 20) < 1e-4
    acc2, _ = metrics.actnet_acc(logits, labels, topk=[1, 2])
    assert acc2[0] == acc[0] and acc[0] <= acc2[1] <= 100.0


def test_actnet_acc_have_softmaxed_skips_the_softmax():
    g = torch.Generator().manual_seed(5)
    logits, labels = 3.0 * torch.randn(33, 4, generator=g), torch.randint(0, 4, (33,), generator=g)
    probs = torch.softmax(logits, dim=1)
    _, a = metrics.actnet_acc(logits, labels)
    _, b = metrics.actnet_acc(probs, labels, have_softmaxed=True)
    assert a == b
    # scores used as they are: AP of the raw values, not of softmax(softmax(.))
    raw = torch.tensor([[.2, .8], [.9, .1], [.6, .4], [.3, .7]])
    y = torch.tensor([0, 0, 1, 1])
    _, c = metrics.actnet_acc(raw, y, have_softmaxed=True)
    assert abs(c - 100.0 * brute_force_ap(raw.numpy(), one_hot(y.numpy(), 2)).mean()) <= 1e-12


# ------------------------------------------------------------------------------------------------ flops_computation
def test_flops_against_the_reference_cases():
    with open(os.path.join(GOLDEN, "flops_cases.json")) as f:
        cases = json.load(f)["cases"]
    assert len(cases) >= 12
    assert {len(c["modality"]) for c in cases} == {2, 3, 4} and {c["num_segments"] for c in cases} == {1, 5, 10}
    for c in cases:
        got = metrics.flops_computation(c["modality"], c["ratios"], c["num_segments"])
        assert isinstance(got, float)
        assert abs(got - c["gflops"]) <= 1e-12 * abs(c["gflops"]), (c, got)


def test_flops_hand_values_and_meters():
    from adamml_amd.train import Meter
    assert abs(metrics.flops_computation(["rgb", "sound"], {"rgb": 0.25, "sound": 0.75}, 5) - 22.89922496) <= 1e-12 * 22.89922496
    three = {"rgb": 0.5, "sound": 1.0, "flow": 0.125}
    assert abs(metrics.flops_computation(["rgb", "sound", "flow"], three, 10) - 111.6092288) <= 1e-12 * 111.6092288
    meters = {k: Meter() for k in three}
    for k, v in three.items():
        meters[k].update(v)
    assert metrics.flops_computation(["rgb", "sound", "flow"], meters, 10) == metrics.flops_computation(["rgb", "sound", "flow"], three, 10)


# ------------------------------------------------------------------------------------------------ scale
def test_scale_50000_by_240():
    g = torch.Generator().manual_seed(1)
    n, k = 50000, 240
    logits = torch.randn(n, k, generator=g)
    labels = torch.randint(0, k, (n,), generator=g)
    t0 = time.time()
    acc, m_ap = metrics.actnet_acc(logits, labels)
    print("actnet_acc at N = %d, K = %d: %.2f s" % (n, k, time.time() - t0))
    assert 0.0 < m_ap < 100.0 and 0.0 <= acc[0] <= acc[1] <= 100.0
    # one class against the float32 restatement (P ~ N / K positives)
    c = 17
    probs = torch.softmax(logits, dim=1)[:, c:c + 1]
    targets = (labels == c).long()[:, None]
    got, ref = metrics.average_precision(probs, targets)[0], float(apmeter_float32(probs, targets)[0])
    assert abs(got - ref) <= (int(targets.sum()) + 1) * 2.0 ** -24 * got
