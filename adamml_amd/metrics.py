"""Validation metrics of the reference on the host: mAP (torchnet's APMeter / mAPMeter restated, utils/utils.py:58-86) and the
GFLOPs-per-video estimate (utils/utils.py:510-535).

No device hot path: the inputs are the `[N, K]` logits of one validation pass, once per epoch, so this is numpy / torch on the
CPU and adds nothing to the C ABI.  torchnet is not a dependency.

Deviation from the reference: APMeter orders the samples of a class with `torch.sort(descending=True)`, which is not stable, so
its result is unspecified where scores tie.  Here ties keep the input order (a stable sort)."""
import numpy as np
import torch

# FLOPs of ONE segment (utils/utils.py:512-523): the main nets (ResNet-50 on rgb / flow, MobileNetV2 on sound) and the policy
# backbones (MobileNetV2 on rgb at 160x160, on sound, on rgbdiff) plus the LSTM
MAIN_FLOPS = {"rgb": 14135984128, "flow": 16338911232, "sound": 381739008}
POLICY_FLOPS = {"rgb": 375446400, "sound": 381739008, "rgbdiff": 909283200, "lstm": 2359296}


def _host(t):
    return t.detach().cpu() if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t))


def average_precision(scores, targets):
    """APMeter.value() without weights.  scores [N, K], targets [N, K] (non-zero = positive) -> float64 [K].
    Per class: samples by descending score, ties in input order; with `truth` the reordered targets,
    AP = sum over positives of cumsum(truth)[i] / (i + 1), over max(#positives, 1) -- a class without a positive has AP 0."""
    scores, targets = _host(scores).double().numpy(), _host(targets).numpy()      # (float64 holds every float32 / bf16 score exactly)
    if scores.ndim == 1:
        scores, targets = scores[:, None], targets[:, None]
    if scores.ndim != 2 or scores.shape != targets.shape:
        raise ValueError("average_precision: scores %s and targets %s must both be [N, K]" % (scores.shape, targets.shape))
    n, k = scores.shape
    ap = np.zeros(k, dtype=np.float64)
    if n == 0:
        return ap
    rank = np.arange(1, n + 1, dtype=np.float64)
    for c in range(k):
        order = np.argsort(-scores[:, c], kind="stable")
        truth = (targets[order, c] != 0).astype(np.float64)
        precision = np.cumsum(truth) / rank
        ap[c] = (precision * truth).sum() / max(truth.sum(), 1.0)
    return ap


def mean_average_precision(scores, targets):
    """mAPMeter.value() * 100: every class counts in the mean, those without a positive with 0."""
    return float(average_precision(scores, targets).mean() * 100.0)


def _topk_accuracy(logits, target, topk):
    """train.accuracy's definition (percent of all N), on the host."""
    maxk = min(max(topk), logits.shape[1])
    pred = logits.topk(maxk, 1, True, True)[1].t()
    correct = pred.eq(target.view(1, -1).expand_as(pred))
    return [float(correct[:min(k, maxk)].reshape(-1).float().sum() * (100.0 / target.size(0))) for k in topk]


def actnet_acc(logits, test_y, topk=None, have_softmaxed=False):
    """utils/utils.py:58-86.  logits [N, K]; test_y [N] integer labels or [N, K] multi-hot -> ([top-k accuracies], mAP), Python floats.
    The logits move to the host once; the softmax runs there in float32, so the result does not depend on the machine."""
    logits, test_y = _host(logits).float(), _host(test_y)
    num_classes = logits.shape[1]
    topk = [1, min(5, num_classes)] if topk is None else list(topk)
    probs = logits if have_softmaxed else torch.softmax(logits, dim=1)
    if test_y.dim() == 1:
        acc = _topk_accuracy(logits, test_y.long(), topk)
        gt = torch.zeros_like(logits)
        gt[torch.arange(gt.size(0)), test_y.long().view(-1)] = 1
    else:
        gt = test_y
        acc = [0.0] * len(topk)
    return acc, mean_average_precision(probs, gt)


def flops_computation(modality, ratios, num_segments):
    """utils/utils.py:510-535: GFLOPs per video of `num_segments` segments when modality m's main net runs on the fraction ratios[m]
    of the segments (a float or anything with `.avg`); the policy nets always run.  `modality` is the major modalities
    (train_adamml.py:169-172); one other than rgb / sound costs the flow main net at ratios['flow'] and the rgbdiff policy net."""
    def ratio(m):
        r = ratios[m]
        return float(r.avg if hasattr(r, "avg") else r)

    total = 0.0
    for m in modality:
        if m in ("sound", "rgb"):
            total += MAIN_FLOPS[m] * num_segments * ratio(m) + POLICY_FLOPS[m] * num_segments
        else:
            total += MAIN_FLOPS["flow"] * num_segments * ratio("flow") + POLICY_FLOPS["rgbdiff"] * num_segments
    total += POLICY_FLOPS["lstm"] * num_segments
    return total / 1e9
