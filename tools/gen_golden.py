#!/usr/bin/env python3
"""Generate golden fixtures by running the REAL reference (IBM/AdaMML, read-only at
$ADAMML_REF, default /root/reference) on CPU fp32 in the build container.

Only this script ever imports the reference.  Nothing from the reference is copied:
weights / inputs / Gumbel draws come from adamml_amd.synth (name-keyed, torch-RNG
independent), so fixtures hold *outputs only* and the GPU box regenerates identical
inputs from the recipe.  Usage:  python tools/gen_golden.py [case ...]
                                 python tools/gen_golden.py --basic       (the ResNet-18 / -34 cases of tests/golden_cases_basic.py and
                                                                           their manifest tests/golden/state_manifest_basic.json.gz)
"""
import os
import sys
import types
import json
import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = os.environ.get("ADAMML_REF", "/root/reference")
sys.path.insert(1, REF)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

# shim: torchvision is absent but utils/utils.py imports it (SURVEY.md section 8c shim 2)
tv, tvt = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
tvt.Compose = lambda ts: None
tvt.CenterCrop = tvt.Resize = lambda *a, **k: None
tv.transforms = tvt
sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt})

import models  # noqa: E402  (the reference package)
import models.policy_net as pn  # noqa: E402
from utils.utils import compute_policy_loss  # noqa: E402

from adamml_amd import synth  # noqa: E402
from tests.golden_cases import CASES, CH, grad_probe, stat_probe, is_head  # noqa: E402
from tests.golden_cases_basic import CASES_BASIC, MANIFEST_ONLY, arch_key as basic_arch_key, case_state_dict  # noqa: E402

# shim 1: policy_net.py:221 always downloads ImageNet weights; serve a local 3-channel state_dict
pn.model_zoo.load_url = lambda url, **kw: pn.MobileNetV2(1000, num_frames=1, input_channels=3).state_dict()

_EXPO = {"q": None, "i": 0}
_orig_gumbel = F.gumbel_softmax


def _gumbel_softmax(logits, tau=1, hard=False, eps=1e-10, dim=-1):
    """F.gumbel_softmax with the Exponential(1) draw replaced by supplied samples."""
    e = _EXPO["q"]
    if e.dim() == 3 and logits.shape[0] == e.shape[1]:
        ex = e[_EXPO["i"]]
        _EXPO["i"] += 1
    else:
        ex = e.reshape(-1, 2)
    gumbels = -ex.log()
    y_soft = ((logits + gumbels) / tau).softmax(dim)
    index = y_soft.max(dim, keepdim=True)[1]
    y_hard = torch.zeros_like(logits).scatter_(dim, index, 1.0)
    return y_hard - y_soft.detach() + y_soft


F.gumbel_softmax = _gumbel_softmax


def build_adamml(c):
    mod = c["modality"]
    return models.adamml(groups=c["groups"], modality=mod, input_channels=[CH[m] for m in mod],
                         num_segments=c["S"], rng_policy=False, rng_threshold=0.5,
                         causality_modeling=c.get("causality", "lstm"), num_classes=31, depth=c.get("depth", 50),
                         without_t_stride=False, dropout=c.get("dropout", 0.0),
                         pooling_method=c.get("pooling", "max"), fusion_point="logits",
                         unimodality_pretrained=[], learnable_lf_weights=True)


def run_case(name, c):
    """For AdaMML cases the Gumbel seed is searched (7, 8, ...) until every hard decision of every mode has a margin
    |(l1+g1)-(l0+g0)| > 0.25, so that decisions are robust to reduced-precision logit errors; the chosen seed is
    stored in the fixture."""
    if c["kind"] != "adamml":
        return _run_case(name, c, 7)
    need = c.get("margin", 0.25)
    if c.get("full"):
        # a full-size run takes minutes: the policy logits do not depend on the noise (the LSTM is fed the previous LOGITS,
        # models/policy_net.py:347-354), so the seed is searched offline on the logits of one pass
        out = _run_case(name, c, 7)
        if out["min_decision_margin"] > need:
            return out
        plogs = [torch.from_numpy(out[m + ".policy_logits"]) for m in c["modes"]]
        for seed in range(8, 5000):
            e = synth.synth_gumbel_exponential(c["S"], plogs[0].shape[1], c["B"], seed=seed)
            gn = -e.log().reshape(plogs[0].shape[0], plogs[0].shape[1], -1, 2)
            if min(float(((p[..., 1] + gn[..., 1]) - (p[..., 0] + gn[..., 0])).abs().min()) for p in plogs) > need:
                out = _run_case(name, c, seed)
                assert out["min_decision_margin"] > need
                return out
        raise RuntimeError("no robust gumbel seed found for " + name)
    for seed in range(7, 200):
        out = _run_case(name, c, seed)
        if out["min_decision_margin"] > need:
            return out
    raise RuntimeError("no robust gumbel seed found for " + name)


def _run_case(name, c, gumbel_seed):
    torch.manual_seed(0)
    out = {"gumbel_seed": np.array(gumbel_seed)}
    margins = []
    kind = c["kind"]
    if kind == "resnet":
        model = models.resnet(depth=c.get("depth", 50), num_classes=31, without_t_stride=False, groups=c["groups"], dropout=0.0,
                              pooling_method=c.get("pooling", "max"), input_channels=CH[c["modality"][0]],
                              imagenet_pretrained=False)
    elif kind == "sound":
        model = models.sound_mobilenet_v2(num_classes=31, input_channels=1, dropout=0.0, imagenet_pretrained=False)
    else:
        model = build_adamml(c)
    sd = case_state_dict(c, model.state_dict(), seed=1234)       # == synth.synth_state_dict unless the case says otherwise
    model.load_state_dict(sd)
    B, S = c["B"], c.get("S", 1)
    if kind == "adamml":
        xs = synth.synth_inputs(c["modality"], B, S, c["groups"], c["size"], c["sound_size"], seed=42)
    elif kind == "resnet":
        xs = synth.synth_inputs(c["modality"], B, 1, c["groups"], c["size"], seed=42)[0]
    else:
        xs = synth.synth_inputs(["sound"], B, 1, sound_size=c["sound_size"], seed=42)[0]
    target = synth.synth_labels(B, 31, seed=42)

    for mode in c["modes"]:
        model.load_state_dict(sd)
        model.zero_grad()
        if kind == "adamml":
            M = model.num_modality
            _EXPO["q"] = synth.synth_gumbel_exponential(S, M, B, seed=gumbel_seed)
            _EXPO["i"] = 0
            cap = {}
            hook = model.policy_net.register_forward_hook(lambda mod, i, o: cap.__setitem__("plog", o[1].detach()))
            model.policy_net.set_temperature(c.get("tau", 5.0))
            model.unfreeze_policy_net()
            model.unfreeze_main_net()
        if mode == "eval_cal":
            # running statistics := batch statistics of this input (one train-mode pass with momentum 1), then eval
            bns = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]
            for m in bns:
                m.momentum = 1.0
            model.train()
            with torch.no_grad():
                model(xs)
            for m in bns:
                m.momentum = 0.1
                m.num_batches_tracked.zero_()
            _EXPO["i"] = 0
            model.eval()
            with torch.no_grad():
                y = model(xs)
        elif mode == "eval":
            model.eval()
            with torch.no_grad():
                y = model(xs)
        else:
            model.train()
            if kind == "adamml":
                if mode == "train_main":
                    model.freeze_policy_net()
                elif mode == "train_policy":
                    model.freeze_main_net()
            y = model(xs)
        if kind == "adamml":
            hook.remove()
            plog = cap["plog"]                                   # [S, M, B, 2]
            out[mode + ".policy_logits"] = plog.numpy()
            gn = -_EXPO["q"].log().reshape(plog.shape[0], plog.shape[1], -1, 2) if plog.dim() == 4 else None
            margins.append(float(((plog[..., 1] + gn[..., 1]) - (plog[..., 0] + gn[..., 0])).abs().min()))
            logits, sel = y
            out[mode + ".logits"] = logits.detach().numpy()
            out[mode + ".decisions"] = sel.detach().numpy()
            cw = torch.tensor(c.get("cost_weights", [1.0] * sel.shape[-1]))
            gam = torch.tensor(10.0)
            pl_b = compute_policy_loss("blockdrop", sel, cw, gam, logits, target)
            pl_m = compute_policy_loss("mean", sel, cw, gam, logits, target)
            out[mode + ".policy_loss_blockdrop"] = pl_b.detach().numpy()
            out[mode + ".policy_loss_mean"] = pl_m.detach().numpy()
        else:
            logits = y
            out[mode + ".logits"] = logits.detach().numpy()
        ce = F.cross_entropy(logits, target)
        out[mode + ".ce"] = ce.detach().numpy()
        if mode not in ("eval", "eval_cal"):
            loss = ce
            if kind == "adamml" and model.update_policy_net:
                loss = loss + pl_b
            loss.backward()
            gp = {k: grad_probe(k, p.grad) for k, p in model.named_parameters() if p.grad is not None}
            out[mode + ".grad_names"] = np.array(sorted(gp.keys()))
            out[mode + ".grad_probe"] = np.stack([gp[k] for k in sorted(gp.keys())])
            st = {k: stat_probe(v) for k, v in model.state_dict().items()
                  if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
            out[mode + ".stat_names"] = np.array(sorted(st.keys()))
            out[mode + ".stat_probe"] = np.stack([st[k] for k in sorted(st.keys())])
            if c.get("full"):
                msd = model.state_dict()
                keys = [k for k in sorted(msd.keys()) if k.endswith(("running_mean", "running_var"))]
                out[mode + ".stats_full_names"] = np.array(keys)
                out[mode + ".stats_full"] = np.concatenate([msd[k].detach().numpy().reshape(-1) for k in keys]).astype(np.float32)
                for k, p in model.named_parameters():
                    if p.grad is not None and is_head(k):
                        out[mode + ".grad." + k] = p.grad.detach().numpy().astype(np.float32)
    if kind == "adamml":
        out["min_decision_margin"] = np.array(min(margins))
        with torch.no_grad():
            p_x, m_x, _ = model.data_layer(xs, S)
        out["eval.p_x_probe"] = np.stack([stat_probe(t) for t in p_x])
        out["eval.m_x_probe"] = np.stack([stat_probe(t) for t in m_x])
    out["n_state"] = np.array(len(sd))
    return out


def main_basic():
    """The BasicBlock cases: fixtures and a manifest of their own (the existing manifest file is left as it is)."""
    import gzip
    gdir = os.path.join(ROOT, "tests", "golden")
    for n, c in CASES_BASIC.items():
        o = run_case(n, c)
        path = os.path.join(gdir, n + ".npz")
        np.savez_compressed(path, **o)
        print(n, "->", path, os.path.getsize(path), "bytes", flush=True)
    man = {}
    for c in list(CASES_BASIC.values()) + list(MANIFEST_ONLY.values()):
        if c["kind"] == "adamml":
            m = build_adamml(c)
        else:
            m = models.resnet(depth=c["depth"], num_classes=31, without_t_stride=False, groups=8, dropout=0.0,
                              pooling_method="max", input_channels=CH[c["modality"][0]], imagenet_pretrained=False)
        man[basic_arch_key(c)] = {k: [list(v.shape), str(v.dtype)] for k, v in m.state_dict().items()}
    with gzip.GzipFile(os.path.join(gdir, "state_manifest_basic.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(man).encode())


def main():
    if sys.argv[1:] == ["--basic"]:
        return main_basic()
    names = sys.argv[1:] or list(CASES.keys())
    os.makedirs(os.path.join(ROOT, "tests", "golden"), exist_ok=True)
    for n in names:
        o = run_case(n, CASES[n])
        path = os.path.join(ROOT, "tests", "golden", n + ".npz")
        np.savez_compressed(path, **o)
        print(n, "->", path, os.path.getsize(path), "bytes", flush=True)
    # state_dict name/shape manifest (the on-disk contract)
    import gzip
    man = {}
    for n, c in CASES.items():
        key = "%s:%s:%s" % (c["kind"], "+".join(c["modality"]), c.get("causality", "lstm"))
        if key in man:
            continue
        if c["kind"] == "adamml":
            m = build_adamml(c)
        elif c["kind"] == "resnet":
            m = models.resnet(depth=50, num_classes=31, without_t_stride=False, groups=8, dropout=0.0,
                              pooling_method="max", input_channels=CH[c["modality"][0]], imagenet_pretrained=False)
        else:
            m = models.sound_mobilenet_v2(num_classes=31, input_channels=1, dropout=0.0, imagenet_pretrained=False)
        man[key] = {k: [list(v.shape), str(v.dtype)] for k, v in m.state_dict().items()}
    with gzip.open(os.path.join(ROOT, "tests", "golden", "state_manifest.json.gz"), "wt") as f:
        json.dump(man, f)


if __name__ == "__main__":
    main()
