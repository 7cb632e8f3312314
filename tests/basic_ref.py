"""TEST INFRASTRUCTURE ONLY: functional restatement of the reference's BasicBlock ResNet forward (models/resnet.py:46-74, depth 18 / 34),
built from the primitives of oracle/adamml_oracle.py (conv, batchnorm, temporal_pool, dropout and the QUANT storage hook), which are
imported and not copied: the same code yields the exact fp32 run (pinned against goldens of the real reference by
tests/test_resnet_basic_cpu.py) and the bf16-storage emulation the HIP path is held to.  basic_case() returns the record layout of
tests/oracle_harness.oracle_case."""
import gzip
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import adamml_oracle as O
from tests.golden_cases import grad_probe, stat_probe
from tests.golden_cases_basic import arch_key, case_state_dict
from tests.oracle_harness import GOLDEN_DIR, case_inputs

BASIC_BLOCKS = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3)}     # models/resnet.py:124-126


def _q(x):
    """The storage hook of the oracle: identity for the fp32 run, bf16 straight-through rounding for the emulation."""
    return x if O.QUANT is None else O.QUANT(x)


def basic_block(sd, p, x, stride, has_down, training):
    """models/resnet.py:59-74."""
    out = O.conv(x, sd[p + ".conv1.weight"], stride=stride, padding=1)
    out = F.relu(O.batchnorm(sd, p + ".bn1", out, training))
    out = O.conv(out, sd[p + ".conv2.weight"], padding=1)
    out = O.batchnorm(sd, p + ".bn2", out, training)
    if has_down:
        idt = O.conv(x, sd[p + ".downsample.0.weight"], stride=stride)
        idt = O.batchnorm(sd, p + ".downsample.1", idt, training)
    else:
        idt = x
    return _q(F.relu(out + idt))            # the block output is stored in bf16, as the Bottleneck's is


def resnet_basic_features(sd, p, x, num_frames, depth, pooling_method="max", without_t_stride=False, training=False):
    """models/resnet.py:195-210 with block = BasicBlock (expansion 1)."""
    n, c_t, h, w = x.shape
    if c_t != 1:
        x = x.reshape(n * num_frames, c_t // num_frames, h, w)
    x = O.conv(x, sd[p + "conv1.weight"], stride=2, padding=3)
    x = F.relu(O.batchnorm(sd, p + "bn1", x, training))
    x = _q(F.max_pool2d(x, 3, 2, 1))
    frames = num_frames
    inplanes = 64
    for li, (planes, nblk) in enumerate(zip((64, 128, 256, 512), BASIC_BLOCKS[depth])):
        stride = 1 if li == 0 else 2
        for bi in range(nblk):
            s = stride if bi == 0 else 1
            has_down = bi == 0 and (s != 1 or inplanes != planes)       # models/resnet.py:163
            x = basic_block(sd, "%slayer%d.%d" % (p, li + 1, bi), x, s, has_down, training)
            inplanes = planes
        if li < 3 and not without_t_stride:
            x = _q(O.temporal_pool(x, frames, pooling_method.lower()))
            frames = max(1, frames // 2)
    return x


def resnet_basic_forward(sd, p, x, num_frames, depth, pooling_method="max", without_t_stride=False, dropout_p=0.5, training=False,
                         dropout_mask=None):
    """models/resnet.py:195-223: features -> GAP -> dropout -> FC (512 inputs) -> mean over the remaining frames."""
    n = x.shape[0]
    f = resnet_basic_features(sd, p, x, num_frames, depth, pooling_method, without_t_stride, training)
    f = f.mean(dim=(2, 3))
    f = O.dropout(f, dropout_p, training, dropout_mask)
    y = F.linear(f, sd[p + "fc.weight"], sd[p + "fc.bias"])
    return y.reshape(n, -1, y.shape[-1]).mean(dim=1)


def manifest_basic(key):
    """Names / shapes / dtypes of one architecture of tests/golden/state_manifest_basic.json.gz, as empty tensors."""
    with gzip.open(os.path.join(GOLDEN_DIR, "state_manifest_basic.json.gz"), "rt") as f:
        man = json.load(f)[key]
    return {k: torch.empty(shp, dtype=getattr(torch, dt.split(".")[1])) for k, (shp, dt) in man.items()}


def case_state(c):
    return case_state_dict(c, manifest_basic(arch_key(c)), seed=1234)


_CACHE = {}


def basic_case(c, emulate_bf16=False, modes=None, keep_grads=False):
    """One ResNet-18 / -34 case through the restatement on the CPU: the record tools/gen_golden.py stores for the real reference
    (logits, ce, gradient and statistic probes per mode), plus full gradients / final state with keep_grads.  Results are computed
    once per (case, arguments) and shared; callers leave them unchanged."""
    key = (id(c), emulate_bf16, tuple(modes or c["modes"]), keep_grads)
    if key in _CACHE:
        return _CACHE[key]
    sd0 = case_state(c)
    xs, target = case_inputs(c)
    old_q = O.QUANT
    O.QUANT = O.bf16_straight_through if emulate_bf16 else None
    out = {}
    try:
        for mode in (modes or c["modes"]):
            training = mode != "eval"
            sd = O.make_leaf_state(sd0, ("",) if training else ())
            with (torch.enable_grad() if training else torch.no_grad()):
                logits = resnet_basic_forward(sd, "", xs, c["groups"], c["depth"], c.get("pooling", "max"), False, 0.0, training)
                out[mode + ".logits"] = logits.detach().numpy()
                ce = F.cross_entropy(logits, target)
                out[mode + ".ce"] = ce.detach().numpy()
                if not training:
                    continue
                ce.backward()
            gp = {k: grad_probe(k, v.grad) for k, v in sd.items() if v.requires_grad and v.grad is not None}
            out[mode + ".grad_names"] = np.array(sorted(gp.keys()))
            out[mode + ".grad_probe"] = np.stack([gp[k] for k in sorted(gp.keys())])
            st = {k: stat_probe(v) for k, v in sd.items() if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
            out[mode + ".stat_names"] = np.array(sorted(st.keys()))
            out[mode + ".stat_probe"] = np.stack([st[k] for k in sorted(st.keys())])
            if keep_grads:
                out[mode + ".grads"] = {k: v.grad.detach() for k, v in sd.items() if v.requires_grad and v.grad is not None}
                out[mode + ".state"] = {k: v.detach() for k, v in sd.items()}
    finally:
        O.QUANT = old_q
    _CACHE[key] = out
    return out


def skipped_fraction(emu, ref, mode="train"):
    """Share of the gradient tensors that tests/test_models_gpu.check_against_emulation would skip (emulation decorrelated from
    fp32: relative L2 > 0.5, or fewer than 16 elements), among those it looks at (analytically-zero gradients excluded)."""
    g_emu, g_ref = emu[mode + ".grads"], ref[mode + ".grads"]
    gmax = max(g.norm().item() for g in g_ref.values())
    seen = skipped = 0
    for k, gr in g_ref.items():
        if gr.norm().item() < 1e-4 * gmax:
            continue
        seen += 1
        d_ef = ((g_emu[k].double() - gr.double()).norm() / (gr.double().norm() + 1e-30)).item()
        if d_ef > 0.5 or gr.numel() < 16:
            skipped += 1
    return skipped, seen
