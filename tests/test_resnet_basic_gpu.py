"""BasicBlock main nets (ResNet-18 / -34) on the MI355X: whole-network parity under the rules of tests/test_models_gpu.py (imported: same
functions, same constants), which data-gradient entry points a train step calls, the fused 3x3 residual data gradient against the
unfused fallback, AdaMML on a ResNet-18 main net, and launch-plan replay of the ResNet-18 step.

The fp32 reference and the bf16-storage emulation come from tests/basic_ref.py (CPU, computed once per case and shared)."""
import collections

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from adamml_amd import synth  # noqa: E402
from tests.basic_ref import basic_case, case_state, manifest_basic, resnet_basic_forward  # noqa: E402
from tests.golden_cases import CH  # noqa: E402
from tests.golden_cases_basic import CASES_BASIC, MANIFEST_ONLY, arch_key  # noqa: E402
from tests.oracle_harness import case_inputs, load_golden  # noqa: E402
from tests.test_models_gpu import check_against_emulation, check_against_golden, calibrated_state, check_eval  # noqa: E402

DEV = "cuda"


def build(c):
    from adamml_amd.resnet import resnet
    model = resnet(depth=c["depth"], num_classes=31, without_t_stride=False, groups=c["groups"], dropout=0.0,
                   pooling_method=c.get("pooling", "max"), input_channels=CH[c["modality"][0]], imagenet_pretrained=False)
    sd = case_state(c)
    assert list(model.state_dict().keys()) == list(sd.keys())
    model.load_state_dict(sd)
    return model.to(DEV), sd


def train_step(model, c):
    x_cpu, target = case_inputs(c)
    model.train()
    model.zero_grad()
    y = model(x_cpu.to(DEV))
    F.cross_entropy(y, target.to(DEV)).backward()
    torch.cuda.synchronize()
    return y.detach().cpu().numpy()


def references(c):
    emu = basic_case(c, emulate_bf16=True, modes=["train"], keep_grads=True)
    ref = basic_case(c, emulate_bf16=False, modes=["train"], keep_grads=True)
    return emu, ref


def count_calls(monkeypatch):
    """-> Counter of the entry points the executor calls from here on (adamml_amd.runtime.call, as tests/test_executor_gpu.py logs them)"""
    from adamml_amd import runtime
    counts = collections.Counter()
    real = runtime.call

    def logged(name, *a):
        counts[name] += 1
        return real(name, *a)
    monkeypatch.setattr(runtime, "call", logged)
    return counts


def refuse_3x3(monkeypatch):
    """adamml_amd.runtime._residual_fusable answers as it did while adamml_conv_bwd_data_res_supported was 0 for 3x3 convs"""
    from adamml_amd import runtime
    real = runtime._residual_fusable
    monkeypatch.setattr(runtime, "_residual_fusable", lambda x, d: d.KH == 1 and real(x, d))


def fusable_blocks(model):
    """blocks without a downsample branch whose input is the previous block's residual add (not the stem's max-pool, not a temporal pool)"""
    return sum(1 for layer in (model.layer1, model.layer2, model.layer3, model.layer4) for bi, b in enumerate(layer)
               if b.downsample is None and bi > 0)


@pytest.mark.parametrize("name", list(CASES_BASIC))
def test_resnet_basic_parity(name):
    c = CASES_BASIC[name]
    gold = load_golden(name)
    emu, ref = references(c)
    model, sd = build(c)
    y = train_step(model, c)
    print(name)
    check_against_emulation(model, emu, ref, "train", y)
    check_against_golden(model, gold, emu, "train", y, name=name)
    if "eval" not in c["modes"]:
        return
    # eval mode with calibrated running statistics: BatchNorm is a fixed affine map -> plain bf16 tolerance vs fp32
    x_cpu, _ = case_inputs(c)
    pool = c.get("pooling", "max")
    cal = calibrated_state(sd, lambda s: resnet_basic_forward(s, "", x_cpu, c["groups"], c["depth"], pool, False, 0.0, True))
    model.load_state_dict(cal)
    model.eval()
    with torch.no_grad():
        y = model(x_cpu.to(DEV))
    check_eval(y, cal, lambda s: resnet_basic_forward(s, "", x_cpu, c["groups"], c["depth"], pool, False, 0.0, False))


@pytest.mark.parametrize("name,blocks", [("resnet18_train", 4), ("resnet34_flow", 12)])
def test_residual_data_gradient_runs_once_per_fusable_block(name, blocks, monkeypatch):
    """conv1 of a block without a downsample branch is the last consumer of the previous block's add output: its data gradient is
    adamml_conv_bwd_data_res, and that add launches no adamml_residual_bwd.  ResNet-18: layer1.1, layer2.1, layer3.1, layer4.1;
    ResNet-34: 13 blocks have no downsample branch, layer1.0 among them, whose input is the stem's max-pool output: 12."""
    c = CASES_BASIC[name]
    model, _ = build(c)
    assert fusable_blocks(model) == blocks
    n_blocks = sum(len(l) for l in (model.layer1, model.layer2, model.layer3, model.layer4))
    counts = count_calls(monkeypatch)
    train_step(model, c)
    print("  %s:" % name, {k: v for k, v in sorted(counts.items()) if "bwd_data" in k or "residual" in k})
    assert counts["adamml_conv_bwd_data_res"] == blocks
    assert counts["adamml_conv_bwd_data_res_prod"] == 0
    # every add's backward is finished exactly once: by the next conv1's data gradient, by the temporal pool behind a stage, or by itself
    assert counts["adamml_conv_bwd_data_res"] + counts["adamml_temporal_pool_bwd_res"] + counts["adamml_residual_bwd"] == n_blocks


def test_resnet50_launches_are_unchanged(monkeypatch):
    """No 3x3 conv of a Bottleneck net is the last consumer of an add output: with the probe's 3x3 answer patched back to 0 a ResNet-50
    train step calls every entry point exactly as often."""
    from tests.golden_cases import CASES
    from adamml_amd.resnet import resnet
    from tests.oracle_harness import manifest
    c = CASES["resnet50_flow"]
    runs = []
    for patched in (False, True):
        with monkeypatch.context() as mp:
            if patched:
                refuse_3x3(mp)
            model = resnet(depth=50, num_classes=31, without_t_stride=False, groups=c["groups"], dropout=0.0, pooling_method="max",
                           input_channels=10, imagenet_pretrained=False)
            model.load_state_dict(synth.synth_state_dict(manifest(c), seed=1234))
            model.to(DEV)
            counts = count_calls(mp)
            train_step(model, c)
            runs.append(dict(counts))
    assert runs[0] == runs[1]
    assert runs[0]["adamml_conv_bwd_data_res"] + runs[0].get("adamml_conv_bwd_data_res_prod", 0) > 0


def test_fused_3x3_residual_data_gradient_against_the_fallback(monkeypatch):
    """The same ResNet-18 step with the 3x3 residual data gradient (fused) and with adamml_conv_bwd_data(accumulate) +
    adamml_residual_bwd (fallback, runtime._residual_fusable refusing 3x3): both pass the parity rules, and the fused run's gradients pass
    the gradient rule of check_against_emulation with the fallback run in the place of the fp32 reference."""
    name = "resnet18_train"
    c = CASES_BASIC[name]
    gold = load_golden(name)
    emu, ref = references(c)
    out = {}
    for which in ("fused", "fallback"):
        with monkeypatch.context() as mp:
            if which == "fallback":
                refuse_3x3(mp)
            model, _ = build(c)
            counts = count_calls(mp)
            y = train_step(model, c)
        assert counts["adamml_conv_bwd_data_res"] == (4 if which == "fused" else 0)
        print(name, which)
        check_against_emulation(model, emu, ref, "train", y)
        check_against_golden(model, gold, emu, "train", y, name=name)
        out[which] = (model, y)
    fb, y_fb = out["fallback"]
    grads = {k: p.grad.detach().cpu() for k, p in fb.named_parameters()}
    assert all(torch.isfinite(g).all() for g in grads.values())
    assert all(torch.isfinite(p.grad).all() for p in out["fused"][0].parameters())
    as_ref = {"train.logits": y_fb, "train.grads": {k: grads[k] for k in ref["train.grads"]},
              "train.state": {k: v.detach().cpu() for k, v in fb.state_dict().items()}}
    print(name, "fused vs fallback")
    check_against_emulation(out["fused"][0], emu, as_ref, "train", out["fused"][1])


def build_adamml18(dropout=0.0):
    from adamml_amd import adamml
    c = MANIFEST_ONLY["adamml18:rgb+sound:lstm"]
    model = adamml(groups=c["groups"], modality=c["modality"], input_channels=[3, 1], num_segments=c["S"], rng_policy=False,
                   rng_threshold=0.5, causality_modeling="lstm", num_classes=31, depth=18, without_t_stride=False, dropout=dropout,
                   pooling_method="max", fusion_point="logits", unimodality_pretrained=[], learnable_lf_weights=True)
    return model, c


def test_adamml_on_a_resnet18_main_net():
    """rgb + sound, B 2, 2 segments of 8 frames, 96 px: one main-net step and one policy step leave a finite gradient in every trainable
    parameter; the state_dict is the reference's for this configuration."""
    model, c = build_adamml18()
    man = manifest_basic(arch_key(c))
    sd = model.state_dict()
    assert list(sd.keys()) == list(man.keys())
    assert all(tuple(sd[k].shape) == tuple(man[k].shape) for k in sd)
    model.load_state_dict(synth.synth_state_dict(man, seed=1234))
    model.to(DEV)
    B, S = 2, c["S"]
    xs = [t.to(DEV) for t in synth.synth_inputs(c["modality"], B, S, c["groups"], 96, 96, seed=42)]
    target = synth.synth_labels(B, 31, seed=42).to(DEV)
    expo = synth.synth_gumbel_exponential(S, 2, B, seed=11).to(DEV)
    for stage in ("main", "policy"):
        model.unfreeze_policy_net()
        model.unfreeze_main_net()
        (model.freeze_policy_net if stage == "main" else model.freeze_main_net)()
        model.train()
        model.zero_grad()
        logits, sel = model(xs, gumbel_exponential=expo)
        loss = F.cross_entropy(logits, target)
        if stage == "policy":
            loss = loss + (sel.mean(dim=1) ** 2).mean()
        loss.backward()
        torch.cuda.synchronize()
        assert torch.isfinite(logits).all()
        trainable = [(k, p) for k, p in model.named_parameters() if p.requires_grad]
        assert trainable
        bad = [k for k, p in trainable if p.grad is None or not torch.isfinite(p.grad).all()]
        assert not bad, "%s stage: no finite gradient in %s" % (stage, bad[:6])
        print("  adamml depth 18, %s stage: %d trainable tensors, all gradients finite" % (stage, len(trainable)))


def test_adamml18_eval_skipping_equals_masking():
    """as tests/test_models_gpu.py test_eval_skipping_equals_masking, on the ResNet-18 main net"""
    torch.manual_seed(0)
    model, c = build_adamml18(dropout=0.5)
    model.to(DEV).eval()
    S, B = c["S"], 4
    xs = [t.to(DEV) for t in synth.synth_inputs(["rgb", "sound"], B, S, 8, 64, seed=5)]
    expo = synth.synth_gumbel_exponential(S, 2, B, seed=11).to(DEV)
    with torch.no_grad():
        model.skip_unselected = False
        ref, dec_ref = model(xs, gumbel_exponential=expo)
        model.skip_unselected = True
        got, dec = model(xs, gumbel_exponential=expo)
    assert torch.equal(dec, dec_ref)
    st = model.last_skip_stats
    assert st["clips"] == S * B and st["executed_per_modality"] == [int(dec[:, :, m].sum().item()) for m in range(2)]
    assert torch.allclose(got, ref, rtol=1e-5, atol=1e-5), (got - ref).abs().max().item()


def test_resnet18_launch_plan_replay_equals_eager_steps():
    """The ResNet-18 train step recorded once and replayed from C (calls 1-2 eager warm-up, call 3 recorded, calls 4-5 replayed) computes
    bit for bit what the eager steps compute: logits, every gradient, every BatchNorm buffer after every step."""
    from adamml_amd import plan
    c = CASES_BASIC["resnet18_train"]
    x_cpu, target = case_inputs(c)
    target = target.to(DEV)

    def steps(planned):
        plan.ENABLED = planned
        try:
            model, _ = build(c)
            model.train()
            trace = []
            for it in range(5):
                model.zero_grad(set_to_none=False)
                y = model(x_cpu.to(DEV))
                F.cross_entropy(y, target).backward()
                torch.cuda.synchronize()
                trace.append((y.detach().cpu().clone(), {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()},
                              {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}))
            return trace
        finally:
            plan.ENABLED = False
    eager = steps(False)
    before = dict(plan.stats)
    planned = steps(True)
    assert plan.stats["recorded"] - before["recorded"] >= 1, "the ResNet-18 step was not recorded"
    assert plan.stats.get("failed_recordings", 0) == before.get("failed_recordings", 0)
    assert plan.stats["replayed_ops"] - before["replayed_ops"] > 100
    for it, ((y0, g0, s0), (y1, g1, s1)) in enumerate(zip(eager, planned)):
        assert torch.equal(y0, y1), "logits differ at step %d" % it
        diff = [k for k in g0 if not torch.equal(g0[k], g1[k])]
        assert not diff, "step %d: %d gradients differ, e.g. %s" % (it, len(diff), diff[:4])
        diff = [k for k in s0 if not torch.equal(s0[k], s1[k])]
        assert not diff, "step %d: %d state tensors differ, e.g. %s" % (it, len(diff), diff[:4])
