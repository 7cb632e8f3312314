"""Golden-fixture case table of the BasicBlock main nets (ResNet-18 / -34), shared by tools/gen_golden.py --basic (reference side),
tests/basic_ref.py and the parity tests: sizes and flags of each case, in the scheme of tests/golden_cases.py, and the one rule by which
a case's synthetic weights differ from adamml_amd.synth's."""
import re

from adamml_amd import synth

CASES_BASIC = {
    # the reduced train step of resnet50_train and the 10-channel stem of resnet50_flow, on the two BasicBlock depths
    "resnet18_train": dict(kind="resnet", depth=18, modality=["rgb"], groups=8, B=2, size=96, modes=["eval", "train"]),
    # 16 BasicBlocks.  synth.synth_state_dict gives the LAST BatchNorm of a residual branch a small gain by name (bn3 of a Bottleneck: with
    # O(1) gains on every branch a random 16-block stack is chaotic); bn2 of a BasicBlock is not on that list, and with its O(1) gains the
    # bf16-storage emulation of this net sits > 0.5 relative L2 from fp32 in 95 of its 110 gradient tensors at every size tried (B 1-4,
    # 64-224 px): the whole-network parity rule would skip them all.  small_residual_gain puts bn2 into the regime bn3 is in; then
    # B 1 / 64 px skips 67 of 110, B 1 / 96 px 20 and B 2 / 96 px none (tests/test_resnet_basic_cpu.py asserts <= a quarter).
    "resnet34_flow": dict(kind="resnet", depth=34, modality=["flow"], groups=8, B=2, size=96, modes=["train"], small_residual_gain=True),
}

_BASIC_RESIDUAL_BN = re.compile(r"layer\d+\.\d+\.bn2\.weight$")


def case_state_dict(c, ref_sd, seed=1234):
    """synth.synth_state_dict of the case's manifest; small_residual_gain: bn2.weight of every BasicBlock drawn from synth's
    residual-BatchNorm range (0.1, 0.3) instead."""
    sd = synth.synth_state_dict(ref_sd, seed=seed)
    if c.get("small_residual_gain"):
        for k, v in sd.items():
            if _BASIC_RESIDUAL_BN.search(k):
                sd[k] = synth.det_uniform(k, tuple(v.shape), seed, 0.1, 0.3).to(v.dtype)
    return sd


# architectures whose state_dict names / shapes tests/golden/state_manifest_basic.json.gz records beside the cases' own
# (key -> case-like dict): the AdaMML RGB+Audio model on a ResNet-18 main net
MANIFEST_ONLY = {
    "adamml18:rgb+sound:lstm": dict(kind="adamml", depth=18, modality=["rgb", "sound"], groups=8, S=2),
}


def arch_key(c):
    if c["kind"] == "resnet":
        return "resnet%d:%s" % (c["depth"], "+".join(c["modality"]))
    return "adamml%d:%s:%s" % (c["depth"], "+".join(c["modality"]), c.get("causality", "lstm"))
