#!/usr/bin/env python3
"""Generate tests/golden/flops_cases.json from the REAL reference (IBM/AdaMML, a checkout at $ADAMML_REF) on the CPU.

Only this script imports the reference, and nothing of its text is copied: the fixture holds the ARGUMENTS this script chose (major
modalities, selection ratios, number of segments) and the number the reference's own `utils.utils.flops_computation` RETURNS for them
-- 2, 3 and 4 modalities, 1 / 5 / 10 segments, ratios including 0 and 1.  tests/test_metrics_cpu.py checks
adamml_amd.metrics.flops_computation against every case.

mAP has no golden: the reference's `actnet_acc` needs torchnet, which is not installed, so it cannot be run.  adamml_amd.metrics'
average precision is pinned instead by independent references inside tests/test_metrics_cpu.py (a brute-force float64 rank count, a
float32 restatement of torchnet's APMeter, and sklearn where it imports).

Usage:  ADAMML_REF=/path/to/AdaMML python tools/gen_golden_metrics.py
"""
import json
import os
import sys
import types

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("ADAMML_REF")
if not REF or not os.path.isfile(os.path.join(REF, "utils", "utils.py")):
    raise SystemExit("set ADAMML_REF to a checkout of the reference (IBM/AdaMML)")
sys.path.insert(0, REF)

# shim: torchvision is absent but utils/utils.py imports it (as in tools/gen_golden.py)
tv, tvt = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
tvt.Compose = lambda ts: None
tvt.CenterCrop = tvt.Resize = lambda *a, **k: None
tv.transforms = tvt
sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt})

from utils.utils import AverageMeter, flops_computation  # noqa: E402  (the reference package)

# (modalities, {modality: selection ratio}, segments).  The launcher never passes rgbdiff beside flow (train_adamml.py:169-172); the
# four-modality cases pin what the function does with it all the same: every entry other than rgb / sound is charged the flow cost
CASES = [
    (["rgb", "sound"], {"rgb": 0.25, "sound": 0.75}, 5),
    (["rgb", "sound"], {"rgb": 0.0, "sound": 0.0}, 1),
    (["rgb", "sound"], {"rgb": 1.0, "sound": 1.0}, 10),
    (["rgb", "sound"], {"rgb": 0.3125, "sound": 0.0}, 10),
    (["rgb", "flow"], {"rgb": 1.0, "flow": 0.0}, 5),
    (["flow", "sound"], {"flow": 0.4375, "sound": 1.0}, 1),
    (["rgb", "flow", "sound"], {"rgb": 0.5, "sound": 1.0, "flow": 0.125}, 10),
    (["rgb", "flow", "sound"], {"rgb": 0.0, "sound": 0.0, "flow": 0.0}, 5),
    (["rgb", "flow", "sound"], {"rgb": 1.0, "sound": 1.0, "flow": 1.0}, 1),
    (["rgb", "flow", "sound"], {"rgb": 0.1, "sound": 0.9, "flow": 0.37}, 5),
    (["rgb", "flow", "rgbdiff", "sound"], {"rgb": 0.6, "flow": 0.2, "rgbdiff": 0.8, "sound": 0.55}, 10),
    (["rgb", "flow", "rgbdiff", "sound"], {"rgb": 1.0, "flow": 0.0, "rgbdiff": 1.0, "sound": 0.0}, 1),
    (["rgb", "flow", "rgbdiff", "sound"], {"rgb": 0.0, "flow": 1.0, "rgbdiff": 0.0, "sound": 1.0}, 5),
]


def meter(value):
    m = AverageMeter()
    m.update(value)
    return m


def main():
    cases = []
    for modality, ratios, segments in CASES:
        gflops = flops_computation(modality, {k: meter(v) for k, v in ratios.items()}, segments)
        cases.append({"modality": modality, "ratios": ratios, "num_segments": segments, "gflops": float(gflops)})
    path = os.path.join(ROOT, "tests", "golden", "flops_cases.json")
    with open(path, "w") as f:
        json.dump({"cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", len(cases), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
