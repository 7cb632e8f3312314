"""The weight-streaming 1x1 kernel (csrc/conv1x1_skinny.hip) next to the tile kernel it replaces, on the same tensors: adamml_conv_fwd
without statistics of this build against that of a build without the kernel (tools/build_prev_lib.sh -> libadamml_hip_prev.so), both
loaded into one process and timed alternately.  Shapes: the 1x1 convs of ResNet-50 layers 3-4 and the tail of the sound MobileNetV2 at
the pixel counts of 1, 2, 4, 8 (and 16, 32) videos per step, plain and lazily normalised input; rows the probe refuses are skipped.
Every launch of a block reads another of COPIES weight packs (32 MB and more in rotation: no launch finds its weights in L2).
Event-timed, warmed; per side the median and the spread of REPEATS blocks of REPS launches, and the outputs of the two sides compared
bit for bit.  GPU box only; nothing here is part of the product path.
usage: python tools/bench_conv1x1_skinny.py [--prev LIB] [--json FILE]"""
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from adamml_amd import hip  # noqa: E402
from adamml_amd.hip import ConvDesc, SIGNATURES  # noqa: E402

REPS, REPEATS, COPIES = 64, 7, 16
dev = torch.device("cuda:0")
# (name, Cin, Cout, pixels per video)
SHAPES = [("layer3.conv1", 1024, 256, 392), ("layer3.conv3", 256, 1024, 392), ("layer4.0.conv1", 1024, 512, 196),
          ("layer4.conv1", 2048, 512, 49), ("layer4.conv3", 512, 2048, 49), ("sound.tail", 320, 1280, 64)]


def arg(flag, default):
    return sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default


def bind(lib):
    for n in ("adamml_conv_fwd", "adamml_pack_conv_weight"):
        getattr(lib, n).argtypes, getattr(lib, n).restype = SIGNATURES[n], ctypes.c_int
    return lib


def block(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(REPS):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


def ab(fa, fb):
    """-> ((median us, spread), (median us, spread)) of the two sides, blocks alternating"""
    for f in (fa, fb, fa, fb):
        block(f)
    ta, tb = [], []
    for _ in range(REPEATS):
        ta.append(block(fa))
        tb.append(block(fb))
    return [(round(statistics.median(t), 2), round((max(t) - min(t)) / statistics.median(t), 3)) for t in (ta, tb)]


new, prev = bind(hip.load()), bind(ctypes.CDLL(arg("--prev", os.path.join(ROOT, "adamml_amd", "libadamml_hip_prev.so"))))
assert not hasattr(prev, "adamml_conv1x1_skinny_supported"), "--prev must be a build without the skinny kernel"
st = torch.cuda.current_stream().cuda_stream
rows = []
for name, cin, cout, ppv in SHAPES:
    w = torch.randn(COPIES, cout, cin, 1, 1, device=dev) * (2.0 / cin) ** 0.5
    wp = torch.empty(COPIES, cout, cin, dtype=torch.bfloat16, device=dev)
    for c in range(COPIES):
        assert new.adamml_pack_conv_weight(w[c].data_ptr(), wp[c].data_ptr(), cout, cin, cin, 1, 1, 0, st) == 0
    vec = torch.cat([torch.rand(cin, device=dev) + 0.5, torch.randn(cin, device=dev) * 0.5]).contiguous()
    for videos in (1, 2, 4, 8, 16, 32):
        P = ppv * videos
        d = ConvDesc(1, 1, P, cin, 1, P, cout, 1, 1, 1, 0, 1, 1, 0, 1, 0)
        if not new.adamml_conv1x1_skinny_supported(ctypes.byref(d), 0):
            continue
        x = torch.randn(P, cin, device=dev).to(torch.bfloat16)
        ya, yb = (torch.empty(P, cout, dtype=torch.bfloat16, device=dev) for _ in range(2))
        for lazy in (False, True):
            sc, sh = (vec.data_ptr(), vec.data_ptr() + 4 * cin) if lazy else (None, None)

            def fwd(lib, y, i):
                assert lib.adamml_conv_fwd(ctypes.byref(d), x.data_ptr(), wp[i % COPIES].data_ptr(), sc, sh, y.data_ptr(), None, st) == 0

            a, b = ab(lambda i: fwd(new, ya, i), lambda i: fwd(prev, yb, i))
            same = bool(torch.equal(ya, yb))
            wbytes = 2.0 * cin * cout
            rows.append({"shape": name, "cin": cin, "cout": cout, "videos": videos, "P": P, "lazy": lazy, "skinny_us": a[0], "skinny_spread": a[1],
                         "tile_us": b[0], "tile_spread": b[1], "speedup": round(b[0] / a[0], 2), "bit_identical": same,
                         "weight_GBps": round(wbytes / a[0] * 1e-3, 1), "reps": REPS, "repeats": REPEATS})
            print(json.dumps(rows[-1]), flush=True)
if "--json" in sys.argv:
    with open(arg("--json", None), "w") as f:
        f.writelines(json.dumps(r) + "\n" for r in rows)
