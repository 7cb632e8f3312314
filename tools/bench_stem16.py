"""The 16-channel 7x7 stem (csrc/conv_stem16.hip) next to the tile kernels it replaces, on the same tensors: adamml_conv_fwd and
adamml_conv_bwd_weight of this build against those of a build without the kernel (tools/build_prev_lib.sh -> libadamml_hip_prev.so),
both loaded into one process and timed alternately.  Shapes: the flow (10) and RGB-diff (15 channel) stems at 224 x 224, N = 360 images
(B = 72 x 5 segments) and the B = 9 share, N = 45.  Event-timed, warmed; per side the median and the spread of REPEATS blocks of REPS
launches.  GPU box only; nothing here is part of the product path.
usage: python tools/bench_stem16.py [--prev LIB] [--json FILE]"""
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from adamml_amd import hip  # noqa: E402
from adamml_amd.hip import ConvDesc, SIGNATURES, _DESC  # noqa: E402

REPS, REPEATS = 20, 7
dev = torch.device("cuda:0")


def arg(flag, default):
    return sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default


def bind(lib):
    for n in ("adamml_conv_fwd", "adamml_conv_bwd_weight", "adamml_pack_conv_weight"):
        getattr(lib, n).argtypes, getattr(lib, n).restype = SIGNATURES[n], ctypes.c_int
    lib.adamml_conv_bwd_weight_workspace.argtypes, lib.adamml_conv_bwd_weight_workspace.restype = [_DESC, ctypes.c_int], ctypes.c_size_t
    return lib


def block(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
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
    return [(round(statistics.median(t), 1), round((max(t) - min(t)) / statistics.median(t), 3)) for t in (ta, tb)]


new, prev = bind(hip.load()), bind(ctypes.CDLL(arg("--prev", os.path.join(ROOT, "adamml_amd", "libadamml_hip_prev.so"))))
assert new.adamml_conv_stem16_supported(ctypes.byref(ConvDesc(45, 224, 224, 16, 112, 112, 64, 7, 7, 2, 3, 1, 0, 0, 1, 0))) == 1
assert not hasattr(prev, "adamml_conv_stem16_supported"), "--prev must be a build without the stem16 kernels"
st = torch.cuda.current_stream().cuda_stream
rows = []
for N in (360, 45):
    for cin in (10, 15):
        d = ConvDesc(N, 224, 224, 16, 112, 112, 64, 7, 7, 2, 3, 1, 0, 0, 1, 0)
        x = torch.randn(N, 224, 224, 16, device=dev).to(torch.bfloat16)
        x[..., cin:] = 0
        w = torch.randn(64, cin, 7, 7, device=dev) * (2.0 / (cin * 49)) ** 0.5
        wp = torch.empty(64, 49 * 16, dtype=torch.bfloat16, device=dev)
        assert new.adamml_pack_conv_weight(w.data_ptr(), wp.data_ptr(), 64, cin, 16, 7, 7, 0, st) == 0
        y = torch.empty(N, 112, 112, 64, dtype=torch.bfloat16, device=dev)
        stats = torch.zeros(1, hip.STAT_SLOTS, 128, dtype=torch.float64, device=dev)
        dz = (torch.randn(N, 112, 112, 64, device=dev) * 0.25).to(torch.bfloat16)
        dw = torch.zeros(64, cin, 7, 7, device=dev)
        q = [lib.adamml_conv_bwd_weight_workspace(ctypes.byref(d), cin) for lib in (new, prev)]
        ws = torch.empty(max(q) // 4 + 1, dtype=torch.float32, device=dev)

        def fwd(lib):
            assert lib.adamml_conv_fwd(ctypes.byref(d), x.data_ptr(), wp.data_ptr(), None, None, y.data_ptr(), stats.data_ptr(), st) == 0

        def wgrad(lib, nbytes):
            assert lib.adamml_conv_bwd_weight(ctypes.byref(d), dz.data_ptr(), x.data_ptr(), None, None, dw.data_ptr(), cin, ws.data_ptr(), nbytes, st) == 0

        flop = 2.0 * N * 112 * 112 * 64 * 49 * cin
        for what, (a, b) in (("fwd", ab(lambda: fwd(new), lambda: fwd(prev))),
                             ("wgrad", ab(lambda: wgrad(new, q[0]), lambda: wgrad(prev, q[1])))):
            rows.append({"what": what, "N": N, "cin": cin, "stem16_us": a[0], "stem16_spread": a[1], "tile_us": b[0], "tile_spread": b[1],
                         "speedup": round(b[0] / a[0], 2), "stem16_tflops": round(flop / a[0] * 1e-6, 1), "reps": REPS, "repeats": REPEATS})
            print(json.dumps(rows[-1]), flush=True)
if "--json" in sys.argv:
    with open(arg("--json", None), "w") as f:
        f.writelines(json.dumps(r) + "\n" for r in rows)
