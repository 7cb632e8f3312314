"""fp32 GEMM of the policy head (adamml_gemm_f32) at the benchmark's shapes -- M = 72 videos x 5 segments = 360 rows; joint FC 2560 -> 2048,
LSTM input gates 2048 -> 2048, a classifier-sized product -- next to torch.addmm.  K-contiguous 16-byte-aligned operands as here run on the
matrix-core kernel; the 64 x 64 VALU tiles serve the rest.  GPU box only; nothing here is part of the product path.
--grad: the two gradient layouts of the same layers instead (dx = g W: b read down its columns; dW = g^T x: both operands), which run on
gemm_f32_tr_kernel; one JSON line per shape (--json FILE appends them), for an A/B of two builds of the library (ADAMML_HIP_LIB).
usage: python tools/bench_gemm.py [--grad [--json FILE]]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from adamml_amd.runtime import gemm_f32  # noqa: E402

dev = torch.device("cuda:0")


def timed(fn, reps=200):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


if "--grad" in sys.argv:
    from adamml_amd import hip
    rows = []
    # (rows S B, out features, in features): joint FC 2560 -> 2048 and 2048 -> 2048, LSTM gates 2048 -> 4 x 256, W_hh 256 -> 4 x 256
    for R, O, I in ((360, 2048, 2560), (360, 2048, 2048), (360, 1024, 2048), (360, 1024, 256)):
        g, x, w = torch.randn(R, O, device=dev), torch.randn(R, I, device=dev), torch.randn(O, I, device=dev)
        dx, dw = torch.empty(R, I, device=dev), torch.zeros(O, I, device=dev)
        for form, (M, N, K), fn, ref in (("dx", (R, I, O), lambda: gemm_f32(g, w, out=dx, trans_b=False), lambda: torch.mm(g, w, out=dx)),
                                        ("dW", (O, I, R), lambda: gemm_f32(g, x, out=dw, trans_a=True, trans_b=False, accumulate=True),
                                         lambda: dw.addmm_(g.t(), x))):
            us, us_ref = timed(fn), timed(ref)
            rows.append({"form": form, "M": M, "N": N, "K": K, "adamml_gemm_f32_us": round(us, 1), "tflops": round(2.0 * M * N * K / us * 1e-6, 1),
                         "torch_us": round(us_ref, 1), "lib": os.path.basename(os.path.dirname(hip.LIB_PATH)) + "/" + os.path.basename(hip.LIB_PATH)})
            print(json.dumps(rows[-1]))
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "a") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)
    sys.exit(0)

for M, N, K in ((360, 2048, 2560), (360, 2048, 2048), (360, 1024, 2048), (2880, 31, 2048), (72, 2048, 512)):
    a, b, bias = torch.randn(M, K, device=dev), torch.randn(N, K, device=dev), torch.randn(N, device=dev)
    out = torch.empty(M, N, device=dev)
    res = []
    for fn in (lambda: gemm_f32(a, b, out=out, bias=bias, act=1), lambda: torch.addmm(bias, a, b.t())):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) / 50 * 1e3)
    print("  M %5d N %5d K %5d: adamml_gemm_f32 %7.1f us (%5.1f TFLOP/s)   torch.addmm %7.1f us" % (M, N, K, res[0], 2.0 * M * N * K / res[0] * 1e-6, res[1]))
