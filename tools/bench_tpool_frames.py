"""Stage boundaries of a ResNet-50 on 16-frame clips (`--groups 16`): the fused launches against the unfused launches they replace, and one
training step.  GPU box only.  Prints one JSON line per figure (median and min..max of `--rounds` rounds of `--iters` launches).

  python tools/bench_tpool_frames.py                    boundary launches, fused and unfused, at the two shapes below
  python tools/bench_tpool_frames.py --unfused-only     only the launches every tree serves at T = 16 (to compare two checkouts)
  python tools/bench_tpool_frames.py --step --batch 36  one training step (forward + backward) of ResNet-50, 16 frames of 224 x 224

Shapes: the end of stage 1 of a 16-frame net (36 clips x 16 frames of 56 x 56, 64 -> 256 channels: the frame count of one benchmark segment
call, 576) and the end of stage 2 of a 32-frame net (18 clips x 16 frames of 28 x 28, 128 -> 512)."""
import argparse
import json
import os
import statistics
import sys
from ctypes import byref

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from adamml_amd import hip  # noqa: E402
from adamml_amd.hip import call, ptr, STAT_SLOTS  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--unfused-only", action="store_true")
ap.add_argument("--step", action="store_true")
ap.add_argument("--batch", type=int, default=36)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=10)
args = ap.parse_args()
dev = torch.device("cuda:0")


def timed(label, fn, **extra):
    ms = []
    for _ in range(args.rounds + 1):                       # (round 0 warms up)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / args.iters)
    ms = ms[1:]
    print(json.dumps(dict(what=label, median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), **extra)), flush=True)


def boundary(clips, T, H, Cin, Cout):
    G, N, To, HW = 1, clips * T, T // 2, H * H
    bf = torch.bfloat16
    x = (torch.randn(N, H, H, Cin, device=dev) * 1.5).to(bf)
    xvec = torch.rand(G, 4, Cin, device=dev) + 0.5
    w3 = (torch.randn(Cout, Cin, device=dev) * 0.1).to(bf)
    vec = torch.rand(G, 4, Cout, device=dev) + 0.5
    idn = torch.randn(N, H, H, Cout, device=dev).to(bf)
    full, mask = torch.empty(N, H, H, Cout, dtype=bf, device=dev), torch.empty(N, H, H, Cout // 8, dtype=torch.uint8, device=dev)
    pooled, code = torch.empty(N // 2, H, H, Cout, dtype=bf, device=dev), torch.empty(N // 2, H, H, Cout // 8, dtype=torch.int16, device=dev)
    gy, gx, g2 = torch.randn(N // 2, H, H, Cout, device=dev).to(bf), torch.empty_like(full), torch.empty_like(full)
    sums = torch.zeros(G, STAT_SLOTS, 2 * Cout, dtype=torch.float64, device=dev)
    d = hip.ConvDesc(N, H, H, Cin, H, H, Cout, 1, 1, 1, 0, 1, 1, 0, G, 4 * Cin)
    head = (byref(d), ptr(x), ptr(w3), ptr(xvec[0, 0]), ptr(xvec[0, 1]), ptr(vec), ptr(idn), None, None, 0, 1)
    tag = dict(shape="%d clips x %d frames x %dx%d, %d -> %d" % (clips, T, H, H, Cin, Cout))

    def unfused_fwd():
        call("adamml_conv_fwd_bn_add", *head, ptr(full), ptr(mask))
        call("adamml_temporal_pool_fwd", ptr(full), None, None, 0, 0, ptr(pooled), clips, T, HW * Cout, Cout, 0, G)

    def unfused_bwd():
        call("adamml_temporal_pool_bwd", ptr(gy), ptr(full), None, None, 0, 0, ptr(gx), clips, T, HW * Cout, Cout, 0, G)
        call("adamml_residual_bwd", ptr(gx), ptr(full), 1, ptr(g2), None, ptr(vec), ptr(sums), None, None, None, N * HW, Cout, G)

    timed("forward unfused: conv_fwd_bn_add + temporal_pool_fwd", unfused_fwd, **tag)
    timed("backward unfused: temporal_pool_bwd + residual_bwd", unfused_bwd, **tag)
    if args.unfused_only:
        return
    kern = ("tile", "conv1x1_fadd_tpool_kernel", "conv1x1_fadd_tpool_stream_kernel")[hip.load().adamml_conv_fwd_bn_add_tpool_streams(byref(d), T)]
    timed("forward fused: conv_fwd_bn_add_tpool", lambda: call("adamml_conv_fwd_bn_add_tpool", *head, T, ptr(pooled), ptr(code)), kernel=kern, **tag)
    timed("backward fused (block output stored): temporal_pool_bwd_res",
          lambda: call("adamml_temporal_pool_bwd_res", ptr(gy), ptr(full), 1, ptr(g2), None, ptr(vec), ptr(sums), clips, T, HW, Cout, G), **tag)
    timed("backward fused (codes): temporal_pool_bwd_code", lambda: call("adamml_temporal_pool_bwd_code", ptr(gy), ptr(code), ptr(g2), ptr(sums), clips, T, HW, Cout, G), **tag)
    if hip.load().adamml_temporal_pool_bwd_code_prod_supported(T, Cout, Cin):
        prod = torch.empty(G, Cout, Cin, device=dev)
        ws = hip.scratch(hip.load().adamml_temporal_pool_bwd_code_prod_workspace(clips, T, HW, Cout, Cin, G), dev)
        timed("backward fused (codes) + product g2^T a: temporal_pool_bwd_code_prod",
              lambda: call("adamml_temporal_pool_bwd_code_prod", ptr(gy), ptr(code), ptr(g2), ptr(sums), ptr(x), ptr(xvec[0, 0]), ptr(xvec[0, 1]), 4 * Cin, 1,
                           ptr(prod), ptr(ws), ws.numel() * ws.element_size(), clips, T, HW, Cout, Cin, G), **tag)


def step():
    import torch.nn.functional as F
    from adamml_amd.resnet import resnet
    torch.manual_seed(0)
    model = resnet(depth=50, num_classes=31, without_t_stride=False, groups=16, dropout=0.0, pooling_method="max", input_channels=3,
                   imagenet_pretrained=False).to(dev).train()
    x = torch.randn(args.batch, 16 * 3, 224, 224, device=dev)
    target = torch.randint(0, 31, (args.batch,), device=dev)

    def fn():
        model.zero_grad(set_to_none=False)
        F.cross_entropy(model(x), target).backward()

    fn()
    timed("ResNet-50 training step, 16 frames of 224 x 224", fn, batch=args.batch, peak_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))


if args.step:
    step()
else:
    boundary(36, 16, 56, 64, 256)
    boundary(18, 16, 28, 128, 512)
