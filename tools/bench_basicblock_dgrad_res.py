"""The 3x3 residual data gradient of the BasicBlock nets against the pair of launches it replaces, and one ResNet-18 / -34 / -50 training step.

Per shape at ResNet-34's training geometry (one segment call of 72 videos x 8 frames: 576 frames of 56 x 56 x 64, 288 of 28 x 28 x 128, 144 of
14 x 14 x 256, 72 of 7 x 7 x 512), device-event time of
  (a) adamml_conv_bwd_data(accumulate) + adamml_residual_bwd   -- what the executor launches when adamml_conv_bwd_data_res_supported says 0
  (b) adamml_conv_bwd_data_res(accumulate, 1-bit mask, z_a)    -- the fused launch
alternating in one process, REPEATS samples each (a sample = INNER back-to-back launches between two events, a window of about 5 ms, each
launch on the next of several buffer sets that together exceed the last-level cache), with min / median / 90th percentile per launch.  keep = median(b) < median(a) - max(spread(a), spread(b)), spread = p90 - min:
the rule by which a shape keeps the fused arm (profiles/basicblock_dgrad_res.json).
Where adamml_conv_bwd_data_res_streams answers 2 (64 channels: the resident-weight kernel of csrc/conv3x3_c64.hip serves (b)) a third arm
  (c) the same launch with a second BatchNorm operand (z_b)    -- which the tile kernel of csrc/conv_gemm.hip serves
alternates with the two: the tile kernel with one more operand stream than (b), the nearest thing to it that the entry point reaches.  The
64-channel kernel keeps the shape only if it also beats (c) by the same rule.
After the timing each shape runs the pair and the fused launch once more from the same identity-path gradient and records how far their
outputs and sums are apart ("check": the launches timed here are the ones compared, at the timed size).

--steps: also one training step (forward + backward, batch 72 x 8 frames of 224 x 224) of resnet(18 / 34) with the fused arm and with
runtime._residual_fusable refusing 3x3 convs, alternating, and of resnet(50).

    python tools/bench_basicblock_dgrad_res.py [--steps] [--out FILE.json]"""
import json
import statistics
import sys

import torch
from ctypes import byref

sys.path.insert(0, ".")
from adamml_amd import hip, runtime  # noqa: E402
from adamml_amd.hip import call, ptr, STAT_SLOTS, ConvDesc  # noqa: E402

DEV = "cuda"
REPEATS = 40
# (name, frames, H = W, channels, launches per sample: a window of about 5 ms -- a window of one launch measures the event pair as much as the kernel)
SHAPES = [("64@56^2", 576, 56, 64, 12), ("128@28^2", 288, 28, 128, 40), ("256@14^2", 144, 14, 256, 64), ("512@7^2", 72, 7, 512, 80)]
CACHE_BYTES = 512 << 20


def sample(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / inner


def summary(ts):
    ts = sorted(ts)
    return {"min_ms": ts[0], "median_ms": statistics.median(ts), "p90_ms": ts[int(0.9 * (len(ts) - 1))], "samples": len(ts)}


def alternate(fns, inner, repeats=REPEATS):
    for f in fns:                       # warm-up: code objects, caches
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(repeats):
        for i, f in enumerate(fns):
            ts[i].append(sample(f, inner))
    return [summary(t) for t in ts]


def bench_shape(name, N, H, C, inner):
    def bf(*shape):
        return torch.randn(*shape, device=DEV).to(torch.bfloat16)
    d = ConvDesc(N, H, H, C, H, H, C, 3, 3, 1, 1, 1, 0, 0, 1, 0)
    w = torch.randn(C, C, 3, 3, device=DEV) * (2.0 / (9 * C)) ** 0.5
    wd = torch.empty(C, 9 * C, dtype=torch.bfloat16, device=DEV)
    call("adamml_pack_conv_weight", ptr(w), ptr(wd), C, C, C, 3, 3, 1)
    w8 = (2 ** torch.arange(8, device=DEV)).to(torch.int32)
    vec = torch.rand(1, 4, C, device=DEV) + 0.5
    sa = torch.zeros(1, STAT_SLOTS, 2 * C, dtype=torch.float64, device=DEV)
    sb = torch.zeros_like(sa)
    P = N * H * H
    # launch i works on buffer set i % nsets: together the sets exceed the 256 MB last-level cache, so that no launch finds the operands
    # of the one before it there (in the network they were written by other layers, long before)
    set_bytes = 9 * P * C * 2
    nsets = max(2, min(48, -(-CACHE_BYTES // set_bytes)))
    sets = []
    for _ in range(nsets):
        out = bf(N, H, H, C).clamp_min(0)
        mask = ((out > 0).view(N, H, H, C // 8, 8).to(torch.int32) * w8).sum(-1).to(torch.uint8).contiguous()
        g_idn = bf(N, H, H, C)
        sets.append(dict(dz=bf(N, H, H, C) * 0.1, out=out, mask=mask, z=bf(N, H, H, C), z2=bf(N, H, H, C), g_idn=g_idn, dx_a=g_idn.clone(), dx_b=g_idn.clone(),
                         dx_c=g_idn.clone(), g2=torch.empty_like(g_idn)))
    turn = [0, 0, 0]

    def pair():
        b = sets[turn[0] % nsets]
        turn[0] += 1
        call("adamml_conv_bwd_data", byref(d), ptr(b["dz"]), ptr(wd), ptr(b["dx_a"]), 1)
        call("adamml_residual_bwd", ptr(b["dx_a"]), ptr(b["out"]), 1, ptr(b["g2"]), ptr(b["z"]), ptr(vec), ptr(sa), None, None, None, P, C, 1)

    def fused():
        b = sets[turn[1] % nsets]
        turn[1] += 1
        call("adamml_conv_bwd_data_res", byref(d), ptr(b["dz"]), ptr(wd), ptr(b["dx_b"]), 1, ptr(b["out"]), ptr(b["mask"]), 1, ptr(b["z"]), ptr(vec), ptr(sa), None, None,
             None)

    def fused_tile():
        b = sets[turn[2] % nsets]
        turn[2] += 1
        call("adamml_conv_bwd_data_res", byref(d), ptr(b["dz"]), ptr(wd), ptr(b["dx_c"]), 1, ptr(b["out"]), ptr(b["mask"]), 1, ptr(b["z"]), ptr(vec), ptr(sa), ptr(b["z2"]),
             ptr(vec), ptr(sb))

    def check():
        """pair and fused once each from the same identity-path gradient (buffer set 0): largest difference of g' in units of its largest
        value (one bf16 ulp = 2^-8 relative) and of the per-channel sums relative to the largest sum"""
        res = {}
        b = sets[0]
        for name, fn, t, dxo in (("pair", pair, 0, b["g2"]), ("fused", fused, 1, b["dx_b"])):
            b["dx_a"].copy_(b["g_idn"])
            b["dx_b"].copy_(b["g_idn"])
            sa.zero_()
            turn[t] = 0
            fn()
            tot = torch.empty(1, 2 * C, dtype=torch.float64, device=DEV)
            call("adamml_stats_collapse", ptr(sa), ptr(tot), C, 1)
            torch.cuda.synchronize()
            res[name] = (dxo.float().clone(), tot)
        (ga, sa_a), (gb, sa_b) = res["pair"], res["fused"]
        return {"dx_max_diff_rel": ((ga - gb).abs().max() / ga.abs().max()).item(), "dx_finite": bool(torch.isfinite(gb).all()),
                "dx_max_abs": ga.abs().max().item(), "sums_max_diff_rel": ((sa_a - sa_b).abs().max() / sa_a.abs().max()).item()}

    streams = int(hip.load().adamml_conv_bwd_data_res_streams(byref(d)))
    supported = bool(hip.load().adamml_conv_bwd_data_res_supported(byref(d)))
    if not supported:                    # the probe refuses the shape: time the pair alone
        a, = alternate([pair], inner)
        return {"shape": name, "frames": N, "pair": a, "fused": None, "probe": 0}
    ck = check()                         # (first: the timed launches accumulate onto their own outputs)
    arms = alternate([pair, fused] + ([fused_tile] if streams == 2 else []), inner)
    a, b = arms[:2]
    spread = max(a["p90_ms"] - a["min_ms"], b["p90_ms"] - b["min_ms"])
    keep = b["median_ms"] < a["median_ms"] - spread
    x_gb = N * H * H * C * 2 / 1e9
    r = {"shape": name, "frames": N, "tensor_GB": x_gb, "inner": inner, "buffer_sets": nsets, "pair": a, "fused": b, "spread_ms": spread, "keep": bool(keep),
         "probe": 1, "streams": streams, "check": ck}
    if streams == 2:
        c = arms[2]
        sp = max(c["p90_ms"] - c["min_ms"], b["p90_ms"] - b["min_ms"])
        r.update({"fused_tile_with_z_b": c, "spread_vs_tile_ms": sp, "keep_vs_tile": bool(b["median_ms"] < c["median_ms"] - sp)})
    return r


def bench_steps():
    import torch.nn.functional as F
    from adamml_amd.resnet import resnet
    real = runtime._residual_fusable
    out = {}
    x = torch.randn(72, 8 * 3, 224, 224, device=DEV)
    target = torch.randint(0, 31, (72,), device=DEV)
    for depth in (18, 34, 50):
        torch.manual_seed(0)
        model = resnet(depth, 31, False, 8, 0.5, "max", 3, imagenet_pretrained=False).to(DEV).train()

        def step(fusable):
            runtime._residual_fusable = fusable
            try:
                model.zero_grad(set_to_none=False)
                F.cross_entropy(model(x), target).backward()
            finally:
                runtime._residual_fusable = real
        forms = [("fused", real)] if depth == 50 else [("fused", real), ("fallback", lambda xx, d: d.KH == 1 and real(xx, d))]
        res = alternate([lambda f=f: step(f) for _, f in forms], 1, repeats=12)
        out["resnet%d" % depth] = {n: r for (n, _), r in zip(forms, res)}
        del model
        torch.cuda.empty_cache()
    return out


def main():
    args = sys.argv[1:]
    if not torch.cuda.is_available():
        raise SystemExit("bench_basicblock_dgrad_res: needs the GPU")
    res = {"device": torch.cuda.get_device_name(0), "geometry": "one segment call of 72 videos x 8 frames (ResNet-34 main net), 1 BatchNorm group",
           "repeats": REPEATS, "rule": "keep iff median(fused) < median(pair) - max(p90 - min of either)",
           "shapes": [bench_shape(*s) for s in SHAPES]}
    for r in res["shapes"]:
        print(json.dumps(r), flush=True)
    if "--steps" in args:
        res["train_step_b72_224px"] = bench_steps()
        print(json.dumps(res["train_step_b72_224px"]), flush=True)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
