"""The 16-channel 7x7 stem kernels (csrc/conv_stem16.hip) against float64: the stem of the flow (10 channels) and RGB-diff (15 channels)
ResNets.  adamml_conv_fwd / adamml_conv_bwd_weight dispatch to them where adamml_conv_stem16_supported says yes, so the rows call those
entry points with the mode-0 weight pack, as the executor does, and assert the probe.  References, checkers and tolerances are those of
tests/conv_ref.py and tests/elementwise_ref.py with n = the reduction length the kernel really sums: 25 steps x 32 = 800 forward
(784 real), the pixel count for the weight gradient; buffers come from tests/guarded.py."""
import pytest
import torch
import torch.nn.functional as F
from ctypes import byref

from tests import conv_ref as R
from tests import elementwise_ref as E

pytestmark = pytest.mark.gpu

from adamml_amd import hip  # noqa: E402
from adamml_amd.hip import ConvDesc, call, ptr  # noqa: E402
from tests.guarded import workspace_launches  # noqa: E402
from tests.test_conv_conformance_gpu import DEV, GB, guard, pack, ssum, zstats  # noqa: E402,F401  (guard: the autouse check of every row)

K_SUMMED = 25 * 32

# (N, H, W, Cin, G, why)
CASES = [
    (2, 7, 10, 10, 2, "every output touches the border; one strip, two groups"),
    (2, 33, 46, 15, 2, "odd H; ragged last strip; a partly dead last pixel tile"),
    (1, 20, 224, 10, 1, "full width: the one-row strip, the maximal patch, the raised LDS limit"),
    (1, 24, 160, 16, 3, "no padded channels, a second width, three groups"),
    # 600 one-strip images: more strips than the cap of 256 workgroups of the forward and of the weight gradient, so a workgroup walks
    # 3 strips, crosses image boundaries and restarts its prefetch
    (600, 14, 20, 10, 1, "more strips than workgroups"),
]


@pytest.mark.parametrize("N,H,W,Cin,G", [c[:5] for c in CASES], ids=["N%d-%dx%d-Cin%d-G%d" % c[:5] for c in CASES])
def test_conv_stem16(N, H, W, Cin, G):
    name = "N%d-%dx%d-Cin%d-G%d" % (N, H, W, Cin, G)
    seed = sum(map(ord, name)) % 10007
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    d = ConvDesc(N, H, W, 16, OH, OW, 64, 7, 7, 2, 3, 1, 0, 0, G, 0)
    assert hip.load().adamml_conv_stem16_supported(byref(d)) == 1
    x = E.rand_bf16(G * N, H, W, 16, seed=seed)
    x[..., Cin:] = 0
    w = R.bf16(torch.randn(64, Cin, 7, 7, generator=E.gen(seed + 1), dtype=torch.float64) * (2.0 / (Cin * 49)) ** 0.5).float()
    ref, ab, _ = R.conv_fwd_ref(x.double(), w, 2, 3)
    xd, wp = GB.frozen(x), pack(w, 16, 0)
    y, st = GB.out((G * N, OH, OW, 64), torch.bfloat16), zstats(G, 64)
    call("adamml_conv_fwd", byref(d), ptr(xd), ptr(wp), None, None, ptr(y), ptr(st))
    h = y.cpu()
    r = R.check(h, ref, ab, K_SUMMED, what="conv_fwd (stem16) " + name)
    R.stats_check(ssum(st), h, what="conv_fwd (stem16) stats " + name, groups=G)
    GB.check("conv_fwd (stem16) " + name)

    g = E.rand_bf16(G * N, OH, OW, 64, seed=seed + 2)
    wref, wab, n = R.conv_wgrad_ref(x.double(), g.double(), (64, Cin, 7, 7), 2, 3)
    base = torch.randn(64, Cin, 7, 7, generator=E.gen(seed + 3))
    gd = GB.frozen(g)

    def launch(outs, ws, nbytes):
        call("adamml_conv_bwd_weight", byref(d), ptr(gd), ptr(xd), None, None, ptr(outs[0]), Cin, ptr(ws), nbytes)

    # exact, dirty, one float short: an undersized workspace is ignored as a whole (the entry point's contract: the tile kernel's atomic form)
    q = hip.load().adamml_conv_bwd_weight_workspace(byref(d), Cin)
    (dw,), (dw_short,) = workspace_launches(GB, q, lambda: (GB.inout(base),), launch, "fallback", "conv_bwd_weight (stem16) " + name)
    rw = E.wgrad_check(dw.cpu(), wref + base.double(), wab + base.double().abs(), n, what="conv_bwd_weight (stem16) " + name, products_round=False)
    E.wgrad_check(dw_short.cpu(), wref + base.double(), wab + base.double().abs(), n, what="conv_bwd_weight (short) " + name, products_round=False)
    print("  stem16 %s: forward err/tol %.3f, weight gradient err/tol %.3f" % (name, r, rw))


@pytest.mark.parametrize("channels", [10, 15])
def test_resnet18_stem_runs_the_stem16_kernels(channels):
    """Through the public model: conv1 of a 10- / 15-channel ResNet-18 is served by the stem16 kernels -- once forward and once in the
    weight gradient of a train step, forward only in eval, and no weight gradient for a frozen conv1."""
    from adamml_amd.resnet import resnet
    torch.manual_seed(channels)
    model = resnet(depth=18, num_classes=5, without_t_stride=False, groups=8, dropout=0.0, pooling_method="max", input_channels=channels,
                   imagenet_pretrained=False).to(DEV)
    x = torch.randn(1, 8 * channels, 32, 32, device=DEV)

    def kernels(train, backward):
        model.train(train)
        model.zero_grad()
        hip.profiler = hip.LaunchProfiler()
        try:
            with torch.set_grad_enabled(backward):
                y = model(x)
                if backward:
                    F.cross_entropy(y, torch.zeros(1, dtype=torch.long, device=DEV)).backward()
            torch.cuda.synchronize()
            recs = hip.profiler.records
        finally:
            hip.profiler = None
        assert torch.isfinite(y).all()
        named = [(name, meta[2]) for name, _, _, meta in recs if len(meta) > 2 and meta[2] and "stem16" in meta[2]]
        sevens = [name for name, _, _, meta in recs if name in ("adamml_conv_stem_fwd", "adamml_conv_stem_bwd_weight")]
        assert not sevens, sevens
        return named

    fwd, wg = ("adamml_conv_fwd", "conv_stem16_kernel"), ("adamml_conv_bwd_weight", "conv_stem16_wgrad_kernel")
    assert sorted(kernels(True, True)) == sorted([fwd, wg])
    assert kernels(False, False) == [fwd]
    model.conv1.weight.requires_grad = False
    assert kernels(True, True) == [fwd]
