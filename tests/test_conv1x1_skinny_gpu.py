"""The weight-streaming 1x1 kernel for serving-size batches (csrc/conv1x1_skinny.hip).  adamml_conv_fwd dispatches to it where
adamml_conv1x1_skinny_supported says yes, so the rows call that entry point with the mode-0 weight pack and no statistics, as the
eval-mode executor does, and assert the probe.  References, checker and tolerance are those of the tile kernel's 1x1 rows
(tests/conv_ref.py, n = Cin); buffers come from tests/guarded.py.  The second test holds the kernel to the tile kernel bit for bit, the
third follows it through the public model."""
import pytest
import torch
from ctypes import byref

from tests import conv_ref as R
from adamml_amd import hip
from adamml_amd.hip import ConvDesc, call, ptr

# (pixels per group, Cin, Cout, groups, what it catches)
CASES = [
    (1, 32, 32, 1, "smallest case: one pixel, a quarter panel, two idle slices"),
    (49, 512, 2048, 1, "layer-4 shape"),
    (49, 2048, 512, 2, "longest K, per-group vectors"),
    (50, 1024, 256, 1, "P not a multiple of 16"),
    (65, 64, 64, 3, "the last pixel chunk holds one pixel; half a panel"),
    (392, 256, 1024, 1, "several chunks of 32 pixels; fewer panels than ring slots"),
    (200, 64, 2048, 1, "chunks of 64 pixels, the last one ragged"),
    (1568, 1024, 512, 1, "the long-K cut-over: 25 chunks of 64 pixels"),
]
IDS = ["P%d-%d-%d-G%d" % c[:4] for c in CASES]
INPUTS = {"plain": None, "lazy-none": 0, "lazy-relu": 1}


def desc(P, Cin, Cout, G, act=None, k=1):
    return ConvDesc(1, 1, P, Cin, 1, P, Cout, k, k, 1, k // 2, 1, act or 0, 0, G, 4 * Cin if (act is not None and G > 1) else 0)


def test_probe_answers_on_the_documented_shapes():
    """the host side of the predicate (no GPU)"""
    import __graft_entry__ as ge
    ge.build()
    probe = hip.load().adamml_conv1x1_skinny_supported
    assert all(probe(byref(desc(*c[:4])), 0) == 1 for c in CASES)
    assert probe(byref(desc(49, 512, 2048, 1)), 1) == 0                     # statistics: a training launch
    assert probe(byref(desc(49, 512, 512, 1, k=3)), 0) == 0                 # 3x3
    assert [probe(byref(desc(P, 1024, 2048, 1)), 0) for P in (896, 897)] == [1, 0]       # 7 x 32 < 256 <= 8 x 32 tile workgroups
    assert [probe(byref(desc(P, 512, 2048, 1)), 0) for P in (392, 393)] == [1, 0]        # the pixel cut-over, Cin < 1024
    assert [probe(byref(desc(P, 1024, 256, 1)), 0) for P in (1568, 1569)] == [1, 0]      # ... and from Cin = 1024 on
    assert probe(byref(desc(49, 520, 512, 1)), 0) == 0 and probe(byref(desc(49, 4096, 512, 1)), 0) == 0
    assert probe(byref(ConvDesc(1, 1, 49, 512, 1, 49, 512, 1, 1, 1, 0, 1, 0, 1, 1, 0)), 0) == 0      # accumulate


def operands(C, P, Cin, Cout, G, act, seed):
    x = C.rand_input(G, 1, P, Cin, Cin, seed)
    vflat = None
    if act is not None:
        vflat = C.lazy_vectors(G, Cin, seed + 1, act).reshape(-1)
        C.plant_bounds(x)
    return x, vflat, C.rand_weight(Cout, Cin, 1, seed + 2)


def launch(C, d, xd, wp, vd, shape):
    y = C.nan_fill(*shape)
    call("adamml_conv_fwd", byref(d), ptr(xd), ptr(wp), ptr(vd) if vd is not None else None, ptr(vd[d.Cin:]) if vd is not None else None,
         ptr(y), None)
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("inp", list(INPUTS))
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_skinny_against_float64(case, inp):
    from tests import test_conv_conformance_gpu as C
    (P, Cin, Cout, G, _), act = case, INPUTS[inp]
    d = desc(P, Cin, Cout, G, act)
    assert hip.load().adamml_conv1x1_skinny_supported(byref(d), 0) == 1
    C.GB.reset()
    x, vflat, w = operands(C, P, Cin, Cout, G, act, sum(map(ord, IDS[CASES.index(case)] + inp)) % 10007)
    a = R.lazy_operand(x, vflat, None if vflat is None else vflat[Cin:], act or 0, groups=G, gstride=d.in_gstride)
    ref, ab, n = R.conv_fwd_ref(a, w, 1, 0)
    y = launch(C, d, C.GB.frozen(x), C.pack(w, Cin, 0), None if vflat is None else C.GB.frozen(vflat), ref.shape)
    C.GB.check("conv_fwd (skinny)")
    R.check(y.cpu(), ref, ab, n, what="conv_fwd (skinny) %s %s" % (case[:4], inp))


@pytest.mark.gpu
@pytest.mark.parametrize("case,inp", [(CASES[1], "plain"), (CASES[2], "lazy-relu"), (CASES[4], "lazy-none")], ids=[IDS[1], IDS[2], IDS[4]])
def test_skinny_is_bit_identical_to_the_tile_kernel(case, inp):
    """the same rows at the head of each group of a launch above the cut-over (the probe answers 0: the tile kernel runs), filler behind"""
    from tests import test_conv_conformance_gpu as C
    (P, Cin, Cout, G, _), act = case, INPUTS[inp]
    probe = hip.load().adamml_conv1x1_skinny_supported
    Pb = next(q for q in range(128, 1 << 16, 128) if not probe(byref(desc(q, Cin, Cout, G, act)), 0))
    C.GB.reset()
    x, vflat, w = operands(C, P, Cin, Cout, G, act, 4242 + P)
    xb = C.rand_input(G, 1, Pb, Cin, Cin, 77)
    xb[:, :, :P] = x
    wp, vd = C.pack(w, Cin, 0), None if vflat is None else C.GB.frozen(vflat)
    small = launch(C, desc(P, Cin, Cout, G, act), C.GB.frozen(x), wp, vd, (G, 1, P, Cout))
    big = launch(C, desc(Pb, Cin, Cout, G, act), C.GB.frozen(xb), wp, vd, (G, 1, Pb, Cout))
    C.GB.check("conv_fwd (skinny and tile)")
    assert torch.equal(big[:, :, :P].cpu(), small.cpu())


@pytest.mark.gpu
def test_resnet50_eval_takes_the_skinny_kernel():
    """Through the public model: the eval-mode forward of one small clip (8 frames of 64 x 64: 16 pixels per frame in layer 3, 4 in
    layer 4) runs conv1 of 8 of the 9 bottlenecks of layers 3-4 on the new kernel -- 1024 -> 256 x 5 and 1024 -> 512 at 128 pixels,
    2048 -> 512 x 2 at 32; layer3.0.conv1 (512 -> 256) still sees layer 2's 512 pixels, above the cut-over of 392, as every 1x1 conv
    before it.  Placed first in a batch in which every layer is above the cut-over, no launch takes it and the clip's logits are the
    same bits."""
    from adamml_amd.resnet import resnet
    torch.manual_seed(50)
    model = resnet(depth=50, num_classes=7, without_t_stride=True, groups=8, dropout=0.0, pooling_method="max", input_channels=3,
                   imagenet_pretrained=False).to("cuda").eval()
    batch = torch.randn(50, 8 * 3, 64, 64, device="cuda")          # layer 4: 50 clips x 8 frames x 2 x 2 pixels = 1600 > 1568

    def run(x):
        hip.profiler = hip.LaunchProfiler()
        try:
            with torch.no_grad():
                y = model(x)
            torch.cuda.synchronize()
            recs = hip.profiler.records
        finally:
            hip.profiler = None
        return y, [name for name, _, _, meta in recs if len(meta) > 2 and meta[2] == "conv1x1_skinny_kernel"]

    y1, named1 = run(batch[:1])
    yb, namedb = run(batch)
    assert named1 == ["adamml_conv_fwd"] * 8, named1
    assert not namedb, namedb
    assert torch.isfinite(y1).all() and torch.equal(y1, yb[:1])
