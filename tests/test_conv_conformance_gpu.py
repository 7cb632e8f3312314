"""Conformance of every conv dispatch branch against a float64 reference (tests/conv_ref.py).

One row per kernel instance that adamml_conv_fwd / adamml_conv_bwd_data(_bn) / adamml_conv_bwd_weight(_grouped) can select (tile width,
MODE, loader and epilogue of conv_gemm_kernel included; profiles/conv_conformance_rows.md lists what each row launched); the row id
names the instance (conv_gemm_kernel<BC, MODE, ...> rows: BC = output-channel tile, MODE 0 = 1x1, 1 = KxK gather, 2 = zero-upsampled,
3 = one parity class of a stride-2 data gradient; loader glds = LDS-DMA, deep = look-ahead ring, reg = register ring).  Where the
library exports a probe, the row asserts it, so that a predicate narrowed later fails here by name instead of quietly testing the
generic kernel.  Operands are generated on the CPU (bf16-representable weights, data that crosses the activation bounds, exact bound
values planted), outputs are pre-filled with NaN (or a base tensor when accumulating) so an element a kernel never writes fails.
Every buffer a row hands to a kernel comes from tests/guarded.py: outputs, accumulators and workspaces lie inside sentinel bands, read-only
operands are compared bit for bit after the launch, and the rows that take a workspace run three times (exactly the size the query
answers, the same on a workspace that held other bytes, one float short).
The second part checks that non-finite operands propagate as they do in torch."""
import time

import pytest
import torch
import torch.nn.functional as F
from ctypes import byref

from tests import conv_ref as R

pytestmark = pytest.mark.gpu

from adamml_amd import hip  # noqa: E402
from adamml_amd.hip import ConvDesc, call, ptr, STAT_SLOTS  # noqa: E402
from adamml_amd.runtime import pad8  # noqa: E402
from tests.guarded import Scope, workspace_launches  # noqa: E402

DEV = "cuda"
GB = Scope(DEV)     # every device buffer of a row (tests/guarded.py)
WORST = {}          # row id -> max err / tol (printed at the end of the module: pytest -s)
T0 = time.time()
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


@pytest.fixture(autouse=True)
def guard():
    GB.reset()
    yield
    GB.check("at the end of the row")
    GB.reset()


def pack(w, cin_pad, mode):
    """adamml_pack_conv_weight on a CPU weight -> the packed weight, from then on a read-only operand"""
    cout, cin, kh, kw = w.shape
    wd = GB.frozen(w.float())
    if mode == 2:
        out = GB.out((kh * kw, cout), F32)
        call("adamml_pack_conv_weight", ptr(wd), ptr(out), cout, 1, 1, kh, kw, 2)
    elif mode == 0:
        out = GB.out((cout, kh * kw * cin_pad), BF16)
        call("adamml_pack_conv_weight", ptr(wd), ptr(out), cout, cin, cin_pad, kh, kw, 0)
    else:
        out = GB.out((cin_pad, kh * kw * cout), BF16)
        call("adamml_pack_conv_weight", ptr(wd), ptr(out), cout, cin, cin_pad, kh, kw, 1)
    return GB.frozen(out)               # (its bands and its interior are checked with the row's next check)


def zstats(G, C):
    return GB.zeros((G, STAT_SLOTS, 2 * C), F64)


def ssum(t):
    """per-channel totals of a statistic accumulator [G][STAT_SLOTS][2C] (adamml_stats_collapse) -> [G][2C] float64"""
    G, _, C2 = t.shape
    out = GB.out((G, C2), F64)
    call("adamml_stats_collapse", ptr(t), ptr(out), C2 // 2, G)
    return out


def probe(name, d, *args):
    return getattr(hip.load(), name)(byref(d), *args)


def record(rid, r):
    WORST[rid] = max(WORST.get(rid, 0.0), r)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    if WORST:
        k = max(WORST, key=WORST.get)
        print("\nconv conformance: C_ACC = %g, largest err/tol %.4f (%s) over %d rows, %.0f s" % (R.C_ACC, WORST[k], k, len(WORST), time.time() - T0))
        for rid in sorted(WORST):
            print("  %-60s %.4f" % (rid, WORST[rid]))


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rand_input(n, h, w, c, cin_true, seed, scale=1.0, offset=0.0):
    """NHWC bf16 on the CPU, padded channels zero"""
    x = (torch.randn(n, h, w, c, generator=gen(seed)) * scale + offset).to(torch.bfloat16)
    x[..., cin_true:] = 0
    return x


def rand_weight(cout, cin, k, seed):
    w = torch.randn(cout, cin, k, k, generator=gen(seed), dtype=torch.float64) * (2.0 / (cin * k * k)) ** 0.5
    return R.bf16(w).float()


def lazy_vectors(groups, c, seed, act):
    """[groups][4][c] (scale, shift, mean, invstd) with channel 0 set to scale 1/2, shift 1: its z = 10 and z = -2 land exactly on 6
    and 0 (see plant_bounds)"""
    g = gen(seed)
    v = torch.empty(groups, 4, c)
    v[:, 0] = torch.rand(groups, c, generator=g) + 0.5
    v[:, 1] = torch.randn(groups, c, generator=g) * (1.0 if act == 2 else 0.5)
    v[:, 2] = torch.randn(groups, c, generator=g) * 0.3
    v[:, 3] = torch.rand(groups, c, generator=g) + 0.5
    v[:, 0, 0], v[:, 1, 0] = 0.5, 1.0
    return v


def plant_bounds(x):
    """pre-activations exactly at the clamp bounds in channel 0 (lazy_vectors)"""
    flat = x.view(-1, x.shape[-1])
    flat[0::7, 0] = 10.0
    flat[3::7, 0] = -2.0
    return x


def nan_fill(*shape):
    return GB.out(shape, BF16)


# ---------------------------------------------------------------------------------------------------------------------- forward
# (id, N, H, W, Cin, Cout, k, stride, pad, act (None = plain input), groups, per-group vectors, accumulate, probes)
# probes: "c64" adamml_conv_fused_input_supported, "narrow" adamml_conv1x1_narrow_supported(kind 0), "wide" adamml_conv1x1_wide_supported(kind 0);
# "!x": the probe must be 0
FWD = [
    ("c64-plain[conv3x3_c64_kernel]", 2, 20, 20, 64, 64, 3, 1, 1, None, 1, False, 0, "c64"),
    ("c64-lazy-relu[conv3x3_c64_kernel]", 2, 20, 20, 64, 64, 3, 1, 1, 1, 1, False, 0, "c64"),
    ("c64-g3-relu6[conv3x3_c64_kernel]", 2, 14, 14, 64, 64, 3, 1, 1, 2, 3, True, 0, "c64"),
    ("c64-ragged57x33-none[conv3x3_c64_kernel]", 1, 57, 33, 64, 64, 3, 1, 1, 0, 1, False, 0, "c64"),
    ("c64-8x8[conv3x3_c64_kernel]", 4, 8, 8, 64, 64, 3, 1, 1, 1, 1, False, 0, "c64"),
]
# narrow: every (ceil(Cin/32), Cout) instance at both ends of its Cin bucket
for ci, co in ((8, 16), (32, 16), (8, 96), (32, 96), (8, 144), (32, 144), (8, 192), (32, 192), (72, 24), (96, 24), (136, 24), (160, 24),
               (136, 32), (160, 32), (168, 32), (192, 32)):
    FWD.append(("narrow-%d-%d[conv1x1_narrow_fwd_kernel<%d,%d>]" % (ci, co, (ci + 31) // 32, co), 2, 21, 19, ci, co, 1, 1, 0,
                (ci + co) % 3, 1, False, 0, "narrow"))
FWD += [
    ("wide-512-P2048[wide_all_kernel]", 2, 32, 32, 256, 512, 1, 1, 0, None, 1, False, 0, "wide"),
    ("wide-640-P2049-relu[wide_all_kernel]", 1, 1, 2049, 256, 640, 1, 1, 0, 1, 1, False, 0, "wide"),
    ("wide-1920-s2-oddH-relu6[wide_all_kernel]", 2, 63, 65, 256, 1920, 1, 2, 0, 2, 1, False, 0, "wide"),
    ("wide-2048-P2049[wide_all_kernel]", 1, 1, 2049, 256, 2048, 1, 1, 0, None, 1, False, 0, "wide"),
    ("wide-1024-g2-lazy[wide_all_kernel]", 2, 32, 32, 256, 1024, 1, 1, 0, 1, 2, True, 0, "wide"),
    ("wide-1024-accumulate[wide_all_kernel]", 2, 32, 32, 256, 1024, 1, 1, 0, None, 1, False, 1, "wide"),
    # a lazy input does not have an accumulating form in the wide kernel: conv_gemm_kernel serves it (it used to fail with EUNSUPPORTED)
    # (the kind-0 probe ignores accumulate and in_scale: "=gemm" pins the routing -- bit-identical to the run with the wide kernel switched off)
    ("wide-shape-accumulate-lazy[conv_gemm_kernel<64,0,3>]", 2, 32, 32, 256, 512, 1, 1, 0, 1, 1, False, 1, "wide,=gemm"),
    ("gemm-bc64-cout200-P2049[conv_gemm_kernel<64,0,glds>]", 1, 1, 2049, 64, 200, 1, 1, 0, None, 1, False, 0, "!narrow"),
    ("gemm-bc64-cout200-accumulate[conv_gemm_kernel<64,0,glds,acc>]", 1, 1, 2049, 64, 200, 1, 1, 0, None, 1, False, 1, ""),
    ("gemm-bc128-cout264-P%128=127[conv_gemm_kernel<128,0,glds>]", 1, 185, 119, 64, 264, 1, 1, 0, None, 1, False, 0, ""),
    ("gemm-k40-lazy-relu[conv_gemm_kernel<64,0,reg>]", 2, 30, 30, 40, 200, 1, 1, 0, 1, 1, False, 0, "!narrow"),
    ("gemm-mode1-3x3s2[conv_gemm_kernel<64,1,glds>]", 2, 31, 31, 128, 128, 3, 2, 1, None, 1, False, 0, ""),
    ("gemm-mode1-3x3s2-lazy-relu6[conv_gemm_kernel<64,1,reg>]", 2, 31, 31, 128, 128, 3, 2, 1, 2, 1, False, 0, ""),
    ("gemm-mode1-7x7s2-cin3[conv_gemm_kernel<64,1,glds>]", 2, 33, 33, 3, 64, 7, 2, 3, None, 1, False, 0, ""),
    ("gemm-mode1-7x7s2-cin10-lazy[conv_gemm_kernel<64,1,reg>]", 1, 32, 32, 10, 64, 7, 2, 3, 1, 1, False, 0, ""),
    ("gemm-deep-k2048-lazy-none[conv_gemm_kernel<64,0,3>]", 2, 7, 7, 2048, 512, 1, 1, 0, 0, 1, False, 0, ""),
    ("gemm-reg-many-wg-lazy-relu[conv_gemm_kernel<64,0,reg>]", 2, 100, 100, 128, 256, 1, 1, 0, 1, 1, False, 0, ""),
    ("gemm-bc128-g3-lazy[conv_gemm_kernel<128,0,reg>]", 6, 64, 64, 128, 256, 1, 1, 0, 1, 3, True, 0, ""),
    # 128-wide tiles need ceil(P / 128) * ceil(Cout / 128) * groups >= 512 (conv_launch): the 3x3 family of the hot path
    ("gemm-bc128-mode1-3x3[conv_gemm_kernel<128,1,glds>]", 6, 61, 61, 64, 384, 3, 1, 1, None, 1, False, 0, "!c64"),
    ("gemm-bc128-mode1-3x3-lazy-relu[conv_gemm_kernel<128,1,reg>]", 6, 61, 61, 64, 384, 3, 1, 1, 1, 1, False, 0, ""),
    ("gemm-bc128-mode1-3x3-accumulate[conv_gemm_kernel<128,1,glds,acc>]", 6, 61, 61, 64, 384, 3, 1, 1, None, 1, False, 1, ""),
    ("gemm-bc128-deep-k512-lazy-relu6[conv_gemm_kernel<128,0,3>]", 4, 64, 64, 512, 512, 1, 1, 0, 2, 1, False, 0, "!wide"),
]


def fwd_desc(row):
    rid, N, H, W, Cin, Cout, k, s, p, act, G, pergroup, acc, probes = row
    cp = pad8(Cin)
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    return ConvDesc(N, H, W, cp, OH, OW, Cout, k, k, s, p, 1, act or 0, acc, G, 4 * cp if (act is not None and pergroup) else 0)


def check_probes(probes, d):
    for pr in filter(None, probes.split(",")):
        if pr.startswith("="):
            continue
        want = 0 if pr.startswith("!") else 1
        name = {"c64": ("adamml_conv_fused_input_supported",), "narrow": ("adamml_conv1x1_narrow_supported", 0),
                "wide": ("adamml_conv1x1_wide_supported", 0)}[pr.lstrip("!")]
        assert probe(name[0], d, *name[1:]) == want, (pr, name)


@pytest.mark.parametrize("row", FWD, ids=[r[0] for r in FWD])
def test_conv_fwd(row, monkeypatch):
    rid, N, H, W, Cin, Cout, k, s, p, act, G, pergroup, acc, probes = row
    d = fwd_desc(row)
    check_probes(probes, d)
    cp, seed = d.Cin, sum(map(ord, rid)) % 10007
    x = rand_input(G * N, H, W, cp, Cin, seed, scale=3.0 if act == 2 else 1.0, offset=1.0 if act == 2 else 0.0)
    scale = shift = None
    if act is not None:
        vec = lazy_vectors(G if pergroup else 1, cp, seed + 1, act)
        vec[..., Cin:] = 0
        plant_bounds(x)
        x[..., Cin:] = 0
        vflat = vec.reshape(-1)
        scale, shift = vflat, vflat[cp:]
    w = rand_weight(Cout, Cin, k, seed + 2)
    a = R.lazy_operand(x, scale, shift, act or 0, groups=G, gstride=d.in_gstride, cin_true=Cin)
    ref, ab, n = R.conv_fwd_ref(a, w, s, p)
    xd, wp = GB.frozen(x), pack(w, cp, 0)
    vd = GB.frozen(vflat) if act is not None else None
    if acc:
        base = (torch.randn(ref.shape, generator=gen(seed + 3)) * ref.abs().mean()).to(torch.bfloat16)
        y = GB.inout(base)
    else:
        y = nan_fill(*ref.shape)
    stats = None if acc else zstats(G, Cout)
    call("adamml_conv_fwd", byref(d), ptr(xd), ptr(wp), ptr(vd) if vd is not None else None,
         ptr(vd[cp:]) if vd is not None else None, ptr(y), ptr(stats) if stats is not None else None)
    GB.check(rid)
    h = y.cpu()
    if acc:
        r = R.check(h, base.double() + ref, ab + base.double().abs(), n, extra=R.RHO_BF16 * ref.abs(), what=rid)
    else:
        r = R.check(h, ref, ab, n, what=rid)
        R.stats_check(ssum(stats), h, what=rid + " stats", groups=G)
    record(rid, r)
    if "=gemm" in probes:
        monkeypatch.setenv("ADAMML_WIDE_STREAM", "0")            # (read at every call)
        y2 = GB.inout(base) if acc else nan_fill(*ref.shape)
        call("adamml_conv_fwd", byref(d), ptr(xd), ptr(wp), ptr(vd) if vd is not None else None,
             ptr(vd[cp:]) if vd is not None else None, ptr(y2), None)
        GB.check(rid + " (wide kernel off)")
        assert torch.equal(y2.cpu(), h), rid + ": not the conv_gemm_kernel result"


# ---------------------------------------------------------------------------------------------------------------- data gradient
# (id, N, H, W, Cin, Cout, k, stride, pad, accumulate, bn (None or act of the fused BatchNorm epilogue), groups, probes)
# probes: "narrow3" / "narrow4": adamml_conv1x1_narrow_supported(kind 3 / 4); "wide3" / "wide4": adamml_conv1x1_wide_supported(kind 3 / 4)
DGRAD = [
    ("s1-1x1-256to64[conv_gemm_kernel<64,0,glds>]", 2, 20, 20, 64, 256, 1, 1, 0, 0, None, 1, "!narrow3,!wide3"),
    ("s1-3x3-128[conv_gemm_kernel<64,1,glds>]", 2, 14, 14, 128, 128, 3, 1, 1, 0, None, 1, ""),
    ("s1-3x3-128-accumulate[conv_gemm_kernel<64,1,glds,acc>]", 2, 14, 14, 128, 128, 3, 1, 1, 1, None, 1, ""),
    ("s2-3x3-odd[conv_gemm_kernel<64,3>]", 2, 15, 13, 64, 128, 3, 2, 1, 0, None, 1, ""),
    ("s2-3x3-even-accumulate[conv_gemm_kernel<64,3,acc>]", 2, 16, 14, 64, 128, 3, 2, 1, 1, None, 1, ""),
    ("s2-3x3-H1[conv_gemm_kernel<64,3>]", 3, 1, 9, 64, 64, 3, 2, 1, 0, None, 1, ""),
    ("s2-3x3-W1-accumulate[conv_gemm_kernel<64,3,acc>]", 3, 9, 1, 64, 64, 3, 2, 1, 1, None, 1, ""),
    ("s2-1x1-odd[conv_gemm_kernel<64,3>]", 2, 15, 15, 128, 256, 1, 2, 0, 0, None, 1, ""),
    ("s2-1x1-even-accumulate[conv_gemm_kernel<64,3,acc>]", 2, 14, 16, 128, 256, 1, 2, 0, 1, None, 1, ""),
    ("mode2-7x7s2[conv_gemm_kernel<64,2,3>]", 1, 16, 16, 16, 64, 7, 2, 3, 0, None, 1, ""),
    ("narrow-96to24[conv1x1_narrow_fwd_kernel<1,96>]", 2, 21, 19, 96, 24, 1, 1, 0, 0, None, 1, "narrow3"),
    ("narrow-epi-16to96-bn-relu6[conv1x1_narrow_dgrad_kernel<3,16,bn>]", 2, 21, 19, 16, 96, 1, 1, 0, 0, 2, 1, "narrow4"),
    ("narrow-epi-24to144-accumulate[conv1x1_narrow_dgrad_kernel<5,24,acc>]", 2, 21, 19, 24, 144, 1, 1, 0, 1, None, 1, "narrow4"),
    ("narrow-epi-32to160-bn-relu6-g3[conv1x1_narrow_dgrad_kernel<5,32,bn>]", 2, 13, 11, 32, 160, 1, 1, 0, 0, 2, 3, "narrow4"),
    ("narrow-epi-32to192-accumulate[conv1x1_narrow_dgrad_kernel<6,32,acc>]", 2, 21, 19, 32, 192, 1, 1, 0, 1, None, 1, "narrow4"),
    ("wide-1024to256[wide_all_kernel]", 2, 32, 32, 1024, 256, 1, 1, 0, 0, None, 1, "wide3"),
    ("wide-1024to256-accumulate[wide_all_kernel]", 2, 32, 32, 1024, 256, 1, 1, 0, 1, None, 1, "wide4"),
    ("2048to512[conv_gemm_kernel<64,0,glds>]", 1, 47, 47, 2048, 512, 1, 1, 0, 0, None, 1, "!wide3"),
    ("bn-epi-g3-relu[conv_gemm_kernel<64,0,glds,bn>]", 2, 20, 20, 64, 256, 1, 1, 0, 0, 1, 3, ""),
    ("bn-epi-s2-3x3-relu6[conv_gemm_kernel<64,3,bn>]", 2, 15, 15, 64, 128, 3, 2, 1, 0, 2, 1, ""),
    ("bn-epi-s1-3x3-relu[conv_gemm_kernel<64,1,glds,bn>]", 2, 14, 14, 128, 128, 3, 1, 1, 0, 1, 1, ""),
    # 128-wide tiles (ceil(P / 128) * ceil(Cout / 128) * groups >= 512 for the executed conv: Cout = the forward Cin)
    ("s1-1x1-bc128-bn-relu[conv_gemm_kernel<128,0,glds,bn>]", 8, 64, 64, 256, 64, 1, 1, 0, 0, 1, 1, "!narrow4,!wide4"),
    ("s1-1x1-bc128-accumulate[conv_gemm_kernel<128,0,glds,acc>]", 8, 64, 64, 256, 64, 1, 1, 0, 1, None, 1, "!narrow4,!wide4"),
    ("s1-3x3-bc128[conv_gemm_kernel<128,1,glds>]", 8, 64, 64, 256, 64, 3, 1, 1, 0, None, 1, ""),
    ("s1-3x3-bc128-accumulate[conv_gemm_kernel<128,1,glds,acc>]", 8, 64, 64, 256, 64, 3, 1, 1, 1, None, 1, ""),
    ("s1-3x3-bc128-bn-relu6[conv_gemm_kernel<128,1,glds,bn>]", 8, 64, 64, 256, 64, 3, 1, 1, 0, 2, 1, ""),
    ("s2-3x3-bc128-odd[conv_gemm_kernel<128,3>]", 6, 123, 123, 384, 32, 3, 2, 1, 0, None, 1, ""),
    ("s2-3x3-bc128-odd-accumulate[conv_gemm_kernel<128,3,acc>]", 6, 123, 123, 384, 32, 3, 2, 1, 1, None, 1, ""),
    ("s2-3x3-bc128-odd-bn-relu[conv_gemm_kernel<128,3,bn>]", 6, 123, 123, 384, 32, 3, 2, 1, 0, 1, 1, ""),
    ("mode2-7x7s2-many-wg[conv_gemm_kernel<64,2,1>]", 2, 224, 224, 16, 8, 7, 2, 3, 0, None, 1, ""),
    ("mode2-7x7s2-accumulate[conv_gemm_kernel<64,2,3,acc>]", 1, 16, 16, 16, 64, 7, 2, 3, 1, None, 1, ""),
    ("mode2-7x7s2-bn-relu[conv_gemm_kernel<64,2,3,bn>]", 1, 16, 16, 16, 64, 7, 2, 3, 0, 1, 1, ""),
    ("mode2-7x7s2-bc128[conv_gemm_kernel<128,2,3>]", 8, 64, 64, 256, 8, 7, 2, 3, 0, None, 1, ""),
    ("mode2-7x7s2-bc128-many-wg[conv_gemm_kernel<128,2,1>]", 9, 64, 64, 384, 8, 7, 2, 3, 0, None, 1, ""),
]


@pytest.mark.parametrize("row", DGRAD, ids=[r[0] for r in DGRAD])
def test_conv_bwd_data(row):
    rid, N, H, W, Cin, Cout, k, s, p, acc, bn, G, probes = row
    cp = pad8(Cin)
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    d = ConvDesc(N, H, W, cp, OH, OW, Cout, k, k, s, p, 1, 0, 0, G, 0)
    for pr in filter(None, probes.split(",")):
        fn = "adamml_conv1x1_narrow_supported" if "narrow" in pr else "adamml_conv1x1_wide_supported"
        assert probe(fn, d, int(pr[-1])) == (0 if pr.startswith("!") else 1), pr
    seed = sum(map(ord, rid)) % 10007
    dz = rand_input(G * N, OH, OW, Cout, Cout, seed, scale=0.5)
    w = rand_weight(Cout, Cin, k, seed + 2)
    ref, ab, n = R.conv_dgrad_ref(R.lazy_operand(dz), w, (H, W), s, p)
    if cp != Cin:
        z0 = torch.zeros(ref.shape[:-1] + (cp - Cin,), dtype=torch.float64)
        ref, ab = torch.cat([ref, z0], -1), torch.cat([ab, z0], -1)
    wp = pack(w, cp, 1)
    dzd = GB.frozen(dz)
    if acc:
        base = (torch.randn(ref.shape, generator=gen(seed + 3)) * ref.abs().mean()).to(torch.bfloat16)
        dx = GB.inout(base)
    else:
        dx = nan_fill(*ref.shape)
    if bn is None:
        call("adamml_conv_bwd_data", byref(d), ptr(dzd), ptr(wp), ptr(dx), acc)
        GB.check(rid)
        h = dx.cpu()
        if acc:
            r = R.check(h, base.double() + ref, ab + base.double().abs(), n, extra=R.RHO_BF16 * ref.abs(), what=rid)
        else:
            r = R.check(h, ref, ab, n, what=rid)
    else:
        z = plant_bounds(rand_input(G * N, H, W, cp, cp, seed + 4, scale=3.0, offset=1.0))
        vec = lazy_vectors(G, cp, seed + 5, bn)
        zd, vd = GB.frozen(z), GB.frozen(vec)
        sums = zstats(G, cp)
        call("adamml_conv_bwd_data_bn", byref(d), ptr(dzd), ptr(wp), ptr(dx), ptr(zd), ptr(vd), bn, ptr(sums))
        GB.check(rid)
        m = R.bn_mask(z, vec, bn, groups=G)
        assert (m == 0).any() and (m == 1).any()
        h = dx.cpu()
        r = R.check(h, ref * m, ab * m, n, what=rid)
        sref, sab = R.bn_dgrad_sums_ref(h.double(), z, vec, groups=G)
        got = ssum(sums).cpu()
        npix = N * H * W
        r = max(r, R.err_ratio(got, sref, sab, npix, 2.0 ** -21))
        assert r <= 1.0, "%s sums: max err/tol %.3g" % (rid, r)
    record(rid, r)


# ------------------------------------------------------------------------------------------------------------- weight gradient
# (id, N, H, W, Cin, cin_true, Cout, k, stride, pad, act (None = plain), groups, workspace)
WGRAD = [
    ("c64-ws[conv3x3_c64_wgrad_kernel]", 2, 20, 20, 64, 64, 64, 3, 1, 1, 1, 1, True),
    ("c64-quadrant-128-ws[conv3x3_c64_wgrad_kernel]", 90, 27, 27, 128, 128, 128, 3, 1, 1, None, 1, True),
    ("lds-patch-192to64-OW33[conv3x3_wgrad_kernel]", 2, 33, 33, 192, 192, 64, 3, 1, 1, None, 1, False),
    ("lds-patch-192to64-OW33-lazy-ws[conv3x3_wgrad_kernel]", 2, 33, 33, 192, 192, 64, 3, 1, 1, 2, 1, True),
    ("glds-256x128[conv_wgrad_glds_kernel<256,128,2>]", 2, 24, 24, 256, 256, 512, 1, 1, 0, None, 1, True),
    ("glds-256x128-lazy[conv_wgrad_glds_kernel<256,128,2,LZB>]", 2, 24, 24, 256, 256, 512, 1, 1, 0, 1, 1, True),
    ("glds-128x256[conv_wgrad_glds_kernel<128,256,2>]", 2, 24, 24, 256, 256, 128, 1, 1, 0, None, 1, True),
    ("glds-128x256-lazy[conv_wgrad_glds_kernel<128,256,2,LZB>]", 2, 24, 24, 256, 256, 128, 1, 1, 0, 1, 1, True),
    ("glds-128x256-ragged-3x3s2[conv_wgrad_glds_kernel<128,256,2>]", 2, 29, 29, 128, 128, 128, 3, 2, 1, None, 1, True),
    ("glds-128x128x3[conv_wgrad_glds_kernel<128,128,3>]", 2, 24, 24, 128, 128, 384, 1, 1, 0, None, 1, True),
    ("glds-128x128x3-lazy[conv_wgrad_glds_kernel<128,128,3,LZB>]", 2, 24, 24, 128, 128, 384, 1, 1, 0, 2, 1, True),
    ("generic-64x64[conv_wgrad_kernel<64,64>]", 2, 24, 24, 64, 64, 64, 1, 1, 0, 1, 1, True),
    ("generic-64x64-atomic[conv_wgrad_kernel<64,64>]", 2, 24, 24, 64, 64, 64, 1, 1, 0, None, 1, False),
    ("generic-64x128[conv_wgrad_kernel<64,128>]", 2, 24, 24, 128, 128, 64, 1, 1, 0, None, 1, True),
    ("generic-128x64[conv_wgrad_kernel<128,64>]", 2, 24, 24, 64, 64, 128, 1, 1, 0, 0, 1, True),
    ("generic-128x128x6-atomic[conv_wgrad_kernel<128,128,6>]", 2, 29, 29, 128, 128, 128, 3, 2, 1, None, 1, False),
    ("generic-128x128x6-lazy-ws[conv_wgrad_kernel<128,128,6>]", 2, 29, 29, 128, 128, 128, 3, 2, 1, 1, 1, True),
    ("generic-128x128-g32[conv_wgrad_kernel<128,128>]", 1, 15, 15, 256, 256, 256, 3, 2, 1, 1, 32, True),
    ("stem-7x7s2-cin3[conv_wgrad_kernel<64,128>]", 2, 33, 33, 8, 3, 64, 7, 2, 3, None, 1, True),
    ("stem-7x7s2-cin10-lazy-atomic[conv_wgrad_kernel<64,128>]", 1, 32, 32, 16, 10, 64, 7, 2, 3, 1, 1, False),
]
for ci, co in ((16, 96), (32, 16), (96, 24), (24, 144), (144, 24), (144, 32), (32, 192), (192, 32)):
    WGRAD.append(("narrow-%dto%d-ws[conv1x1_narrow_wgrad_kernel]" % (ci, co), 2, 21, 19, ci, ci, co, 1, 1, 0, (ci + co) % 3, 1, True))


@pytest.mark.parametrize("row", WGRAD, ids=[r[0] for r in WGRAD])
def test_conv_bwd_weight(row):
    rid, N, H, W, Cin, cin_true, Cout, k, s, p, act, G, use_ws = row
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    d = ConvDesc(N, H, W, Cin, OH, OW, Cout, k, k, s, p, 1, act or 0, 0, G, 4 * Cin if act is not None and G > 1 else 0)
    if "narrow" in rid:
        assert probe("adamml_conv1x1_narrow_supported", d, 1) == 1
    seed = sum(map(ord, rid)) % 10007
    x = rand_input(G * N, H, W, Cin, cin_true, seed, scale=3.0 if act == 2 else 1.0, offset=1.0 if act == 2 else 0.0)
    scale = shift = None
    if act is not None:
        vec = lazy_vectors(G, Cin, seed + 1, act)
        plant_bounds(x)
        x[..., cin_true:] = 0
        vflat = vec.reshape(-1)
        scale, shift = vflat, vflat[Cin:]
    dz = rand_input(G * N, OH, OW, Cout, Cout, seed + 2, scale=0.25)
    a = R.lazy_operand(x, scale, shift, act or 0, groups=G, gstride=d.in_gstride, cin_true=cin_true)
    ref, ab, n = R.conv_wgrad_ref(a, R.lazy_operand(dz), (Cout, cin_true, k, k), s, p)
    base = torch.randn(ref.shape, generator=gen(seed + 3)) * ref.abs().mean().item()
    vd = GB.frozen(vflat) if act is not None else None
    xd, dzd = GB.frozen(x), GB.frozen(dz)

    def launch(outs, ws, nbytes):
        call("adamml_conv_bwd_weight", byref(d), ptr(dzd), ptr(xd), ptr(vd) if vd is not None else None, ptr(vd[Cin:]) if vd is not None else None,
             ptr(outs[0]), cin_true, ptr(ws), nbytes)

    if not use_ws:                                                      # the atomic path: no workspace at all
        dw = GB.inout(base)
        launch((dw,), None, 0)
        GB.check(rid)
        record(rid, R.check(dw.cpu(), base.double() + ref, ab, n, rho=R.RHO_F32, what=rid))
        return
    # exact, dirty, one float short: an undersized workspace is ignored (atomic accumulation), csrc/conv_wgrad.hip wgrad_launch
    q = hip.load().adamml_conv_bwd_weight_workspace(byref(d), cin_true)
    (dw,), (dw_short,) = workspace_launches(GB, q, lambda: (GB.inout(base),), launch, "fallback", rid)
    record(rid, R.check(dw.cpu(), base.double() + ref, ab, n, rho=R.RHO_F32, what=rid))
    record(rid + "+dirty", 0.0)
    record(rid + "+short", R.check(dw_short.cpu(), base.double() + ref, ab, n, rho=R.RHO_F32, what=rid + "+short"))


@pytest.mark.parametrize("C", [64, 128])
def test_conv_bwd_weight_grouped_lazy_dz(C):
    """adamml_conv_bwd_weight_grouped: per-group products with both operands lazily normalised (the Gram matrix a^T a of the algebraic
    BatchNorm backward), conv_wgrad_kernel<64, 64, 1, true> / <128, 128, 1, true>; out[g] is overwritten"""
    rid = "grouped-lazy-dz-%d[conv_wgrad_kernel<%d,%d,1,dz>]" % (C, min(C, 128), min(C, 128))
    G, N, H, W = 3, 2, 17, 15
    seed = C
    d = ConvDesc(N, H, W, C, H, W, C, 1, 1, 1, 0, 1, 1, 0, G, 4 * C)
    x = plant_bounds(rand_input(G * N, H, W, C, C, seed))
    vec = lazy_vectors(G, C, seed + 1, 1)
    vflat = vec.reshape(-1)
    a = R.lazy_operand(x, vflat, vflat[C:], 1, groups=G, gstride=4 * C)
    xd, vd = GB.frozen(x), GB.frozen(vflat)

    def launch(outs, ws, nbytes):
        call("adamml_conv_bwd_weight_grouped", byref(d), ptr(xd), ptr(vd), ptr(vd[C:]), 1, 4 * C, ptr(xd), ptr(vd), ptr(vd[C:]), ptr(outs[0]), C,
             ptr(ws), nbytes)

    # the per-group form has no atomic path: one float short is refused (EINVAL) before anything is launched
    q = hip.load().adamml_conv_bwd_weight_workspace(byref(d), C)
    (out,), _ = workspace_launches(GB, q, lambda: (GB.out((G, C, C), F32),), launch, "refuse", rid, sync=torch.cuda.synchronize)
    h = out.cpu()
    worst = 0.0
    for g in range(G):
        ag = a[g * N:(g + 1) * N]
        ref, ab, n = R.conv_wgrad_ref(ag, ag, (C, C, 1, 1), 1, 0)
        worst = max(worst, R.check(h[g], ref.view(C, C), ab.view(C, C), n, rho=R.RHO_F32, what="%s group %d" % (rid, g)))
    record(rid, worst)
    record(rid + "+dirty", 0.0)
    record(rid + "+short", 0.0)


def test_conv_bwd_weight_grouped_lazy_dz_unsupported_shape():
    """the lazy-dz form has instances for Cout == Cin in {64, >= 128} only: 64 -> 128 channels must be refused, not computed wrongly"""
    G, N, H, W, Cin, Cout = 2, 1, 8, 8, 128, 64
    d = ConvDesc(N, H, W, Cin, H, W, Cout, 1, 1, 1, 0, 1, 0, 0, G, 0)
    x = GB.frozen(torch.zeros(G * N, H, W, Cin, dtype=torch.bfloat16))
    dz = GB.frozen(torch.zeros(G * N, H, W, Cout, dtype=torch.bfloat16))
    v = GB.frozen(torch.ones(2 * Cout))
    q = hip.load().adamml_conv_bwd_weight_workspace(byref(d), Cin)
    assert q > 0
    ws = GB.workspace(q)
    out = GB.inout(torch.zeros(G, Cout, Cin))
    with pytest.raises(RuntimeError):
        call("adamml_conv_bwd_weight_grouped", byref(d), ptr(dz), ptr(v), ptr(v[Cout:]), 1, 0, ptr(x), None, None, ptr(out), Cin,
             ptr(ws), q)
    torch.cuda.synchronize()
    assert GB.untouched(out) and GB.untouched(ws)


# ----------------------------------------------------------------------------------------------------------- non-finite operands
NAN = float("nan")


def finite_pattern_matches(h, ref, what):
    fh, fr = torch.isfinite(h.detach().cpu().double()), torch.isfinite(ref)
    assert (~fr).any() and fr.any(), what + ": the row must produce both finite and non-finite reference outputs"
    assert torch.equal(fh, fr), "%s: %d outputs non-finite in torch are finite here, %d finite in torch are not" % (
        what, int((fh & ~fr).sum()), int((~fh & fr).sum()))


NAN_FWD = [r for r in FWD if r[0] in ("c64-lazy-relu[conv3x3_c64_kernel]", "narrow-32-96[conv1x1_narrow_fwd_kernel<1,96>]",
                                      "wide-1024-g2-lazy[wide_all_kernel]", "gemm-k40-lazy-relu[conv_gemm_kernel<64,0,reg>]")]


@pytest.mark.parametrize("where", ["input", "vectors"])
@pytest.mark.parametrize("row", NAN_FWD, ids=[r[0] for r in NAN_FWD])
def test_conv_fwd_propagates_nan(row, where):
    """A NaN in a lazily read input (one pixel, one channel) or in the BatchNorm scale of one channel of group 0 (two groups): the
    outputs torch makes non-finite are non-finite and the others finite (clamp_act is NaN-propagating: fminf / fmaxf turned the
    NaN into 0 under ReLU, so a poisoned BatchNorm vanished instead of reaching the loss)"""
    rid, N, H, W, Cin, Cout, k, s, p, act, G, pergroup, acc, probes = row
    cp, images = pad8(Cin), N * G
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    d = ConvDesc(images // 2, H, W, cp, OH, OW, Cout, k, k, s, p, 1, act, 0, 2, 4 * cp)
    check_probes(probes, d)
    x = rand_input(images, H, W, cp, Cin, 5)
    vec = lazy_vectors(2, cp, 6, act)
    vec[..., Cin:] = 0
    if where == "input":
        x[0, H // 2, W // 2, 1] = NAN
    else:
        vec[0, 0, 1] = NAN
    vflat = vec.reshape(-1)
    a = R.lazy_operand(x, vflat, vflat[cp:], act, groups=2, gstride=4 * cp, cin_true=Cin)
    w = rand_weight(Cout, Cin, k, 7)
    ref = R.conv_fwd_ref(a, w, s, p)[0]
    # (NaN is what the row expects in y: an unwritten element cannot be told from a propagated one here)
    y = GB.out(ref.shape, BF16, written=False) if where == "input" else GB.inout(torch.zeros(ref.shape, dtype=torch.bfloat16))
    stats = zstats(2, Cout)
    xd, vd = GB.frozen(x), GB.frozen(vflat)
    call("adamml_conv_fwd", byref(d), ptr(xd), ptr(pack(w, cp, 0)), ptr(vd), ptr(vd[cp:]), ptr(y), ptr(stats))
    GB.check(rid)
    finite_pattern_matches(y, ref, "%s NaN %s" % (rid, where))


@pytest.mark.parametrize("act", [0, 1, 2])
def test_bn_act_add_propagates_nan(act):
    P, C = 999, 64
    z = rand_input(1, 1, P, C, C, 8).view(P, C)
    idn = rand_input(1, 1, P, C, C, 9).view(P, C)
    v = lazy_vectors(2, C, 10, act)
    z[17, 5] = NAN
    v[0, 1, 9] = NAN                          # shift of channel 9
    idn[400, 33] = NAN
    zd, idd, vd = GB.frozen(z), GB.frozen(idn), GB.frozen(v)
    out = GB.out((P, C), BF16, written=False)
    call("adamml_bn_act_add", ptr(zd), ptr(vd[0, 0]), ptr(vd[0, 1]), 0, act, ptr(idd), ptr(vd[1, 0]), ptr(vd[1, 1]), 0, ptr(out), P, C, 1)
    zz, ii, vv = z.double(), idn.double(), v.double()
    pre = zz * vv[0, 0] + vv[0, 1] + ii * vv[1, 0] + vv[1, 1]
    ref = {0: pre, 1: F.relu(pre), 2: F.relu6(pre)}[act]
    finite_pattern_matches(out, ref, "bn_act_add act %d" % act)


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("H,W", [(30, 30), (66, 38)])          # OH 15: the per-output kernel, OH 33: the column walker
def test_maxpool_fwd_propagates_nan(H, W, lazy):
    N, C = 2, 64
    x = rand_input(N, H, W, C, C, 11)
    x[0, 7, 9, 3] = NAN
    x[1, H - 1, W - 1, 60] = NAN              # a corner: windows with padding taps
    v = lazy_vectors(1, C, 12, 1)
    if lazy:
        v[0, 0, 20] = NAN                     # every window of channel 20
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = GB.out((N, OH, OW, C), BF16, written=False)
    idx = GB.out((N, OH, OW, C), torch.uint8)
    xd, vd = GB.frozen(x), GB.frozen(v)
    call("adamml_maxpool2d_fwd", ptr(xd), ptr(vd[0, 0]) if lazy else None, ptr(vd[0, 1]) if lazy else None, 0, 1 if lazy else 0, ptr(y),
         ptr(idx), None, N, H, W, C, OH, OW, 1)
    a = R.lazy_operand(x, v[0, 0], v[0, 1], 1) if lazy else x.double()
    ref = R.to_nhwc(F.max_pool2d(R.to_nchw(a), 3, 2, 1))
    finite_pattern_matches(y, ref, "maxpool %dx%d lazy %d" % (H, W, lazy))
    fin = torch.isfinite(ref)
    assert torch.equal(y.cpu().double()[fin], R.bf16(ref[fin])), "finite pooled values"


@pytest.mark.parametrize("T", [8, 5])                           # T = 8: the frame walker, T = 5: the per-output kernel
def test_temporal_max_pool_propagates_nan(T):
    NB, H, W, C = 2, 5, 6, 32
    x = rand_input(NB * T, H, W, C, C, 13)
    x[3, 2, 2, 4] = NAN
    v = lazy_vectors(1, C, 14, 1)
    v[0, 0, 11] = NAN
    To = (T - 1) // 2 + 1
    y = GB.out((NB * To, H, W, C), BF16, written=False)
    xd, vd = GB.frozen(x), GB.frozen(v)
    call("adamml_temporal_pool_fwd", ptr(xd), ptr(vd[0, 0]), ptr(vd[0, 1]), 0, 1, ptr(y), NB, T, H * W * C, C, 0, 1)
    a = R.lazy_operand(x, v[0, 0], v[0, 1], 1).view(NB, T, H, W, C)
    ref = F.max_pool3d(a.permute(0, 4, 1, 2, 3), (3, 1, 1), (2, 1, 1), (1, 0, 0)).permute(0, 2, 3, 4, 1).reshape(NB * To, H, W, C)
    finite_pattern_matches(y, ref, "temporal max pool T %d" % T)


def test_resnet50_nan_pixel_gives_nonfinite_logits():
    """One NaN pixel of a small ResNet-50 input poisons the first BatchNorm's statistics; in train mode torch then returns non-finite
    logits for every sample, and so must the HIP network (the lazy reads used to turn the NaN vectors into zeros and a finite loss)"""
    from adamml_amd import synth
    from adamml_amd.resnet import resnet
    from tests.golden_cases import CASES
    from tests.oracle_harness import manifest, case_inputs
    c = CASES["resnet50_train"]
    sd = synth.synth_state_dict(manifest(c), seed=1234)
    model = resnet(depth=50, num_classes=31, without_t_stride=False, groups=c["groups"], dropout=0.0,
                   pooling_method=c.get("pooling", "max"), input_channels=3, imagenet_pretrained=False)
    model.load_state_dict(sd)
    model.to(DEV).train()
    x, _ = case_inputs(c)
    x = x.clone()
    x.view(-1)[x.numel() // 3] = NAN
    with torch.no_grad():
        y = model(x.to(DEV))
    assert not torch.isfinite(y).any(), "%d of %d logits finite" % (int(torch.isfinite(y).sum()), y.numel())


@pytest.mark.parametrize("T,clips,H,Cin,Cout,G,lazy,slice_mode", [(8, 3, 56, 64, 256, 2, True, "0"), (8, 3, 56, 64, 256, 2, True, "2"),
                                                                   (4, 5, 28, 128, 512, 3, True, "1"), (8, 2, 13, 64, 128, 1, False, "0")])
def test_fused_temporal_max_pool_propagates_nan(T, clips, H, Cin, Cout, G, lazy, slice_mode, monkeypatch):
    """adamml_conv_fwd_bn_add_tpool (conv3 + bn3 + identity + ReLU + temporal max-pool in one kernel: the round-5 streaming kernel, the
    wave-slice streaming kernel and the tile kernel, by shape and ADAMML_FADD_TPOOL_SLICE) against adamml_conv_fwd_bn_add followed by
    adamml_temporal_pool_fwd, with NaN identity values in taps 1 and 2 of windows whose tap 0 is finite: the same outputs non-finite, the
    finite ones bit-identical"""
    from adamml_amd.runtime import ACT_RELU
    monkeypatch.setenv("ADAMML_FADD_TPOOL_SLICE", slice_mode)
    N, Q, To = clips * T, H * H, T // 2
    x = GB.frozen(rand_input(G * N, H, H, Cin, Cin, 21, scale=1.5))
    xvec = GB.frozen(lazy_vectors(G, Cin, 22, 1))
    wp = pack(rand_weight(Cout, Cin, 1, 23), Cin, 0)
    d = ConvDesc(N, H, H, Cin, H, H, Cout, 1, 1, 1, 0, 1, ACT_RELU if lazy else 0, 0, G, 4 * Cin if lazy else 0)
    assert hip.load().adamml_conv_fwd_bn_add_tpool_supported(byref(d), T, ACT_RELU, 1 if lazy else 0)
    vec = GB.frozen(torch.rand(G, 4, Cout, generator=gen(24)) * 0.5 + 0.25)
    idn = torch.relu(torch.randn(G * N, H, H, Cout, generator=gen(25))).to(torch.bfloat16)
    idn[2, 3, 4, 5] = NAN                       # clip 0, frame 2: tap 1 of window 1
    idn[T + 5, H - 1, H - 1, Cout - 1] = NAN     # clip 1, frame 5: tap 2 of window 2 (and tap 0 of window 3)
    idn = GB.frozen(idn)
    sc, sh = (ptr(xvec[0, 0]), ptr(xvec[0, 1])) if lazy else (None, None)
    full = GB.out((G * N, H, H, Cout), BF16, written=False)
    call("adamml_conv_fwd_bn_add", byref(d), ptr(x), ptr(wp), sc, sh, ptr(vec), ptr(idn), None, None, 0, ACT_RELU, ptr(full), None)
    GB.check("conv_fwd_bn_add")
    full = GB.frozen(full)                                               # (from here on an operand)
    ref = GB.out((G * clips * To, H, H, Cout), BF16, written=False)
    call("adamml_temporal_pool_fwd", ptr(full), None, None, 0, 0, ptr(ref), clips, T, Q * Cout, Cout, 0, G)
    GB.check("temporal_pool_fwd")
    pooled = GB.inout(torch.zeros(ref.shape, dtype=torch.bfloat16))
    code = GB.out((G * clips * To, H, H, Cout // 8), torch.int16)
    call("adamml_conv_fwd_bn_add_tpool", byref(d), ptr(x), ptr(wp), sc, sh, ptr(vec), ptr(idn), None, None, 0, ACT_RELU, T, ptr(pooled),
         ptr(code))
    GB.check("conv_fwd_bn_add_tpool (slice %s)" % slice_mode)
    r = ref.cpu().double()
    finite_pattern_matches(pooled, r, "fused temporal max-pool (slice %s)" % slice_mode)
    fin = torch.isfinite(r)
    assert int((~fin).sum()) == 3 and torch.equal(pooled.cpu().double()[fin], r[fin])
