"""adamml_conv_bwd_data_res on 3x3 / pad 1 / stride 1 convs with Cin == Cout (conv1 of a BasicBlock without a downsample branch), through
the C ABI, against a float64 host reference and against the unfused pair it replaces.

Every device buffer comes from tests/guarded.py (guard bands checked after each launch and at the end of each test, operands frozen).
Reference: the full 3x3 transposed conv of dz in float64 (tests/conv_ref.conv_dgrad_ref), plus the identity-path gradient when
accumulating, times the mask; the error model is the one tests/fused_ref.dgrad_epi_ref states for the 1x1 form with n = 9 * Cout products
per output in place of Cout (the same expressions over tests/conv_ref's constants; no constant of its own).  The per-channel sums are
checked by tests/fused_ref.res_sums_check against float64 sums of the STORED g'.

Shapes: the smallest at which this kernel can go wrong.  7 x 7: every pixel tile touches all four borders and 49 pixels are no tile
multiple; 9: odd; 14; one and two images per group, one and two groups; 512 channels at 7 x 7 with one image (the channel loop: 8 cout
tiles, 72 K steps).  Channel counts 64 / 128 / 512 at these sizes run the 64-wide cout tile; one row is large enough (512 workgroups of
128 x 128) for the 128-wide instance that the training shapes take.

Two kernels serve these launches, and adamml_conv_bwd_data_res_streams says which (every row asserts it): the tile kernel of
csrc/conv_gemm.hip, and for 64 channels, W >= 8 and no second BatchNorm operand the resident-weight kernel of csrc/conv3x3_c64.hip
(answer 2).  Rows of its own: every (accumulate, mask form, z_a) at 8 x 8 -- the narrowest width it takes -- and 12 x 12; 9 and 14 from
the common table; 24 x 24, where a strip is 20 rows and the last strip of an image is ragged (4 rows); and 1026 images of 8 x 8 in two
groups: two strips per workgroup, so the prefetch of the next strip runs, and workgroup 256 crosses the group boundary and publishes the
first group's sums mid-way.  64 channels at 7 x 7, or with a second BatchNorm operand, stay with the tile kernel."""
import math

import pytest
import torch
from ctypes import byref

from tests import conv_ref as R
from tests import elementwise_ref as E
from tests import fused_ref as F

pytestmark = pytest.mark.gpu

from adamml_amd import hip  # noqa: E402
from adamml_amd.hip import ConvDesc, call, ptr  # noqa: E402
from tests.test_conv_conformance_gpu import GB, guard, pack, ssum, zstats, rand_weight, finite_pattern_matches  # noqa: E402,F401  (guard: the autouse check)

NAN = float("nan")
RELU = 1


def lib():
    return hip.load()


def desc(N, H, C, G, k=3, stride=1, pad=1, cout=None):
    OH = (H + 2 * pad - k) // stride + 1
    return ConvDesc(N, H, H, C, OH, OH, cout or C, k, k, stride, pad, 1, 0, 0, G, 0)


def row_id(r):
    return "C%d-H%d-N%d-G%d-%s-%s%s%s" % (r["C"], r["H"], r["N"], r["G"], "acc" if r["acc"] else "noacc", r["form"],
                                           "-za" if r["za"] else "-noza", "-zb" if r["zb"] else "")


def _row(C, H, N, G, acc, form, za, zb):
    return dict(C=C, H=H, N=N, G=G, acc=acc, form=form, za=za, zb=zb)


def _rows():
    rows = []
    # every combination of (accumulate, mask form, z_a, second BatchNorm operand) at one shape of each narrow channel count
    for C, H in ((64, 9), (128, 7)):
        for acc in (0, 1):
            for form in ("out", "bits"):
                for za in (True, False):
                    for zb in (False, True):
                        rows.append(_row(C, H, 2, 2, acc, form, za, zb))
    # every (groups, images per group, size) of the table, the epilogue forms taking turns
    forms = [(1, "bits", True, False), (0, "out", True, True), (1, "out", False, False), (0, "bits", False, True)]
    i = 0
    for C, sizes in ((64, (7, 8, 9, 12, 14)), (128, (7, 9, 14))):
        for H in sizes:
            for G in (1, 2):
                for N in (1, 2):
                    rows.append(_row(C, H, N, G, *forms[i % 4]))
                    i += 1
    # the 64-channel kernel: every form it takes at its narrowest width and at 12; a ragged last strip
    for H in (8, 12):
        for acc in (0, 1):
            for form in ("out", "bits"):
                for za in (True, False):
                    rows.append(_row(64, H, 2, 2, acc, form, za, False))
    rows.append(_row(64, 24, 1, 2, 1, "bits", True, False))
    rows.append(_row(64, 24, 2, 1, 0, "out", False, False))
    rows.append(_row(512, 7, 1, 1, 1, "bits", True, False))
    rows.append(_row(512, 7, 1, 2, 0, "out", True, True))
    seen, out = set(), []
    for r in rows:
        if row_id(r) not in seen:
            seen.add(row_id(r))
            out.append(r)
    return out


ROWS = _rows()
# the 128-wide cout tile: ceil(P / 128) * ceil(C / 128) * G >= 512 workgroups (csrc/conv_gemm.hip conv_launch), 128 channels at 64 x 64
WIDE = _row(128, 64, 8, 2, 1, "bits", True, True)
# the 64-channel kernel with two strips per workgroup (more than 1024 strips) and a group boundary inside a workgroup
C64_MANY = _row(64, 8, 513, 2, 1, "bits", True, False)


def served_by(r):
    """what adamml_conv_bwd_data_res_streams answers for the shape, and whether THIS launch goes to the 64-channel kernel"""
    probe = 2 if r["C"] == 64 and r["H"] >= 8 else 0
    return probe, probe == 2 and not r["zb"]


def operands(r):
    C, H, N, G = r["C"], r["H"], r["N"], r["G"]
    n = G * N
    s = F.seed_of(row_id(r))
    op = {"dz": E.rand_bf16(n, H, H, C, scale=0.5, seed=s), "w": rand_weight(C, C, 3, s + 1)}
    op["dx_in"] = E.rand_bf16(n, H, H, C, seed=s + 2) if r["acc"] else None
    op["res_out"] = E.rand_bf16(n, H, H, C, scale=3.0, offset=1.0, seed=s + 3).float().clamp_min(0).to(torch.bfloat16)    # exact 0 occurs
    op["m"] = E.act_mask(op["res_out"].double(), RELU)
    op["bits"] = F.pack_bits(op["m"].bool())
    op["za"], op["va"] = E.rand_bf16(n, H, H, C, seed=s + 4), E.bn_vectors(G, C, s + 5)
    op["zb"], op["vb"] = E.rand_bf16(n, H, H, C, seed=s + 6), E.bn_vectors(G, C, s + 7)
    return op


def reference(r, op, m=None):
    """-> (ref, ab, n, extra) NHWC float64: tests/fused_ref.dgrad_epi_ref with the 3x3 transposed conv in place of dz @ w"""
    conv, ab, n = R.conv_dgrad_ref(op["dz"].double(), op["w"], (r["H"], r["H"]), 1, 1)
    assert n == 9 * r["C"]
    ref, extra = conv, None
    if op["dx_in"] is not None:
        b = op["dx_in"].double()
        ref = conv + b
        extra = R.RHO_BF16 * (conv.abs() + R.C_ACC * math.sqrt(n) * R.U32 * ab) + R.U32 * (conv.abs() + b.abs())
    m = op["m"] if m is None else m
    return ref * m, ab * m, n, None if extra is None else extra * m


def launch(r, op, keep=None, wp=None):
    """-> (dx, sums_a [G, 2C], sums_b [G, 2C]) on the device, guard bands checked"""
    C, H, N, G = r["C"], r["H"], r["N"], r["G"]
    d = desc(N, H, C, G)
    assert lib().adamml_conv_bwd_data_res_supported(byref(d)) == 1
    assert lib().adamml_conv_bwd_data_res_streams(byref(d)) == served_by(r)[0]
    keep = keep or {k: GB.frozen(v) for k, v in op.items() if torch.is_tensor(v) and k not in ("dx_in", "m", "w")}
    wp = wp if wp is not None else pack(op["w"], C, 1)
    dx = GB.inout(op["dx_in"]) if r["acc"] else GB.out((G * N, H, H, C), torch.bfloat16)
    sa, sb = zstats(G, C), zstats(G, C)
    bits = r["form"] == "bits"
    call("adamml_conv_bwd_data_res", byref(d), ptr(keep["dz"]), ptr(wp), ptr(dx), r["acc"], ptr(keep["res_out"]), ptr(keep["bits"]) if bits else None,
         RELU, ptr(keep["za"]) if r["za"] else None, ptr(keep["va"]), ptr(sa), ptr(keep["zb"]) if r["zb"] else None,
         ptr(keep["vb"]) if r["zb"] else None, ptr(sb) if r["zb"] else None)
    return dx, sa, sb, keep, wp


def check_row(r):
    C, G = r["C"], r["G"]
    op = operands(r)
    dx, sa, sb, _, _ = launch(r, op)
    GB.check(row_id(r))
    h = dx.cpu()
    ref, ab, n, extra = reference(r, op)
    assert (op["m"] == 1).any() and (op["m"] == 0).any()
    q = R.check(h, ref, ab, n, extra=extra, what=row_id(r), bias=ref.numel() >= R.BIAS_MIN_ELEMENTS and extra is None)
    hs = h.reshape(-1, C)
    F.res_sums_check(ssum(sa).cpu(), hs, op["za"].reshape(-1, C) if r["za"] else None, op["va"], G, row_id(r) + " sums_a")
    if r["zb"]:
        F.res_sums_check(ssum(sb).cpu(), hs, op["zb"].reshape(-1, C), op["vb"], G, row_id(r) + " sums_b")
    else:
        assert (ssum(sb).cpu() == 0).all()
    print("  %-44s max err/tol %.4f" % (row_id(r), q))


@pytest.mark.parametrize("r", ROWS, ids=[row_id(r) for r in ROWS])
def test_conv3x3_bwd_data_res_against_float64(r):
    check_row(r)


def test_conv3x3_bwd_data_res_wide_tile_against_float64():
    check_row(WIDE)


def test_conv3x3_bwd_data_res_c64_many_strips_against_float64():
    assert served_by(C64_MANY)[1]
    check_row(C64_MANY)


def test_rows_reach_both_kernels():
    c64 = [r for r in ROWS if served_by(r)[1]]
    assert {r["H"] for r in c64} >= {8, 9, 12, 14, 24}
    for H in (8, 12):
        assert {(r["acc"], r["form"], r["za"]) for r in c64 if r["H"] == H} == {(a, f, z) for a in (0, 1) for f in ("out", "bits") for z in (True, False)}
    tile = [r for r in ROWS if not served_by(r)[1]]
    assert {r["C"] for r in tile} == {64, 128, 512} and any(r["C"] == 64 and r["zb"] and r["H"] >= 8 for r in tile)


EQ_ROWS = [_row(64, 9, 2, 2, 1, "out", True, False), _row(64, 12, 2, 2, 0, "out", True, False), _row(64, 7, 2, 2, 1, "out", True, False),
           _row(128, 14, 2, 1, 1, "out", True, True), _row(128, 7, 1, 2, 0, "out", True, True),
           _row(512, 7, 1, 1, 1, "out", True, False)]


@pytest.mark.parametrize("r", EQ_ROWS, ids=[row_id(r) for r in EQ_ROWS])
def test_conv3x3_bwd_data_res_equals_dgrad_then_residual_bwd(r):
    """Against adamml_conv_bwd_data(accumulate) + adamml_residual_bwd, with the assertions and constants of
    tests/test_kernels_gpu.py test_conv_bwd_data_res_equals_dgrad_then_residual_bwd: the fused form rounds the block-output gradient once
    instead of twice (1 bf16 ulp of slack on g', i.e. 1.6e-2 of the scale), sums 2e-3 against the stored values and 2e-2 against the
    pair's; the 1-bit mask form is bit-identical to the res_out form."""
    C, H, N, G = r["C"], r["H"], r["N"], r["G"]
    P = N * H * H
    op = operands(r)
    acc, second = r["acc"], r["zb"]
    d = desc(N, H, C, G)
    dx, sa, sb, keep, wp = launch(r, op)
    # the unfused pair on the device
    dx_ref = GB.inout(op["dx_in"]) if acc else GB.out((G * N, H, H, C), torch.bfloat16)
    call("adamml_conv_bwd_data", byref(d), ptr(keep["dz"]), ptr(wp), ptr(dx_ref), acc)
    g2 = GB.out((G * N, H, H, C), torch.bfloat16)
    sa_ref, sb_ref = zstats(G, C), zstats(G, C)
    call("adamml_residual_bwd", ptr(dx_ref), ptr(keep["res_out"]), RELU, ptr(g2), ptr(keep["za"]), ptr(keep["va"]), ptr(sa_ref),
         ptr(keep["zb"]) if second else None, ptr(keep["vb"]) if second else None, ptr(sb_ref) if second else None, P, C, G)
    GB.check(row_id(r))
    full = reference(r, op)[0].float()
    scale = full.abs().max().item()
    assert (dx.cpu().float() - full).abs().max().item() <= 1e-2 * scale
    assert (dx.float() - g2.float()).abs().max().item() <= 1.6e-2 * scale      # double vs single rounding
    gq = dx.float().view(G, P, C).double()
    for s_got, s_ref, z, vec in ((sa, sa_ref, keep["za"], keep["va"]),) + (((sb, sb_ref, keep["zb"], keep["vb"]),) if second else ()):
        got = ssum(s_got)
        zhat = (z.float().view(G, P, C) - vec[:, 2].view(G, 1, C)) * vec[:, 3].view(G, 1, C)
        exp = torch.cat([gq.sum(1), (gq * zhat.double()).sum(1)], dim=1)        # from the values the kernel stored
        tol = 2e-3 * exp.abs().max().item() + 1e-3
        assert (got - exp).abs().max().item() <= tol
        assert (got - ssum(s_ref)).abs().max().item() <= 2e-2 * ssum(s_ref).abs().max().item() + 1e-2
    if not second:
        assert ssum(sb).abs().max().item() == 0.0
    dx_m, sa_m, sb_m, _, _ = launch(dict(r, form="bits"), op, keep, wp)
    GB.check(row_id(r) + " bits")
    assert torch.equal(dx_m, dx)
    assert torch.equal(ssum(sa_m), ssum(sa)) and torch.equal(ssum(sb_m), ssum(sb))     # (per-channel totals: the slot a workgroup publishes into is free)


NAN_ROWS = [_row(64, 9, 2, 2, 1, "out", True, False), _row(64, 8, 2, 1, 1, "bits", True, False), _row(128, 7, 2, 1, 1, "bits", True, True)]


@pytest.mark.parametrize("r", NAN_ROWS, ids=[row_id(r) for r in NAN_ROWS])
def test_conv3x3_bwd_data_res_selects_under_a_closed_mask(r):
    """NaN in dz (all channels of one pixel: it reaches the 3 x 3 neighbourhood, every channel) and inf / NaN in the identity-path
    gradient under CLOSED mask bits: +0 there, non-finite exactly where the mask passes the gradient."""
    C, H = r["C"], r["H"]
    op = operands(r)
    op["dz"][1, H // 2, H // 2, :] = NAN
    closed = (op["m"][0] == 0).nonzero()
    assert len(closed) >= 2
    (h0, w0, c0), (h1, w1, c1) = closed[0].tolist(), closed[-1].tolist()
    op["dx_in"][0, h0, w0, c0] = float("inf")
    op["dx_in"][0, h1, w1, c1] = NAN
    dx, _, _, _, _ = launch(r, op)
    GB.unwritten_ok(dx)
    GB.check(row_id(r))
    h = dx.cpu()
    ones = torch.ones_like(op["m"])
    ref = reference(r, op, ones)[0]
    ref = torch.where(op["m"] > 0, ref, torch.zeros_like(ref))
    finite_pattern_matches(h, ref, row_id(r) + " NaN")
    under = op["m"] == 0
    hv = h[under].view(torch.int16)
    assert (hv == 0).all(), "a closed mask bit must give +0, whatever the gradient holds"


@pytest.mark.parametrize("r", [_row(128, 14, 2, 2, 1, "bits", True, True), _row(64, 24, 2, 2, 1, "bits", True, False)], ids=row_id)
def test_conv3x3_bwd_data_res_is_deterministic(r):
    op = operands(r)
    dx0, sa0, sb0, keep, wp = launch(r, op)
    dx1, sa1, sb1, _, _ = launch(r, op, keep, wp)
    GB.check(row_id(r))
    assert torch.equal(dx0, dx1) and torch.equal(ssum(sa0), ssum(sa1)) and torch.equal(ssum(sb0), ssum(sb1))


def test_probes():
    sup = lib().adamml_conv_bwd_data_res_supported
    for C, H in ((64, 56), (128, 28), (256, 14), (512, 7), (64, 7), (128, 9)):
        assert sup(byref(desc(2, H, C, 1))) == 1, (C, H)
        # 2: the 64-channel kernel (W >= 8) serves launches without a second BatchNorm operand; 0: the tile kernel serves them all
        assert lib().adamml_conv_bwd_data_res_streams(byref(desc(2, H, C, 1))) == (2 if C == 64 and H >= 8 else 0)
        assert lib().adamml_conv_bwd_data_res_prod_supported(byref(desc(2, H, C, 1)), 64) == 0          # the product form stays 1x1
        assert lib().adamml_conv_bwd_data_res_prod_streams(byref(desc(2, H, C, 1)), 64) == 0
    assert sup(byref(desc(2, 14, 128, 1, stride=2))) == 0                       # stride 2
    assert sup(byref(desc(2, 14, 128, 1, pad=0))) == 0                          # pad 0
    assert sup(byref(desc(2, 14, 64, 1, cout=128))) == 0 and sup(byref(desc(2, 14, 128, 1, cout=64))) == 0     # Cin != Cout
    assert sup(byref(desc(2, 14, 96, 1))) == 0                                  # not a power of two (the KxK loaders)
    # the 1x1 shapes the header documents
    for cin, cout in ((256, 64), (512, 128), (24, 144), (2048, 512)):
        assert sup(byref(ConvDesc(2, 14, 14, cin, 14, 14, cout, 1, 1, 1, 0, 1, 0, 0, 1, 0))) == 1
    assert sup(byref(ConvDesc(2, 14, 14, 256, 7, 7, 64, 1, 1, 2, 0, 1, 0, 0, 1, 0))) == 0
    # an unsupported 3x3 is refused without a write
    r = _row(128, 8, 1, 1, 0, "out", True, False)
    op = operands(r)
    d = desc(1, 8, 128, 1, pad=0)
    dx = GB.out((1, 8, 8, 128), torch.bfloat16)
    sa = zstats(1, 128)
    wp = pack(op["w"], 128, 1)
    dz, ro, za, va = (GB.frozen(op[k]) for k in ("dz", "res_out", "za", "va"))
    with pytest.raises(RuntimeError):
        call("adamml_conv_bwd_data_res", byref(d), ptr(dz), ptr(wp), ptr(dx), 0, ptr(ro), None, RELU, ptr(za), ptr(va), ptr(sa), None, None, None)
    GB.unwritten_ok(dx)
    assert GB.untouched(dx) and GB.untouched(sa)
