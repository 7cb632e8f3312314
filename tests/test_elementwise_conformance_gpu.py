"""Conformance of the BatchNorm, pooling, depthwise and stem kernels against float64 references (tests/elementwise_ref.py).

One row per kernel instance the entry points of csrc/bn.hip and csrc/pool.hip (BatchNorm / residual / pooling launchers), csrc/dwconv_gemm32.hip,
csrc/dwconv_bwd_fused.hip and csrc/conv_stem.hip can launch; the row id names the entry point and the case, and
profiles/elementwise_conformance_rows.md lists the kernel instance each row launched.  Operands are generated on the CPU from seeded
generators (the three large rows generate on the device: 0.3 - 0.6 GB per tensor), outputs are pre-filled with NaN (or a base tensor where
the entry point accumulates) so that an element a kernel never writes fails, every call goes through the C ABI with hip.call, and where
the library exports a probe the row asserts it.  Every buffer handed to a kernel comes from tests/guarded.py: outputs, accumulators and
workspaces inside sentinel bands, read-only operands compared bit for bit, both checked at the end of every row (and after each launch
where a row launches the same entry point twice); the weight-gradient rows run on a workspace of exactly the size their query answers,
again on a workspace that held other bytes, and with workspace_bytes one float short.  Tolerances are those derived in
tests/elementwise_ref.py; none is fitted to an observed error.  The module prints its WORST table (row id -> largest err / tol) at the end: pytest -s.

Environment switches read once per process: ADAMML_DWB_SEGW (pixels per thread of dwconv_bwd_fused_kernel<1, SEGW>; default 3) and
ADAMML_DW_S2_QUADS (0: the stride-2 data gradient through the per-pixel dwconv_bwd_data_kernel instead of the quad kernel) -- the rows run
the defaults in this process, and SEGW = 2 / QUADS = 0 in one fresh child process (test_switch_only_instances_child: rows
`dwconv_bwd_fused[segw2-..]` and `dwconv_bwd_data[quads0-..]`)."""
import math
import os
import subprocess
import sys
import time

import pytest
import torch
from ctypes import byref

from tests import conv_ref as R
from tests import elementwise_ref as E

pytestmark = pytest.mark.gpu

from adamml_amd import hip  # noqa: E402
from adamml_amd.hip import ConvDesc, call, ptr, STAT_SLOTS  # noqa: E402
from tests.guarded import workspace_launches  # noqa: E402
from tests.test_conv_conformance_gpu import DEV, GB, guard, pack, ssum, zstats  # noqa: E402,F401  (guard: the autouse check of every row)

T0 = time.time()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}          # row id -> max err / tol (exact rows record 0)
NOTES = {}          # row id -> a measured figure worth reporting


def record(rid, r):
    WORST[rid] = max(WORST.get(rid, 0.0), r)


def print_table():
    if WORST:
        k = max(WORST, key=WORST.get)
        print("\nelementwise conformance: largest err/tol %.4f (%s) over %d rows, %.0f s" % (WORST[k], k, len(WORST), time.time() - T0))
        for rid in sorted(WORST):
            print("  %-72s %.4f%s" % (rid, WORST[rid], ("   " + NOTES[rid]) if rid in NOTES else ""))


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print_table()


def nan_bf16(*shape):
    return GB.out(shape, torch.bfloat16)


def nan_f32(*shape):
    return GB.out(shape, torch.float32)


def zsums(G, C):
    return zstats(G, C)


def seed_of(rid):
    return sum(map(ord, rid)) % 10007


def group_args(vec, pergroup):
    """(device vector, scale ptr, shift ptr, gstride) of a [G or 1][4][C] vector tensor"""
    C = vec.shape[-1]
    vd = GB.frozen(vec.reshape(-1))
    return vd, ptr(vd), ptr(vd[C:]), (4 * C if pergroup else 0)


# ------------------------------------------------------------------------------------------------------------------------ bn_act_add
# (id, act, identity (None / "plain" / "lazy"), mask, G, per-group vectors, z scale given, C, P)
ACT_ADD = [
    ("act0-noidn-G1", 0, None, False, 1, False, True, 64, 1000),
    ("act1-plainidn-mask-G3-pergroup", 1, "plain", True, 3, True, True, 64, 700),
    ("act2-lazyidn-mask-G3-pergroup", 2, "lazy", True, 3, True, True, 64, 700),
    ("act1-lazyidn-G1-shared", 1, "lazy", False, 1, False, True, 256, 333),
    ("act2-noidn-mask-G1", 2, None, True, 1, False, True, 64, 1000),
    ("act1-noscale-plainidn-G1", 1, "plain", False, 1, False, False, 64, 500),
    ("act2-lazyidn-mask-C24-P777-G2", 2, "lazy", True, 2, True, True, 24, 777),
    ("act1-plainidn-mask-C2048-P98", 1, "plain", True, 1, False, True, 2048, 98),
    ("act2-lazyidn-mask-C8-P4099-3wg-ragged", 2, "lazy", True, 1, False, True, 8, 4099),
]


@pytest.mark.parametrize("row", ACT_ADD, ids=[r[0] for r in ACT_ADD])
def test_bn_act_add(row):
    name, act, idk, mask, G, pergroup, zscale, C, P = row
    rid, seed = "bn_act_add%s[%s]" % ("_mask" if mask else "", name), seed_of(name)
    z = E.act_data(G * P, C, act, seed)
    vz = E.bn_vectors(G if pergroup else 1, C, seed + 1, act)
    idn = vi = None
    if idk:
        idn = E.rand_bf16(G * P, C, seed=seed + 2)
        idn[:, 0] = 0                                               # the planted bounds of channel 0 stay on the bounds
        if idk == "lazy":
            vi = E.bn_vectors(G if pergroup else 1, C, seed + 3, act)
            vi[:, 1, 0] = 0.0
    gs = 4 * C if pergroup else 0
    vzf = vz.reshape(-1)
    vif = vi.reshape(-1) if vi is not None else None
    ref, ab, k = E.bn_act_add_ref(z, vzf if zscale else None, vzf[C:] if zscale else None, gs, act, idn,
                                  vif, vif[C:] if vif is not None else None, gs, groups=G)
    zd, idd = GB.frozen(z), GB.frozen(idn) if idn is not None else None
    vzd, zs, zt, _ = group_args(vz, pergroup)
    vid, is_, it = None, None, None
    if vi is not None:
        vid, is_, it, _ = group_args(vi, pergroup)
    out = nan_bf16(G * P, C)
    bits = GB.inout(torch.full((G * P * C // 8,), 0xAA, dtype=torch.uint8))
    args = (ptr(zd), zs if zscale else None, zt if zscale else None, gs, act, ptr(idd), is_, it, gs, ptr(out))
    if mask:
        call("adamml_bn_act_add_mask", *args, ptr(bits), P, C, G)
    else:
        call("adamml_bn_act_add", *args, P, C, G)
    h = out.cpu()
    record(rid, E.point_check(h, ref, ab, k, what=rid))
    if act:
        lo, hi = R.ACT_BOUNDS[act]
        assert (h[:, 0] == lo).any() and (act != 2 or (h[:, 0] == hi).any()), rid + ": planted bounds missing"
    if mask:
        want = E.mask_bits_ref(h, act)
        assert torch.equal(bits.cpu(), want), rid + ": mask bits"
        assert act == 0 or ((want != 0xFF).any() and (want != 0).any())


def test_act_bwd_from_output():
    rid = "act_bwd_from_output[P777-C24-act2]"
    P, C = 777, 24
    out = E.rand_bf16(P, C, scale=3.0, offset=1.0, seed=5).float().clamp(0, 6).to(torch.bfloat16)
    g = E.rand_bf16(P, C, seed=6)
    assert (out == 0).any() and (out == 6).any()
    od, gd, g2 = GB.frozen(out), GB.frozen(g), nan_bf16(P, C)
    call("adamml_act_bwd_from_output", ptr(gd), ptr(od), 2, ptr(g2), P * C)
    assert torch.equal(g2.cpu().double(), E.act_bwd_ref(g, out, 2)), rid
    record(rid, 0.0)


# ------------------------------------------------------------------------------------------------------------- row walkers at their edges
def walk_pixels(C, kind):
    rows = max(256 // (C // 8), 1)
    return {"P1": 1, "rows-1": max(rows - 1, 2), "rows+1": rows + 1, "multi-wg-ragged": 50 * rows + 3}[kind]


@pytest.mark.parametrize("G", [1, 5])
@pytest.mark.parametrize("kind", ["P1", "rows-1", "rows+1", "multi-wg-ragged"])
@pytest.mark.parametrize("C", [8, 24, 64, 2048])
def test_row_walk_edges(C, kind, G):
    """bn_bwd_reduce, residual_bwd (a only, a and b, neither; in place with ACT_NONE) and bn_bwd_apply at the edges of ChanMap /
    block_channel_publish: C = 8 (256 row slots) and C = 2048 (one) use exactly 2 * MAXC floats of LDS, C = 24 leaves a thread idle;
    P = 1, one less and one more than the row slots, and a multi-workgroup count with a ragged tail."""
    P, act = walk_pixels(C, kind), 2
    tag = "C%d-%s(P%d)-G%d" % (C, kind, P, G)
    seed = seed_of(tag)
    z, g = E.act_data(G * P, C, act, seed), E.rand_bf16(G * P, C, seed=seed + 1)
    vec = E.bn_vectors(G, C, seed + 2, act)
    zd, gd, vd = GB.frozen(z), GB.frozen(g), GB.frozen(vec)
    # bn_bwd_reduce
    gp = g.double() * R.bn_mask(z, vec, act, groups=G)
    sref, sab = R.bn_dgrad_sums_ref(gp, z, vec, groups=G)
    sums = zsums(G, C)
    call("adamml_bn_bwd_reduce", ptr(gd), ptr(zd), ptr(vd), act, ptr(sums), P, C, G)
    record("bn_bwd_reduce[%s]" % tag, E.sums_check(ssum(sums).cpu(), sref, sab, P, what="bn_bwd_reduce " + tag))
    # bn_bwd_apply
    coef = torch.stack([vec[:, 3] * 1.3, torch.randn(G, C, generator=E.gen(seed + 3)) * 0.1, torch.randn(G, C, generator=E.gen(seed + 4)) * 0.2], 1)
    ref, ab = E.bn_bwd_apply_ref(gp, z, vec, coef, groups=G)
    dz, cd = nan_bf16(G * P, C), GB.frozen(coef.contiguous())
    call("adamml_bn_bwd_apply", ptr(gd), ptr(zd), ptr(vd), act, ptr(cd), ptr(dz), P, C, G)
    record("bn_bwd_apply[%s]" % tag, E.point_check(dz.cpu(), ref, ab, E.K_BN_BWD_APPLY, what="bn_bwd_apply " + tag))
    # residual_bwd
    out = E.rand_bf16(G * P, C, scale=3.0, offset=1.0, seed=seed + 5).float().clamp(0, 6).to(torch.bfloat16)
    zb, vecb = E.rand_bf16(G * P, C, seed=seed + 6), E.bn_vectors(G, C, seed + 7)
    od, zbd, vbd = GB.frozen(out), GB.frozen(zb), GB.frozen(vecb)
    g2ref = E.act_bwd_ref(g, out, act)
    for mode in ("a", "ab", "none"):
        g2, sa, sb = nan_bf16(G * P, C), zsums(G, C), zsums(G, C)
        call("adamml_residual_bwd", ptr(gd), ptr(od), act, ptr(g2), ptr(zd) if mode != "none" else None, ptr(vd) if mode != "none" else None,
             ptr(sa) if mode != "none" else None, ptr(zbd) if mode == "ab" else None, ptr(vbd) if mode == "ab" else None,
             ptr(sb) if mode == "ab" else None, P, C, G)
        GB.check("residual_bwd %s %s" % (mode, tag))
        assert torch.equal(g2.cpu().double(), g2ref), "residual_bwd %s %s: g2" % (mode, tag)
        r = 0.0
        if mode != "none":
            ra, aa = R.bn_dgrad_sums_ref(g2ref, z, vec, groups=G)
            r = E.sums_check(ssum(sa).cpu(), ra, aa, P, what="residual_bwd a " + tag)
        if mode == "ab":
            rb_, ab_ = R.bn_dgrad_sums_ref(g2ref, zb, vecb, groups=G)
            r = max(r, E.sums_check(ssum(sb).cpu(), rb_, ab_, P, what="residual_bwd b " + tag))
        record("residual_bwd[%s-%s]" % (mode, tag), r)
    # ACT_NONE in place (g2 == g_out: the store is skipped, the sums still come from g_out)
    gin, sa = GB.inout(g), zsums(G, C)
    call("adamml_residual_bwd", ptr(gin), ptr(od), 0, ptr(gin), ptr(zd), ptr(vd), ptr(sa), None, None, None, P, C, G)
    assert torch.equal(gin.cpu(), g)
    ra, aa = R.bn_dgrad_sums_ref(g.double(), z, vec, groups=G)
    record("residual_bwd[inplace-act0-%s]" % tag, E.sums_check(ssum(sa).cpu(), ra, aa, P, what="residual_bwd in place " + tag))


# ------------------------------------------------------------------------------------------------- finalize kernels (per-channel vectors)
def finalize_stats(G, C, count, seed):
    g = E.gen(seed)
    mean = torch.randn(G, C, generator=g, dtype=torch.float64) * (1.0 + torch.arange(G).double().view(G, 1) * 0.05)
    std = torch.rand(G, C, generator=g, dtype=torch.float64) + 0.5
    mean[:, 1] = 30.0 * std[:, 1]                                   # |mean| / std = 30
    return torch.cat([mean * count, (std ** 2 + mean ** 2) * count], 1)


@pytest.mark.parametrize("with_running", [True, False])
@pytest.mark.parametrize("nslots", [1, STAT_SLOTS])
@pytest.mark.parametrize("G", [1, 5, 32, 33, 40])
def test_bn_finalize(G, nslots, with_running):
    C, count = 20, 3137.0                                            # (C = 20: the last block of 8 channels is partly filled)
    rid = "bn_finalize[G%d-nslots%d-%s]" % (G, nslots, "rm" if with_running else "rmNULL")
    s = finalize_stats(G, C, count, seed_of(rid))
    if nslots == STAT_SLOTS:
        s, _ = E.det_decode_host(E.det_encode_host(s))             # the value the bins hold (three float32 pieces)
    g = E.gen(seed_of(rid) + 1)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    ref = E.bn_finalize_ref(s, count, gamma, beta, rm if with_running else None, rv, 0.1, 1e-5)
    sd = GB.frozen(E.stats_to_slots(s, nslots))
    gd, bd, rmd, rvd, vec = GB.frozen(gamma), GB.frozen(beta), GB.inout(rm), GB.inout(rv), nan_f32(G, 4, C)
    call("adamml_bn_finalize", ptr(sd), nslots, G, count, ptr(gd), ptr(bd), ptr(rmd) if with_running else None,
         ptr(rvd) if with_running else None, 0.1, 1e-5, ptr(vec), C)
    r = E.vec_ratio(vec.cpu(), *ref["vec"])
    if with_running:
        r = max(r, E.vec_ratio(rmd.cpu(), *ref["rm"]), E.vec_ratio(rvd.cpu(), *ref["rv"]))
    else:
        assert torch.equal(rmd.cpu(), rm) and torch.equal(rvd.cpu(), rv)
    assert r <= 1.0, "%s: max err/tol %.3g" % (rid, r)
    record(rid, r)
    if nslots == STAT_SLOTS and with_running:
        out = ssum(sd)
        val, ab = E.det_decode_host(sd.cpu().permute(0, 2, 1).contiguous())
        rc = E.vec_ratio(out.cpu(), val, 32 * E.U64 * ab)
        assert rc <= 1.0, "stats_collapse G%d: %.3g" % (G, rc)
        record("stats_collapse[G%d-C20]" % G, rc)


@pytest.mark.parametrize("nslots", [1, STAT_SLOTS])
@pytest.mark.parametrize("G", [1, 5, 32, 33, 40])
def test_bn_bwd_finalize(G, nslots):
    C, count, gs = 20, 3137.0, 0.5
    rid = "bn_bwd_finalize[G%d-nslots%d]" % (G, nslots)
    g = E.gen(seed_of(rid))
    sums = torch.randn(G, 2 * C, generator=g, dtype=torch.float64) * 40 * (1.0 + torch.arange(G).double().view(G, 1) * 0.1)
    if nslots == STAT_SLOTS:
        sums, _ = E.det_decode_host(E.det_encode_host(sums))
    gamma = torch.rand(C, generator=g) + 0.5
    vec = E.bn_vectors(G, C, seed_of(rid) + 1)
    dg0, db0 = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = E.bn_bwd_finalize_ref(sums, count, gamma, vec, dg0, db0, gs)
    sd, gd, vd = GB.frozen(E.stats_to_slots(sums, nslots)), GB.frozen(gamma), GB.frozen(vec)
    dg, db, coef = GB.inout(dg0), GB.inout(db0), nan_f32(G, 3, C)
    call("adamml_bn_bwd_finalize", ptr(sd), nslots, G, count, ptr(gd), ptr(vd), ptr(dg), ptr(db), ptr(coef), C, gs)
    r = max(E.vec_ratio(coef.cpu(), *ref["coef"]), E.vec_ratio(dg.cpu(), *ref["dgamma"]), E.vec_ratio(db.cpu(), *ref["dbeta"]))
    assert r <= 1.0, "%s: max err/tol %.3g" % (rid, r)
    record(rid, r)
    # bn_bwd_affine on the coefficients the kernel wrote, then the one-launch form: bit for bit
    aff = nan_f32(G, 3, C)
    call("adamml_bn_bwd_affine", ptr(coef), ptr(vd), ptr(aff), C, G)
    aref, atol = E.bn_bwd_affine_ref(coef.cpu(), vec)
    ra = E.vec_ratio(aff.cpu(), aref, atol)
    assert ra <= 1.0, "bn_bwd_affine G%d: %.3g" % (G, ra)
    record("bn_bwd_affine[G%d-C20]" % G, ra)
    dg2, db2, coef2, aff2 = GB.inout(dg0), GB.inout(db0), nan_f32(G, 3, C), nan_f32(G, 3, C)
    call("adamml_bn_bwd_finalize_affine", ptr(sd), nslots, G, count, ptr(gd), ptr(vd), ptr(dg2), ptr(db2), ptr(coef2), ptr(aff2), C, gs)
    assert torch.equal(coef2, coef) and torch.equal(aff2, aff) and torch.equal(dg2, dg) and torch.equal(db2, db), rid + ": finalize_affine"
    rf = E.vec_ratio(aff2.cpu(), *ref["aff"])
    assert rf <= 1.0, "bn_bwd_finalize_affine G%d: %.3g" % (G, rf)
    record("bn_bwd_finalize_affine[G%d-nslots%d]" % (G, nslots), rf)
    # dgamma / dbeta == NULL is accepted (a frozen BatchNorm)
    coef3 = nan_f32(G, 3, C)
    call("adamml_bn_bwd_finalize", ptr(sd), nslots, G, count, ptr(gd), ptr(vd), None, None, ptr(coef3), C, gs)
    assert torch.equal(coef3, coef)


def test_bn_eval_affine():
    C = 200
    g = E.gen(77)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) * 2 + 0.01
    (sref, stol), (href, htol) = E.bn_eval_affine_ref(gamma, beta, rm, rv, 1e-5)
    sc, sh = nan_f32(C), nan_f32(C)
    dv = [GB.frozen(t) for t in (gamma, beta, rm, rv)]
    call("adamml_bn_eval_affine", ptr(dv[0]), ptr(dv[1]), ptr(dv[2]), ptr(dv[3]), 1e-5, ptr(sc), ptr(sh), C)
    r = max(E.vec_ratio(sc.cpu(), sref, stol), E.vec_ratio(sh.cpu(), href, htol))
    assert r <= 1.0, "bn_eval_affine: %.3g" % r
    record("bn_eval_affine[C200]", r)


# --------------------------------------------------------------------------------------------------------------------------- maxpool2d
def tied_vectors(G, C, seed, act):
    """bn_vectors whose upper half of the channels sends whole neighbourhoods below 0: windows that tie at relu(..) = 0"""
    v = E.bn_vectors(G, C, seed, act)
    v[:, 1, C // 2:] = -2.5
    return v


# (id, N, H, W, C, G, act (None = plain), z_sel)
MAXPOOL = [
    ("fwd<0>-13x18-plain", 2, 13, 18, 16, 1, None, False),
    ("fwd<1>-13x18-plain-zsel", 2, 13, 18, 16, 1, None, True),
    ("fwd<0>-29x31-relu-G3", 1, 29, 31, 32, 3, 1, False),
    ("fwd<1>-30x28-relu-zsel-G2", 2, 30, 28, 64, 2, 1, True),
    ("walk<1>-33x47-relu-zsel-OH17", 1, 33, 47, 64, 1, 1, True),
    ("walk<0>-66x38-relu6-G2", 1, 66, 38, 32, 2, 2, False),
    ("walk<1>-63x65-plain-zsel", 1, 63, 65, 8, 1, None, True),
    ("walk<0>-40x34-plain", 2, 40, 34, 16, 1, None, False),
]


@pytest.mark.parametrize("row", MAXPOOL, ids=[r[0] for r in MAXPOOL])
def test_maxpool2d(row):
    name, N, H, W, C, G, act, zsel = row
    seed = seed_of(name)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert (OH >= 16) == name.startswith("walk")
    x = E.plant_bounds(E.rand_bf16(G * N, H, W, C, seed=seed))
    vec = tied_vectors(G, C, seed + 1, act) if act is not None else None
    vf = vec.reshape(-1) if vec is not None else None
    yref, iref, zref = E.maxpool2d_fwd_ref(x, vf, vf[C:] if vf is not None else None, 4 * C, act or 0, groups=G)
    if act == 1:
        taps = E._taps2d(E.lazy_f32(x, vf, vf[C:], act, G, 4 * C), OH, OW, -math.inf)
        tied = ((taps == taps.max(0).values) | torch.isinf(taps)).all(0)
        assert tied.double().mean().item() >= 0.01, name + ": fewer than 1 % of the windows fully tied"
    xd = GB.frozen(x)
    vd = GB.frozen(vec).reshape(-1) if vec is not None else None
    y, idx = nan_bf16(G * N, OH, OW, C), GB.inout(torch.full((G * N, OH, OW, C), 0xEE, dtype=torch.uint8))
    zs = nan_bf16(G * N, OH, OW, C) if zsel else None
    call("adamml_maxpool2d_fwd", ptr(xd), ptr(vd), ptr(vd[C:]) if vd is not None else None, 4 * C, act or 0, ptr(y), ptr(idx), ptr(zs),
         N, H, W, C, OH, OW, G)
    GB.check("maxpool2d_fwd " + name)
    idx = GB.frozen(idx)                                                 # (read-only from here on)
    assert torch.equal(y.cpu().double(), yref), name + ": y"
    assert torch.equal(idx.cpu().long(), iref), name + ": idx (first arg-max in torch's window order)"
    if zsel:
        assert torch.equal(zs.cpu().double(), zref), name + ": z_sel"
    record("maxpool2d_fwd[%s]" % name, 0.0)
    # backward from the recorded indices, plain and accumulating
    g = E.rand_bf16(G * N, OH, OW, C, seed=seed + 2)
    gd = GB.frozen(g)
    for acc in (0, 1):
        base = E.rand_bf16(G * N, H, W, C, seed=seed + 3) if acc else None
        gx = GB.inout(base) if acc else nan_bf16(G * N, H, W, C)
        call("adamml_maxpool2d_bwd", ptr(gd), ptr(idx), ptr(gx), G * N, H, W, C, OH, OW, acc)
        GB.check("maxpool2d_bwd acc%d %s" % (acc, name))
        ref, ab = E.maxpool2d_route(g, iref, H, W, base)
        record("maxpool2d_bwd[acc%d-%s]" % (acc, name), E.point_check(gx.cpu(), ref, ab, E.K_MAXPOOL_BWD + acc, what="maxpool2d_bwd " + name))
    if act is None:
        return
    # fused with the BatchNorm backward of the pool's input, against float64 (the routed gradient is rounded to bf16, as the kernel does)
    routed, _ = E.maxpool2d_route(g, iref, H, W)
    gp = R.bf16(routed) * R.bn_mask(x, vec, act, groups=G)
    sref, sab = R.bn_dgrad_sums_ref(gp, x, vec, groups=G)
    sums = zsums(G, C)
    v4 = GB.frozen(vec)
    call("adamml_maxpool2d_bwd_bn_reduce", ptr(gd), ptr(idx), ptr(xd), ptr(v4), act, ptr(sums), N, H, W, C, OH, OW, G)
    record("maxpool2d_bwd_bn_reduce[%s]" % name, E.sums_check(ssum(sums).cpu(), sref, sab, N * H * W, what="maxpool2d_bwd_bn_reduce " + name))
    coef = torch.stack([vec[:, 3] * 1.3, torch.randn(G, C, generator=E.gen(seed + 4)) * 0.1, torch.randn(G, C, generator=E.gen(seed + 5)) * 0.2], 1)
    cd, dz = GB.frozen(coef.contiguous()), nan_bf16(G * N, H, W, C)
    call("adamml_maxpool2d_bwd_bn_apply", ptr(gd), ptr(idx), ptr(xd), ptr(v4), act, ptr(cd), ptr(dz), N, H, W, C, OH, OW, G)
    ref, ab = E.bn_bwd_apply_ref(gp.reshape(-1, C), x.reshape(-1, C), vec, coef, groups=G)
    record("maxpool2d_bwd_bn_apply[%s-%s]" % ("even" if H % 2 == 0 and W % 2 == 0 else "odd", name),
           E.point_check(dz.cpu().reshape(-1, C), ref, ab, E.K_BN_BWD_APPLY, what="maxpool2d_bwd_bn_apply " + name))
    # and z_sel feeds the plain reduction over the windows with the same sums
    if zsel:
        s2 = zsums(G, C)
        call("adamml_bn_bwd_reduce", ptr(gd), ptr(zs), ptr(v4), act, ptr(s2), N * OH * OW, C, G)
        gpw = g.double() * R.bn_mask(zs.cpu(), vec, act, groups=G)
        r2, a2 = R.bn_dgrad_sums_ref(gpw, zs.cpu(), vec, groups=G)
        E.sums_check(ssum(s2).cpu(), r2, a2, N * OH * OW, what="bn_bwd_reduce over z_sel " + name)


# ------------------------------------------------------------------------------------------------------------------------ temporal pool
TPOOL = [(T, mode, act) for T in (8, 4, 2, 1, 3, 5, 6) for mode in (0, 1) for act in (None, 1, 2) if not (mode == 1 and T < 3)]


@pytest.mark.parametrize("T,mode,act", TPOOL, ids=["T%d-%s-%s" % (t, "avg" if m else "max", {None: "plain", 1: "relu", 2: "relu6"}[a]) for t, m, a in TPOOL])
def test_temporal_pool(T, mode, act):
    """HW * C / 8 = 296 chunks per frame: not a multiple of the 256-thread block, four ragged workgroups per group with NB = 3"""
    NB, HW, C = 3, 37, 64
    G = 1 if act is None else 2
    name = "T%d-%s-%s-G%d" % (T, "avg" if mode else "max", {None: "plain", 1: "relu", 2: "relu6"}[act], G)
    seed = seed_of(name)
    To = (T - 1) // 2 + 1
    x = E.act_data(G * NB * T * HW, C, act or 1, seed).reshape(G * NB * T, HW, C)
    vec = tied_vectors(G, C, seed + 1, act) if act is not None else None
    vf = vec.reshape(-1) if vec is not None else None
    sc, sh = (vf, vf[C:]) if vf is not None else (None, None)
    xd = GB.frozen(x)
    vd = GB.frozen(vf) if vf is not None else None
    y = nan_bf16(G * NB * To, HW, C)
    call("adamml_temporal_pool_fwd", ptr(xd), ptr(vd), ptr(vd[C:]) if vd is not None else None, 4 * C, act or 0, ptr(y), NB, T, HW * C, C, mode, G)
    kern = "walk<%d>" % T if T in (8, 4, 2) else "generic"
    h = y.cpu().reshape(G * NB, To, HW * C)
    g = E.rand_bf16(G * NB * To, HW, C, seed=seed + 2)
    if mode == 0:
        yref, arg = E.temporal_pool_fwd_ref(x, sc, sh, 4 * C, act or 0, T, 0, groups=G)
        assert torch.equal(h.double(), yref), name + ": y"
        record("temporal_pool_fwd[%s-%s]" % (kern, name), 0.0)
        gref, gab = E.temporal_pool_bwd_ref(g, arg, T, 0)
        k = E.K_TPOOL_MAX_BWD
    else:
        ref, ab = E.temporal_pool_fwd_ref(x, sc, sh, 4 * C, act or 0, T, 1, groups=G)
        record("temporal_pool_fwd[%s-%s]" % (kern, name), E.point_check(h, ref, ab, E.K_TPOOL_AVG_FWD, what="temporal_pool_fwd " + name))
        gref, gab = E.temporal_pool_bwd_ref(g, None, T, 1)
        k = E.K_TPOOL_AVG_BWD
    gd, gx = GB.frozen(g), nan_bf16(G * NB * T, HW, C)
    call("adamml_temporal_pool_bwd", ptr(gd), ptr(xd), ptr(vd), ptr(vd[C:]) if vd is not None else None, 4 * C, act or 0, ptr(gx), NB, T, HW * C, C, mode, G)
    record("temporal_pool_bwd[%s]" % name, E.point_check(gx.cpu().reshape(G * NB, T, HW * C), gref, gab, k, what="temporal_pool_bwd " + name))


@pytest.mark.parametrize("T", [1, 2])
def test_temporal_avg_short_T_is_refused(T):
    x, y = GB.frozen(torch.zeros(T, 4, 8, dtype=torch.bfloat16)), nan_bf16(1, 4, 8)
    with pytest.raises(RuntimeError):
        call("adamml_temporal_pool_fwd", ptr(x), None, None, 0, 0, ptr(y), 1, T, 32, 8, 1, 1)
    torch.cuda.synchronize()
    assert GB.untouched(y)
    GB.unwritten_ok(y)


@pytest.mark.parametrize("with_z", [True, False])
@pytest.mark.parametrize("T", [8, 4, 2])
def test_temporal_pool_bwd_res(T, with_z):
    NB, HW, C, G, act = 3, 37, 64, 2, 1
    name = "T%d-%s-G%d" % (T, "z" if with_z else "zNULL", G)
    seed = seed_of(name)
    assert hip.load().adamml_temporal_pool_bwd_res_supported(T, C, 0) == 1
    To = (T - 1) // 2 + 1
    out = E.rand_bf16(G * NB * T, HW, C, seed=seed).float().clamp(min=0).to(torch.bfloat16)          # a block output: ties at 0
    g = E.rand_bf16(G * NB * To, HW, C, seed=seed + 1)
    z, vec = E.rand_bf16(G * NB * T, HW, C, seed=seed + 2), E.bn_vectors(G, C, seed + 3)
    _, arg = E.temporal_pool_fwd_ref(out, None, None, 0, 0, T, 0)
    routed, rab = E.temporal_pool_bwd_ref(g, arg, T, 0)
    m = E.act_mask(out.double(), act).reshape(routed.shape)
    od, gd, zd, vd = GB.frozen(out), GB.frozen(g), GB.frozen(z), GB.frozen(vec)
    g2, sums = nan_bf16(G * NB * T, HW, C), zsums(G, C)
    call("adamml_temporal_pool_bwd_res", ptr(gd), ptr(od), act, ptr(g2), ptr(zd) if with_z else None, ptr(vd) if with_z else None, ptr(sums),
         NB, T, HW, C, G)
    h = g2.cpu()
    r = E.point_check(h.reshape(routed.shape), routed * m, rab * m, E.K_TPOOL_MAX_BWD, what="temporal_pool_bwd_res " + name)
    got = ssum(sums).cpu()
    sref, sab = R.bn_dgrad_sums_ref(h.double().reshape(-1, C), z.reshape(-1, C), vec, groups=G)
    if not with_z:
        assert (got[:, C:] == 0).all(), name + ": the second moment stays 0 without z_a"
        got, sref, sab = got[:, :C], sref[:, :C], sab[:, :C]
    r = max(r, E.sums_check(got, sref, sab, NB * T * HW, what="temporal_pool_bwd_res sums " + name))
    record("temporal_pool_bwd_res[%s]" % name, r)


@pytest.mark.parametrize("T", [8, 4, 2])
def test_temporal_pool_bwd_code(T):
    NB, HW, C, G = 3, 37, 64, 2
    name = "T%d-G%d" % (T, G)
    seed = seed_of(name)
    To = T // 2
    g = E.rand_bf16(G * NB * To, HW, C, seed=seed)
    code = torch.randint(0, 4, (G * NB, To, HW, C), generator=E.gen(seed + 1))
    first = code[:, 0]
    first[first == 0] = 1                                            # tap 0 of window 0 is the padding frame: never recorded
    ref, ab = E.temporal_code_route(g, code.reshape(G * NB * To, HW, C), T)
    cd = GB.frozen(E.pack_codes(code))
    gd, g2, sums = GB.frozen(g), nan_bf16(G * NB * T, HW, C), zsums(G, C)
    call("adamml_temporal_pool_bwd_code", ptr(gd), ptr(cd), ptr(g2), ptr(sums), NB, T, HW, C, G)
    h = g2.cpu()
    r = E.point_check(h.reshape(ref.shape), ref, ab, E.K_TPOOL_MAX_BWD, what="temporal_pool_bwd_code " + name)
    got = ssum(sums).cpu()
    assert (got[:, C:] == 0).all()
    f = h.double().reshape(G, -1, C)
    r = max(r, E.sums_check(got[:, :C], f.sum(1), f.abs().sum(1), NB * T * HW, what="temporal_pool_bwd_code sums " + name))
    record("temporal_pool_bwd_code[%s]" % name, r)


# --------------------------------------------------------------------------------------------------------------------------------- gap
@pytest.mark.parametrize("N,HW,C,G,act", [(5, 49, 1280, 1, 2), (3, 25, 64, 3, 1), (2, 1, 8, 1, None)])
def test_gap(N, HW, C, G, act):
    name = "N%d-HW%d-C%d-G%d-%s" % (N, HW, C, G, {None: "plain", 1: "relu", 2: "relu6"}[act])
    seed = seed_of(name)
    x = E.act_data(G * N * HW, C, act or 1, seed)
    vec = E.bn_vectors(G, C, seed + 1, act) if act is not None else None
    vf = vec.reshape(-1) if vec is not None else None
    ref, ab, n = E.gap_fwd_ref(x, vf, vf[C:] if vf is not None else None, 4 * C, act or 0, N, HW, groups=G)
    xd = GB.frozen(x)
    vd = GB.frozen(vf) if vf is not None else None
    out = nan_f32(G * N, C)
    call("adamml_gap_fwd", ptr(xd), ptr(vd), ptr(vd[C:]) if vd is not None else None, 4 * C, act or 0, ptr(out), N, HW, C, G)
    r = R.err_ratio(out.cpu(), ref, ab, n, R.RHO_F32)
    assert r <= 1.0, "gap_fwd %s: %.3g" % (name, r)
    record("gap_fwd[%s]" % name, r)
    g = torch.randn(G * N, C, generator=E.gen(seed + 2))
    gd, gx = GB.frozen(g), nan_bf16(G * N, HW, C)
    call("adamml_gap_bwd", ptr(gd), ptr(gx), G * N, HW, C)
    gref = (g.double() / HW).view(G * N, 1, C).expand(G * N, HW, C)
    record("gap_bwd[%s]" % name, E.point_check(gx.cpu(), gref, gref.abs(), E.K_GAP_BWD, what="gap_bwd " + name))


# --------------------------------------------------------------------------------------------------------------------------- depthwise
# (id, N, H, W, C, stride, G)
DWCONV = [
    ("s1-OW%4=0-20x20-C96", 2, 20, 20, 96, 1, 1),
    ("s1-OW%4=2-9x14-C24-G2", 3, 9, 14, 24, 1, 2),
    ("s2-OWeven-21x19-C144-G2", 2, 21, 19, 144, 2, 2),
    ("s2-OWodd-16x18-C16-G3", 1, 16, 18, 16, 2, 3),
    ("s2-H1-1x7-C16", 2, 1, 7, 16, 2, 1),
    ("s1-W1-3x1-C8-G3", 2, 3, 1, 8, 1, 3),
    ("s1-2x2-C8", 2, 2, 2, 8, 1, 1),
    ("s2-2x2-C8", 2, 2, 2, 8, 2, 1),
    ("s1-7x7-C960", 2, 7, 7, 960, 1, 1),
    ("s2-5x6-C2048", 1, 5, 6, 2048, 2, 1),
    ("s1-40x40-C192-G5", 1, 40, 40, 192, 1, 5),
]


def dw_case(row):
    name, N, H, W, C, s, G = row
    seed = seed_of(name)
    OH, OW = (H - 1) // s + 1, (W - 1) // s + 1
    x = E.act_data(G * N * H * W, C, 2, seed).reshape(G * N, H, W, C)
    vec = E.bn_vectors(G, C, seed + 1, 2)
    # channel 1: the single-tap plant (activation exactly 1.5 through scale 1, shift 0; tap SINGLE_TAP)
    x[..., 1] = 1.5
    vec[:, 0, 1], vec[:, 1, 1] = 1.0, 0.0
    w = E.single_tap_weights(torch.randn(C, 1, 3, 3, generator=E.gen(seed + 2)) * 0.4, [1])
    return name, N, H, W, C, s, G, OH, OW, seed, x, vec, w


@pytest.mark.parametrize("row", DWCONV, ids=[r[0] for r in DWCONV])
def test_dwconv(row):
    name, N, H, W, C, s, G, OH, OW, seed, x, vec, w = dw_case(row)
    d = ConvDesc(N, H, W, C, OH, OW, C, 3, 3, s, 1, 1, 2, 0, G, 4 * C)
    vf = vec.reshape(-1)
    a = E.lazy_f32(x, vf, vf[C:], 2, G, 4 * C)
    xd, vd = GB.frozen(x), GB.frozen(vf)
    wp = pack(w, C, 2)
    # forward
    ref, ab, nt = E.dwconv_fwd_ref(a, w, s)
    y, stats = nan_bf16(G * N, OH, OW, C), zsums(G, C)
    call("adamml_dwconv_fwd", byref(d), ptr(xd), ptr(wp), ptr(vd), ptr(vd[C:]), ptr(y), ptr(stats))
    h = y.cpu()
    r = R.check(h, ref, ab, 9, acc=E.dw_acc(nt), what="dwconv_fwd " + name)
    assert torch.equal(h[..., 1].double(), E.single_tap_expected(a, w, s)[..., 1]), name + ": single-tap channel (float32 taps, unrounded)"
    R.stats_check(ssum(stats), h, what="dwconv_fwd stats " + name, groups=G)
    record("dwconv_fwd[%s]" % name, r)
    # data gradient, plain and accumulating
    g = E.rand_bf16(G * N, OH, OW, C, seed=seed + 3)
    gd = GB.frozen(g)
    dref, dab, dnt = E.dwconv_dgrad_ref(g.double(), w, (H, W), s)
    for acc in (0, 1):
        base = E.rand_bf16(G * N, H, W, C, seed=seed + 4) if acc else None
        dx = GB.inout(base) if acc else nan_bf16(G * N, H, W, C)
        call("adamml_dwconv_bwd_data", byref(d), ptr(gd), ptr(wp), ptr(dx), acc)
        GB.check("dwconv_bwd_data acc%d %s" % (acc, name))
        if acc:
            r = R.check(dx.cpu(), dref + base.double(), dab + base.double().abs(), 10, acc=E.dw_acc(dnt, 1), extra=R.RHO_BF16 * dref.abs(),
                        what="dwconv_bwd_data accumulate " + name)
        else:
            r = R.check(dx.cpu(), dref, dab, 9, acc=E.dw_acc(dnt), what="dwconv_bwd_data " + name)
        record("dwconv_bwd_data[acc%d-%s]" % (acc, name), r)
    # data gradient with the BatchNorm epilogue of the tensor it is the gradient of
    assert hip.load().adamml_dwconv_bwd_data_bn_supported(byref(d)) == 1
    m = R.bn_mask(x, vec, 2, groups=G)
    gpd, sums = nan_bf16(G * N, H, W, C), zsums(G, C)
    v4 = GB.frozen(vec)
    call("adamml_dwconv_bwd_data_bn", byref(d), ptr(gd), ptr(wp), ptr(gpd), ptr(xd), ptr(v4), 2, ptr(sums))
    hp = gpd.cpu()
    r = R.check(hp, dref * m, dab * m, 9, acc=E.dw_acc(dnt), what="dwconv_bwd_data_bn " + name)
    assert (m == 0).any() and (m == 1).any()
    sref, sab = R.bn_dgrad_sums_ref(hp.double(), x, vec, groups=G)
    r = max(r, E.sums_check(ssum(sums).cpu(), sref, sab, N * H * W, what="dwconv_bwd_data_bn sums " + name))
    record("dwconv_bwd_data_bn[%s]" % name, r)
    # weight gradient: atomic and workspace reductions, accumulated onto a base over all groups
    wref, wab = torch.zeros(C, 1, 3, 3, dtype=torch.float64), torch.zeros(C, 1, 3, 3, dtype=torch.float64)
    for gi in range(G):
        r1, a1, _ = E.dwconv_wgrad_ref(a[gi * N:(gi + 1) * N], g.double()[gi * N:(gi + 1) * N], s)
        wref, wab = wref + r1, wab + a1
    base = torch.randn(C, 1, 3, 3, generator=E.gen(seed + 5))
    def launch(outs, ws, nbytes):
        call("adamml_dwconv_bwd_weight", byref(d), ptr(gd), ptr(xd), ptr(vd), ptr(vd[C:]), ptr(outs[0]), ptr(ws), nbytes)

    def checked(dw, path):
        return E.wgrad_check(dw.cpu(), wref + base.double(), wab + base.double().abs(), G * N * OH * OW, what="dwconv_bwd_weight %s %s" % (path, name))

    dw = GB.inout(base)
    launch((dw,), None, 0)
    GB.check("dwconv_bwd_weight atomic " + name)
    record("dwconv_bwd_weight[atomic-%s]" % name, checked(dw, "atomic"))
    # exact, dirty, one float short: an undersized workspace is ignored (p.ws = nullptr in csrc/dwconv_gemm32.hip: atomic accumulation)
    q = hip.load().adamml_dwconv_bwd_weight_workspace(byref(d))
    (dw,), (dw_short,) = workspace_launches(GB, q, lambda: (GB.inout(base),), launch, "fallback", "dwconv_bwd_weight workspace " + name)
    record("dwconv_bwd_weight[workspace-%s]" % name, checked(dw, "workspace"))
    record("dwconv_bwd_weight[workspace-%s]+dirty" % name, 0.0)
    record("dwconv_bwd_weight[workspace-%s]+short" % name, checked(dw_short, "workspace one float short"))


def test_bn_finalize_on_a_channel_with_mean_30_std():
    """Statistics of a channel with |mean| / std = 30 from a kernel's own float32 partial sums (dwconv_fwd with a centre tap of 1: y = x),
    through bn_finalize: the stats_check bound on the two sums, propagated through var = s2 / n - mu^2, bounds invstd.  The derived bound
    is asserted; the observed error is recorded next to it."""
    N, H, W, C = 2, 40, 40, 16
    rid = "bn_finalize[mean30-from-dwconv_fwd-stats]"
    x = E.rand_bf16(N, H, W, C, seed=9)
    x[..., 1] = (E.rand_bf16(N, H, W, seed=10).double() * 0.5 + 15.0).to(torch.bfloat16)           # std 0.5, mean 15
    w = torch.zeros(C, 1, 3, 3)
    w[:, 0, 1, 1] = 1.0
    d = ConvDesc(N, H, W, C, H, W, C, 3, 3, 1, 1, 1, 0, 0, 1, 0)
    xd = GB.frozen(x)
    y, stats = nan_bf16(N, H, W, C), zsums(1, C)
    call("adamml_dwconv_fwd", byref(d), ptr(xd), ptr(pack(w, C, 2)), None, None, ptr(y), ptr(stats))
    assert torch.equal(y.cpu(), x)
    R.stats_check(ssum(stats), y.cpu(), what=rid, groups=1)
    n = float(N * H * W)
    gamma, beta, vec = GB.frozen(torch.ones(C)), GB.frozen(torch.zeros(C)), nan_f32(1, 4, C)
    call("adamml_bn_finalize", ptr(stats), STAT_SLOTS, 1, n, ptr(gamma), ptr(beta), None, None, 0.1, 1e-5, ptr(vec), C)
    sref, sab = R.stats_ref(x.double())
    tol = R.tolerance(sref, sab, int(n), 2.0 ** -23)
    mu, ex2 = sref[:C] / n, sref[C:] / n
    var = ex2 - mu * mu
    dvar = tol[C:] / n + 2 * mu.abs() * tol[:C] / n + (tol[:C] / n) ** 2
    eps = torch.tensor(1e-5, dtype=torch.float32).item()
    lo = 1.0 / torch.sqrt(var + dvar + eps) * (1 - 2 * R.U32)
    hi = 1.0 / torch.sqrt(torch.clamp(var - dvar, min=0.0) + eps) * (1 + 2 * R.U32)
    got = vec.cpu().double()[0, 3]
    exact = 1.0 / torch.sqrt(var + eps)
    assert ((got >= lo) & (got <= hi)).all(), rid
    rel = ((got - exact).abs() / exact)
    bound = torch.maximum(hi - exact, exact - lo) / exact
    record(rid, (rel / bound).max().item())
    NOTES[rid] = "channel 1 (|mean|/std = 30): observed relative invstd error %.3g, derived bound %.3g" % (rel[1].item(), bound[1].item())


# ------------------------------------------------------------------------------------------------------------------- dwconv_bwd_fused
# (id, N, H, W, C, stride, G)
FUSED = [
    ("s1-20x20-C96", 2, 20, 20, 96, 1, 1),
    ("s1-9x14-C24-G2", 3, 9, 14, 24, 1, 2),
    ("s1-1x5-C16", 2, 1, 5, 16, 1, 1),
    ("s1-7x7-C960", 2, 7, 7, 960, 1, 1),
    ("s2-21x19-C144-G2", 2, 21, 19, 144, 2, 2),
    ("s2-16x16-C32-G3", 1, 16, 16, 32, 2, 3),
    ("s2-3x1-C32", 2, 3, 1, 32, 2, 1),
]


def run_fused(row, segw):
    """dz, dW and the data gradient of adamml_dwconv_bwd_fused against float64 A g + B z + C directly; the kernel's bf16 rounding of dz
    (mkdz(): f32_to_bf4) enters as the `extra` term E carried through the same contractions"""
    name, N, H, W, C, s, G = row
    seed = seed_of(name)
    OH, OW = (H - 1) // s + 1, (W - 1) // s + 1
    d = ConvDesc(N, H, W, C, OH, OW, C, 3, 3, s, 1, 1, 2, 0, G, 4 * C)
    assert hip.load().adamml_dwconv_bwd_fused_supported(byref(d)) == 1
    g = E.rand_bf16(G * N, OH, OW, C, seed=seed)
    g = (g.float() * (torch.rand(g.shape, generator=E.gen(seed + 1)) > 0.3)).to(torch.bfloat16)      # masked gradient: exact zeros
    z = E.rand_bf16(G * N, OH, OW, C, scale=1.5, seed=seed + 2)
    aff = torch.randn(G, 3, C, generator=E.gen(seed + 3)) * 0.5
    x = E.act_data(G * N * H * W, C, 2, seed + 4).reshape(G * N, H, W, C)
    xvec = E.bn_vectors(G, C, seed + 5, 2)
    w = torch.randn(C, 1, 3, 3, generator=E.gen(seed + 6)) * 0.4
    dz, Ez = E.fused_dz_ref(g, z, aff, G)
    dref, dab, dnt = E.dwconv_dgrad_ref(dz, w, (H, W), s)
    dextra, _, _ = E.dwconv_dgrad_ref(Ez, w.abs(), (H, W), s)
    m = R.bn_mask(x, xvec, 2, groups=G)
    vf = xvec.reshape(-1)
    a = E.lazy_f32(x, vf, vf[C:], 2, G, 4 * C)
    wref, wab, wextra = (torch.zeros(C, 1, 3, 3, dtype=torch.float64) for _ in range(3))
    for gi in range(G):
        sl = slice(gi * N, (gi + 1) * N)
        r1, a1, _ = E.dwconv_wgrad_ref(a[sl], dz[sl], s)
        e1, _, _ = E.dwconv_wgrad_ref(a[sl].abs(), Ez[sl], s)
        wref, wab, wextra = wref + r1, wab + a1, wextra + e1
    base = torch.randn(C, 1, 3, 3, generator=E.gen(seed + 7))
    gd, zd, ad, xd, vd, wp = GB.frozen(g), GB.frozen(z), GB.frozen(aff), GB.frozen(x), GB.frozen(xvec), pack(w, C, 2)
    rid = "dwconv_bwd_fused[segw%d-%s]" % (segw, name)

    def launch(outs, ws, nbytes):
        call("adamml_dwconv_bwd_fused", byref(d), ptr(gd), ptr(zd), ptr(ad), ptr(wp), ptr(xd), ptr(vd), 2, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
             ptr(ws), nbytes)

    # exact, dirty, one float short: refused with EINVAL before the launch (csrc/dwconv_bwd_fused.hip)
    q = hip.load().adamml_dwconv_bwd_fused_workspace(byref(d))
    (dx, sums, dw), _ = workspace_launches(GB, q, lambda: (nan_bf16(G * N, H, W, C), zsums(G, C), GB.inout(base)), launch, "refuse", rid,
                                           sync=torch.cuda.synchronize)
    record(rid + "+dirty", 0.0)
    record(rid + "+short", 0.0)
    h = dx.cpu()
    r_dx = R.check(h, dref * m, dab * m, 9, acc=E.dw_acc(dnt), extra=dextra * m, what="dwconv_bwd_fused dx " + name)
    sref, sab = R.bn_dgrad_sums_ref(h.double(), x, xvec, groups=G)
    r_s = E.sums_check(ssum(sums).cpu(), sref, sab, N * H * W, what="dwconv_bwd_fused sums " + name)
    r_w = E.wgrad_check(dw.cpu(), wref + base.double(), wab + base.double().abs(), G * N * OH * OW, extra=wextra, what="dwconv_bwd_fused dW " + name)
    # how much of the bound the rounding of dz takes: the same outputs against the kernel's own rounded dz (no extra term)
    A, B, Cc = (aff[:, k].double().view(G, 1, 1, 1, C) for k in range(3))
    gg, zz = g.double().view(G, N, OH, OW, C), z.double().view(G, N, OH, OW, C)
    dzk = R.bf16(E.f32(A * gg + E.f32(B * zz + Cc))).view(G * N, OH, OW, C)
    kref, kab, _ = E.dwconv_dgrad_ref(dzk, w, (H, W), s)
    r_k = R.err_ratio(h, kref * m, kab * m, 9, R.RHO_BF16, acc=E.dw_acc(dnt))
    record(rid, max(r_dx, r_s, r_w))
    NOTES[rid] = "dx %.3f sums %.3f dW %.3f; dx against the kernel's own bf16 dz, no extra term: %.3f" % (r_dx, r_s, r_w, r_k)
    assert r_k <= 1.0, rid + ": dx against the emulated bf16 dz"


@pytest.mark.parametrize("row", FUSED, ids=[r[0] for r in FUSED])
def test_dwconv_bwd_fused(row):
    assert os.environ.get("ADAMML_DWB_SEGW", "3") != "2"
    run_fused(row, 3)


def fused_child_main():
    """entry of the child process of test_switch_only_instances_child (both switches are read once per process)"""
    assert os.environ.get("ADAMML_DWB_SEGW") == "2" and os.environ.get("ADAMML_DW_S2_QUADS") == "0"
    for row in FUSED:
        if row[5] == 1:
            run_fused(row, 2)
            GB.check(row[0])                                             # (no fixture in the child: the check of the row by hand)
            GB.reset()
    before = set(WORST)
    for row in DWCONV:
        if row[5] == 2:
            test_dwconv(row)
            GB.check(row[0])
            GB.reset()
    for k in set(WORST) - before:
        v = WORST.pop(k)
        if k.startswith("dwconv_bwd_data["):                         # (the other entry points of the row do not read the switch)
            WORST[k.replace("[", "[quads0-", 1)] = v
    print_table()


def test_switch_only_instances_child():
    """dwconv_bwd_fused_kernel<1, 2> (ADAMML_DWB_SEGW=2) and the stride-2 branch of dwconv_bwd_data_kernel (ADAMML_DW_S2_QUADS=0): both
    switches are read once per process -> one fresh child process (never an exec over this one, which has the GPU open)"""
    env = dict(os.environ, ADAMML_DWB_SEGW="2", ADAMML_DW_S2_QUADS="0")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", "from tests.test_elementwise_conformance_gpu import fused_child_main; fused_child_main()"]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    n = [0, 0]
    for ln in out.stdout.splitlines():
        p = ln.split()
        for i, prefix in enumerate(("dwconv_bwd_fused[segw2-", "dwconv_bwd_data[quads0-")):
            if p and p[0].startswith(prefix):
                record(p[0], float(p[1]))
                if len(p) > 2:
                    NOTES[p[0]] = " ".join(p[2:])
                n[i] += 1
    # (every dwconv_bwd_fused row three times: exact, +dirty, +short)
    assert n == [3 * sum(1 for r in FUSED if r[5] == 1), 2 * sum(1 for r in DWCONV if r[5] == 2)], n


# ------------------------------------------------------------------------------------------------------------------------------- stems
@pytest.mark.parametrize("N,H,W,Cin,G,xc", [(3, 64, 64, 3, 1, 8), (2, 30, 50, 1, 1, 8), (1, 96, 96, 4, 3, 8), (1, 7, 10, 3, 2, 8), (2, 33, 46, 3, 2, 4)])
def test_conv_stem(N, H, W, Cin, G, xc):
    """xc = channels per stored pixel: 8 (padded) or the 4-channel layout of adamml_clip_to_nhwc(c_pad = 4)"""
    name = "N%d-%dx%d-Cin%d-G%d-xc%d" % (N, H, W, Cin, G, xc)
    seed = seed_of(name)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    d = ConvDesc(N, H, W, xc, OH, OW, 64, 7, 7, 2, 3, 1, 0, 0, G, 0)
    assert hip.load().adamml_conv_stem_supported(byref(d)) == 1
    x = E.rand_bf16(G * N, H, W, xc, seed=seed)
    x[..., Cin:] = 0
    w = R.bf16(torch.randn(64, Cin, 7, 7, generator=E.gen(seed + 1), dtype=torch.float64) * (2.0 / (Cin * 49)) ** 0.5).float()
    ref, ab, _ = R.conv_fwd_ref(x.double(), w, 2, 3)
    xd, wd = GB.frozen(x), GB.frozen(w)
    wsp = GB.out((64, 224), torch.bfloat16)
    call("adamml_pack_stem_weight", ptr(wd), ptr(wsp), 64, Cin)
    GB.check("pack_stem_weight " + name)
    wsp = GB.frozen(wsp)
    y, st = nan_bf16(G * N, OH, OW, 64), zsums(G, 64)
    call("adamml_conv_stem_fwd", byref(d), ptr(xd), ptr(wsp), ptr(y), ptr(st))
    h = y.cpu()
    r = R.check(h, ref, ab, E.STEM_K, what="conv_stem_fwd " + name)
    R.stats_check(ssum(st), h, what="conv_stem_fwd stats " + name, groups=G)
    record("conv_stem_fwd[%s]" % name, r)
    g = E.rand_bf16(G * N, OH, OW, 64, seed=seed + 2)
    wref, wab, n = R.conv_wgrad_ref(x.double(), g.double(), (64, Cin, 7, 7), 2, 3)
    base = torch.randn(64, Cin, 7, 7, generator=E.gen(seed + 3))
    gd = GB.frozen(g)

    def launch(outs, ws, nbytes):
        call("adamml_conv_stem_bwd_weight", byref(d), ptr(gd), ptr(xd), ptr(outs[0]), Cin, ptr(ws), nbytes)

    # exact, dirty, one float short: refused with EINVAL before the launch (csrc/conv_stem.hip)
    q = hip.load().adamml_conv_stem_bwd_weight_workspace(byref(d))
    (dw,), _ = workspace_launches(GB, q, lambda: (GB.inout(base),), launch, "refuse", "conv_stem_bwd_weight " + name, sync=torch.cuda.synchronize)
    record("conv_stem_bwd_weight[%s]+dirty" % name, 0.0)
    record("conv_stem_bwd_weight[%s]+short" % name, 0.0)
    record("conv_stem_bwd_weight[%s]" % name, E.wgrad_check(dw.cpu(), wref + base.double(), wab + base.double().abs(), n,
                                                            what="conv_stem_bwd_weight " + name, products_round=False))


@pytest.mark.parametrize("B,G,H,W,C", [(3, 2, 64, 64, 32), (1, 1, 33, 47, 32), (2, 3, 20, 30, 8), (2, 5, 2, 1, 64)])
def test_conv_stem1(B, G, H, W, C):
    """neither the float32 image nor the float32 taps are rounded (X1 branch of xform() in csrc/dwconv_gemm32.hip): float64 reference on both"""
    name = "B%d-G%d-%dx%d-C%d" % (B, G, H, W, C)
    seed = seed_of(name)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    d = ConvDesc(B, H, W, 8, OH, OW, C, 3, 3, 2, 1, 1, 0, 0, G, 0)
    assert hip.load().adamml_conv_stem1_supported(byref(d)) == 1
    x = torch.randn(B, G, H, W, generator=E.gen(seed)) * 3.0 - 5.0
    w = torch.randn(C, 1, 3, 3, generator=E.gen(seed + 1)) * 0.4
    a = x.transpose(0, 1).reshape(G * B, H, W, 1).double().expand(G * B, H, W, C).contiguous()        # group-major, broadcast over the channels
    ref, ab, nt = E.dwconv_fwd_ref(a, w, 2)
    xd = GB.frozen(x)
    wp = pack(w, 1, 2)
    y, st = nan_bf16(G * B, OH, OW, C), zsums(G, C)
    call("adamml_conv_stem1_fwd", byref(d), ptr(xd), G * H * W, H * W, ptr(wp), ptr(y), ptr(st))
    h = y.cpu()
    r = R.check(h, ref, ab, 9, acc=E.dw_acc(nt), what="conv_stem1_fwd " + name)
    R.stats_check(ssum(st), h, what="conv_stem1_fwd stats " + name, groups=G)
    record("conv_stem1_fwd[%s]" % name, r)
    g = E.rand_bf16(G * B, OH, OW, C, scale=0.1, seed=seed + 2)
    wref, wab, n = E.dwconv_wgrad_ref(a, g.double(), 2)
    base = torch.randn(C, 1, 3, 3, generator=E.gen(seed + 3))
    gd = GB.frozen(g)

    def launch(outs, ws, nbytes):
        call("adamml_conv_stem1_bwd_weight", byref(d), ptr(gd), ptr(xd), G * H * W, H * W, ptr(outs[0]), ptr(ws), nbytes)

    def checked(dw, path):
        return E.wgrad_check(dw.cpu(), wref + base.double(), wab + base.double().abs(), n, what="conv_stem1_bwd_weight %s %s" % (path, name))

    dw = GB.inout(base)
    launch((dw,), None, 0)
    GB.check("conv_stem1_bwd_weight atomic " + name)
    record("conv_stem1_bwd_weight[atomic-%s]" % name, checked(dw, "atomic"))
    # exact, dirty, one float short: an undersized workspace is ignored (p.ws = nullptr in csrc/dwconv_gemm32.hip: atomic accumulation)
    q = hip.load().adamml_conv_stem1_bwd_weight_workspace(byref(d))
    (dw,), (dw_short,) = workspace_launches(GB, q, lambda: (GB.inout(base),), launch, "fallback", "conv_stem1_bwd_weight workspace " + name)
    record("conv_stem1_bwd_weight[workspace-%s]" % name, checked(dw, "workspace"))
    record("conv_stem1_bwd_weight[workspace-%s]+dirty" % name, 0.0)
    record("conv_stem1_bwd_weight[workspace-%s]+short" % name, checked(dw_short, "workspace one float short"))


# -------------------------------------------------------------------------------------------------------------------------- large rows
def large_P(mb):
    """C = 256, G = 5: the smallest multiple of 64 pixels per group with groups * P * C * 2 bytes above `mb` MB"""
    return ((mb << 20) // (5 * 256 * 2) // 64 + 1) * 64


def dev_bf16(rows, C, seed, scale=1.0, offset=0.0, relu=False):
    """a read-only operand generated on the device (0.3 - 0.6 GB: not through the host)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    t = (torch.randn(rows, C, generator=g, device=DEV) * scale + offset).to(torch.bfloat16)
    return GB.frozen(t.clamp_(min=0) if relu else t)


def sums_ref_gpu(gp, z, vec, G, P, C):
    """float64 (sum g', sum g' zhat) per group, accumulated on the device in chunks -> CPU ([G, 2C], abs)"""
    out, ab = torch.zeros(G, 2 * C, dtype=torch.float64, device=DEV), torch.zeros(G, 2 * C, dtype=torch.float64, device=DEV)
    step = 1 << 15
    for g in range(G):
        mu, inv = vec[g, 2].double(), vec[g, 3].double()
        for p in range(0, P, step):
            f = gp[g * P + p:g * P + min(p + step, P)].double()
            t = f * ((z[g * P + p:g * P + min(p + step, P)].double() - mu) * inv)
            out[g, :C] += f.sum(0)
            out[g, C:] += t.sum(0)
            ab[g, :C] += f.abs().sum(0)
            ab[g, C:] += t.abs().sum(0)
    return out.cpu(), ab.cpu()


@pytest.mark.parametrize("mb", [256, 512])
@pytest.mark.parametrize("kernel", ["bn_act_add_mask", "bn_bwd_apply", "residual_bwd"])
def test_large_rows(kernel, mb):
    """The variants the benchmark runs -- non-temporal loads and stores above 256 MB, four instead of eight rows per workgroup above
    512 MB -- must give bit for bit what the same entry point gives on per-group slices (54 / 107 MB each: the instance the small rows
    tie to float64).  Operands are generated on the device."""
    C, G, act = 256, 5, 1
    P = large_P(mb)
    assert G * P * C * 2 > (mb << 20) and P * C * 2 < (256 << 20)
    rid = "%s[large-%dMB-G5-C256-P%d]" % (kernel, mb, P)
    vec = GB.frozen(E.bn_vectors(G, C, 3, act))
    z = dev_bf16(G * P, C, 1)
    r = 0.0
    if kernel == "bn_act_add_mask":
        idn, vi = dev_bf16(G * P, C, 2), GB.frozen(E.bn_vectors(G, C, 4, act))
        out, bits = nan_bf16(G * P, C), GB.out((G * P * C // 8,), torch.uint8)
        call("adamml_bn_act_add_mask", ptr(z), ptr(vec), ptr(vec.reshape(-1)[C:]), 4 * C, act, ptr(idn), ptr(vi), ptr(vi.reshape(-1)[C:]), 4 * C,
             ptr(out), ptr(bits), P, C, G)
        o1, b1 = nan_bf16(P, C), GB.out((P * C // 8,), torch.uint8)
        for g in range(G):
            sl = slice(g * P, (g + 1) * P)
            call("adamml_bn_act_add_mask", ptr(z[sl]), ptr(vec[g, 0]), ptr(vec[g, 1]), 0, act, ptr(idn[sl]), ptr(vi[g, 0]), ptr(vi[g, 1]), 0,
                 ptr(o1), ptr(b1), P, C, 1)
            assert torch.equal(out[sl], o1) and torch.equal(bits[g * P * C // 8:(g + 1) * P * C // 8], b1), "%s: group %d" % (rid, g)
        del idn, out, bits, o1, b1
    elif kernel == "bn_bwd_apply":
        gq = dev_bf16(G * P, C, 2)
        coef = GB.frozen(torch.stack([vec[:, 3] * 1.3, vec[:, 2] * 0.3, vec[:, 1] * 0.4], 1).contiguous())
        dz, d1 = nan_bf16(G * P, C), nan_bf16(P, C)
        call("adamml_bn_bwd_apply", ptr(gq), ptr(z), ptr(vec), act, ptr(coef), ptr(dz), P, C, G)
        for g in range(G):
            sl = slice(g * P, (g + 1) * P)
            call("adamml_bn_bwd_apply", ptr(gq[sl]), ptr(z[sl]), ptr(vec[g]), act, ptr(coef[g]), ptr(d1), P, C, 1)
            assert torch.equal(dz[sl], d1), "%s: group %d" % (rid, g)
        del gq, dz, d1
    else:
        gq, out = dev_bf16(G * P, C, 2), dev_bf16(G * P, C, 5, relu=True)
        zb, vb = dev_bf16(G * P, C, 6), GB.frozen(E.bn_vectors(G, C, 7, act))
        g2, sa, sb = nan_bf16(G * P, C), zsums(G, C), zsums(G, C)
        call("adamml_residual_bwd", ptr(gq), ptr(out), act, ptr(g2), ptr(z), ptr(vec), ptr(sa), ptr(zb), ptr(vb), ptr(sb), P, C, G)
        g1 = nan_bf16(P, C)
        for g in range(G):
            sl = slice(g * P, (g + 1) * P)
            s1, s2 = zsums(1, C), zsums(1, C)
            call("adamml_residual_bwd", ptr(gq[sl]), ptr(out[sl]), act, ptr(g1), ptr(z[sl]), ptr(vec[g]), ptr(s1), ptr(zb[sl]), ptr(vb[g]), ptr(s2),
                 P, C, 1)
            assert torch.equal(g2[sl], g1), "%s: group %d" % (rid, g)
        assert torch.equal(g2, gq * (out > 0).to(torch.bfloat16))
        for zz, vv, ss, nm in ((z, vec, sa, "a"), (zb, vb, sb, "b")):
            sref, sab = sums_ref_gpu(g2, zz, vv, G, P, C)
            r = max(r, E.sums_check(ssum(ss).cpu(), sref, sab, P, what="%s sums %s" % (rid, nm)))
        del gq, out, zb, g2, g1
    record(rid, r)
    GB.check(rid)
    GB.reset()
    del z
    torch.cuda.empty_cache()
