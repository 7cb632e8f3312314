"""Conformance of the algebraic BatchNorm backward, adamml_gemm_f32, the classifier head, the column sums, the input re-layout kernels, the
optimizer steps, the policy head, the Gumbel gate, the late fusion and adamml_copy2d against float64 references (tests/abi_ref.py).

One row per kernel instance or dispatch branch; the row id names the entry point and the case, and profiles/abi_conformance_rows.md lists
the kernel each row launched.  Operands are generated on the CPU from seeded generators, outputs are pre-filled with NaN (or a base
tensor where the entry point accumulates) so that an element a kernel never writes fails, every call goes through the C ABI with
hip.call, and the rows assert the library's dispatch probes (adamml_conv_bwd_data_alg_streams, adamml_gemm_f32_uses_mfma,
adamml_clip_to_nhwc_four_pixel: the launchers call the same functions).  Operand buffers end in NaN slack, so a read past an operand shows in the result.
Every buffer handed to a kernel comes from tests/guarded.py: outputs, accumulators, optimizer state and workspaces inside sentinel bands,
read-only operands compared bit for bit, both checked at the end of every row and after each launch of a row that launches twice.  Tolerances are those derived in
tests/abi_ref.py; none is fitted to an observed error: counted roundings everywhere except the policy head and the gate forward, whose
bound is 16 x the distance of the same computation in float32 on the CPU from float64, measured in the row.  The module prints its
WORST table (row id -> largest err / tol): pytest -s."""
import math
import time

import pytest
import torch
from ctypes import byref

from tests import abi_ref as A
from tests import conv_ref as R
from tests import elementwise_ref as E

pytestmark = pytest.mark.gpu

from adamml_amd import hip  # noqa: E402
from adamml_amd.hip import ConvDesc, call, ptr, STAT_SLOTS  # noqa: E402
from tests.guarded import workspace_launches  # noqa: E402
from tests.test_conv_conformance_gpu import GB, guard, ssum, zstats  # noqa: E402,F401  (guard: the autouse check of every row)

T0 = time.time()
WORST = {}
NOTES = {}
NAN = float("nan")


def record(rid, r, note=None):
    WORST[rid] = max(WORST.get(rid, 0.0), r)
    if note:
        NOTES[rid] = note


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    if WORST:
        k = max(WORST, key=WORST.get)
        print("\nabi conformance: largest err/tol %.4f (%s) over %d rows, %.0f s" % (WORST[k], k, len(WORST), time.time() - T0))
        for rid in sorted(WORST):
            print("  %-64s %.4f   %s" % (rid, WORST[rid], NOTES.get(rid, "")))


def seed_of(rid):
    return sum(map(ord, rid)) % 10007


def nan_f32(*shape):
    return GB.out(shape, torch.float32)


def nan_bf16(*shape):
    return GB.out(shape, torch.bfloat16)


def passed(rid, r, what=""):
    assert r <= 1.0, "%s %s: max err/tol %.3g" % (rid, what, r)
    return r


# ------------------------------------------------------------------------------------------------------------------------------ alg_pack
ALG_PACK = [("256x64-G1", 256, 64, 1, False), ("256x64-G3-mpre", 256, 64, 3, True), ("512x128-G3", 512, 128, 3, False),
            ("512x128-G1-mpre", 512, 128, 1, True), ("1024x256-G1", 1024, 256, 1, False), ("1024x256-G3-mpre", 1024, 256, 3, True)]


@pytest.mark.parametrize("row", ALG_PACK, ids=[r[0] for r in ALG_PACK])
def test_alg_pack(row):
    name, Cout, Cin, G, pre = row
    rid, seed = "alg_pack[%s]" % name, seed_of(name)
    w, aff = A.alg_operands(Cout, Cin, G, seed)
    # (an asymmetric m_pre: the kernel copies it, and a transposed read would show)
    m_pre = A.randn32(G, Cin, Cin, seed=seed + 1, scale=0.05) if pre else None
    ref = A.alg_pack_ref(w, aff, m_pre)
    wd, ad, md = GB.frozen(w), GB.frozen(aff), GB.frozen(m_pre) if pre else None
    w_alg, epi = nan_bf16(G, Cin, Cout + Cin), nan_f32(G, Cin)
    call("adamml_alg_pack", ptr(wd), ptr(ad), ptr(md), ptr(w_alg), ptr(epi), Cout, Cin, G)
    wa, m = A.alg_pack_split(w_alg.cpu(), Cout)
    r = passed(rid, A.ratio(wa, *ref["wa"]), "W^T diag(A)")
    if pre:
        assert torch.equal(m, ref["m"][0]), rid + ": bf16(m_pre)"
    else:
        r = max(r, passed(rid, A.ratio(m, *ref["m"]), "W^T diag(B) W"))
    r = max(r, passed(rid, A.ratio(epi.cpu(), *ref["epi"]), "epi_add"))
    record(rid, r, "alg_pack_kernel" + (" (m_pre read)" if pre else " (M formed)"))


# --------------------------------------------------------------------------------------------------------------------- alg_wgrad_combine
WGRAD = [("256x64-G1-Gform", 256, 64, 1, False), ("256x64-G3-Gform-base", 256, 64, 3, False), ("512x128-G3-wgpre-base", 512, 128, 3, True),
         ("512x256-G1-wgpre", 512, 256, 1, True)]


@pytest.mark.parametrize("row", WGRAD, ids=[r[0] for r in WGRAD])
def test_alg_wgrad_combine(row):
    name, Cout, Cin, G, pre = row
    rid, seed = "alg_wgrad_combine[%s]" % name, seed_of(name)
    w, aff = A.alg_operands(Cout, Cin, G, seed)
    P = A.randn32(G, Cout, Cin, seed=seed + 1, scale=20.0)
    Gm = A.randn32(G, Cin, Cin, seed=seed + 2, scale=30.0)
    sv = A.randn32(G, Cin, seed=seed + 3, scale=50.0)
    wg = A.randn32(Cout, G * Cin, seed=seed + 4, scale=25.0) if pre else None
    base = A.randn32(Cout, Cin, seed=seed + 5) if "base" in name else torch.zeros(Cout, Cin)
    ref, tol = A.alg_wgrad_combine_ref(w, aff, P, G=None if pre else Gm, wg_pre=wg, s=sv, dw0=base)
    wd, ad, Pd, Gd, sd, dw = GB.frozen(w), GB.frozen(aff), GB.frozen(P), GB.frozen(Gm), GB.frozen(sv), GB.inout(base)
    wgd = GB.frozen(wg) if pre else None
    # (G is passed in the wg_pre form too, as the runtime does; it is then not read)
    call("adamml_alg_wgrad_combine", ptr(wd), ptr(ad), ptr(Pd), ptr(Gd), ptr(wgd), ptr(sd), ptr(dw), Cout, Cin, G)
    record(rid, passed(rid, A.ratio(dw.cpu(), ref, tol)), "alg_wgrad_combine_kernel" + (" (wg_pre)" if pre else " (W G formed)"))


# ---------------------------------------------------------------------------------------------------------------------------- alg_sumfix
@pytest.mark.parametrize("name,ratio_mean_std", [("benign-256x64-G3", 0.5), ("mean40std-256x64-G3", 40.0), ("mean40std-512x128-G1", 40.0)])
def test_alg_sumfix(name, ratio_mean_std):
    """P = g'^T a of real operands (float64, rounded once to float32 as a product kernel stores it), z = W a; the hard rows put the
    BatchNorm mean 40 standard deviations from z and correlate g' with z so that sum(g' zhat) is small: dot and mean * s1 cancel"""
    rid, seed = "alg_sumfix[%s]" % name, seed_of(name)
    Cout, Cin = (512, 128) if "512" in name else (256, 64)
    G, Pn = (1 if name.endswith("G1") else 3), 300
    w, _ = A.alg_operands(Cout, Cin, G, seed)
    a = E.rand_bf16(G * Pn, Cin, seed=seed + 1).double().reshape(G, Pn, Cin).clamp(min=0) + 0.25
    z = torch.einsum("gpi,oi->gpo", a, w.double())
    mean, std = z.mean(1), z.std(1)
    gp = E.rand_bf16(G * Pn, Cout, seed=seed + 2).double().reshape(G, Pn, Cout)
    vec = torch.zeros(G, 4, Cout)
    if ratio_mean_std > 1:
        # the BatchNorm mean at 40 standard deviations: zhat = zeta + delta, zeta the standardised z, |delta| = 40.  g' = c (1 - delta zeta)
        # + noise has sum(g') = c P and sum(g' zeta) = -delta c P, so sum(g' zhat) = delta sum(g') + sum(g' zeta) ~ 0; the rest is removed
        # along zeta (sum zeta = 0: sum(g') keeps its size) and comes back only as the bf16 rounding of g'
        zeta = (z - mean.unsqueeze(1)) / std.unsqueeze(1)
        mu = mean - torch.sign(mean) * ratio_mean_std * std
        delta = ((mean - mu) / std).unsqueeze(1)
        zh = zeta + delta
        gp = 0.05 * (1.0 - delta * zeta) + 0.1 * gp
        gp = (gp - zeta * ((gp * zh).sum(1) / (zeta * zeta).sum(1)).unsqueeze(1)).to(torch.bfloat16).double()
        mean = mu
    vec[:, 2], vec[:, 3] = mean.float(), (1.0 / std).float()
    assert ratio_mean_std <= 1 or (vec[:, 2].abs() * vec[:, 3]).min().item() >= 30.0
    Pm = torch.einsum("gpo,gpi->goi", gp, a).float()
    s1 = gp.sum(1)                                                      # exact: bf16 values, 300 of them
    sums = torch.zeros(G, 2 * Cout, dtype=torch.float64)
    sums[:, :Cout] = s1
    bins = E.stats_to_slots(sums, STAT_SLOTS)
    bins[:, :, Cout:] = NAN                                             # the second halves are overwritten, whatever they hold
    ref, tol = A.alg_sumfix_ref(w, Pm, vec, s1)
    if ratio_mean_std > 1:
        big = (vec[:, 3].double() * vec[:, 2].double() * s1).abs()
        assert (ref.abs() < 1e-2 * big).float().mean().item() > 0.5, rid + ": the operands do not cancel"
    wd, Pd, vd, sd = GB.frozen(w), GB.frozen(Pm), GB.frozen(vec), GB.inout(bins)
    call("adamml_alg_sumfix", ptr(wd), ptr(Pd), ptr(vd), ptr(sd), Cout, Cin, G)
    out = ssum(sd).cpu()
    assert torch.equal(out[:, :Cout], s1), rid + ": sum(g') changed"
    record(rid, passed(rid, A.ratio(out[:, Cout:], ref, tol)), "alg_sumfix_kernel")


# --------------------------------------------------------------------------------------------------------------------- conv_bwd_data_alg
# (id, Cout, Cin, G, N, H, mode, lazy a)   pixel counts per group that fill no tile: 169 = 13^2, 225 = 15^2
DGRAD = [("stream-256x64-acc0-plain", 256, 64, 2, 1, 13, "acc0", False), ("stream-256x64-acc1-lazy", 256, 64, 3, 1, 15, "acc1", True),
         ("stream-256x64-bn-lazy", 256, 64, 2, 1, 15, "bn", True), ("stream-256x64-bn-plain-P1", 256, 64, 1, 1, 1, "bn", False),
         ("tile-512x128-acc0-lazy", 512, 128, 2, 1, 13, "acc0", True), ("tile-512x128-acc1-plain", 512, 128, 2, 1, 15, "acc1", False),
         ("tile-512x128-bn-lazy", 512, 128, 3, 1, 13, "bn", True), ("tile-512x256-acc0-plain", 512, 256, 1, 1, 15, "acc0", False),
         ("tile-512x256-acc1-lazy", 512, 256, 2, 1, 13, "acc1", True), ("tile-512x256-bn-lazy", 512, 256, 1, 2, 13, "bn", True)]


@pytest.mark.parametrize("row", DGRAD, ids=[r[0] for r in DGRAD])
def test_conv_bwd_data_alg(row):
    name, Cout, Cin, G, N, H, mode, lazy = row
    rid, seed = "conv_bwd_data_alg[%s]" % name, seed_of(name)
    Pn = N * H * H
    d = ConvDesc(N, H, H, Cin, H, H, Cout, 1, 1, 1, 0, 1, 1 if lazy else 0, 0, G, 4 * Cin if lazy else 0)
    streams = hip.load().adamml_conv_bwd_data_alg_streams(byref(d))
    assert streams == (1 if name.startswith("stream") else 0), rid + ": dispatch probe"
    g = E.rand_bf16(G * Pn, Cout, seed=seed)
    a = E.act_data(G * Pn, Cin, 1, seed + 1)
    vec = E.bn_vectors(G, Cin, seed + 2)
    vf = vec.reshape(-1)
    w_alg = E.rand_bf16(G, Cin, Cout + Cin, scale=math.sqrt(1.0 / Cin), seed=seed + 3)
    epi = A.randn32(G, Cin, seed=seed + 4, scale=0.2)
    base = E.rand_bf16(G * Pn, Cin, seed=seed + 5) if mode == "acc1" else None
    ref, ab, n, extra, k = A.dgrad_alg_ref(g, a, vf if lazy else None, vf[Cin:] if lazy else None, 1 if lazy else 0, 4 * Cin if lazy else 0,
                                           w_alg, epi, G, tile=not streams, base=base)
    gd, ad, vd, wd, ed = GB.frozen(g), GB.frozen(a), GB.frozen(vec), GB.frozen(w_alg), GB.frozen(epi)
    dx = GB.inout(base) if base is not None else nan_bf16(G * Pn, Cin)
    sc, sh = (ptr(vd.reshape(-1)), ptr(vd.reshape(-1)[Cin:])) if lazy else (None, None)
    kern = "alg_stream_kernel" if streams else "conv_gemm tile kernel (CatIn)"
    if mode == "bn":
        # the epilogue of a sole consumer: the mask of the lazily normalised a itself (z_in = a, its BatchNorm vectors, ReLU)
        sums = zstats(G, Cin)
        call("adamml_conv_bwd_data_alg", byref(d), ptr(gd), ptr(ad), sc, sh, ptr(wd), ptr(ed), ptr(dx), 0, ptr(ad), ptr(vd), 1, ptr(sums))
        mask = R.bn_mask(a.reshape(G * Pn, 1, 1, Cin), vec, 1, groups=G).reshape(G * Pn, Cin)
        assert 0.2 < mask.mean().item() < 0.95
        h = dx.cpu()
        r = A.dgrad_alg_check(h, ref * mask, ab * mask, n, extra * mask, k, what=rid)
        sref, sab = R.bn_dgrad_sums_ref(h.double().reshape(G * Pn, 1, 1, Cin), a.reshape(G * Pn, 1, 1, Cin), vec, groups=G)
        r = max(r, E.sums_check(ssum(sums).cpu(), sref, sab, Pn, what=rid + " sums"))
        kern += " + BatchNorm epilogue"
    else:
        call("adamml_conv_bwd_data_alg", byref(d), ptr(gd), ptr(ad), sc, sh, ptr(wd), ptr(ed), ptr(dx), 1 if base is not None else 0,
             None, None, 0, None)
        r = A.dgrad_alg_check(dx.cpu(), ref, ab, n, extra, k, what=rid)
    record(rid, r, kern)


# --------------------------------------------------------------------------------------------------------------------------- lazy_colsum
@pytest.mark.parametrize("name,C,G,P,act,lazy", [("C64-G3-P777-relu", 64, 3, 777, 1, True), ("C24-G1-P1-plain", 24, 1, 1, 0, False),
                                                 ("C256-G2-P33-relu6-shared", 256, 2, 33, 2, True)])
def test_lazy_colsum(name, C, G, P, act, lazy):
    rid, seed = "lazy_colsum[%s]" % name, seed_of(name)
    x = E.act_data(G * P, C, act or 1, seed)
    shared = "shared" in name
    vec = E.bn_vectors(1 if shared else G, C, seed + 1, act or 1)
    vf, gs = vec.reshape(-1), (0 if shared else 4 * C)
    ref, ab, n = A.lazy_colsum_ref(x, vf if lazy else None, vf[C:] if lazy else None, gs, act, G)
    xd, vd, s = GB.frozen(x), GB.frozen(vf), nan_f32(G, C)
    call("adamml_lazy_colsum", ptr(xd), ptr(vd) if lazy else None, ptr(vd[C:]) if lazy else None, gs, act, ptr(s), P, C, G)
    record(rid, A.f32_sum_check(s.cpu(), ref, ab, n, what=rid), "lazy_colsum_kernel")


# ------------------------------------------------------------------------------------------------------------------------------ gemm_f32
SLACK = 64      # NaN floats behind every operand buffer


def lay(values, kind, ld_pad=0, offset=0):
    """values [R, K] float32 -> (device buffer, pointer, row stride, k stride); kind: row (K contiguous), col (R contiguous), bcast (row
    stride 0: every row is values[0]); ld_pad widens the leading dimension, offset shifts the first element (elements)"""
    Rn, K = values.shape
    if kind == "bcast":
        buf = torch.full((offset + K + SLACK,), NAN, dtype=torch.float32)
        buf[offset:offset + K] = values[0]
        sr, sk = 0, 1
    elif kind == "row":
        ld = K + ld_pad
        buf = torch.full((offset + Rn * ld + SLACK,), NAN, dtype=torch.float32)
        buf[offset:offset + Rn * ld].view(Rn, ld)[:, :K] = values
        sr, sk = ld, 1
    else:
        ld = Rn + ld_pad
        buf = torch.full((offset + K * ld + SLACK,), NAN, dtype=torch.float32)
        buf[offset:offset + K * ld].view(K, ld)[:, :Rn] = values.t()
        sr, sk = 1, ld
    d = GB.frozen(buf)
    return d, d.data_ptr() + 4 * offset, sr, sk


def run_gemm(rid, M, N, K, want_mfma, a_kind="row", b_kind="row", a_pad=0, b_pad=0, a_off=0, b_off=0, c_t=False, bias=False, act=0, accumulate=False):
    seed = seed_of(rid)
    a, b = A.randn32(M, K, seed=seed), A.randn32(N, K, seed=seed + 1)
    if a_kind == "bcast":
        a = a[:1].expand(M, K).contiguous()
    bv = A.randn32(N, seed=seed + 2) if bias else None
    c0 = A.randn32(M, N, seed=seed + 3) if accumulate else None
    ref, tol = A.gemm_f32_ref(a, b, bv, act, c0)
    abuf, pa, a_sm, a_sk = lay(a, a_kind, a_pad, a_off)
    bbuf, pb, b_sn, b_sk = lay(b, b_kind, b_pad, b_off)
    assert hip.load().adamml_gemm_f32_uses_mfma(pa, a_sm, a_sk, pb, b_sn, b_sk, K) == int(want_mfma), rid + ": the row does not reach the kernel it names"
    # output with 3 padding columns that must stay NaN; transposed: c[m, n] at n * (M + 3) + m
    ldc = (M if c_t else N) + 3
    cfull = torch.full((N if c_t else M, ldc), NAN, dtype=torch.float32)
    view = cfull[:, :M].t() if c_t else cfull[:, :N]
    if c0 is not None:
        view.copy_(c0)
    cd = GB.inout(cfull)
    bd = GB.frozen(bv) if bias else None
    call("adamml_gemm_f32", pa, a_sm, a_sk, pb, b_sn, b_sk, ptr(cd), 1 if c_t else ldc, ldc if c_t else 1, ptr(bd), act, 1 if accumulate else 0,
         M, N, K)
    GB.check(rid)                                                        # (a test runs several rows: each launch its own check)
    out = cd.cpu()
    h = out[:, :M].t() if c_t else out[:, :N]
    assert torch.isnan(out[:, -3:]).all(), rid + ": wrote outside the strided output"
    record(rid, passed(rid, A.ratio(h, ref, tol)), "gemm_f32_mfma_kernel" if want_mfma else "gemm_f32_kernel")


@pytest.mark.parametrize("K", [0, 3, 15, 16, 20, 63, 64, 65, 128, 2560])
def test_gemm_f32_k_sweep(K):
    """M = 37 and N = 70 are ragged against the 32 x 64 matrix-core tile and the 64 x 64 VALU tile; K on both sides of the 16-deep minimum
    and of the 64-deep step"""
    mf = K >= 16 and K % 4 == 0
    run_gemm("gemm_f32[K%d-M37-N70]" % K, 37, 70, K, mf, bias=True, act=1)
    run_gemm("gemm_f32[K%d-M65-N129-acc]" % K, 65, 129, K, mf, accumulate=True)


# one row on each side of each term of the predicate (K = 20: a 16-deep step and a 4-wide tail; 24 = K + 4 keeps the stride a multiple of 4)
PRED = [("K20-aligned", 20, True, {}), ("K12-below16", 12, False, {}), ("K18-Kmod4", 18, False, {}),
        ("K20-lda24", 20, True, {"a_pad": 4}), ("K20-lda21", 20, False, {"a_pad": 1}),
        ("K20-ldb24", 20, True, {"b_pad": 4}), ("K20-ldb22", 20, False, {"b_pad": 2}),
        ("K20-a+16B", 20, True, {"a_off": 4}), ("K20-a+4B", 20, False, {"a_off": 1}),
        ("K20-b+16B", 20, True, {"b_off": 4}), ("K20-b+8B", 20, False, {"b_off": 2}),
        ("K20-a-transposed", 20, False, {"a_kind": "col"}), ("K20-b-transposed", 20, False, {"b_kind": "col"}),
        ("K64-ab-transposed-ct", 64, False, {"a_kind": "col", "b_kind": "col", "c_t": True, "a_pad": 1}),
        ("K64-c-transposed", 64, True, {"c_t": True}), ("K68-c-transposed-acc", 68, True, {"c_t": True, "accumulate": True, "bias": True}),
        ("K64-a-broadcast", 64, True, {"a_kind": "bcast"}), ("K15-a-broadcast", 15, False, {"a_kind": "bcast"}),
        ("K84-a-broadcast-tail", 84, True, {"a_kind": "bcast", "bias": True})]


@pytest.mark.parametrize("row", PRED, ids=[r[0] for r in PRED])
def test_gemm_f32_predicate(row):
    name, K, mf, kw = row
    run_gemm("gemm_f32[%s]" % name, 37, 70, K, mf, **kw)


@pytest.mark.parametrize("K", [20, 19])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("bias", [False, True])
def test_gemm_f32_epilogues(bias, act, accumulate, K):
    run_gemm("gemm_f32[K%d-bias%d-act%d-acc%d]" % (K, bias, act, accumulate), 33, 65, K, K == 20, bias=bias, act=act, accumulate=accumulate)


# ---------------------------------------------------------------------------------------------------------------------------------- head
# (id, K, T, HW, C, G, act, lazy, keep ("none" / "mask" / "zero-row"), g_rows)
HEAD = [("K1-T1-HW1-C64-G1-plain-nokeep", 1, 1, 1, 64, 1, 0, False, "none", True),
        ("K3-T2-HW49-C64-G3-relu6-zero-row", 3, 2, 49, 64, 3, 2, True, "zero-row", True),
        ("K31-T3-HW49-C2048-G1-relu6-mask", 31, 3, 49, 2048, 1, 2, True, "mask", True),
        ("K400-T4-HW49-C64-G3-none-mask", 400, 4, 49, 64, 3, 0, True, "mask", True),
        ("K1000-T4-HW1-C1280-G1-relu6-nokeep-nogrows", 1000, 4, 1, 1280, 1, 2, True, "none", False),
        ("K3-T1-HW49-C8-G1-plain-mask", 3, 1, 49, 8, 1, 0, False, "mask", False)]


@pytest.mark.parametrize("row", HEAD, ids=[r[0] for r in HEAD])
def test_head(row):
    name, K, T, HW, C, G, act, lazy, keepk, grows = row
    seed = seed_of(name)
    clips = 2 * G
    rows = clips * T
    x = E.act_data(rows * HW, C, act or 1, seed).reshape(rows, HW, C)
    vec = E.bn_vectors(G, C, seed + 1, act or 1)
    vf = vec.reshape(-1)
    keep = None
    if keepk != "none":
        keep = (torch.rand(rows, C, generator=E.gen(seed + 2)) > 0.4).to(torch.uint8)
        if keepk == "zero-row":
            keep[T:2 * T] = 0                                            # every frame of clip 1
    inv_keep = 1.0 / 0.6
    W, bias = A.randn32(K, C, seed=seed + 3, scale=1.0 / math.sqrt(C)), A.randn32(K, seed=seed + 4)
    xd, vd, Wd, bd = GB.frozen(x), GB.frozen(vf), GB.frozen(W), GB.frozen(bias)
    kd = GB.frozen(keep) if keep is not None else None
    feat, logits = nan_f32(rows, C), nan_f32(clips, K)
    call("adamml_head_fwd", ptr(xd), ptr(vd) if lazy else None, ptr(vd[C:]) if lazy else None, 4 * C, act if lazy else 0, ptr(kd), inv_keep, ptr(Wd),
         ptr(bd), ptr(feat), ptr(logits), clips, T, HW, C, K, G)
    fref, ftol = A.head_feat_ref(x, vf if lazy else None, vf[C:] if lazy else None, 4 * C, act if lazy else 0, keep, inv_keep, T, HW, G)
    hf = feat.cpu()
    record("head_fwd.feat[%s]" % name, passed(name, A.ratio(hf, fref, ftol), "feat"), "head_fwd_kernel")
    if keepk == "zero-row":
        assert (hf[T:2 * T] == 0).all()
    lref, ltol = A.head_logits_ref(hf, W, bias, T)
    hl = logits.cpu()
    record("head_fwd.logits[%s]" % name, passed(name, A.ratio(hl, lref, ltol), "logits"), "head_fwd_kernel")
    if keepk == "zero-row":
        assert torch.equal(hl[1], bias), name + ": an all-dropped clip must give the bias"
    # backward
    g = A.randn32(clips, K, seed=seed + 5)
    gd, gx = GB.frozen(g), nan_bf16(rows, HW, C)
    gr = nan_f32(rows, K) if grows else None
    call("adamml_head_bwd", ptr(gd), ptr(kd), inv_keep, ptr(Wd), ptr(gx), ptr(gr), clips, T, HW, C, K)
    xref, xab, k, rref = A.head_bwd_ref(g, keep, inv_keep, W, T, HW)
    record("head_bwd.g_x[%s]" % name, R.check(gx.cpu(), xref, xab, 1, acc=k, what="head_bwd g_x " + name), "head_bwd_kernel")
    if grows:
        record("head_bwd.g_rows[%s]" % name, passed(name, A.ratio(gr.cpu(), rref, A.U32 * rref.abs()), "g_rows"), "head_bwd_kernel")


@pytest.mark.parametrize("rows,cols,accumulate", [(0, 17, 0), (0, 17, 1), (1, 17, 0), (1, 300, 1), (777, 1000, 0), (777, 1000, 1), (4096, 2, 1)])
def test_colsum_f32(rows, cols, accumulate):
    rid = "colsum_f32[rows%d-cols%d-acc%d]" % (rows, cols, accumulate)
    seed = seed_of(rid)
    a, o = A.randn32(max(rows, 1), cols, seed=seed)[:rows], A.randn32(cols, seed=seed + 1)
    ref, tol = A.colsum_ref(a, o if accumulate else None)
    ad = GB.frozen(torch.cat([a.reshape(-1), torch.full((SLACK,), NAN)]))
    out = GB.inout(o) if accumulate else nan_f32(cols)
    call("adamml_colsum_f32", ptr(ad), ptr(out), rows, cols, accumulate)
    record(rid, passed(rid, A.ratio(out.cpu(), ref, tol)), "colsum_f32_kernel")


# ---------------------------------------------------------------------------------------------------------------------------- optimizers
GRID_CAP = 4096 * 256       # grid_for: at most 4096 workgroups of 256 threads; beyond, the grid-stride loop takes a second trip
SGD_CASES = [(mu, nes, first, wd) for mu in (0.0, 0.9) for nes in (0, 1) for first in (1, 0) for wd in (0.0, 5e-4) if not (nes and mu == 0.0)]


def sgd_row(n, mu, nes, first, wd):
    rid = "sgd_step[n%d-mom%g-nesterov%d-first%d-wd%g]" % (n, mu, nes, first, wd)
    seed, lr = seed_of(rid), 0.05
    p, g, mom = A.randn32(n, seed=seed, scale=0.05), A.randn32(n, seed=seed + 1), A.randn32(n, seed=seed + 2)
    out = A.sgd_ref(p, g, mom, lr, mu, wd, nes, first)
    pd, gd = GB.inout(p), GB.frozen(g)
    md = (nan_f32(n) if first else GB.inout(mom)) if mu != 0 else None      # first step: the buffer is written, not read
    call("adamml_sgd_step", ptr(pd), ptr(gd), ptr(md), n, lr, mu, wd, nes, first)
    GB.check(rid)
    r = passed(rid, A.ratio(A.update_of(pd.cpu(), p), *out["upd"]), "update")
    if mu != 0:
        r = max(r, passed(rid, A.ratio(md.cpu(), *out["mom"]), "mom"))
    record(rid, r, "sgd_step_kernel")


@pytest.mark.parametrize("mu,nes,first,wd", SGD_CASES)
@pytest.mark.parametrize("n", [255, 100003])
def test_sgd_step(n, mu, nes, first, wd):
    sgd_row(n, mu, nes, first, wd)


@pytest.mark.parametrize("n", [1, GRID_CAP + 300])
def test_sgd_step_sizes(n):
    sgd_row(n, 0.9, 1, 0, 5e-4)
    sgd_row(n, 0.0, 0, 0, 0.0)


ADAM = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=5e-4)


def adam_row(rid, p, g, m, v, step):
    """one adamml_adam_step from the float32 state (p, m, v) with gradient g -> the new state (CPU tensors)"""
    out = A.adam_ref(p, g, m, v, ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["wd"], step)
    pd, gd, md, vd = GB.inout(p), GB.frozen(g), GB.inout(m), GB.inout(v)
    call("adamml_adam_step", ptr(pd), ptr(gd), ptr(md), ptr(vd), p.numel(), ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["wd"], step)
    GB.check(rid)
    pn, mn, vn = pd.cpu(), md.cpu(), vd.cpu()
    ru = A.ratio(A.update_of(pn, p), *out["upd"])
    rm, rv = A.ratio(mn, *out["m"]), A.ratio(vn, *out["v"])
    print("  %s: update %.3f m %.3f v %.3f of tolerance" % (rid, ru, rm, rv))
    record(rid, max(ru, rm, rv), "adam_step_kernel")
    assert ru <= 1.0 and rm <= 1.0 and rv <= 1.0, "%s: update %.3g, m %.3g, v %.3g of tolerance" % (rid, ru, rm, rv)
    return pn, mn, vn


def test_adam_step_sequence_and_resume():
    """steps 1, 2, 3 from the zero state with a fresh gradient each (the state the kernel wrote is the next step's input), then resumed
    at steps 10 and 1000 from a loaded state; parameters of the size of the update (0.02 against lr = 0.01), so that the rounding of the
    stored parameter does not hide the step"""
    n = 100003
    p, m, v = A.randn32(n, seed=1, scale=0.02), torch.zeros(n), torch.zeros(n)
    p[::17] = 0.0
    for step in (1, 2, 3):
        p, m, v = adam_row("adam_step[n%d-step%d]" % (n, step), p, A.randn32(n, seed=10 + step), m, v, step)
    for step in (10, 1000):
        m, v = A.randn32(n, seed=20 + step, scale=0.3), A.randn32(n, seed=30 + step).abs() * 0.5
        adam_row("adam_step[n%d-resumed-step%d]" % (n, step), p, A.randn32(n, seed=40 + step), m, v, step)


@pytest.mark.parametrize("n", [1, 255, GRID_CAP + 300])
def test_adam_step_sizes(n):
    m, v = A.randn32(n, seed=5, scale=0.3), A.randn32(n, seed=6).abs() * 0.5
    adam_row("adam_step[n%d-step2]" % n, A.randn32(n, seed=4, scale=0.02), A.randn32(n, seed=7), m, v, 2)


# ------------------------------------------------------------------------------------------------------------ policy head, gate, fusion
def e32_rows(rid, hip_t, r64, r32, names):
    """|HIP - ref64| <= 16 E32 per tensor (tests/abi_ref.py); records the worst ratio and notes E32 and the HIP distance of every tensor"""
    worst, parts, bad = 0.0, [], []
    for k in names:
        e32, eh, r = A.e32_ratio(hip_t[k].cpu(), r64[k], r32[k])
        parts.append("%s E32 %.1e HIP %.1e" % (k, e32, eh))
        worst = max(worst, r)
        if r > 1.0:
            bad.append("%s: HIP %.3g, E32 %.3g, ratio %.3g" % (k, eh, e32, r))
    print("  %s: %s" % (rid, "; ".join(parts)))
    return worst, "; ".join(parts), bad


@pytest.mark.parametrize("row", A.POLICY_ROWS, ids=[A.policy_id(r) for r in A.POLICY_ROWS])
def test_policy_head(row):
    M, B, S, dlin = row
    rid, tau = "policy_head[%s]" % A.policy_id(row), A.POLICY_TAU
    op = A.policy_operands(M, B, S, A.policy_seed(row))
    r64, r32 = A.policy_run(op, tau, torch.float64, dlin), A.policy_run(op, tau, torch.float32, dlin)
    dv = {k: (GB.frozen(v) if torch.is_tensor(v) else [GB.frozen(t) for t in v]) for k, v in op.items()}
    H, ld = A.HID, A.FEAT + 2 * M
    w_prev = dv["w_ih"].data_ptr() + 4 * A.FEAT                          # W_ih[:, F:], row stride ld_ih = F + 2 M
    fcw, fcb = hip.ptr_array(dv["fc_w"]), hip.ptr_array(dv["fc_b"])
    out = {"decisions": nan_f32(S, M, B), "logits": nan_f32(S, M, B, 2), "h_all": nan_f32(S + 1, B, H), "c_all": nan_f32(S + 1, B, H),
           "gate_act": nan_f32(S, B, 4 * H), "prev_all": nan_f32(S, B, 2 * M), "ysoft": nan_f32(S, M, B, 2), "d_gates": nan_f32(S, B, 4 * H),
           "d_logits": nan_f32(S, M, B, 2)}
    call("adamml_policy_head_fwd", ptr(dv["gates_x"]), w_prev, ld, ptr(dv["w_hh"]), ptr(dv["b_hh"]), fcw, fcb, ptr(dv["expo"]), tau,
         ptr(out["decisions"]), ptr(out["logits"]), ptr(out["h_all"]), ptr(out["c_all"]), ptr(out["gate_act"]), ptr(out["prev_all"]),
         ptr(out["ysoft"]), S, B, M, H)
    GB.unwritten_ok(out["d_gates"], out["d_logits"])                     # (the backward's outputs: required again below)
    GB.check(rid + " forward")
    GB.written_required(out["d_gates"], out["d_logits"])
    for k in ("c_all", "gate_act", "ysoft"):
        GB.frozen(out[k])                                                # (read-only operands of the backward)
    call("adamml_policy_head_bwd", ptr(dv["d_dec"]), ptr(dv["d_logits_in"]) if dlin else None, w_prev, ld, ptr(dv["w_hh"]), fcw, tau,
         ptr(out["c_all"]), ptr(out["gate_act"]), ptr(out["ysoft"]), ptr(out["d_gates"]), ptr(out["d_logits"]), S, B, M, H)
    worst, note, bad = e32_rows(rid, out, r64, r32, A.POLICY_TENSORS)
    record(rid, worst, "policy_head_fwd_kernel + policy_head_bwd_kernel; " + note)
    A.decision_check(out["decisions"].cpu(), r64["ysoft"], r32["ysoft"], rid)
    assert not bad, rid + ": " + " | ".join(bad)


@pytest.mark.parametrize("rows", [1, 37, 4096])
def test_gumbel_gate(rows):
    rid, tau = "gumbel_gate[rows%d]" % rows, A.POLICY_TAU
    # (one row's two scores cannot measure E32: the rows = 1 launch takes the first row of the 37-row operands, E32 is theirs)
    lg, ex, dd = A.gate_operands(max(rows, 37), seed_of(rid))
    e32_all = A.rel_max(A.gate(lg, ex, torch.tensor(tau))[1], A.gate(lg.double(), ex.double(), A.h32(tau))[1])
    lg, ex, dd = lg[:rows].contiguous(), ex[:rows].contiguous(), dd[:rows].contiguous()
    d64_, y64 = A.gate(lg.double(), ex.double(), A.h32(tau))
    _, y32 = A.gate(lg, ex, torch.tensor(tau))
    ld, ed, dec, ys = GB.frozen(lg), GB.frozen(ex), nan_f32(rows), nan_f32(rows, 2)
    call("adamml_gumbel_gate_fwd", ptr(ld), ptr(ed), tau, ptr(dec), ptr(ys), rows)
    eh = A.rel_max(ys.cpu(), y64)
    worst = eh / (A.E32_FACTOR * e32_all)
    record("gumbel_gate_fwd[rows%d]" % rows, worst, "gumbel_gate_fwd_kernel; ysoft E32 %.1e HIP %.1e" % (e32_all, eh))
    A.decision_check(dec.cpu(), y64, y32.double(), rid, e32=e32_all)
    assert worst <= 1.0, "%s: ysoft HIP %.3g, E32 %.3g" % (rid, eh, e32_all)
    # backward from the float32 ysoft it is given: no transcendental, a counted bound
    ref, tol = A.gate_bwd_ref(dd, y32, tau)
    yd, ddd, dl = GB.frozen(y32.contiguous()), GB.frozen(dd), nan_f32(rows, 2)
    call("adamml_gumbel_gate_bwd", ptr(ddd), ptr(yd), tau, ptr(dl), rows)
    record("gumbel_gate_bwd[rows%d]" % rows, passed(rid, A.ratio(dl.cpu(), ref, tol), "d_logits"), "gumbel_gate_bwd_kernel")


# (id, M, S, B, C, learnable, gated, outputs "all" / "nodx1" (d_x[1] NULL) / "only-dx" (d_decisions, d_lf_part NULL) / "no-dx" (d_x NULL))
FUSION = [("M1-C1-uniform-gated", 1, 3, 5, 1, False, True, "all"), ("M2-C31-uniform-nodec", 2, 3, 5, 31, False, False, "all"),
          ("M3-C400-learn-gated", 3, 3, 5, 400, True, True, "all"), ("M4-C31-learn-gated-nodx1", 4, 2, 3, 31, True, True, "nodx1"),
          ("M4-C400-uniform-gated-S10-B72", 4, 10, 72, 400, False, True, "all"), ("M3-C31-learn-nodec-only-dx", 3, 3, 5, 31, True, False, "only-dx"),
          ("M2-C1-learn-gated-no-dx", 2, 1, 1, 1, True, True, "no-dx")]


@pytest.mark.parametrize("row", FUSION, ids=[r[0] for r in FUSION])
def test_fusion(row):
    name, M, S, B, C, learn, gated, outs = row
    seed = seed_of(name)
    xs = [A.randn32(S * B, C, seed=seed + m) for m in range(M)]
    dec = (torch.rand(S, M, B, generator=E.gen(seed + 5)) > 0.4).float() if gated else None
    lf = (torch.rand(M - 1, generator=E.gen(seed + 6)) * 0.4).float() if learn else None
    g = A.randn32(B, C, seed=seed + 7)
    xd, dd, gd = [GB.frozen(t) for t in xs], GB.frozen(dec) if gated else None, GB.frozen(g)
    lfd = GB.frozen(torch.cat([lf, torch.full((SLACK,), NAN)])) if learn else None
    xp = hip.ptr_array(xd)
    out = nan_f32(B, C)
    call("adamml_fusion_fwd", xp, ptr(dd), ptr(lfd), ptr(out), S, B, C, M)
    record("fusion_fwd[%s]" % name, passed(name, A.ratio(out.cpu(), *A.fusion_fwd_ref(xs, dec, lf, S, B)), "out"), "fusion_fwd_kernel")
    dx = [None if (outs == "no-dx" or (outs == "nodx1" and m == 1)) else nan_f32(S * B, C) for m in range(M)]
    ddec = nan_f32(S, M, B) if outs != "only-dx" else None
    dlf = nan_f32(S * B, M) if outs != "only-dx" else None
    call("adamml_fusion_bwd", xp, ptr(dd), ptr(lfd), ptr(gd), hip.ptr_array(dx) if outs != "no-dx" else None, ptr(ddec), ptr(dlf), S, B, C, M)
    ref = A.fusion_bwd_ref(xs, dec, lf, g, S, B)
    r = 0.0
    for m in range(M):
        if dx[m] is not None:
            r = max(r, passed(name, A.ratio(dx[m].cpu(), ref["d_x"][0][m], ref["d_x"][1][m]), "d_x[%d]" % m))
    if ddec is not None:
        r = max(r, passed(name, A.ratio(ddec.cpu(), *ref["d_dec"]), "d_decisions"), passed(name, A.ratio(dlf.cpu(), *ref["d_lf"]), "d_lf_part"))
    record("fusion_bwd[%s]" % name, r, "fusion_bwd_kernel")


# ------------------------------------------------------------------------------------------------------------------------ input kernels
def floats(v):
    import ctypes
    return (ctypes.c_float * len(v))(*v)


# (id, B, S, C, H, W, OH, OW, frame_step, c_pad, x offset in elements)   F = 8
CLIP = [("nhwc4-C3-6x8-step1", 2, 2, 3, 6, 8, 6, 8, 1, 4, 0), ("nhwc4-C4-6x8-step3", 1, 2, 4, 6, 8, 6, 8, 3, 4, 0), ("nhwc4-C1-6x8-step2", 2, 1, 1, 6, 8, 6, 8, 2, 4, 0),
        ("generic-cpad4-W10", 2, 2, 3, 6, 10, 6, 10, 1, 4, 0), ("generic-cpad4-x+4B", 2, 2, 3, 6, 8, 6, 8, 2, 4, 1),
        ("generic-cpad4-down", 1, 2, 3, 12, 20, 7, 9, 3, 4, 0), ("generic-cpad8-up", 2, 1, 3, 6, 5, 13, 11, 2, 8, 0),
        ("generic-cpad8-C1-noresize", 1, 2, 1, 5, 7, 5, 7, 3, 8, 0), ("generic-cpad16-C4-nonsquare", 1, 1, 4, 9, 14, 12, 6, 1, 16, 0),
        ("generic-cpad8-C4-down-x+4B", 1, 1, 4, 12, 20, 7, 9, 2, 8, 1)]


@pytest.mark.parametrize("row", CLIP, ids=[r[0] for r in CLIP])
def test_clip_to_nhwc(row):
    name, B, S, C, H, W, OH, OW, step, c_pad, off = row
    rid, Fr = "clip_to_nhwc[%s]" % name, 8
    x = A.randn32(B, S * Fr * C, H, W, seed=seed_of(name))
    assert A.taps_stable(H, OH) and A.taps_stable(W, OW), rid + ": a source index depends on the contraction of the coordinate"
    ref, tol = A.clip_ref(x, B, S, Fr, C, OH, OW, step, c_pad)
    buf = GB.frozen(torch.cat([torch.full((off,), NAN), x.reshape(-1), torch.full((SLACK,), NAN)]))
    px = buf.data_ptr() + 4 * off
    y = nan_bf16(*ref.shape)
    four = hip.load().adamml_clip_to_nhwc_four_pixel(px, ptr(y), H, W, OH, OW, c_pad)
    assert four == int(name.startswith("nhwc4")), rid + ": the row does not reach the kernel it names"
    call("adamml_clip_to_nhwc", px, ptr(y), B, S, Fr, C, H, W, OH, OW, step, c_pad)
    record(rid, passed(rid, A.ratio(y.cpu(), ref, tol)), "clip_to_nhwc4_kernel" if four else "clip_to_nhwc_kernel")


def u8_call(x, B, S, Fr, C, H, W, OH, OW, step, c_pad, mean, std, div255, misalign):
    """adamml_clip_u8_to_nhwc on x [B, H, W, S*F*C] uint8 placed `misalign` bytes behind an aligned address"""
    buf = GB.frozen(torch.cat([torch.zeros(misalign, dtype=torch.uint8), x.reshape(-1), torch.zeros(SLACK, dtype=torch.uint8)]))
    Fk = (Fr + step - 1) // step
    y = nan_bf16(S, B * Fk, OH, OW, c_pad)
    call("adamml_clip_u8_to_nhwc", buf.data_ptr() + misalign, ptr(y), B, S, Fr, C, H, W, OH, OW, step, c_pad, floats(mean), floats(std), len(mean), div255)
    GB.check("clip_u8_to_nhwc")                                          # (a row calls this twice: each launch its own check)
    return y.cpu()


RGB_MEAN, RGB_STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


@pytest.mark.parametrize("resize", [False, True])
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("S", [1, 2, 3, 4, 5])
def test_clip_u8_rgb_instances(S, step, resize):
    """each of the 20 instances of clip_u8_rgb_kernel<S, STEP, RESIZE> against float64, and bit for bit against the generic kernel (the same
    call with the source 1 byte off an 8-byte boundary)"""
    rid = "clip_u8_to_nhwc[rgb-S%d-step%d-%s]" % (S, step, "resize" if resize else "noresize")
    B, Fr, C, H, W = 2, 8, 3, 6, 5
    OH, OW = (4, 7) if resize else (H, W)
    c_pad, div255 = (4 if S % 2 else 8), (0 if S == 4 else 1)
    x = torch.randint(0, 256, (B, H, W, S * Fr * C), generator=E.gen(seed_of(rid)), dtype=torch.uint8)
    x[0, 0, 0, :2], x[0, 0, 1, :2] = torch.tensor([0, 255], dtype=torch.uint8), torch.tensor([255, 0], dtype=torch.uint8)
    assert A.taps_stable(H, OH) and A.taps_stable(W, OW)
    mean, std = (RGB_MEAN, RGB_STD) if div255 else ([104.0, 117.0, 128.0], [1.0, 57.0, 58.5])
    ref, tol = A.clip_u8_ref(x, B, S, Fr, C, OH, OW, step, c_pad, mean, std, div255)
    fast = u8_call(x, B, S, Fr, C, H, W, OH, OW, step, c_pad, mean, std, div255, 0)
    record(rid, passed(rid, A.ratio(fast, ref, tol)), "clip_u8_rgb_kernel<%d, %d, %s>" % (S, step, "true" if resize else "false"))
    generic = u8_call(x, B, S, Fr, C, H, W, OH, OW, step, c_pad, mean, std, div255, 1)
    passed(rid, A.ratio(generic, ref, tol), "generic kernel")
    ndiff = int((fast.view(torch.int16) != generic.view(torch.int16)).sum())
    assert ndiff == 0, "%s: the RGB kernel and the generic kernel differ in %d of %d elements (largest difference %.3g)" % (
        rid, ndiff, fast.numel(), (fast.double() - generic.double()).abs().max().item())


# (id, C, n_mean, div255, c_pad, resize)   frame_step 3 on F = 8, S = 2
U8_GENERIC = [("C1-n1-div255-cpad8", 1, 1, 1, 8, False), ("C1-n1-raw-cpad4-resize", 1, 1, 0, 4, True), ("C10-n2-div255-cpad16-resize", 10, 2, 1, 16, True),
              ("C15-n3-raw-cpad16", 15, 3, 0, 16, False), ("C12-n4-div255-cpad16-resize", 12, 4, 1, 16, True), ("C3-n3-div255-cpad8-step3", 3, 3, 1, 8, True)]


@pytest.mark.parametrize("row", U8_GENERIC, ids=[r[0] for r in U8_GENERIC])
def test_clip_u8_generic(row):
    name, C, n, div255, c_pad, resize = row
    rid = "clip_u8_to_nhwc[generic-%s]" % name
    B, S, Fr, H, W, step = 2, 2, 8, 6, 5, 3
    OH, OW = (9, 4) if resize else (H, W)
    x = torch.randint(0, 256, (B, H, W, S * Fr * C), generator=E.gen(seed_of(rid)), dtype=torch.uint8)
    mean = [0.45, 0.4, 0.5, 0.3][:n] if div255 else [110.0, 100.0, 120.0, 90.0][:n]
    std = [0.225, 0.25, 0.2, 0.3][:n] if div255 else [58.0, 60.0, 1.0, 57.0][:n]
    assert A.taps_stable(H, OH) and A.taps_stable(W, OW)
    ref, tol = A.clip_u8_ref(x, B, S, Fr, C, OH, OW, step, c_pad, mean, std, div255)
    record(rid, passed(rid, A.ratio(u8_call(x, B, S, Fr, C, H, W, OH, OW, step, c_pad, mean, std, div255, 0), ref, tol)), "clip_u8_to_nhwc_kernel<false>")


@pytest.mark.parametrize("D,resize,step", [(1, False, 1), (5, True, 2), (5, False, 3)])
def test_clip_u8_rgbdiff(D, resize, step):
    rid = "clip_u8_rgbdiff_to_nhwc[D%d-%s-step%d]" % (D, "resize" if resize else "noresize", step)
    B, S, Fr, H, W = 2, 2, 4, 6, 5
    C, CS = 3 * D, 3 * D + 3
    OH, OW = (4, 7) if resize else (H, W)
    c_pad = 8 if D == 1 else 16
    x = torch.randint(0, 256, (B, H, W, S * Fr * CS), generator=E.gen(seed_of(rid)), dtype=torch.uint8)
    # bytes 0 and 255 next to each other in time: the differences 255 (0 -> 255) and 0 (255 -> 0) at the ends of the quantiser
    x[0, 0, 0, 0], x[0, 0, 0, 3] = 0, 255
    x[0, 0, 1, 1], x[0, 0, 1, 4] = 255, 0
    assert A.taps_stable(H, OH) and A.taps_stable(W, OW)
    ref, tol = A.clip_u8_ref(x, B, S, Fr, C, OH, OW, step, c_pad, RGB_MEAN, RGB_STD, 1, diff=True)
    buf = GB.frozen(torch.cat([x.reshape(-1), torch.zeros(SLACK, dtype=torch.uint8)]))
    y = nan_bf16(*ref.shape)
    call("adamml_clip_u8_rgbdiff_to_nhwc", ptr(buf), ptr(y), B, S, Fr, D, H, W, OH, OW, step, c_pad, floats(RGB_MEAN), floats(RGB_STD), 3)
    record(rid, passed(rid, A.ratio(y.cpu(), ref, tol)), "clip_u8_to_nhwc_kernel<true>")


# -------------------------------------------------------------------------------------------------------------------------------- copy2d
@pytest.mark.parametrize("rows,width,spitch,dpitch", [(1, 64, 64, 64), (96, 512, 1024, 1024), (7, 12, 40, 24), (0, 16, 16, 16), (5, 0, 16, 16)])
def test_copy2d(rows, width, spitch, dpitch):
    """the strided device copy the runtime uses on statistic accumulators: the `width` bytes of every row, and nothing beside them"""
    rid = "copy2d[rows%d-width%d-pitch%d-%d]" % (rows, width, spitch, dpitch)
    n = max(rows, 1)
    src = torch.randint(0, 256, (n, spitch), generator=E.gen(seed_of(rid)), dtype=torch.uint8)
    dst0 = torch.full((n, dpitch), 0xA5, dtype=torch.uint8)
    sd, dd = GB.frozen(src), GB.inout(dst0)
    call("adamml_copy2d", ptr(dd), dpitch, ptr(sd), spitch, width, rows)
    want = dst0.clone()
    want[:rows, :width] = src[:rows, :width]
    assert torch.equal(dd.cpu(), want), rid
    record(rid, 0.0, "hipMemcpy2DAsync")


# ----------------------------------------------------------------------------------------------------------------------------- chain row
@pytest.mark.parametrize("name,Cout,Cin,G,H", [("stream-256x64-G2-P169", 256, 64, 2, 13), ("tile-512x128-G2-P169", 512, 128, 2, 13),
                                               ("stream-256x64-G3-P225", 256, 64, 3, 15)])
def test_alg_chain(name, Cout, Cin, G, H):
    """The algebraic BatchNorm backward composed as adamml_amd/runtime.py _conv1x1_backward_alg composes it (products, alg_sumfix,
    bn_bwd_finalize_affine, alg_pack, conv_bwd_data_alg, alg_wgrad_combine) against the float64 BatchNorm backward of the forward that ran,
    z = bf16(W) a: |h - T| <= the terms first order in W - bf16(W) + the per-kernel models (tests/abi_ref.py chain_model).  The rows file
    records how far the exact-arithmetic composition F is from T, and how much of the model the kernels use."""
    rid, Pn = "alg_chain[%s]" % name, H * H
    op = A.chain_operands(Cout, Cin, G, Pn, seed_of(name))
    d = ConvDesc(1, H, H, Cin, H, H, Cout, 1, 1, 1, 0, 1, 1, 0, G, 4 * Cin)
    streams = hip.load().adamml_conv_bwd_data_alg_streams(byref(d))
    assert streams == (1 if name.startswith("stream") else 0), rid + ": dispatch probe"
    fw, T, Fa, tol_dx, tol_dw, fig = A.chain_model(op, tile=not streams)
    wd, ad, gd, vin, vec, gam = (GB.frozen(op["w"]), GB.frozen(op["a_raw"]), GB.frozen(op["g"]), GB.frozen(op["vin"].reshape(-1)), GB.frozen(fw["vec"]),
                                 GB.frozen(op["gamma"]))
    sc, sh = ptr(vin), ptr(vin[Cin:])
    lib = hip.load()

    def step(what, *outs):
        """each launch of the composition gets its own check; what a kernel wrote is the next kernel's read-only operand"""
        GB.check("%s %s" % (rid, what))
        for t in outs:
            GB.frozen(t)

    # the products: the per-group workspace form, exact / dirty / one float short (refused: the per-group form has no atomic path)
    q = lib.adamml_conv_bwd_weight_workspace(byref(d), Cin)
    (Pm,), _ = workspace_launches(
        GB, q, lambda: (nan_f32(G, Cout, Cin),),
        lambda outs, ws, nbytes: call("adamml_conv_bwd_weight_grouped", byref(d), ptr(gd), None, None, 0, 0, ptr(ad), sc, sh, ptr(outs[0]), Cin, ptr(ws), nbytes),
        "refuse", rid + " products", sync=torch.cuda.synchronize)
    step("products", Pm)
    sums = torch.zeros(G, 2 * Cout, dtype=torch.float64)
    sums[:, :Cout] = fw["g"].sum(1)                                     # (the producer of g' leaves sum(g') and a zero second half)
    sd = GB.inout(E.stats_to_slots(sums, STAT_SLOTS))
    call("adamml_alg_sumfix", ptr(wd), ptr(Pm), ptr(vec), ptr(sd), Cout, Cin, G)
    step("alg_sumfix", sd)
    dgam, dbet, coef, aff = GB.inout(torch.zeros(Cout)), GB.inout(torch.zeros(Cout)), nan_f32(G, 3, Cout), nan_f32(G, 3, Cout)
    call("adamml_bn_bwd_finalize_affine", ptr(sd), STAT_SLOTS, G, float(Pn), ptr(gam), ptr(vec), ptr(dgam), ptr(dbet), ptr(coef), ptr(aff), Cout, 1.0)
    step("bn_bwd_finalize_affine", aff)
    w_alg, epi = nan_bf16(G, Cin, Cout + Cin), nan_f32(G, Cin)
    call("adamml_alg_pack", ptr(wd), ptr(aff), None, ptr(w_alg), ptr(epi), Cout, Cin, G)
    step("alg_pack", w_alg, epi)
    dx = nan_bf16(G * Pn, Cin)
    call("adamml_conv_bwd_data_alg", byref(d), ptr(gd), ptr(ad), sc, sh, ptr(w_alg), ptr(epi), ptr(dx), 0, None, None, 0, None)
    step("conv_bwd_data_alg")
    dG = ConvDesc(1, H, H, Cin, H, H, Cin, 1, 1, 1, 0, 1, 1, 0, G, 4 * Cin)
    qg = lib.adamml_conv_bwd_weight_workspace(byref(dG), Cin)
    (Gm,), _ = workspace_launches(
        GB, qg, lambda: (nan_f32(G, Cin, Cin),),
        lambda outs, ws, nbytes: call("adamml_conv_bwd_weight_grouped", byref(dG), ptr(ad), sc, sh, 1, 4 * Cin, ptr(ad), sc, sh, ptr(outs[0]), Cin, ptr(ws), nbytes),
        "refuse", rid + " Gram", sync=torch.cuda.synchronize)
    step("Gram", Gm)
    sv, dw = nan_f32(G, Cin), GB.inout(torch.zeros(Cout, Cin))
    call("adamml_lazy_colsum", ptr(ad), sc, sh, 4 * Cin, 1, ptr(sv), Pn, Cin, G)
    step("lazy_colsum", sv)
    call("adamml_alg_wgrad_combine", ptr(wd), ptr(aff), ptr(Pm), ptr(Gm), None, ptr(sv), ptr(dw), Cout, Cin, G)
    step("alg_wgrad_combine")
    hx, hw = dx.cpu().double().reshape(G, Pn, Cin), dw.cpu().double()
    rx, rw = A.ratio(hx, T["dx"], tol_dx), A.ratio(hw, T["dw"], tol_dw)
    note = ("F - T (exact arithmetic, fp32 W against bf16 W): dx %.2e, dW %.2e of max; HIP - T: dx %.2e, dW %.2e of max; model at most dx %.2e, dW %.2e of max"
            % (fig["dx"], fig["dw"], A.rel_max(hx, T["dx"]), A.rel_max(hw, T["dw"]), (tol_dx.max() / T["dx"].abs().max()).item(),
               (tol_dw.max() / T["dw"].abs().max()).item()))
    print("  %s: dx %.3f dW %.3f of the model; %s" % (rid, rx, rw, note))
    record(rid + "+dirty", 0.0, "products and Gram matrix bit-identical on a workspace of 0x00")
    record(rid + "+short", 0.0, "workspace_bytes one float short: EINVAL, nothing written")
    record(rid, max(rx, rw), ("alg_stream_kernel" if streams else "conv_gemm tile kernel (CatIn)") + " + the kernels of the composition; " + note)
    assert rx <= 1.0 and rw <= 1.0, "%s: dx %.3g, dW %.3g of the model" % (rid, rx, rw)
