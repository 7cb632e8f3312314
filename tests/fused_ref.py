"""float64 references and counted error models of the FUSED 1x1 kernels that carry ResNet-50 layers 1 and 2 in training
(csrc/conv1x1_fadd_stream.hip, conv1x1_fadd_next.hip, res_prod_stream.hip, tpool_bwd_prod.hip, gram.hip, the FADD / RES / DUAL / PF / TP
instances of csrc/conv_gemm.hip and the DUAL instances of csrc/conv1x1_narrow.hip), built on tests/conv_ref.py.

Plain CPU module (it never touches torch.cuda): tests/test_fused_conformance_gpu.py checks the kernels with it, tests/test_fused_ref_cpu.py
anchors every reference to torch and self-tests every model.  It also owns the operand generators of the GPU rows, so that the CPU test
can assert the condition the rows put on their inputs (undecided share <= UNDECIDED_CAP) from the reference alone.

Layout.  Activations are [G, P, C] float64 views of the NHWC bf16 tensors ([groups * N, H, W, C], P = N * H * W pixels per group); the
operand of a conv is `operand()` = conv_ref.lazy_operand: the exact value bf16(clamp(fmaf(x, scale, shift))) the loaders stage.  Weights
are bf16-representable float32 [Cout, Cin], so both packs are exact.

Roundings, read off the kernels (every term of a bound is the output rounding rho |ref|, the accumulation term
C_ACC sqrt(n) 2^-24 abs of conv_ref.tolerance, or one of these, passed as `extra`):

 forward (adamml_conv_fwd_bn_add / _next / _tpool: conv_gemm.hip FADD epilogue, conv1x1_fadd_stream.hip, conv1x1_fadd_next.hip -- one
 expression in all of them):   out = bf16(clamp(fmaf(zb, scale, shift) + fmaf(idn, isc, ish)))   with zb = bf16(z32), z32 the float32 GEMM
   * the GEMM tile is STAGED AS bf16 before the epilogue reads it ("f32_to_bf4(acc)" into LDS): |scale| * 2^-8 * (|z| + its accumulation term);
   * the epilogue's float32 operations, k of them on E = |scale z| + |shift| + |isc idn| + |ish|: the fma of z (1), the fma of a lazy
     identity (1; a plain identity is fmaf(idn, 1, 0) = idn, exact), the addition of the two (1 when there is an identity);
   * the identity is NOT clamped and NOT rounded to bf16 on the way (unlike a conv input): fadd_identity evaluates it in float64;
   * where the GEMM contributes nothing (every product of the element is 0: abs == 0) the remaining expression is a fixed sequence of
     float32 operations on exactly known inputs; the reference evaluates it with the same roundings (as lazy_operand does for the input
     transform) and the element is compared EXACTLY -- that is how pre-activations are planted on the bounds 0 and 6.
   mask_out is computed from the STORED bf16 output (strict inequalities, bit c % 8 of byte c / 8): mask_from_output is exact; against the
   float64 pre-activation an element within its own tolerance of a bound is UNDECIDED and may take either bit, every other must match.
   y_next = W_next . out reads the stored out from LDS: a plain conv of the stored values (conv_ref model, n = Cout), statistics from the
   stored y_next (conv_ref.stats_check).
   The temporal max-pool compares the candidates AFTER their bf16 rounding ("vb[j] = f32_to_bf8(f)", "bf8_to_f32(f32_to_bf8(f))"), first
   maximum in frame order, and stores the winning bf16 value: |pooled - max_t ref_t| <= max_t tol_t, no further rounding; code = window tap
   of the first maximum, 3 when the stored maximum is not > 0.
 residual data gradient (adamml_conv_bwd_data_res[_prod]: conv_gemm.hip RES epilogue, res_prod_stream.hip):
   g' = bf16((bf16(conv32) + dx_in) * m):  the staged tile again (2^-8 (|conv| + its accumulation term)) and ONE float32 addition
   (2^-24 (|conv| + |dx_in|)) when accumulating; without accumulate the staged bf16 value is stored as it is (no extra).  m is exact
   (act'(res_out) with strict inequalities, or the given bit).  sum(g'), sum(g' zhat) are float32 sums over the STORED g'
   (conv_ref.bn_dgrad_sums_ref + elementwise_ref.sums_check: K_REDUCE_TERM roundings per addend).  prod = g'^T a is a float32 MFMA
   accumulation over the pixels of the stored g' and the staged a, per-workgroup partials summed by a second pass: n = P, rho = RHO_F32.
 dual loader (adamml_conv_bwd_data_dual: conv_gemm.hip store_tile DUAL, conv1x1_narrow.hip): dz = bf16(fmaf(A, g, fmaf(B, z, C))): two
   float32 roundings (acc = 2, elementwise_ref.fused_dz_ref); dx is the data gradient of the STORED dz_side with the plain, accumulating
   (dgrad_epi_ref) or BatchNorm-fused (mask exact, no extra) epilogue.
 Gram (gram.hip): float32 MFMA accumulation inside a split of the pixels, the splits summed in float64 and rounded once: n = P,
   rho = RHO_F32, per element; C = 256 mirrors each off-diagonal block pair: G == G^T bitwise.
 gram_stats (conv_alg.hip gram_stats_kernel): float64 throughout (products of a float32 and a bf16 value are exact in float64): at most
   Cin + GRAM_STATS_OPS float64 roundings on |W| |G| |W|^T per output.
 temporal_pool_bwd_code_prod (tpool_bwd_prod.hip): g2 = bf16(sum of at most two routed bf16 gradients): exact in float64, rounded once --
   compared EXACTLY; prod as above over the stored g2.
"""
import math

import numpy as np
import torch

from tests import conv_ref as R
from tests.conv_ref import (C_ACC, RHO_BF16, RHO_F32, U32, ACT_BOUNDS, bf16, lazy_operand, bn_mask, bn_dgrad_sums_ref, tolerance, check,  # noqa: F401
                            stats_check, rounding_bias, group_vec)
from tests import elementwise_ref as E
from tests.elementwise_ref import U64, f32, fma32

UNDECIDED_CAP = 0.01      # largest share of undecided elements a row's inputs may produce
DUAL_OPS = 2             # float32 roundings of the dual loader's fmaf(A, g, fmaf(B, z, C))
GRAM_STATS_OPS = 10       # float64 operations of gram_stats_kernel on top of the Cin additions of a lane: 2 multiplies, 2 pair sums, 6 shuffle adds


def d64(t):
    return t.detach().cpu().double()


def gview(t, groups):
    """NHWC [groups*N, H, W, C] (or [groups*P, C]) -> [G, P, C]"""
    return t.reshape(groups, -1, t.shape[-1])


def ratio(h, ref, tol):
    """max |h - ref| / tol (tol == 0: exact; NaN where ref is finite -> inf)"""
    return E.vec_ratio(h, ref, tol)


def operand(x, scale=None, shift=None, act=0, groups=1, gstride=0):
    """[G, P, C] float64: the staged conv operand bf16(clamp(fmaf(x, scale, shift))) (scale None: x itself)"""
    v = x.reshape(-1, 1, 1, x.shape[-1])
    return gview(lazy_operand(v, scale, shift, act, groups, gstride), groups)


# ------------------------------------------------------------------------------------------------------------------------------ forward
def fadd_identity(idn, id_scale, id_shift, id_gstride, groups):
    """-> (value [G, P, C] in float64, its float32 evaluation fmaf(idn, isc, ish), abs, k = float32 roundings) of the identity operand"""
    w = gview(d64(idn), groups)
    if id_scale is None:
        return w, w.clone(), w.abs(), 0
    C = w.shape[-1]
    val, ab = torch.empty_like(w), torch.empty_like(w)
    for g in range(groups):
        s, t = group_vec(id_scale, g, id_gstride, C), group_vec(id_shift, g, id_gstride, C)
        val[g], ab[g] = w[g] * s + t, (w[g] * s).abs() + t.abs()
    return val, f32(val), ab, 1


def fwd_bn_add_ref(a, w, vec, act, idn=None, id_scale=None, id_shift=None, id_gstride=0):
    """out = act(scale * z + shift + idn'), z = W a.  a: [G, P, Cin] float64 operand; w: [Cout, Cin]; vec: [G, 4, Cout] (scale, shift, ..).
    -> dict: ref (float64 out), ab, n, extra (the four of conv_ref.tolerance), pre (float64 pre-activation), tol / tol_pre (per element,
    0 on the exact elements), exact (bool: abs == 0, ref / pre hold the float32 evaluation), z"""
    G = a.shape[0]
    wd = d64(w)
    v = d64(vec).reshape(G, 4, -1)
    sc, sh = v[:, 0].unsqueeze(1), v[:, 1].unsqueeze(1)
    z, abz = a @ wd.t(), a.abs() @ wd.abs().t()
    n = wd.shape[1]
    t1 = sc * z + sh
    E1 = (sc * z).abs() + sh.abs()
    pre, pre32, k = t1, sh.expand_as(z).clone(), 1
    if idn is not None:
        iv, iv32, iab, ik = fadd_identity(idn, id_scale, id_shift, id_gstride, G)
        pre, pre32, E1, k = t1 + iv, f32(sh + iv32), E1 + iab, k + 1 + ik
    ab = sc.abs() * abz
    zacc = C_ACC * math.sqrt(n) * U32 * abz
    extra = sc.abs() * RHO_BF16 * (z.abs() + zacc) + k * U32 * E1
    exact = abz == 0                                  # fmaf(0, scale, shift) = shift: the epilogue alone, evaluated as the kernel does
    pre = torch.where(exact, pre32, pre)
    ref = E.clamp(pre, act)
    ref = torch.where(exact, bf16(ref), ref)
    zero = torch.zeros_like(ref)
    tol = torch.where(exact, zero, tolerance(ref, ab, n, RHO_BF16, extra))
    tol_pre = torch.where(exact, zero, tolerance(pre, ab, n, RHO_BF16, extra))
    return dict(ref=ref, ab=ab, n=n, extra=extra, pre=pre, tol=tol, tol_pre=tol_pre, exact=exact, z=z)


def act_mask_ref(pre, tol, act):
    """-> (mask = act'(pre) with strict inequalities as conv_ref.bn_mask, undecided = within its own tolerance of a bound; tol == 0
    (exact elements) is always decided)"""
    lo, hi = ACT_BOUNDS[act]
    m = (pre > lo) & (pre < hi)
    und = torch.zeros_like(m)
    for b in (lo, hi):
        if math.isfinite(b):
            und |= ((pre - b).abs() <= tol) & (tol > 0)
    return m, und


def mask_from_output(out, act):
    """the bytes the kernels store: bit (c % 8) of byte (p * C + c) / 8 = act'(STORED out) != 0"""
    return E.mask_bits_ref(out, act)


def unpack_bits(mask, shape):
    """uint8 [numel / 8] -> bool `shape` (bit c % 8 of byte c / 8)"""
    m = mask.detach().cpu().reshape(-1, 1).to(torch.int64)
    return ((m >> torch.arange(8)) & 1).bool().reshape(shape)


def pack_bits(m):
    """bool [..] -> uint8 [numel / 8], the layout of unpack_bits"""
    return (m.reshape(-1, 8).to(torch.int64) << torch.arange(8)).sum(1).to(torch.uint8)


def fadd_check(h, r, act, mask=None, what="", bias=True):
    """stored out h (bf16, any shape with r['ref'].numel() elements) against fwd_bn_add_ref's dict; mask: the stored bytes or None.
    -> (max err / tol, undecided share)"""
    hh = d64(h).reshape(r["ref"].shape)
    q = ratio(hh, r["ref"], r["tol"])
    assert q <= 1.0, "%s: max err/tol %.3g (n = %d)" % (what, q, r["n"])
    if bias and r["ref"].numel() >= R.BIAS_MIN_ELEMENTS:
        b, cnt = rounding_bias(hh, r["ref"], r["ab"], r["n"], r["extra"])
        if cnt >= 1000:
            assert abs(b) <= R.BIAS_LIMIT, "%s: rounding bias %.3f ulp over %d elements" % (what, b, cnt)
    m, und = act_mask_ref(r["pre"], r["tol_pre"], act)
    if mask is not None:
        assert torch.equal(mask.detach().cpu().reshape(-1), mask_from_output(h, act)), what + ": mask_out is not act'(stored out)"
        got = unpack_bits(mask, m.shape)
        bad = (got != m) & ~und
        assert not bad.any(), "%s: %d decided mask bits differ from act'(float64 pre-activation)" % (what, int(bad.sum()))
    return q, und.double().mean().item()


def fwd_bn_add_next_ref(out_stored, w_next, groups):
    """y_next = W_next . out over the STORED block output -> (ref, ab, n) [G, P, next_cout]"""
    o = gview(d64(out_stored), groups)
    wd = d64(w_next)
    return o @ wd.t(), o.abs() @ wd.abs().t(), wd.shape[1]


def pool_windows(T):
    """k3 s2 p1 over T frames: window `to` holds frames 2 to - 1 + k, k = tap 0..2 -> list over to of [(tap, frame)]"""
    return [[(k, 2 * to - 1 + k) for k in range(3) if 0 <= 2 * to - 1 + k < T] for to in range(T // 2)]


def fwd_bn_add_tpool_ref(r, T, dup_of=None):
    """Temporal max pool over the reference block output of fwd_bn_add_ref (rows of P = clips * T frames x Q pixels, frame-major).
    dup_of [T]: frame t is a bit-for-bit copy of frame dup_of[t] <= t (duplicated consecutive frames: exact ties).
    -> dict: ref / tol [G, clips, To, Q, C]; near [G, clips, To, Q, C, 3] (tap within tolerance of the maximum and not a later copy of
    a tap of the same window: the FIRST of an exact tie); must3 / undecided3 (code 3 exactly when the maximum is <= 0, outside the band)"""
    G, P, C = r["ref"].shape
    dup_of = list(range(T)) if dup_of is None else dup_of
    Q = r["Q"]                                                        # pixels per frame: rows are (clip, frame, pixel)
    ref, tol, pre, tolp = (r[k].reshape(G, -1, T, Q, C) for k in ("ref", "tol", "pre", "tol_pre"))
    outs = {k: [] for k in ("ref", "tol", "near", "must3", "und3")}
    for win in pool_windows(T):
        ts = [t for _, t in win]
        rr, tt = ref[:, :, ts], tol[:, :, ts]
        best = rr.max(2).values
        floor = (rr - tt).max(2).values                               # the largest value some tap is certain to reach
        near = torch.zeros(best.shape + (3,), dtype=torch.bool)
        for i, (k, t) in enumerate(win):
            ok = (rr[:, :, i] + tt[:, :, i]) >= floor
            if any(dup_of[t] == dup_of[t2] for _, t2 in win[:i]):        # a copy of an earlier tap can never be the FIRST maximum
                ok = torch.zeros_like(ok)
            for j in range(i):                                           # nor can a tap that an earlier one certainly reaches
                ok = ok & ~((rr[:, :, j] - tt[:, :, j]) >= (rr[:, :, i] + tt[:, :, i]))
            near[..., k] = ok
        mp, mt = pre[:, :, ts].max(2).values, tolp[:, :, ts].max(2).values
        und3 = (mp.abs() <= mt) & (mt > 0)
        outs["ref"].append(best); outs["tol"].append(tt.max(2).values); outs["near"].append(near)
        outs["must3"].append((mp <= 0) & ~und3); outs["und3"].append(und3)
    return {k: torch.stack(v, 2) for k, v in outs.items()}


def unpack_codes(code, shape):
    """uint16 per 8 channels (2 bits each) -> int64 `shape`"""
    c = code.detach().cpu().reshape(-1, 1).to(torch.int64) & 0xffff
    return ((c >> (2 * torch.arange(8))) & 3).reshape(shape)


def tpool_check(pooled, code, p, what=""):
    """pooled [G*clips*To, Q, C] bf16 and code (uint16 words or None) against fwd_bn_add_tpool_ref's dict -> (err / tol, undecided share)"""
    q = ratio(d64(pooled).reshape(p["ref"].shape), p["ref"], p["tol"])
    assert q <= 1.0, "%s: pooled max err/tol %.3g" % (what, q)
    multi = p["near"].sum(-1) > 1
    und = (p["und3"] | (multi & ~p["must3"])).double().mean().item()
    if code is not None:
        c = unpack_codes(code, p["ref"].shape)
        is3 = c == 3
        named = torch.gather(p["near"], -1, c.clamp(max=2).unsqueeze(-1))[..., 0] & ~is3
        ok = torch.where(p["must3"], is3, torch.where(p["und3"], is3 | named, named))
        assert ok.all(), "%s: %d codes name no near-maximal first tap (or 3 / not 3 against the sign of the maximum)" % (what, int((~ok).sum()))
    return q, und


# ----------------------------------------------------------------------------------------------------------------------------- backward
def dgrad_epi_ref(dz, w, base=None, m=None):
    """g' = (W^T dz [+ base]) * m for the STORED dz [G, P, K] (float64), w [K, C] forward weight -> (ref, ab, n, extra, conv)"""
    wd = d64(w)
    conv, ab = dz @ wd, dz.abs() @ wd.abs()
    n = wd.shape[0]
    ref, extra = conv, None
    if base is not None:
        b = d64(base)
        ref = conv + b
        extra = RHO_BF16 * (conv.abs() + C_ACC * math.sqrt(n) * U32 * ab) + U32 * (conv.abs() + b.abs())
    if m is not None:
        ref, ab = ref * m, ab * m
        extra = None if extra is None else extra * m
    return ref, ab, n, extra, conv


def res_mask(res_out=None, bits=None, res_act=1, shape=None):
    """act'(res_out) (strict inequalities, exact on the stored block output) or the given 1-bit mask -> float64 0 / 1"""
    if bits is not None:
        return unpack_bits(bits, shape).double()
    return E.act_mask(d64(res_out).reshape(shape), res_act)


def res_ref(dz, w, m, dx_in=None):
    """adamml_conv_bwd_data_res: dz [G, P, K] float64 (stored bf16 values), w [K, C], m [G, P, C], dx_in [G, P, C] or None"""
    return dgrad_epi_ref(dz, w, dx_in, m)[:4]


def res_sums_check(got, gp_stored, z, vec, groups, what=""):
    """got [G, 2C] (adamml_stats_collapse) against the float64 sums of the STORED g'; z None: sum(g') only and the second half exactly 0"""
    got = d64(got)
    gp = d64(gp_stored)
    C = gp.shape[-1]
    P = gp.numel() // C // groups
    if z is None:
        f = gp.reshape(groups, P, C)
        assert (got[:, C:] == 0).all(), what + ": second moment written without z"
        return E.sums_check(got[:, :C], f.sum(1), f.abs().sum(1), P, what)
    ref, ab = bn_dgrad_sums_ref(gp.reshape(groups * P, 1, 1, C), z.reshape(groups * P, 1, 1, C), vec, groups)
    return E.sums_check(got, ref, ab, P, what)


def res_prod_ref(gp_stored, a):
    """prod[g] = g'^T a: gp_stored [G, P, C] float64 (the stored dx), a [G, P, Ca] operand -> (ref [G, C, Ca], ab, n = P)"""
    return gp_stored.transpose(1, 2) @ a, gp_stored.abs().transpose(1, 2) @ a.abs(), gp_stored.shape[1]


def prod_check(h, ref, ab, n, what=""):
    r = R.err_ratio(h, ref, ab, n, RHO_F32)
    assert r <= 1.0, "%s: max err/tol %.3g per element (n = %d)" % (what, r, n)
    return r


def dual_dz_ref(g, z, aff, groups):
    """dz = A g + B z + C per channel -> (ref, abs) [G, P, C]; the loader's fmaf(A, g, fmaf(B, z, C)) is two float32 roundings: acc = DUAL_OPS"""
    gg, zz = gview(d64(g), groups), gview(d64(z), groups)
    a = d64(aff).reshape(groups, 3, 1, -1)
    return a[:, 0] * gg + a[:, 1] * zz + a[:, 2], (a[:, 0] * gg).abs() + (a[:, 1] * zz).abs() + a[:, 2].abs()


def dual_ref(dz_stored, w, base=None, z_in=None, bn_vec=None, act=0, groups=1):
    """dx of adamml_conv_bwd_data_dual from the STORED dz_side [G, P, K]: plain, accumulating (base) or BatchNorm-fused (z_in, bn_vec, act)"""
    m = None
    if z_in is not None:
        C = z_in.shape[-1]
        m = gview(bn_mask(z_in.reshape(-1, 1, 1, C), bn_vec, act, groups), groups)
    return dgrad_epi_ref(dz_stored, w, None if base is None else gview(d64(base), groups), m)[:4]


def gram_ref(a):
    """a [G, P, C] operand -> (G ref [G, C, C], G abs, s ref [G, C], s abs, n = P)"""
    return a.transpose(1, 2) @ a, a.abs().transpose(1, 2) @ a.abs(), a.sum(1), a.abs().sum(1), a.shape[1]


def gram_check(Gh, sh, a, what=""):
    Gr, Ga, sr, sa, n = gram_ref(a)
    r = max(R.err_ratio(Gh, Gr, Ga, n, RHO_F32), R.err_ratio(sh, sr, sa, n, RHO_F32))
    assert r <= 1.0, "%s: max err/tol %.3g per element (n = %d)" % (what, r, n)
    if a.shape[-1] == 256:
        assert torch.equal(Gh, Gh.transpose(1, 2)), what + ": G != G^T bitwise"
    return r


def gram_stats_ref(w, Gm, s):
    """sums[g] = (W s, diag(W G W^T)) from the float32 G [G, Cin, Cin], s [G, Cin] the kernel is given -> (ref [G, 2 Cout], tol)"""
    wd, Gd, sd = d64(w), d64(Gm), d64(s)
    Cin = wd.shape[1]
    r1, a1 = sd @ wd.t(), sd.abs() @ wd.abs().t()
    r2 = torch.einsum("oi,gij,oj->go", wd, Gd, wd)
    a2 = torch.einsum("oi,gij,oj->go", wd.abs(), Gd.abs(), wd.abs())
    ref, ab = torch.cat([r1, r2], 1), torch.cat([a1, a2], 1)
    return ref, (Cin + GRAM_STATS_OPS) * U64 * ab


def tpool_bwd_code_prod_ref(gy, code, a, T, groups):
    """gy [G*clips*To, Q, C] bf16, code int64 of the same shape in 0..3, a [G, P, Cin] operand (P = clips * T * Q)
    -> (g2 [G, P, C] EXACT bf16 values, prod ref [G, C, Cin], prod abs, n = P)"""
    gx, _ = E.temporal_code_route(gy, code, T)
    C = gy.shape[-1]
    g2 = bf16(gx).reshape(groups, -1, C)                               # (<= two bf16 addends: exact in float64, one rounding)
    ref, ab, n = res_prod_ref(g2, a)
    return g2, ref, ab, n


# -------------------------------------------------------------------------------------------------------------------------------- packs
def pack_ref(w, cin_pad, mode):
    """adamml_pack_conv_weight as an index map: w [Cout, Cin, KH, KW] float32 ->
    mode 0: [Cout][tap][cin_pad] bf16; mode 1: [cin_pad][taps - 1 - tap][Cout] bf16 (padded channels 0); mode 2: [tap][C] float32"""
    wn = w.detach().cpu().numpy()
    co, ci, kh, kw = wn.shape
    taps = kh * kw
    flat = wn.reshape(co, ci, taps)
    if mode == 2:
        return torch.from_numpy(np.ascontiguousarray(flat[:, 0, :].T))
    out = np.zeros((co, taps, cin_pad) if mode == 0 else (cin_pad, taps, co), dtype=np.float32)
    c, i, t = np.meshgrid(np.arange(co), np.arange(ci), np.arange(taps), indexing="ij")
    if mode == 0:
        out[c, t, i] = flat[c, i, t]
    else:
        out[i, taps - 1 - t, c] = flat[c, i, t]
    return torch.from_numpy(out).to(torch.bfloat16)


def pack_table(specs, ptrs, epb):
    """the int64 table of adamml_pack_conv_weights_batched: rows {w, out, cout | cin << 32, cin_pad | kh << 32, kw | mode << 32, first block},
    a tensor of n elements owning ceil(n / epb) blocks -> (rows, total blocks)"""
    rows, blk = [], 0
    for (cout, cin, kh, kw, mode, cp), (pw, po) in zip(specs, ptrs):
        n = kh * kw * cout if mode == 2 else cout * kh * kw * cp
        rows.append([pw, po, cout | ((1 if mode == 2 else cin) << 32), (1 if mode == 2 else cp) | (kh << 32), kw | (mode << 32), blk])
        blk += (n + epb - 1) // epb
    return rows, blk


# -------------------------------------------------------------------------------------------------------------------------------- chain
def chain_reference(row, op, gamma, beta, eps):
    """gram_colsum -> gram_stats -> bn_finalize -> conv_fwd_bn_add against the float64 train-mode act(BN(W a) + idn) of the same bf16
    operands.  The statistics reach the last kernel with the errors of their kernels: eG, es (gram_check's per-element model), carried
    through |W| into sum z and sum z^2 (+ gram_stats_ref's own float64 bound), then to first order
        e_mu = e_s1 / n,  e_var = e_s2 / n + 2 |mu| e_mu,  e_inv = inv^3 e_var / 2,  e_scale = |gamma| e_inv,  e_shift = |mu| e_scale + |scale| e_mu
    on top of the counted bound of adamml_bn_finalize itself (elementwise_ref.bn_finalize_ref).  The output then carries
    |z| e_scale + e_shift as `extra` of fwd_bn_add_ref evaluated at the true vectors.
    -> dict: vec / vec_tol [G, 4, Cout], ref / tol [G, P, Cout]"""
    r0 = fadd_reference(row, dict(op, vec=torch.zeros_like(op["vec"])))
    a, w = r0["a"], d64(op["w"])
    G, P, _ = a.shape
    n = float(P)
    z = a @ w.t()
    s_true = torch.cat([z.sum(1), (z * z).sum(1)], 1)
    (vec, ftol) = E.bn_finalize_ref(s_true, n, gamma, beta, None, None, 0.1, eps)["vec"]
    Gr, Ga, sr, sa, _ = gram_ref(a)
    wacc = C_ACC * math.sqrt(P) * U32
    eG, es = RHO_F32 * Gr.abs() + wacc * Ga, RHO_F32 * sr.abs() + wacc * sa
    _, gst = gram_stats_ref(op["w"], Gr, sr)
    Cout = w.shape[0]
    e_s1 = es @ w.abs().t() + gst[:, :Cout]
    e_s2 = torch.einsum("oi,gij,oj->go", w.abs(), eG, w.abs()) + gst[:, Cout:]
    sc, mu, inv = vec[:, 0], vec[:, 2], vec[:, 3]
    e_mu = e_s1 / n
    e_var = e_s2 / n + 2 * mu.abs() * e_mu
    e_inv = 0.5 * inv ** 3 * e_var
    e_sc = d64(gamma).abs() * e_inv
    e_sh = mu.abs() * e_sc + sc.abs() * e_mu
    vec_tol = ftol + torch.stack([e_sc, e_sh, e_mu, e_inv], 1)
    r = fadd_reference(row, dict(op, vec=vec))
    tol = r["tol"] + r["z"].abs() * vec_tol[:, 0].unsqueeze(1) + vec_tol[:, 1].unsqueeze(1)
    return dict(vec=vec, vec_tol=vec_tol, ref=r["ref"], tol=tol)


# ---------------------------------------------------------------------------------------------------------------------------- generators
def gen(seed):
    return torch.Generator().manual_seed(seed)


def seed_of(rid):
    return sum(map(ord, rid)) % 10007


def weight(cout, cin, seed, zero_rows=0):
    """bf16-representable [cout, cin]; the first zero_rows output channels see no input (the planted channels of fadd_operands)"""
    w = torch.randn(cout, cin, generator=gen(seed), dtype=torch.float64) * (2.0 / cin) ** 0.5
    w[:zero_rows] = 0
    return bf16(w).float()


def vectors(groups, c, seed, spread=0.5, centre=0.0):
    """[groups][4][c] float32 (scale, shift, mean, invstd): scale in +-[0.5, 1.5]"""
    g = gen(seed)
    v = torch.empty(groups, 4, c)
    v[:, 0] = (torch.rand(groups, c, generator=g) + 0.5) * (torch.randint(0, 2, (groups, c), generator=g) * 2 - 1)
    v[:, 1] = torch.randn(groups, c, generator=g) * spread + centre
    v[:, 2] = torch.randn(groups, c, generator=g) * 0.3
    v[:, 3] = torch.rand(groups, c, generator=g) + 0.5
    return v


PLANTED = 3      # output channels 0..2 of a forward row: pre-activation exactly 0 (whole channel), exactly 6 (whole channel), -+ planted via idn


def fadd_operands(row):
    """Operands of a forward row (dict: id, G, P, Cin, Cout, in_act (None: plain input), act, idn in (None, 'plain', 'lazy0', 'lazyg')).
    Output channels 0 and 1 have zero weights and shift 0 / 6 with a zero identity: pre-activation EXACTLY on the bounds; channel 2 has
    shift 1 and (with an identity) idn = -1 / 5 planted every 7th pixel: exactly 0 and 6 again, between ordinary values."""
    rid, G, P, Cin, Cout, act = row["id"], row["G"], row["P"], row["Cin"], row["Cout"], row["act"]
    s = seed_of(rid)
    x = E.rand_bf16(G * P, Cin, scale=1.5, seed=s)
    op = {"x": x, "xvec": None, "in_act": row["in_act"]}
    if row["in_act"] is not None:
        op["xvec"] = E.bn_vectors(G, Cin, s + 1, row["in_act"])
    op["w"] = weight(Cout, Cin, s + 2, PLANTED)
    vec = vectors(G, Cout, s + 3, spread=2.5 if act == 2 else 0.7, centre=2.0 if act == 2 else 0.0)
    vec[:, 1, 0], vec[:, 1, 1], vec[:, 1, 2] = 0.0, 6.0, 1.0
    op["vec"] = vec
    op["idn"] = op["ivec"] = None
    op["id_gstride"] = 0
    if row["idn"] is not None:
        idn = E.rand_bf16(G * P, Cout, scale=row.get("idn_scale", 1.0), seed=s + 4)
        idn[:, :PLANTED] = 0
        idn[0::7, 2], idn[3::7, 2] = -1.0, 5.0
        op["idn"] = idn
        if row["idn"] != "plain":
            gi = G if row["idn"] == "lazyg" else 1
            iv = vectors(gi, Cout, s + 5)
            iv[:, 0, :PLANTED], iv[:, 1, :PLANTED] = 1.0, 0.0
            op["ivec"], op["id_gstride"] = iv, (4 * Cout if row["idn"] == "lazyg" else 0)
    return op


def fadd_reference(row, op):
    G, Cin = row["G"], row["Cin"]
    xv = op["xvec"]
    a = operand(op["x"], None if xv is None else xv.reshape(-1), None if xv is None else xv.reshape(-1)[Cin:], op["in_act"] or 0, G,
                0 if xv is None else 4 * Cin)
    iv = op["ivec"]
    r = fwd_bn_add_ref(a, op["w"], op["vec"], row["act"], op["idn"], None if iv is None else iv.reshape(-1),
                       None if iv is None else iv.reshape(-1)[row["Cout"]:], op["id_gstride"])
    r["a"] = a
    return r


def tpool_operands(row):
    """fadd_operands for a pool row (T frames, clips, Q pixels per frame; act ReLU, identity required): the identity of frame t is scaled
    by a per-frame factor so that the frames of a window are rarely within tolerance of each other; `dup` duplicates consecutive frames
    (x and identity copied: exact ties); output channels >= Cout - 8 get a shift of -40: block output <= 0 everywhere (code 3)"""
    T, clips, Q, G, Cout = row["T"], row["clips"], row["Q"], row["G"], row["Cout"]
    op = fadd_operands(dict(row, P=clips * T * Q, act=1))
    op["vec"][:, 1, Cout - 8:] = -40.0
    fac = torch.tensor([0.3, 1.7, 0.8, 2.6, 0.5, 2.1, 1.2, 3.0])[:T].reshape(1, 1, T, 1, 1)
    idn = op["idn"].float().reshape(G, clips, T, Q, Cout)
    idn[..., PLANTED:] = idn[..., PLANTED:] * fac
    x = op["x"].reshape(G, clips, T, Q, -1).clone()
    dup_of = list(range(T))
    for t in row.get("dup", ()):                       # frame t := frame t - 1
        idn[:, :, t], x[:, :, t] = idn[:, :, t - 1], x[:, :, t - 1]
        dup_of[t] = dup_of[t - 1]
    op["idn"], op["x"], op["dup_of"] = idn.to(torch.bfloat16).reshape(-1, Cout), x.reshape(-1, x.shape[-1]), dup_of
    return op


def tpool_reference(row, op):
    r = fadd_reference(dict(row, P=row["clips"] * row["T"] * row["Q"], act=1), op)
    r["Q"] = row["Q"]
    return r, fwd_bn_add_tpool_ref(r, row["T"], op["dup_of"])


def undecided_share(row):
    """the condition a forward / pool row puts on its inputs, from the reference alone"""
    if "T" in row:
        op = tpool_operands(row)
        r, p = tpool_reference(row, op)
        multi = p["near"].sum(-1) > 1
        pool = (p["und3"] | (multi & ~p["must3"])).double().mean().item()
        return pool
    op = fadd_operands(row)
    r = fadd_reference(row, op)
    return act_mask_ref(r["pre"], r["tol_pre"], row["act"])[1].double().mean().item()


def _frow(rid, G, P, Cin, Cout, in_act, act, idn, **kw):
    return dict(id=rid, G=G, P=P, Cin=Cin, Cout=Cout, in_act=in_act, act=act, idn=idn, **kw)


# adamml_conv_fwd_bn_add: (kernel label in brackets; `stream`: what adamml_conv_fwd_bn_add_streams must answer; env: ADAMML_FADD_STREAM)
FADD_ROWS = [
    # tile kernel (instances: cout tile 64 / 128 -- 128 needs ceil(P / 128) * ceil(Cout / 128) * groups >= 512 --, EID = with an identity,
    # LZF = lazily normalised input; K > 512 with a lazy input: the register-staged loader "reg")
    _frow("tile-96to24-none-noid[conv_gemm_kernel<64,FADD,LZF>]", 1, 399, 96, 24, 0, 0, None, mask=False, stream=0),
    _frow("tile-96to24-relu6-plain-g3[conv_gemm_kernel<64,FADD,EID,LZF>]", 3, 133, 96, 24, 2, 2, "plain", mask=True, stream=0),
    _frow("tile-16to8-relu-lazy0-g5[conv_gemm_kernel<64,FADD,EID>]", 5, 77, 16, 8, None, 1, "lazy0", mask=True, stream=0),
    _frow("tile-64to256-relu-lazyg-g3[conv_gemm_kernel<64,FADD,EID,LZF>]", 3, 1000, 64, 256, 1, 1, "lazyg", mask=True, stream=0),
    _frow("tile-256to512-relu6-noid[conv_gemm_kernel<64,FADD>]", 1, 515, 256, 512, None, 2, None, mask=True, stream=0),
    _frow("tile-64to256-relu-lazyg-g3-wide[conv_gemm_kernel<128,FADD,EID,LZF>]", 3, 11000, 64, 256, 1, 1, "lazyg", mask=True, stream=0),
    _frow("tile-64to256-none-noid-g3-wide[conv_gemm_kernel<128,FADD>]", 3, 11000, 64, 256, None, 0, None, mask=False, stream=0),
    _frow("tile-256to512-relu-lazy0-g5-wide[conv_gemm_kernel<128,FADD,EID>]", 5, 3300, 256, 512, None, 1, "lazy0", mask=True, stream=0),
    _frow("tile-256to512-relu6-noid-g5-wide[conv_gemm_kernel<128,FADD,LZF>]", 5, 3300, 256, 512, 1, 2, None, mask=True, stream=0),
    _frow("tile-520to24-relu-plain[conv_gemm_kernel<64,FADD,reg>]", 1, 333, 520, 24, 1, 1, "plain", mask=True, stream=0),
    _frow("tile-520to256-relu-plain-g3-wide[conv_gemm_kernel<128,FADD,reg>]", 3, 11000, 520, 256, 1, 1, "plain", mask=False, stream=0),
    # the layer-2 shape around the pixel-count threshold of the streaming kernel (4096 per group), both forms against float64
    _frow("l2-P4095-relu-lazyg-g3[conv_gemm_kernel<64,FADD,EID,LZF>]", 3, 4095, 128, 512, 1, 1, "lazyg", mask=True, stream=0),
    _frow("l2-P4096-relu-plain[conv1x1_fadd_stream_kernel<128,8,true>]", 1, 4096, 128, 512, 1, 1, "plain", mask=True, stream=1),
    _frow("l2-P4097-relu6-lazy0-g3[conv1x1_fadd_stream_kernel<128,8,true>]", 3, 4097, 128, 512, 1, 2, "lazy0", mask=True, stream=1),
    _frow("l2-P4097-none-plain-nomask[conv1x1_fadd_stream_kernel<128,8,false>]", 1, 4097, 128, 512, None, 0, "plain", mask=False, stream=1),
    _frow("l2-P4097-relu-noid[conv_gemm_kernel<64,FADD,LZF>]", 1, 4097, 128, 512, 1, 1, None, mask=True, stream=1),
    _frow("l2-P4097-relu-lazyg-g3-streamoff[conv_gemm_kernel<64,FADD,EID,LZF>]", 3, 4097, 128, 512, 1, 1, "lazyg", mask=True, stream=0,
          env={"ADAMML_FADD_STREAM": "0"}),
    _frow("l2-full-P28224-relu-lazyg-g2[conv1x1_fadd_stream_kernel<128,8,true>]", 2, 28224, 128, 512, 1, 1, "lazyg", mask=True, stream=1),
]

# adamml_conv_fwd_bn_add_next (64 -> 256 -> 64): P % 16 != 0, P = 1, groups 1 and 5, the three identity forms, stats_next NULL
NEXT_ROWS = [
    _frow("next-P1-noid[conv1x1_fadd_next_kernel<true,false,true>]", 1, 1, 64, 256, 1, 1, None, mask=True, stats=True),
    _frow("next-P1571-plain-g5[conv1x1_fadd_next_kernel<true,false,true>]", 5, 1571, 64, 256, 1, 1, "plain", mask=True, stats=True),
    _frow("next-P3136-lazyg-g5-nomask[conv1x1_fadd_next_kernel<true,true,false>]", 5, 3136, 64, 256, 1, 1, "lazyg", mask=False, stats=True),
    _frow("next-P845-lazy0-nostats[conv1x1_fadd_next_kernel<true,false,true>]", 1, 845, 64, 256, None, 1, "lazy0", mask=True, stats=False),
    _frow("next-P4099-relu6-plain-g5[conv1x1_fadd_next_kernel<true,false,true>]", 5, 4099, 64, 256, 1, 2, "plain", mask=True, stats=True),
]


def _trow(rid, T, clips, Q, G, Cin, Cout, in_act, idn, probe, slice_mode, code=True, dup=()):
    return dict(id=rid, T=T, clips=clips, Q=Q, G=G, Cin=Cin, Cout=Cout, in_act=in_act, act=1, idn=idn, probe=probe, slice=slice_mode,
                code=code, dup=dup)


# adamml_conv_fwd_bn_add_tpool: probe value (adamml_conv_fwd_bn_add_tpool_streams) under ADAMML_FADD_TPOOL_SLICE = slice
TPOOL_ROWS = [
    _trow("tp-T8-128ch-tile[conv_gemm_kernel<128,FADD,EID,TP8>]", 8, 2, 169, 1, 64, 128, None, "plain", 0, "0", dup=(3, 4)),
    _trow("tp-T4-l2-small-tile[conv_gemm_kernel<128,FADD,EID,LZF,TP4>]", 4, 3, 81, 2, 128, 512, 1, "lazyg", 0, "1"),
    _trow("tp-T2-1024ch-tile[conv_gemm_kernel<128,FADD,EID,LZF,TP2>]", 2, 7, 196, 2, 256, 1024, 1, "plain", 0, "1", dup=(1,)),
    _trow("tp-T8-l1[conv1x1_fadd_tpool_kernel<false,true>]", 8, 2, 169, 2, 64, 256, 1, "plain", 1, "1", dup=(2, 5)),
    _trow("tp-T4-l1-full16[conv1x1_fadd_tpool_kernel<true,true>]", 4, 3, 256, 1, 64, 256, 1, "lazy0", 1, "0"),
    _trow("tp-T2-l1-nocode[conv1x1_fadd_tpool_kernel<false,false>]", 2, 5, 49, 3, 64, 256, None, "plain", 1, "1", code=False, dup=(1,)),
    _trow("tp-T8-l1-slice[conv1x1_fadd_tpool_stream_kernel<64,4,true>]", 8, 3, 196, 1, 64, 256, 1, "plain", 2, "2", dup=(6, 7)),
    _trow("tp-T4-l2-slice[conv1x1_fadd_tpool_stream_kernel<128,8,true>]", 4, 2, 784, 1, 128, 512, 1, "lazyg", 2, "1", dup=(2,)),
    _trow("tp-T2-l2-slice-nocode[conv1x1_fadd_tpool_stream_kernel<128,8,false>]", 2, 3, 777, 1, 128, 512, 1, "plain", 2, "1", code=False),
    _trow("tp-T8-l2-slice-g3[conv1x1_fadd_tpool_stream_kernel<128,8,true>]", 8, 1, 529, 3, 128, 512, None, "lazy0", 2, "1", dup=(1, 2)),
]

FORWARD_ROWS = FADD_ROWS + NEXT_ROWS + TPOOL_ROWS
