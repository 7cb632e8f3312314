"""float64 references and error models of the BatchNorm, pooling, depthwise and stem kernels (csrc/bn.hip, csrc/pool.hip,
csrc/dwconv_gemm32.hip, csrc/dwconv_bwd_fused.hip, csrc/conv_stem.hip).

Plain CPU module (it never touches torch.cuda): tests/test_elementwise_conformance_gpu.py and tests/test_elementwise_ref_cpu.py import it;
the operand emulation, the checker and the constants are those of tests/conv_ref.py (C_ACC, U32, RHO_*, BIAS_*: the project's values).

Exact operands.  Every reference is built from the values the kernel reads: bf16 tensors widened exactly, float32 vectors as they are,
a lazy read as `lazy_operand` (the fma in float64 rounded once to float32, NaN-propagating clamp).  Which of these kernels round that
value to bf16 (read from the sources):
  * none of them.  The pools compare / add the float32 value (maxpool_fwd_kernel `t > best[i]`, temporal_pool_fwd_kernel
    `__builtin_elementwise_maximum(accv[i], tv)`), gap_fwd_kernel adds it (`acc += transform8(..)`), the depthwise walkers multiply it with
    the float32 tap (dwconv_gemm32.hip xform(): `v[i] = ok ? clamp_act(fmaf(v[i], sc[i], sh[i]), lo, hi) : 0.f`), and every mask is
    mask_act(fmaf(z, scale, shift)) on the float32 pre-activation (strict inequalities, 0 at a bound).  -> round_bf16 = False everywhere.
  * depthwise taps are float32 and are NOT rounded (`wt[t] = *(const f32x4*)(p.w + ..)`); conv_stem1 reads the float32 image and the
    float32 taps unrounded (X1 branch of xform(): `v = ok ? r.f[j] : 0.f`); conv_stem multiplies bf16 x bf16 in the MFMA.

Tolerances: |h - ref| <= rho |ref| + k 2^-24 abs (+ extra), abs = the same expression over the absolute values of its terms, u = 2^-24
one float32 rounding (relative), rho = 2^-8 for a bf16 output.  k is counted from the source line; an expression of r roundings in which
no term passes through more than r of them is bounded by r u abs to first order (the second-order terms are below 2^-40 abs):

  bn_act_add_kernel            `clamp_act(fmaf(v, sc, sh) + fmaf(w, isc, ish), lo, hi)`: fma, fma, add -> k = 3 with a lazy identity;
                               a plain identity has isc = 1, ish = 0 (its fma is exact) -> k = 2; no identity -> k = 1; scale == NULL
                               (sc = 1, sh = 0) one less.  clamp is 1-Lipschitz, so the bound survives it.
                               mask bit = `r > lo && r < hi` on the STORED bf16 value: compared exactly.
  bn_bwd_apply_kernel          `zh = (zv - mu) * is; o = k0 * (gp - k1 - zh * k2)`: sub, mul | mul, sub, sub, mul -> k = 6
                               (gp = g * {0, 1} is exact), abs = |k0| (|g'| + |k1| + |zh k2|).  maxpool_bwd_bn_kernel<APPLY>: same line.
  act_bwd_from_output_kernel,  `gv[i] *= mask_act(ov[i], lo, hi)` then a bf16 rounding of a bf16 value: k = 0, bit-exact.
  residual_bwd_kernel g2
  gap_bwd_kernel               `inv = 1.f / HW; v *= inv`: k = 2.
  gap_fwd_kernel               float32 sum of HW lazy values then `acc * inv`: the summation model, n = HW, rho = RHO_F32.
  temporal_pool_fwd (avg)      `accv + tv` twice (the first add is to 0: exact), `accv *= (1.f / 3.f)`: constant, mul -> k = 4.
  temporal_pool_bwd (avg)      `acc += g * (1.f / 3.f)` for <= 2 windows: constant, mul, add -> k = 3.
  temporal_pool_bwd (max),     a sum of <= 2 (temporal) / <= 4 (2-D) bf16 values in float32 (+ the base when accumulating): k = 1 / 3 / 4
  maxpool_bwd_kernel           (exact unless the exponents are > 16 apart), then the one bf16 rounding.
  max pools forward            y = bf16(max of the float32 values): rounding is monotone -> torch.equal; idx / z_sel / routing: first
                               arg-max of those float32 values in torch's window order (kh, kw ascending, strict >).

  per-channel sums             bn_bwd_reduce_kernel `s += gp; q += gp * (zv - mu) * is`: the `stats_check` model (C_ACC sqrt(n) u abs,
                               n = pixels of the group) + 3 u abs for the sub, mul, mul of every addend of q; rho = 2^-23.
  dwconv_fwd_kernel emit()     nine `acc += r * wt` in float32 of float32 x float32 products: inner product of n <= 9 taps,
                               gamma_n = n u -> k = min(n, C_ACC sqrt(n)) = n, n = the taps inside the image per element.
  dwconv_bwd_data(_s2)_kernel  same (`acc += g * wt` / fma8); accumulate: acc starts from the stored bf16 value (`acc = bf8_to_f32(prev)`),
                               n + 1 terms; the issue's `extra` = rho |conv| term of the conv suite is kept although these kernels do
                               not round the convolution before adding it (it is slack, not a licence).
  dwconv_bwd_weight_kernel     `acc[kw] += g * r0[..]`: float32 output, n = pixels, the conv weight-gradient model (rho = RHO_F32) + 1 u abs
                               for the rounding of every product (bf16 x float32 is not exact in float32).
  dwconv_bwd_fused             mkdz(): `o = fmaf(ca, gv, fmaf(cb, zv, cc)); ob = f32_to_bf4(o)` -- dz IS rounded to bf16 (it is the value the
                               per-layer kernels exchange).  Against float64 A g + B z + C directly this is
                               E = 2^-8 |dz| + 2 u (|A g| + |B z| + |C|) per dz element, carried into dx and dW as `extra` = the same
                               contraction over E and |w| / |a|.
  conv_stem_fwd / _bwd_weight  bf16 MFMA operands: conv_ref's model, n = 7 * 8 * 4 = 224 (the padded reduction) / n = pixels.

  bn_finalize_kernel           fp64 `mu = s1 / count; var = s2 / count - mu * mu` (relative error of var <= 4 * 2^-53 (s2 / count) / var,
                               carried as `f64`), then float32: `is = (float)(1 / sqrt(var + eps))` 1 u; `sc = ga * is` 2 u;
                               `(float)mu` 1 u; `be - (float)mu * sc`: 5 u (|be| + |mu sc|); running statistics, per group in order
                               `(1.f - momentum) * rmean + momentum * (float)mu`: 5 roundings per step on values bounded by
                               A = max(|r0|, max_g |x_g|), errors contract by (1 - momentum) <= 1 -> 5 G u A.
  bn_eval_affine_kernel        `gamma / sqrtf(rv + eps)`: 3 u; `beta - rm * sc`: 5 u (|beta| + |rm sc|).
  bn_bwd_finalize_kernel       `k0 = gamma * is`, `k1 = (float)(sg / count)`, `k2 = ..`: 1 u each; `-k0 * k2 * is`: 4 u;
                               `k0 * (k2 * mu * is - k1)`: 6 u |k0| (|k2 mu is| + |k1|); `dgamma += dg * grad_scale` with
                               `dg += (float)sgz` over the groups in order: (G + 3) u (|base| + |grad_scale| sum_g |sgz_g|).
  bn_bwd_affine_kernel         from the float32 coefficients it reads: `-k0 * k2 * is`: 2 u; `k0 * (k2 * mu * is - k1)`: 4 u |k0| (|k2 mu is| + |k1|);
                               adamml_bn_bwd_finalize_affine must equal finalize then affine bit for bit (torch.equal).
  stats_collapse_kernel        the 32 exact bin values added in fp64: 32 * 2^-53 sum |bin|.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.conv_ref import ACT_BOUNDS, C_ACC, RHO_BF16, RHO_F32, U32, bf16, check, err_ratio, group_vec, lazy_operand, to_nchw, to_nhwc

U64 = 2.0 ** -53
STAT_SLOTS = 32

K_BN_BWD_APPLY = 6
K_GAP_BWD = 2
K_TPOOL_AVG_FWD = 4
K_TPOOL_AVG_BWD = 3
K_TPOOL_MAX_BWD = 1
K_MAXPOOL_BWD = 3
K_REDUCE_TERM = 3
STEM_K = 7 * 8 * 4


def f32(x):
    """float64 -> float32 (one rounding) -> float64"""
    return x.to(torch.float32).double()


def fma32(a, b, c):
    """fmaf on float32-representable float64 tensors (exact product in float64, rounded once; = fmaf up to a double-rounding tie)"""
    return f32(a * b + c)


def lazy_f32(z, scale=None, shift=None, act=0, groups=1, gstride=0):
    """the float32 value clamp(fmaf(z, scale, shift)) these kernels use unrounded (plain z when scale is None)"""
    return lazy_operand(z, scale, shift, act, groups, gstride, round_bf16=False)


def clamp(v, act):
    lo, hi = ACT_BOUNDS[act]
    if lo == -math.inf and hi == math.inf:
        return v
    return torch.clamp(v, min=None if lo == -math.inf else lo, max=None if hi == math.inf else hi)


def act_mask(v, act):
    """mask_act: strict inequalities, 0 at a bound"""
    lo, hi = ACT_BOUNDS[act]
    return ((v > lo) & (v < hi)).double()


def point_check(h, ref, ab, k, what="", bias=None):
    """|h - ref| <= 2^-8 |ref| + k 2^-24 abs, and the rounding bias of a bf16 output of >= 10^4 elements"""
    return check(h, ref, ab, 1, acc=k, what=what, bias=bias)


# ---------------------------------------------------------------------------------------------------------------- BatchNorm, pointwise
def bn_act_add_ref(z, scale, shift, z_gs, act, idn=None, id_scale=None, id_shift=None, id_gs=0, groups=1):
    """z, idn: [groups*P, C] bf16 -> (ref, abs, k)"""
    zz = z.detach().cpu().double()
    C = zz.shape[-1]
    n = zz.shape[0] // groups
    ref, ab = torch.empty_like(zz), torch.empty_like(zz)
    for g in range(groups):
        t = zz[g * n:(g + 1) * n]
        a = t.abs()
        if scale is not None:
            s, b = group_vec(scale, g, z_gs, C), group_vec(shift, g, z_gs, C)
            a = (t * s).abs() + b.abs()
            t = t * s + b
        if idn is not None:
            w = idn.detach().cpu().double()[g * n:(g + 1) * n]
            wa = w.abs()
            if id_scale is not None:
                s, b = group_vec(id_scale, g, id_gs, C), group_vec(id_shift, g, id_gs, C)
                wa = (w * s).abs() + b.abs()
                w = w * s + b
            t, a = t + w, a + wa
        ref[g * n:(g + 1) * n], ab[g * n:(g + 1) * n] = clamp(t, act), a
    k = (1 if scale is not None else 0) + (0 if idn is None else 1 + (1 if id_scale is not None else 0))
    return ref, ab, k


def mask_bits_ref(out, act):
    """bn_act_add_mask: bit (c % 8) of byte (p * C + c) / 8 = act'(STORED out) != 0 -> uint8 [numel / 8]"""
    m = act_mask(out.detach().cpu().double().reshape(-1, 8), act).to(torch.int64)
    return (m << torch.arange(8)).sum(1).to(torch.uint8)


def act_bwd_ref(g_out, out, act):
    """g_out * act'(stored out): exact"""
    return g_out.detach().cpu().double() * act_mask(out.detach().cpu().double(), act)


def bn_bwd_apply_ref(gp, z, vec, coef, groups=1):
    """dz = k0 (g' - k1 - zhat k2) from the masked gradient g' (float64 [groups*P, C]) -> (ref, abs); k = K_BN_BWD_APPLY"""
    zz = z.detach().cpu().double()
    C = zz.shape[-1]
    n = zz.shape[0] // groups
    ref, ab = torch.empty_like(zz), torch.empty_like(zz)
    v = vec.detach().cpu().double().reshape(groups, 4, C)
    cf = coef.detach().cpu().double().reshape(groups, 3, C)
    for g in range(groups):
        zh = (zz[g * n:(g + 1) * n] - v[g, 2]) * v[g, 3]
        f = gp[g * n:(g + 1) * n]
        ref[g * n:(g + 1) * n] = cf[g, 0] * (f - cf[g, 1] - zh * cf[g, 2])
        ab[g * n:(g + 1) * n] = cf[g, 0].abs() * (f.abs() + cf[g, 1].abs() + (zh * cf[g, 2]).abs())
    return ref, ab


def sums_check(got, ref, ab, npix, what="sums"):
    """[G, 2C] BatchNorm-backward sums against float64 sums of the stored operands (the stats_check model + the addend's own roundings)"""
    r = err_ratio(got, ref, ab, npix, 2.0 ** -23, acc=C_ACC * math.sqrt(npix) + K_REDUCE_TERM)
    assert r <= 1.0, "%s: max err/tol %.3g (n = %d)" % (what, r, npix)
    return r


# ---------------------------------------------------------------------------------------------------------- BatchNorm, per-channel vectors
def det_encode_host(values):
    """float64 [...] -> the 32 integer bins of csrc/common.h det_encode (value = f1 + f2 + f3, each float added as det_add does), as the
    float64-typed [..., 32] tensor whose BITS are the int64 bins"""
    r = np.asarray(values.detach().cpu().double().numpy(), dtype=np.float64)
    bins = np.zeros(r.shape + (32,), dtype=np.int64)
    for _ in range(3):
        f = r.astype(np.float32)
        u = f.view(np.uint32).astype(np.int64)
        e, m = (u >> 23) & 0xff, u & 0x7fffff
        m = np.where(e > 0, m | 0x800000, m)
        e = np.where(e > 0, e, 1)
        c = np.where((u >> 31) & 1, -(m << (e & 7)), m << (e & 7))
        np.add.at(bins, tuple(np.indices(r.shape)) + (e >> 3,), c)
        r = r - f.astype(np.float64)
    return torch.from_numpy(bins.view(np.float64).copy())


def det_decode_host(bins):
    """inverse of det_encode_host in exact integer arithmetic -> float64 [...] (the value), and sum |bin values|"""
    b = bins.detach().cpu().numpy().view(np.int64)
    val = np.zeros(b.shape[:-1], dtype=np.float64)
    ab = np.zeros(b.shape[:-1], dtype=np.float64)
    for k in range(31, -1, -1):
        t = np.ldexp(b[..., k].astype(np.float64), 8 * k - 150)
        val, ab = val + t, ab + np.abs(t)
    return torch.from_numpy(val), torch.from_numpy(ab)


def stats_to_slots(s, nslots):
    """[G, 2C] float64 sums -> the accumulator layout a finalize kernel reads: nslots == 1: [G, 1, 2C] plain doubles;
    nslots == STAT_SLOTS: [G, 32, 2C] integer bins"""
    if nslots == 1:
        return s.reshape(s.shape[0], 1, -1).clone()
    return det_encode_host(s).permute(0, 2, 1).contiguous()


def bn_finalize_ref(s, count, gamma, beta, rm, rv, momentum, eps):
    """s: [G, 2C] float64 sums.  -> dict name -> (ref, tol): vec [G, 4, C], rm [C], rv [C] (rm is None: only vec)"""
    s = s.detach().cpu().double()
    G, C = s.shape[0], s.shape[1] // 2
    ga, be = gamma.detach().cpu().double(), beta.detach().cpu().double()
    m = float(np.float32(momentum))
    e = float(np.float32(eps))
    mu = s[:, :C] / count
    ex2 = s[:, C:] / count
    var = torch.clamp(ex2 - mu * mu, min=0.0)
    f64 = 4 * U64 * ex2 / (var + e)                      # relative error of (var + eps) from the fp64 cancellation
    inv = 1.0 / torch.sqrt(var + e)
    sc = ga * inv
    ref = torch.stack([sc, be - mu * sc, mu, inv], 1)
    tol = torch.stack([sc.abs() * (2 * U32 + f64), (5 * U32 + f64) * (be.abs() + (mu * sc).abs()), mu.abs() * U32, inv.abs() * (U32 + f64)], 1)
    out = {"vec": (ref, tol)}
    if rm is not None:
        unb = var * count / (count - 1.0) if count > 1.0 else var
        for name, r0, x, extra in (("rm", rm, mu, 0.0), ("rv", rv, unb, f64 * (var + e))):
            r = r0.detach().cpu().double().clone()
            for g in range(G):
                r = (1.0 - m) * r + m * x[g]
            A = torch.maximum(r0.detach().cpu().double().abs(), x.abs().max(0).values)
            out[name] = (r, 5 * G * U32 * A + (extra.max(0).values if torch.is_tensor(extra) else 0.0))
    return out


def bn_eval_affine_ref(gamma, beta, rm, rv, eps):
    ga, be, rm, rv = (t.detach().cpu().double() for t in (gamma, beta, rm, rv))
    sc = ga / torch.sqrt(rv + float(np.float32(eps)))
    return (sc, 3 * U32 * sc.abs()), (be - rm * sc, 5 * U32 * (be.abs() + (rm * sc).abs()))


def bn_bwd_affine_ref(coef, vec):
    """coef [G, 3, C], vec [G, 4, C] (the float32 values the kernel reads) -> (aff ref [G, 3, C], tol)"""
    cf, v = coef.detach().cpu().double(), vec.detach().cpu().double()
    k0, k1, k2, mu, inv = cf[:, 0], cf[:, 1], cf[:, 2], v[:, 2], v[:, 3]
    ref = torch.stack([k0, -k0 * k2 * inv, k0 * (k2 * mu * inv - k1)], 1)
    tol = torch.stack([torch.zeros_like(k0), 2 * U32 * (k0 * k2 * inv).abs(), 4 * U32 * k0.abs() * ((k2 * mu * inv).abs() + k1.abs())], 1)
    return ref, tol


def bn_bwd_finalize_ref(sums, count, gamma, vec, dgamma0, dbeta0, grad_scale):
    """sums [G, 2C] float64 -> dict: coef, aff [G, 3, C], dgamma, dbeta [C] -> (ref, tol)"""
    s = sums.detach().cpu().double()
    G, C = s.shape[0], s.shape[1] // 2
    ga, v = gamma.detach().cpu().double(), vec.detach().cpu().double().reshape(G, 4, C)
    gs = float(np.float32(grad_scale))
    mu, inv = v[:, 2], v[:, 3]
    k0, k1, k2 = ga * inv, s[:, :C] / count, s[:, C:] / count
    coef = torch.stack([k0, k1, k2], 1)
    aff = torch.stack([k0, -k0 * k2 * inv, k0 * (k2 * mu * inv - k1)], 1)
    aff_tol = torch.stack([k0.abs() * U32, 4 * U32 * (k0 * k2 * inv).abs(), 6 * U32 * k0.abs() * ((k2 * mu * inv).abs() + k1.abs())], 1)
    out = {"coef": (coef, coef.abs() * U32), "aff": (aff, aff_tol)}
    for name, base, x in (("dgamma", dgamma0, s[:, C:]), ("dbeta", dbeta0, s[:, :C])):
        b = base.detach().cpu().double()
        out[name] = (b + gs * x.sum(0), (G + 3) * U32 * (b.abs() + abs(gs) * x.abs().sum(0)))
    return out


def vec_ratio(h, ref, tol):
    """max |h - ref| / tol of a float32 vector output (tol == 0: exact)"""
    err = (h.detach().cpu().double() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    r = err / torch.where(tol > 0, tol, torch.full_like(tol, 1e-300))
    return r.max().item()


# ----------------------------------------------------------------------------------------------------------------------------- pools
def _taps2d(v, OH, OW, fill):
    """v: [N, H, W, C] float64 -> the nine taps [9, N, OH, OW, C] of MaxPool2d(3, 2, 1) in torch's scan order (padding = fill)"""
    N, H, W, C = v.shape
    p = torch.full((N, 2 * OH + 2, 2 * OW + 2, C), fill, dtype=v.dtype)
    p[:, 1:H + 1, 1:W + 1] = v
    return torch.stack([p[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2] for kh in range(3) for kw in range(3)])


def first_argmax(taps, last=False):
    """scan `if (t > best) { best = t; idx = i; }` from best = -inf, idx = 0 -> (best, idx); last: `>=` (the planted defect)"""
    best = torch.full_like(taps[0], -math.inf)
    idx = torch.zeros(taps[0].shape, dtype=torch.int64)
    for i in range(taps.shape[0]):
        upd = (taps[i] >= best) if last else (taps[i] > best)
        best = torch.where(upd, taps[i], best)
        idx = torch.where(upd, torch.full_like(idx, i), idx)
    return best, idx


def maxpool2d_fwd_ref(x, scale, shift, gstride, act, groups=1):
    """x: [groups*N, H, W, C] bf16 -> y (bf16 values, float64), idx (int64 tap 0..8), z_sel (raw x at the arg-max tap)"""
    v = lazy_f32(x, scale, shift, act, groups, gstride)
    H, W = v.shape[1:3]
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    best, idx = first_argmax(_taps2d(v, OH, OW, -math.inf))
    raw = _taps2d(x.detach().cpu().double(), OH, OW, 0.0)
    zsel = torch.gather(raw, 0, idx.unsqueeze(0))[0]
    return bf16(best), idx, zsel


def maxpool2d_route(g, idx, H, W, base=None):
    """float64 sum of the pooled gradients g [N, OH, OW, C] whose recorded tap is the pixel -> (gx [N, H, W, C], abs)"""
    gg = g.detach().cpu().double()
    N, OH, OW, C = gg.shape
    out = torch.zeros(2, N, 2 * OH + 2, 2 * OW + 2, C, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            sel = (idx == kh * 3 + kw).double() * gg
            out[0, :, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2] += sel
            out[1, :, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2] += sel.abs()
    # (a recorded tap is never a padding position: the forward takes -inf there, and tap 0 of an all-(-inf) window does not occur)
    gx, ab = out[0, :, 1:H + 1, 1:W + 1].clone(), out[1, :, 1:H + 1, 1:W + 1].clone()
    if base is not None:
        b = base.detach().cpu().double()
        gx, ab = gx + b, ab + b.abs()
    return gx, ab


def temporal_windows(T):
    To = (T - 1) // 2 + 1
    return To, [[t for t in (2 * to - 1, 2 * to, 2 * to + 1) if 0 <= t < T] for to in range(To)]


def temporal_pool_fwd_ref(x, scale, shift, gstride, act, T, mode, groups=1):
    """x: [groups*NB*T, HW, C] bf16 -> max: (y exact bf16 values, arg [rows, To, HWC] = frame of the first maximum);
    avg (zeros counted, / 3): (ref, abs)"""
    v = lazy_f32(x, scale, shift, act, groups, gstride)
    f = v.reshape(v.shape[0] // T, T, -1)
    To, win = temporal_windows(T)
    if mode == 0:
        ys, args = [], []
        for w in win:
            best, i = first_argmax(torch.stack([f[:, t] for t in w]))
            ys.append(bf16(best))
            args.append(torch.tensor(w)[i])
        return torch.stack(ys, 1), torch.stack(args, 1)
    ref = torch.stack([sum(f[:, t] for t in w) / 3.0 for w in win], 1)
    ab = torch.stack([sum(f[:, t].abs() for t in w) / 3.0 for w in win], 1)
    return ref, ab


def temporal_pool_bwd_ref(g, arg, T, mode):
    """g: [rows*To, HW, C] -> (gx [rows, T, HWC], abs); max: arg from temporal_pool_fwd_ref; avg: arg ignored"""
    To, win = temporal_windows(T)
    gg = g.detach().cpu().double()
    gg = gg.reshape(gg.shape[0] // To, To, -1)
    gx = torch.zeros(gg.shape[0], T, gg.shape[2], dtype=torch.float64)
    ab = torch.zeros_like(gx)
    for to, w in enumerate(win):
        for t in w:
            c = gg[:, to] / 3.0 if mode == 1 else gg[:, to] * (arg[:, to] == t).double()
            gx[:, t] += c
            ab[:, t] += c.abs()
    return gx, ab


def temporal_code_route(g, code, T):
    """adamml_temporal_pool_bwd_code: code [rows*To, HW, C] in {0, 1, 2, 3} = window tap of the first maximum (3: nothing) -> (gx, abs)"""
    To = T // 2
    gg = g.detach().cpu().double()
    gg = gg.reshape(gg.shape[0] // To, To, -1)
    cc = code.reshape(gg.shape)
    gx = torch.zeros(gg.shape[0], T, gg.shape[2], dtype=torch.float64)
    ab = torch.zeros_like(gx)
    for to in range(To):
        for tap in range(3):
            t = 2 * to - 1 + tap
            if 0 <= t < T:
                c = gg[:, to] * (cc[:, to] == tap).double()
                gx[:, t] += c
                ab[:, t] += c.abs()
    return gx, ab


def pack_codes(code):
    """[.., C] int64 in 0..3 -> uint16 per 8 channels (2 bits each), as adamml_conv_fwd_bn_add_tpool stores them"""
    c = code.reshape(-1, 8).to(torch.int64)
    return (c << (2 * torch.arange(8))).sum(1).to(torch.int16)


def gap_fwd_ref(x, scale, shift, gstride, act, N, HW, groups=1):
    v = lazy_f32(x, scale, shift, act, groups, gstride).reshape(groups * N, HW, -1)
    return v.mean(1), v.abs().mean(1), HW


# ------------------------------------------------------------------------------------------------------------------------- depthwise
def _dw(x, w, stride):
    C = w.shape[0]
    return F.conv2d(x, w, stride=stride, padding=1, groups=C)


def dwconv_fwd_ref(a, w, stride):
    """a: float64 NHWC operand (lazy_f32), w: [C, 1, 3, 3] float32 taps (unrounded) -> (ref, abs, ntaps) NHWC"""
    x, ww = to_nchw(a), w.detach().cpu().double()
    ref, ab = _dw(x, ww, stride), _dw(x.abs(), ww.abs(), stride)
    nt = _dw(torch.ones_like(x[:1]), torch.ones_like(ww), stride)
    return to_nhwc(ref), to_nhwc(ab), to_nhwc(nt)


def dwconv_dgrad_ref(g, w, in_hw, stride):
    """g: float64 NHWC [N, OH, OW, C] -> (dx, abs, ntaps) NHWC [N, H, W, C]"""
    gn, ww = to_nchw(g), w.detach().cpu().double()
    C = ww.shape[0]
    size = (gn.shape[0], C, in_hw[0], in_hw[1])

    def tr(a, b):
        return torch.nn.grad.conv2d_input(size, b, a, stride=stride, padding=1, groups=C)
    dx, ab = tr(gn, ww), tr(gn.abs(), ww.abs())
    nt = torch.nn.grad.conv2d_input((1,) + size[1:], torch.ones_like(ww), torch.ones_like(gn[:1]), stride=stride, padding=1, groups=C)
    return to_nhwc(dx), to_nhwc(ab), to_nhwc(nt)


def dwconv_wgrad_ref(a, g, stride):
    """a: float64 NHWC [N, H, W, C] operand, g: float64 NHWC [N, OH, OW, C] -> (dw [C, 1, 3, 3], abs), n = pixels"""
    N, H, W, C = a.shape
    OH, OW = g.shape[1:3]
    p = torch.zeros(N, stride * OH + 3, stride * OW + 3, C, dtype=torch.float64)
    p[:, 1:H + 1, 1:W + 1] = a
    dw, ab = torch.zeros(C, 1, 3, 3, dtype=torch.float64), torch.zeros(C, 1, 3, 3, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            t = p[:, kh:kh + stride * OH:stride, kw:kw + stride * OW:stride] * g
            dw[:, 0, kh, kw], ab[:, 0, kh, kw] = t.sum((0, 1, 2)), t.abs().sum((0, 1, 2))
    return dw, ab, N * OH * OW


def dw_acc(ntaps, extra_terms=0):
    """min(n, C_ACC sqrt(n)) per element, n = taps inside the image (+ the base of an accumulating form)"""
    n = ntaps + extra_terms
    return torch.minimum(n, C_ACC * torch.sqrt(n))


def wgrad_check(h, ref, ab, n, what="", extra=None, products_round=True):
    """float32 weight gradient: the conv weight-gradient model, + 1 u abs when the products themselves round (bf16 x float32)"""
    r = err_ratio(h, ref, ab, n, RHO_F32, extra, acc=C_ACC * math.sqrt(n) + (1 if products_round else 0))
    assert r <= 1.0, "%s: max err/tol %.3g (n = %d)" % (what, r, n)
    return r


def fused_dz_ref(g, z, aff, groups):
    """dz = A g + B z + C in float64 and the bound E of the kernel's own bf16(fmaf(A, g, fmaf(B, z, C))) against it"""
    gg, zz = g.detach().cpu().double(), z.detach().cpu().double()
    C = gg.shape[-1]
    n = gg.shape[0] // groups
    a = aff.detach().cpu().double().reshape(groups, 3, 1, 1, 1, C)
    gg, zz = gg.reshape(groups, n, *gg.shape[1:]), zz.reshape(groups, n, *zz.shape[1:])
    dz = a[:, 0] * gg + a[:, 1] * zz + a[:, 2]
    ab = (a[:, 0] * gg).abs() + (a[:, 1] * zz).abs() + a[:, 2].abs()
    shape = g.shape
    dz, ab = dz.reshape(shape), ab.reshape(shape)
    return dz, RHO_BF16 * dz.abs() + 2 * U32 * ab


# ------------------------------------------------------------------------------------------------------------------------ test data
def gen(seed):
    return torch.Generator().manual_seed(seed)


def rand_bf16(*shape, scale=1.0, offset=0.0, seed=0):
    return (torch.randn(*shape, generator=gen(seed), dtype=torch.float64) * scale + offset).to(torch.bfloat16)


def bn_vectors(groups, c, seed, act=1):
    """[groups][4][c] float32 (scale, shift, mean, invstd); channel 0 has scale 1/2, shift 1: its z = 10 and z = -2 land exactly on the
    bounds 6 and 0 (plant_bounds), as tests/test_conv_conformance_gpu.py lazy_vectors"""
    g = gen(seed)
    v = torch.empty(groups, 4, c)
    v[:, 0] = torch.rand(groups, c, generator=g) + 0.5
    v[:, 1] = torch.randn(groups, c, generator=g) * (1.0 if act == 2 else 0.5)
    v[:, 2] = torch.randn(groups, c, generator=g) * 0.3
    v[:, 3] = torch.rand(groups, c, generator=g) + 0.5
    v[:, 0, 0], v[:, 1, 0] = 0.5, 1.0
    return v


def plant_bounds(x):
    """pre-activations exactly at the clamp bounds in channel 0 (bn_vectors)"""
    flat = x.view(-1, x.shape[-1])
    flat[0::7, 0] = 10.0
    flat[3::7, 0] = -2.0
    return x


def act_data(rows, c, act, seed):
    """[rows, c] bf16 whose pre-activations under bn_vectors cross the bounds of `act`, bound values planted in channel 0"""
    return plant_bounds(rand_bf16(rows, c, scale=3.0 if act == 2 else 1.0, offset=1.0 if act == 2 else 0.0, seed=seed))


SINGLE_TAP = 1.0 + 2.0 ** -9 * (4.0 / 3.0) + 2.0 ** -16


def single_tap_weights(w, channels):
    """depthwise taps [C, 1, 3, 3] with `channels` reduced to the centre tap SINGLE_TAP: times the activation 1.5 the exact product lies
    just above the bf16 midpoint 1.50390625 (-> 1.5078125); a tap rounded to bf16 first (-> 1.0) gives 1.5"""
    w = w.clone()
    for c in channels:
        w[c] = 0.0
        w[c, 0, 1, 1] = SINGLE_TAP
    return w


def single_tap_expected(a, w, stride):
    """the output of the single-tap channels is exactly bf16(float32(a * w_centre)): float64 NHWC (other channels: whatever the formula gives)"""
    v = a[:, ::stride, ::stride]
    return bf16(f32(v * w.detach().cpu().double()[:, 0, 1, 1]))
