"""float64 references and error models of the C-ABI entry points outside the conv / elementwise conformance suites: the algebraic
BatchNorm backward (csrc/conv_alg.hip alg_*_kernel, csrc/conv1x1_stream.hip), adamml_gemm_f32 (csrc/dwconv_gemm32.hip), the classifier
head, adamml_colsum_f32 / adamml_lazy_colsum, the input re-layout kernels and the optimizer steps (csrc/head.hip, bn.hip, clip_input.hip,
param.hip), the policy head, the Gumbel gate and the late fusion (csrc/policy_head.hip).

Plain CPU module (it never touches torch.cuda): tests/test_abi_conformance_gpu.py and tests/test_abi_ref_cpu.py import it; the operand
emulation, the checker and the constants are those of tests/conv_ref.py (check, err_ratio, C_ACC, U32, RHO_*, lazy_operand, bf16) and
tests/elementwise_ref.py (lazy_f32, clamp, vec_ratio; the rows also use its sums_check and det_* bin codecs).

Exact operands.  Every reference is built from the values the kernel reads: bf16 tensors widened exactly, float32 tensors as they are,
hyper-parameters rounded to float32 as the ABI receives them (`h32`).  Where a kernel reads a tensor an earlier kernel of the same row
wrote (head_fwd reads its own `feat`), the reference reads the STORED tensor, so every bound is the bound of one kernel.

Tolerances: |h - ref| <= rho |ref| + k u abs (+ extra), u = 2^-24, abs = the same expression over the absolute values of its terms,
rho = 2^-8 for a bf16 output and 0 for a float32 one whose final rounding is counted in k.  Every float32 accumulation of n terms uses the
project's inner-product model acc(n) = min(n, C_ACC sqrt(n)) (tests/conv_ref.py; the deterministic gamma_n where it is the smaller).
k is counted from the source line (a contracted fma rounds less often than the separate operations counted here, never more):

  alg_pack_kernel              `v = w[k][ci] * A[k]` then `(__bf16)v`: one float32 product, one bf16 rounding -> rho = 2^-8, k = 1.
                               M columns: `a_j = fmaf(w * B, w', a_j)` in four split accumulators, `(a0 + a1) + (a2 + a3)`: an inner product of
                               n = Cout terms whose addends carry one more rounding (`w * B`) -> k = acc(Cout) + 1, then the bf16 rounding.
                               m_pre given: `v = m_pre[(g Cin + ci) Cin + cj]` -> the stored value is exactly bf16(m_pre[g][ci][cj]).
                               epi_add: `acc = fmaf(w, Cc, acc)` over Cout -> k = acc(Cout), float32 (rho = 0).
  alg_wgrad_combine_kernel     `acc += A P + B wg + C s` per group, `dw[e] += acc`: every term passes its product, the two adds of the
                               line, the add into acc of its own and of every later group, and the final add -> k = G + 4 on
                               abs = |dw0| + sum_g |A P| + |B| abs(wg) + |C s|; wg = the split fma inner product over Cin (conv_alg.hip, the w0..w3 loop)
                               adds |B| acc(Cin) u abs(wg) (nothing when wg_pre is given: it is read).
  alg_sumfix_kernel            fp64: `dot += (double)w * (double)P` (products of two float32 are exact in fp64) over Cin, then
                               `r = invstd * (dot - mean * s1)`: Cin - 1 adds, one product, one subtraction, one product ->
                               |r - ref| <= (Cin + 3) 2^-53 |invstd| (|W|.|P| + |mean| |s1|): an ABSOLUTE bound that carries the cancellation
                               of dot against mean * s1; det_encode stores r exactly (three float32 pieces hold 53 bits).
  conv_bwd_data_alg            one GEMM over [g' | a] (bf16 x bf16 exact, float32 accumulation, n = Cout + Cin: conv_ref's model), a = the lazy
                               read rounded to bf16 as the loaders stage it.  CatIn tile path (conv_gemm_kernel's epi_add reads in its epilogue): the tile is staged in
                               LDS as bf16 BEFORE epi_add is added (extra 2^-8 |gemm|), `f += epi_add; v = f32_to_bf8(f)` (the output rounding,
                               1 u for the add), accumulate: `f += y; v = f32_to_bf8(f)` (extra 2^-8 |gemm + epi_add|, 1 u).  Streaming kernel
                               (conv1x1_stream.hip:154-177): `f += s_add` on the float32 accumulator (1 u), accumulate: the tile is rounded
                               first (extra 2^-8 |gemm + epi_add|).  BatchNorm epilogue: the mask multiplies exactly; the sums are those of the
                               STORED g' (tests/conv_ref.py bn_dgrad_sums_ref, tests/elementwise_ref.py sums_check).
  lazy_colsum_kernel           float32 sum over the P pixels of a group of the bf16-rounded lazy operand: acc(P), rho = 2^-22 (conv_ref's
                               float32-output rounding: the row-slot partials are added in a second stage).
  gemm_f32 (both kernels)      `acc = fmaf(a, b, acc)` / v_mfma_f32_16x16x4_f32: float32 products enter the accumulation unrounded, n = K ->
                               acc(K) u abs; `v += bias`, `v += *dst`: one rounding each on (abs + |bias| [+ |c0|]); the clamp is exact and
                               1-Lipschitz.  K = 0: the result is exactly act(bias) (+ c0: one rounding).
  head_fwd_kernel  feat        `acc += transform8(..)` over HW float32 lazy values (not rounded to bf16), `inv = 1.f / HW; v = acc * inv;
                               v * inv_keep`: acc(HW) + 3 (the dropout select is exact).
                   logits      `a = fmaf(f[e], W[..], a)` over lane slices of the T C stored feat values, six shuffle adds, `a / (float)T + bias`:
                               acc(T C) + 2 on abs = |feat|.|W| / T + |bias|.
  head_bwd_kernel  g_x         `acc = fmaf(gk, w, acc)` over K, `sc = 1.f / ((float)T * (float)HW)` (the product is exact below 2^24),
                               `acc * sc`, `v * inv_keep`, bf16: rho = 2^-8, k = acc(K) + 3.
                   g_rows      `g / (float)T`: one rounding, k = 1.
  colsum_f32_kernel            `s += a[r][c]` in row order, `out[c] + s` when accumulating: acc(rows) (+ 1) on sum |a| (+ |out0|).
  sgd_step_kernel              `d = g + wd * p` (2 roundings; exact when wd == 0), `b = momentum * mom + d` (2), `d = d + momentum * b` (2,
                               Nesterov), `p -= lr * d` (product, subtraction).  mom: k = 4 on |g| + |wd p| + |momentum mom|.  The update
                               p_new - p_old: (k_d + 1) u lr abs(d) for the step lr d and its product, + 1 u (|p_old| + lr abs(d)) for the
                               rounding of the stored parameter, k_d = 2 (no momentum), 4 (momentum), 6 (Nesterov).
  adam_step_kernel             `mi = b1 * m + (1.f - b1) * d`: constant, two products, add on top of the 2 of d -> k = 6;
                               `vi = b2 * v + (1.f - b2) * d * d`: d enters twice (2 x 2), constant, two products, add -> k = 8;
                               `denom = sqrtf(vi) / sqrtf(bc2) + eps; p -= (lr / bc1) * mi / denom`: sqrtf is correctly rounded (no fast-math
                               flag in the build) and halves the relative error of vi; roundings sqrt, sqrt, divide, add in denom, divide,
                               product, divide in the step, the float32 roundings of bc1 (1) and of bc2 (1/2 after the square root) as the
                               host passes them -> relative 6 abs(m) / |mi| + 4 abs(v) / vi + K_ADAM_STEP = 9 on the step, + 1 u (|p_old| + |step|).
                               The bias corrections of the REFERENCE are evaluated in float64 from the float32 betas: a host that forms
                               1 - powf(beta2, step) in float32 is off by up to 2^-25 / bc2 = 1.5e-5 in bc2 at step 2 (beta2 = 0.999), half
                               of that in the step: several times K_ADAM_STEP u.
  clip_to_nhwc / clip_u8_*     source index and weights in float32 as the kernel forms them (`resize_taps`; the rows assert that a contracted
                               and an uncontracted evaluation of the coordinate agree on every index), pixel values in float64: the four-tap
                               expression 4 u abs, the normalisation `((t / 255.f) - m) / sd` 3 u (|t / 255| + |m|) / |sd| per tap (2 u without
                               the division by 255), the weights' contraction ambiguity, then the bf16 rounding; padded channels exactly 0
                               (`bilinear_ref`, `u8_values`).  rgbdiff: floor((next - cur + 255) * 0.5) is exact in float32.
  fusion_fwd / fusion_bwd      no transcendental: counted (`fusion_fwd_ref`, `fusion_bwd_ref`, `fuse_weights`); gumbel_gate_bwd too (`gate_bwd_ref`).
  the chain row                the algebraic pieces composed as the runtime composes them, against the float64 BatchNorm backward of the forward
                               that ran (z = bf16(W) a): the terms first order in W - bf16(W) + the per-kernel models carried through the
                               composition; derived in the comment above `chain_operands`.
  policy_head_fwd / _bwd,      depend on the device's expf / logf / tanhf, whose accuracy is not derived here: per tensor, E32 = the distance of
  gumbel_gate_fwd              the SAME computation in float32 on the CPU from float64 (max |x32 - x64| / max |x64|, computed in the row), and
                               the gate is |HIP - x64| <= E32_FACTOR E32 = 16 E32 in the same measure: the factor is for another libm and
                               another summation order over 256-term rows across up to 10 recurrent steps; at E32 ~ 1e-7 the gate is ~600
                               times below the 1e-3 of tests/test_kernels_gpu.py.  Hard decisions: identical wherever the float64 scores
                               differ by more than the bound on them; closer rows are excluded (<= 1 % of a row's decisions,
                               asserted on the CPU for every row's seed) and still must be 0 or 1 to 3e-7.
"""
import math

import numpy as np
import torch

from tests.conv_ref import C_ACC, RHO_BF16, RHO_F32, U32, bf16, check, err_ratio, lazy_operand
from tests.elementwise_ref import U64, clamp, gen, lazy_f32, vec_ratio

K_ADAM_M = 6
K_ADAM_V = 8
K_ADAM_STEP = 9
K_SGD_MOM = 4


def acc(n):
    """coefficient of u abs of a float32 accumulation of n terms: min(n, C_ACC sqrt(n))"""
    return min(float(n), C_ACC * math.sqrt(n)) if n > 0 else 0.0


def h32(x):
    """a float hyper-parameter as the ABI receives it (c_float)"""
    return float(np.float32(x))


def d64(t):
    return t.detach().cpu().double()


def ratio(h, ref, tol):
    """max |h - ref| / tol, elementwise tolerance tensor (tol == 0: exact; NaN in h: inf)"""
    return vec_ratio(h, ref, tol)


# ------------------------------------------------------------------------------------------------------------- algebraic BatchNorm backward
def alg_pack_ref(w, aff, m_pre=None):
    """w [Cout, Cin] float32, aff [G, 3, Cout], m_pre [G, Cin, Cin] or None -> dict:
    wa (ref [G, Cin, Cout], tol), m (ref [G, Cin, Cin], tol; tol == 0 with m_pre: exact), epi (ref [G, Cin], tol)"""
    W, a = d64(w), d64(aff)
    Cout, Cin = W.shape
    A, B, Cc = a[:, 0], a[:, 1], a[:, 2]
    wa = W.t().unsqueeze(0) * A.unsqueeze(1)                                    # [G, Cin, Cout]
    out = {"wa": (wa, (RHO_BF16 + U32) * wa.abs())}
    if m_pre is not None:
        m = bf16(d64(m_pre))
        out["m"] = (m, torch.zeros_like(m))
    else:
        m = torch.einsum("oi,go,oj->gij", W, B, W)
        mab = torch.einsum("oi,go,oj->gij", W.abs(), B.abs(), W.abs())
        out["m"] = (m, RHO_BF16 * m.abs() + (acc(Cout) + 1) * U32 * mab)
    epi = torch.einsum("oi,go->gi", W, Cc)
    eab = torch.einsum("oi,go->gi", W.abs(), Cc.abs())
    out["epi"] = (epi, acc(Cout) * U32 * eab)
    return out


def alg_pack_split(w_alg, Cout):
    """the stored pack [G, Cin, Cout + Cin] -> (wa [G, Cin, Cout], m [G, Cin, Cin])"""
    t = d64(w_alg)
    return t[..., :Cout], t[..., Cout:]


def alg_wgrad_combine_ref(w, aff, P, G=None, wg_pre=None, s=None, dw0=None):
    """dW = dw0 + sum_g A_g (.) P_g + B_g (.) (W G_g) + C_g (x) s_g.  G [g, Cin, Cin] or wg_pre [Cout, g * Cin] -> (ref, tol)"""
    W, a, Pm, sv = d64(w), d64(aff), d64(P), d64(s)
    Cout, Cin = W.shape
    ng = a.shape[0]
    if wg_pre is not None:
        wg = d64(wg_pre).reshape(Cout, ng, Cin).permute(1, 0, 2)
        wg_ab, wg_err = wg.abs(), torch.zeros_like(wg)
    else:
        Gm = d64(G)
        wg = torch.einsum("oj,gji->goi", W, Gm)
        wg_ab = torch.einsum("oj,gji->goi", W.abs(), Gm.abs())
        wg_err = acc(Cin) * U32 * wg_ab
    A, B, Cc = a[:, 0].unsqueeze(2), a[:, 1].unsqueeze(2), a[:, 2].unsqueeze(2)
    base = d64(dw0) if dw0 is not None else torch.zeros_like(W)
    ref = base + (A * Pm + B * wg + Cc * sv.unsqueeze(1)).sum(0)
    ab = base.abs() + ((A * Pm).abs() + B.abs() * wg_ab + (Cc * sv.unsqueeze(1)).abs()).sum(0)
    tol = (ng + 4) * U32 * ab + (B.abs() * wg_err).sum(0)
    return ref, tol


def alg_sumfix_ref(w, P, vec, s1):
    """sum(g' zhat) = invstd (W . P - mean s1) per group and output channel.  vec [G, 4, Cout], s1 [G, Cout] float64 (the decoded first
    halves) -> (ref [G, Cout], tol): the absolute fp64 bound of the module docstring"""
    W, Pm, v, s = d64(w), d64(P), d64(vec), d64(s1)
    Cin = W.shape[1]
    mean, inv = v[:, 2], v[:, 3]
    dot = (W.unsqueeze(0) * Pm).sum(2)
    dab = (W.unsqueeze(0) * Pm).abs().sum(2)
    ref = inv * (dot - mean * s)
    tol = (Cin + 3) * U64 * inv.abs() * (dab + (mean * s).abs())
    return ref, tol


def dgrad_alg_ref(g, a, a_scale, a_shift, a_act, a_gs, w_alg, epi_add, groups, tile, base=None):
    """dx = [g' | a] w_alg^T + epi_add per group from the stored pack.  g [G*P, Cout] bf16, a [G*P, Cin] bf16 (raw, lazy),
    w_alg [G, Cin, Cout + Cin] bf16, epi_add [G, Cin] -> (ref, abs, n, extra, k): check(h, ref, abs, n, extra=extra, acc=C_ACC sqrt(n) + k)"""
    gg = d64(g)
    Cout = gg.shape[-1]
    av = lazy_operand(a.reshape(a.shape[0], 1, 1, -1), a_scale, a_shift, a_act, groups, a_gs).reshape(a.shape[0], -1)
    Cin = av.shape[-1]
    x = torch.cat([gg, av], 1).reshape(groups, -1, Cout + Cin)
    wp, ea = d64(w_alg), d64(epi_add).unsqueeze(1)
    gemm = torch.einsum("gpk,gck->gpc", x, wp)
    gab = torch.einsum("gpk,gck->gpc", x.abs(), wp.abs())
    ref, ab = gemm + ea, gab + ea.abs()
    extra = RHO_BF16 * gemm.abs() if tile else torch.zeros_like(gemm)
    k = 1
    if base is not None:
        b = d64(base).reshape(groups, -1, Cin)
        extra = extra + RHO_BF16 * ref.abs()
        ref, ab, k = ref + b, ab + b.abs(), 2
    shape = (gg.shape[0], Cin)
    return ref.reshape(shape), ab.reshape(shape), Cout + Cin, extra.reshape(shape), k


def dgrad_alg_check(h, ref, ab, n, extra, k, what=""):
    return check(h, ref, ab, n, extra=extra, what=what, acc=C_ACC * math.sqrt(n) + k)


def lazy_colsum_ref(x, scale, shift, gs, act, groups):
    """x [G*P, C] bf16 -> (ref [G, C], abs, n = P) of the bf16-rounded lazy operand"""
    v = lazy_operand(x.reshape(x.shape[0], 1, 1, -1), scale, shift, act, groups, gs).reshape(groups, -1, x.shape[-1])
    return v.sum(1), v.abs().sum(1), v.shape[1]


def f32_sum_check(h, ref, ab, n, what="", extra_k=0):
    """float32 output of an n-term float32 accumulation: rho = 2^-22, acc(n) (+ extra_k counted roundings)"""
    r = err_ratio(h, ref, ab, n, RHO_F32, acc=acc(n) + extra_k)
    assert r <= 1.0, "%s: max err/tol %.3g (n = %d)" % (what, r, n)
    return r


# ----------------------------------------------------------------------------------------------------------------------------- gemm_f32
def gemm_f32_ref(a, b, bias=None, act=0, c0=None):
    """a [M, K], b [N, K] float32 VALUES (however they are laid out) -> (ref [M, N], tol)"""
    A, B = d64(a), d64(b)
    K = A.shape[1]
    ref, ab = A @ B.t(), A.abs() @ B.abs().t()
    tol = acc(K) * U32 * ab
    if bias is not None:
        bb = d64(bias).unsqueeze(0)
        ref, ab = ref + bb, ab + bb.abs()
        tol = tol + U32 * ab
    ref = clamp(ref, act)
    if c0 is not None:
        c = d64(c0)
        ref = ref + c
        tol = tol + U32 * (ab + c.abs())
    return ref, tol


# --------------------------------------------------------------------------------------------------------------------------------- head
def head_feat_ref(x, scale, shift, gs, act, keep, inv_keep, T, HW, groups):
    """x [clips*T, HW, C] bf16 -> (feat ref [clips*T, C], tol)"""
    rows, C = x.shape[0], x.shape[-1]
    v = lazy_f32(x.reshape(rows, HW, 1, C), scale, shift, act, groups, gs).reshape(rows, HW, C)
    ik = h32(inv_keep)
    ref, ab = v.sum(1) / HW, v.abs().sum(1) / HW
    if keep is not None:
        kf = (d64(keep) != 0).double() * ik
        ref, ab = ref * kf, ab * kf.abs()
    return ref, (acc(HW) + 3) * U32 * ab


def head_logits_ref(feat, weight, bias, T):
    """from the STORED feat [clips*T, C] -> (logits ref [clips, K], tol)"""
    f, W = d64(feat), d64(weight)
    C = f.shape[1]
    fs = f.reshape(-1, T, C)
    ref = torch.einsum("ntc,kc->nk", fs, W) / T
    ab = torch.einsum("ntc,kc->nk", fs.abs(), W.abs()) / T
    if bias is not None:
        b = d64(bias).unsqueeze(0)
        ref, ab = ref + b, ab + b.abs()
    return ref, (acc(T * C) + 2) * U32 * ab


def head_bwd_ref(g, keep, inv_keep, weight, T, HW, wrong_scale=False):
    """g [clips, K] -> (g_x ref [clips*T, HW, C], abs, k, g_rows ref [clips*T, K]); wrong_scale: 1 / HW (the planted defect)"""
    gg, W = d64(g), d64(weight)
    K = gg.shape[1]
    sc = 1.0 / HW if wrong_scale else 1.0 / (T * HW)
    row = (gg @ W * sc).repeat_interleave(T, 0)
    rab = (gg.abs() @ W.abs() * sc).repeat_interleave(T, 0)
    if keep is not None:
        kf = (d64(keep) != 0).double() * h32(inv_keep)
        row, rab = row * kf, rab * kf.abs()
    gx = row.unsqueeze(1).expand(-1, HW, -1).contiguous()
    gab = rab.unsqueeze(1).expand(-1, HW, -1).contiguous()
    return gx, gab, acc(K) + 3, (gg / T).repeat_interleave(T, 0)


def colsum_ref(a, out0=None):
    """a [rows, cols] float32 -> (ref [cols], tol)"""
    A = d64(a)
    rows = A.shape[0]
    ref, ab, k = A.sum(0), A.abs().sum(0), acc(rows)
    if out0 is not None:
        o = d64(out0)
        ref, ab, k = ref + o, ab + o.abs(), k + 1
    return ref, k * U32 * ab


# --------------------------------------------------------------------------------------------------------------------------- optimizers
def sgd_ref(p, g, mom, lr, momentum, wd, nesterov, first):
    """one step in float64 from the float32 state -> dict: upd (ref, tol) for p_new - p_old, mom (ref, tol) (momentum != 0)"""
    P, Gr = d64(p), d64(g)
    lr, mu, wd = h32(lr), h32(momentum), h32(wd)
    d = Gr + wd * P
    dab = Gr.abs() + (wd * P).abs()
    kd = 2 if wd != 0.0 else 0
    out = {}
    if mu != 0.0:
        Mo = d64(mom)
        b = d if first else mu * Mo + d
        bab = dab if first else (mu * Mo).abs() + dab
        kb = kd if first else K_SGD_MOM
        out["mom"] = (b, kb * U32 * bab)
        if nesterov:
            d, dab, kd = d + mu * b, dab + abs(mu) * bab, kb + 2
        else:
            d, dab, kd = b, bab, kb
    step = lr * d
    out["upd"] = (-step, (kd + 1) * U32 * abs(lr) * dab + U32 * (P.abs() + abs(lr) * dab))
    return out


def adam_bias_corrections(beta1, beta2, step):
    """float64, from the float32 betas"""
    return 1.0 - h32(beta1) ** step, 1.0 - h32(beta2) ** step


def adam_ref(p, g, m, v, lr, beta1, beta2, eps, wd, step, bc=None):
    """one step in float64 from the float32 state -> dict upd / m / v -> (ref, tol); bc = (bc1, bc2) overrides the bias corrections
    (the CPU self-test plants a wrong one)"""
    P, Gr, M, V = d64(p), d64(g), d64(m), d64(v)
    lr, b1, b2, eps, wd = h32(lr), h32(beta1), h32(beta2), h32(eps), h32(wd)
    bc1, bc2 = bc if bc is not None else adam_bias_corrections(beta1, beta2, step)
    d = Gr + wd * P
    dab = Gr.abs() + (wd * P).abs()
    mi = b1 * M + (1.0 - b1) * d
    mab = (b1 * M).abs() + (1.0 - b1) * dab
    vi = b2 * V + (1.0 - b2) * d * d
    vab = (b2 * V).abs() + (1.0 - b2) * dab * dab
    denom = torch.sqrt(vi) / math.sqrt(bc2) + eps
    c = lr / bc1
    step_ = c * mi / denom
    vrel = torch.where(vi > 0, vab / torch.where(vi > 0, vi, torch.ones_like(vi)), torch.zeros_like(vi))
    tol = U32 * abs(c) / denom * (K_ADAM_M * mab + (0.5 * K_ADAM_V * vrel + K_ADAM_STEP) * mi.abs()) + U32 * (P.abs() + step_.abs())
    return {"upd": (-step_, tol), "m": (mi, K_ADAM_M * U32 * mab), "v": (vi, K_ADAM_V * U32 * vab)}


def update_of(p_new, p_old):
    """p_new - p_old exactly (float64 of two float32)"""
    return d64(p_new) - d64(p_old)


# ------------------------------------------------------------------------------------------------------------------------ test data
def randn32(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=gen(seed), dtype=torch.float64) * scale).float()


def alg_operands(Cout, Cin, G, seed):
    """w [Cout, Cin] (He-scaled float32 master weight), aff [G, 3, Cout] with A in [0.5, 1.5], |B| <= 0.15, |C| <= 0.1"""
    g = gen(seed)
    w = (torch.randn(Cout, Cin, generator=g, dtype=torch.float64) * math.sqrt(2.0 / Cin)).float()
    aff = torch.empty(G, 3, Cout)
    aff[:, 0] = torch.rand(G, Cout, generator=g) + 0.5
    aff[:, 1] = (torch.rand(G, Cout, generator=g) - 0.5) * 0.3
    aff[:, 2] = (torch.rand(G, Cout, generator=g) - 0.5) * 0.2
    return w, aff


# ------------------------------------------------------------------------------------------------------------ policy head, gate, fusion
HID = 256
E32_FACTOR = 16.0        # |HIP - ref64| <= 16 E32: another libm and another summation order over 256-term rows across <= 10 recurrent steps
FEAT = 8                 # feature columns in front of the fed-back logits in W_ih (ld_ih = FEAT + 2 M: w_prev is a strided view)

# (M, B, S, d_logits_in given)
POLICY_ROWS = [(M, B, S, (M + S + B) % 2 == 0) for M in (1, 2, 3, 4) for B in (1, 72) for S in (1, 10)] + [(3, 5, 3, True), (3, 5, 3, False)]


POLICY_TAU = 5.0         # the reference's initial temperature (train_adamml.py)


def policy_seed(row):
    return 1000 + 100 * row[0] + 10 * row[2] + row[1] + (5000 if row[3] else 0)


def policy_id(row):
    return "M%d-B%d-S%d-%s" % (row[0], row[1], row[2], "dlin" if row[3] else "nodlin")


def exponential(shape, g):
    return (-torch.log(torch.rand(*shape, generator=g, dtype=torch.float64).clamp(min=1e-12))).float()


def policy_operands(M, B, S, seed):
    """float32 operands of one policy-head row (nn.LSTMCell / nn.Linear initial scale 1 / sqrt(256))"""
    g = gen(seed)
    u = lambda *s: ((torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) / 16.0).float()      # noqa: E731
    return {"gates_x": torch.randn(S, B, 4 * HID, generator=g, dtype=torch.float64).float(), "w_ih": u(4 * HID, FEAT + 2 * M),
            "w_hh": u(4 * HID, HID), "b_hh": u(4 * HID), "fc_w": [u(2, HID) * 4 for _ in range(M)], "fc_b": [u(2) for _ in range(M)],
            "expo": exponential((S, M, B, 2), g), "d_dec": torch.randn(S, M, B, generator=g, dtype=torch.float64).float(),
            "d_logits_in": torch.randn(S, M, B, 2, generator=g, dtype=torch.float64).float() * 0.5}


def gate(lg, expo, tau):
    """F.gumbel_softmax(logits, tau, hard=True)[..., -1] with the Exponential(1) draw given -> (decision, y_soft)"""
    y = torch.softmax((lg - torch.log(expo)) / tau, -1)
    hard = (y[..., 1] > y[..., 0]).to(y.dtype)                           # ties -> index 0, the first maximum
    return (hard - y[..., 1].detach()) + y[..., 1], y


def policy_run(op, tau, dtype, with_dlin, detach_feedback=False, swap_prev=False):
    """The recurrence of oracle/adamml_oracle.py policy_head (LSTMCell over the segments, previous logits fed back, FC heads, hard Gumbel
    gate) in `dtype`, with the gradients of sum(decisions * d_dec) [+ sum(logits * d_logits_in)] by autograd -> dict of float64 tensors
    in the kernel's layouts.  detach_feedback / swap_prev: the planted defects of the CPU self-test."""
    c = lambda t: t.to(dtype)      # noqa: E731
    gx, w_prev, w_hh, b_hh = c(op["gates_x"]), c(op["w_ih"])[:, FEAT:], c(op["w_hh"]), c(op["b_hh"])
    fw, fb, expo = [c(t) for t in op["fc_w"]], [c(t) for t in op["fc_b"]], c(op["expo"])
    S, B = gx.shape[0], gx.shape[1]
    M = len(fw)
    tau = float(np.float32(tau)) if dtype == torch.float64 else torch.tensor(tau, dtype=dtype)
    h = torch.zeros(B, HID, dtype=dtype)
    cc = torch.zeros(B, HID, dtype=dtype)
    prev = torch.zeros(B, 2 * M, dtype=dtype)
    hs, cs, gates_l, acts, prevs, lgs, ys, decs = [h], [cc], [], [], [], [], [], []
    for s in range(S):
        gates = gx[s] + b_hh + h @ w_hh.t() + prev @ w_prev.t()
        if not gates.requires_grad:
            gates.requires_grad_(True)
        gates.retain_grad()
        gi, gf, gg, go = gates.chunk(4, 1)
        ig, fg, g_, og = torch.sigmoid(gi), torch.sigmoid(gf), torch.tanh(gg), torch.sigmoid(go)
        cc = fg * cc + ig * g_
        h = og * torch.tanh(cc)
        lg = torch.stack([h @ fw[m].t() + fb[m] for m in range(M)], 0)           # [M, B, 2]
        lg.retain_grad()
        d, y = gate(lg, expo[s], tau)
        prevs.append(prev.detach())
        fed = lg.detach() if detach_feedback else lg
        prev = fed.permute(1, 0, 2).reshape(B, 2 * M)
        if swap_prev:
            prev = fed.permute(1, 2, 0).reshape(B, 2 * M)                         # laid out [j][m]
        hs.append(h), cs.append(cc), gates_l.append(gates), acts.append(torch.cat([ig, fg, g_, og], 1)), lgs.append(lg), ys.append(y), decs.append(d)
    loss = sum((d * c(op["d_dec"])[s]).sum() for s, d in enumerate(decs))
    if with_dlin:
        loss = loss + sum((lg * c(op["d_logits_in"])[s]).sum() for s, lg in enumerate(lgs))
    loss.backward()
    st = lambda l: torch.stack([t.detach() for t in l], 0).double()      # noqa: E731
    return {"decisions": st(decs), "logits": st(lgs), "h_all": st(hs), "c_all": st(cs), "gate_act": st(acts), "prev_all": st(prevs),
            "ysoft": st(ys), "d_gates": torch.stack([t.grad for t in gates_l], 0).double(), "d_logits": torch.stack([t.grad for t in lgs], 0).double()}


POLICY_TENSORS = ("logits", "h_all", "c_all", "gate_act", "prev_all", "ysoft", "d_gates", "d_logits")


def rel_max(x, ref):
    """max |x - ref| relative to the tensor's maximum (NaN -> inf); a zero reference: 0 when x is zero too, else inf"""
    x, ref = d64(x), d64(ref)
    err = (x - ref).abs()
    if torch.isnan(err).any():
        return math.inf
    m = ref.abs().max().item() if ref.numel() else 0.0
    e = err.max().item() if err.numel() else 0.0
    return (e / m) if m > 0 else (0.0 if e == 0 else math.inf)


def e32_ratio(h, r64, r32):
    """(E32, HIP distance, HIP distance / (16 E32)) of one tensor"""
    e32, eh = rel_max(r32, r64), rel_max(h, r64)
    return e32, eh, (0.0 if eh == 0 else (eh / (E32_FACTOR * e32) if e32 > 0 else math.inf))


def decided(ys64, ys32, e32=None):
    """mask of the decisions the float64 soft scores settle: |y1 - y0| > bound, bound = 16 E32 max|y|, the bound on the scores (e32: measured
    over a larger operand set than ys32, where that is one row) -> (mask, excluded share)"""
    bound = E32_FACTOR * (rel_max(ys32, ys64) if e32 is None else e32) * ys64.abs().max().item()
    m = (ys64[..., 1] - ys64[..., 0]).abs() > bound
    return m, 1.0 - m.double().mean().item()


def decision_check(dec_h, ys64, ys32, what="", e32=None):
    """decisions identical where decided; every value 0 or 1 to 3e-7 ((hard - y1) + y1 is one rounding away); <= 1 % excluded"""
    m, share = decided(ys64, ys32, e32)
    assert share <= 0.01, "%s: %.2f %% of the decisions are ties of the reference" % (what, 100 * share)
    d = d64(dec_h)
    assert ((d - d.round()).abs() <= 3e-7).all() and ((d.round() == 0) | (d.round() == 1)).all(), what + ": a decision is neither 0 nor 1"
    hard = (ys64[..., 1] > ys64[..., 0]).double()
    assert torch.equal(d.round()[m], hard[m]), what + ": hard decisions differ"
    return share


def gate_operands(rows, seed):
    """logits / draws of the stand-alone gate with very small (1e-30) and very large (80) exponential draws planted"""
    g = gen(seed)
    lg = torch.randn(rows, 2, generator=g, dtype=torch.float64).float() * 2
    ex = exponential((rows, 2), g)
    ex[0::5, 0], ex[1::5, 1], ex[2::5, 0] = 1e-30, 80.0, 80.0
    return lg, ex, torch.randn(rows, generator=g, dtype=torch.float64).float()


def gate_bwd_ref(d_dec, ysoft, tau):
    """gumbel_gate_bwd_kernel from the ysoft it reads (no transcendental): `dot = dy1 * y1; g0 = y0 * (0.f - dot) / tau` 3 roundings,
    `g1 = y1 * (dy1 - dot) / tau` 4 on y1 (|dy1| + |dot|) / tau -> (ref [rows, 2], tol)"""
    y, dy, t = d64(ysoft), d64(d_dec), h32(tau)
    dot = dy * y[:, 1]
    ref = torch.stack([y[:, 0] * (0.0 - dot) / t, y[:, 1] * (dy - dot) / t], 1)
    tol = torch.stack([3 * U32 * ref[:, 0].abs(), 4 * U32 * y[:, 1].abs() * (dy.abs() + dot.abs()) / t], 1)
    return ref, tol


def fuse_weights(lf, M):
    """(w [M] float64, abs error of each): 1.f / M: one rounding; lf[m] as read; the last one 1.f - (lf[0] + ..): M - 1 roundings"""
    if lf is None:
        return torch.full((M,), 1.0 / M, dtype=torch.float64), torch.full((M,), U32 / M, dtype=torch.float64)
    l = d64(lf)
    w = torch.cat([l, (1.0 - l.sum()).reshape(1)])
    err = torch.zeros(M, dtype=torch.float64)
    err[M - 1] = (M - 1) * U32 * (1.0 + l.abs().sum())
    return w, err


def fusion_fwd_ref(xs, dec, lf, S, B):
    """`v += w * (x * d)` over m, `acc += v` over s, `acc / (float)S`: product, product, M adds, S adds, division -> k = M + S + 3 on
    abs = sum |w x d| / S, + the weight's own error.  xs: M tensors [S*B, C], dec [S, M, B] or None -> (ref [B, C], tol)"""
    M, C = len(xs), xs[0].shape[1]
    w, werr = fuse_weights(lf, M)
    x = torch.stack([d64(t).reshape(S, B, C) for t in xs], 1)                         # [S, M, B, C]
    d = d64(dec).unsqueeze(3) if dec is not None else torch.ones(S, M, B, 1, dtype=torch.float64)
    ref = (w.reshape(1, M, 1, 1) * x * d).sum((0, 1)) / S
    ab = (w.abs().reshape(1, M, 1, 1) * (x * d).abs()).sum((0, 1)) / S
    return ref, (M + S + 3) * U32 * ab + (werr.reshape(1, M, 1, 1) * (x * d).abs()).sum((0, 1)) / S


def fusion_bwd_ref(xs, dec, lf, g, S, B):
    """`gv = g * inv_s` (inv_s = 1.f / S: 2 roundings), `dx = gv * w * d` (2 more) -> k = 4; `dot += gv * xv` over lane slices of C and a
    butterfly: acc(C) + 3 (gv, the product), `w * dot` / `d * dot` one more -> dict d_x [M][S*B, C], d_dec [S, M, B], d_lf [S*B, M] -> (ref, tol)"""
    M, C = len(xs), xs[0].shape[1]
    w, werr = fuse_weights(lf, M)
    x = torch.stack([d64(t).reshape(S, B, C) for t in xs], 1)
    d = d64(dec) if dec is not None else torch.ones(S, M, B, dtype=torch.float64)
    gv = d64(g).reshape(1, 1, B, C) / S
    dx = gv * w.reshape(1, M, 1, 1) * d.unsqueeze(3)
    dx_tol = 4 * U32 * dx.abs() + werr.reshape(1, M, 1, 1) * (gv * d.unsqueeze(3)).abs()
    dot, dab = (gv * x).sum(3), (gv * x).abs().sum(3)                                  # [S, M, B]
    kd = acc(C) + 3
    wv, we = w.reshape(1, M, 1), werr.reshape(1, M, 1)
    out = {"d_x": (dx.permute(1, 0, 2, 3).reshape(M, S * B, C), dx_tol.permute(1, 0, 2, 3).reshape(M, S * B, C)),
           "d_dec": (wv * dot, (kd + 1) * U32 * wv.abs() * dab + we * dab),
           "d_lf": ((d * dot).permute(0, 2, 1).reshape(S * B, M), ((kd + 1) * U32 * d.abs() * dab).permute(0, 2, 1).reshape(S * B, M))}
    return out


# ------------------------------------------------------------------------------------------------------------------------ input kernels
def resize_taps(n_in, n_out, fma=False):
    """source index and weights of one axis of the bilinear resize (align_corners = False) in float32 as the kernels evaluate them:
    `s = (float)n_in / (float)n_out; f = fmaxf(s * (o + 0.5f) - 0.5f, 0.f); i0 = (int)f; i1 = i0 + (i0 < n_in - 1); l1 = f - i0; l0 = 1.f - l1`
    -> (i0, i1, l0, l1, f) as int64 / float64 arrays.  fma: the product and the subtraction contracted (one rounding); the rows assert that
    both give the same indices, and the weights' difference (<= 2 u (f + 1)) is in the tolerance."""
    o = np.arange(n_out, dtype=np.float32)
    s = np.float32(n_in) / np.float32(n_out)
    if fma:
        f = (np.float64(s) * (o.astype(np.float64) + 0.5) - 0.5).astype(np.float32)
    else:
        f = s * (o + np.float32(0.5)) - np.float32(0.5)
    f = np.maximum(f, np.float32(0))
    i0 = f.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = f - i0.astype(np.float32)
    l0 = np.float32(1) - l1
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))      # noqa: E731
    return torch.from_numpy(i0), torch.from_numpy(i1), t(l0), t(l1), t(f)


def taps_stable(n_in, n_out):
    return bool(torch.equal(resize_taps(n_in, n_out)[0], resize_taps(n_in, n_out, fma=True)[0]))


def bilinear_ref(v, verr, OH, OW):
    """v [..., H, W] float64 values (verr: the float32 error bound of each, or None for stored float32 values) -> (ref [..., OH, OW], tol32):
    `lh0 * (lw0 * p00 + lw1 * p01) + lh1 * (lw0 * p10 + lw1 * p11)`: product, add, product, add -> 4 u abs, + the interpolated verr,
    + the weights' fma ambiguity (4 u (fh + 1) + 4 u (fw + 1) + 2 u) max |p|.  No resize: the value itself."""
    H, W = v.shape[-2:]
    if OH == H and OW == W:
        return v, (verr if verr is not None else torch.zeros_like(v))
    h0, h1, lh0, lh1, fh = resize_taps(H, OH)
    w0, w1, lw0, lw1, fw = resize_taps(W, OW)
    lh0, lh1, fh = lh0.reshape(-1, 1), lh1.reshape(-1, 1), fh.reshape(-1, 1)

    def interp(t):
        r0, r1 = t[..., h0, :], t[..., h1, :]
        return lh0 * (lw0 * r0[..., w0] + lw1 * r0[..., w1]) + lh1 * (lw0 * r1[..., w0] + lw1 * r1[..., w1])
    ref, ab = interp(v), interp(v.abs())
    a = v.abs()
    mx = torch.maximum(torch.maximum(a[..., h0, :][..., w0], a[..., h0, :][..., w1]), torch.maximum(a[..., h1, :][..., w0], a[..., h1, :][..., w1]))
    tol = 4 * U32 * ab + (4 * U32 * (fh + 1) + 4 * U32 * (fw + 1) + 2 * U32) * mx
    if verr is not None:
        tol = tol + interp(verr)
    return ref, tol


def to_segments(ref, tol, c_pad):
    """[B, S, Fk, C, OH, OW] -> the kernels' [S, B*Fk, OH, OW, c_pad] with exact zeros in the padded channels; tol gets the bf16 rounding"""
    B, S, Fk, C, OH, OW = ref.shape
    out = torch.zeros(2, S, B * Fk, OH, OW, c_pad, dtype=torch.float64)
    for i, t in enumerate((ref, RHO_BF16 * ref.abs() + tol)):
        out[i, ..., :C] = t.permute(1, 0, 2, 4, 5, 3).reshape(S, B * Fk, OH, OW, C)
    return out[0], out[1]


def clip_ref(x, B, S, F, C, OH, OW, frame_step, c_pad, frame_offset=0):
    """adamml_clip_to_nhwc: x [B, S*F*C, H, W] float32 -> (ref, tol) [S, B*Fk, OH, OW, c_pad]; frames f = fk * frame_step"""
    H, W = x.shape[-2:]
    frames = [min(f + frame_offset, F - 1) for f in range(0, F, frame_step)]
    v = d64(x).reshape(B, S, F, C, H, W)[:, :, frames]
    return to_segments(*bilinear_ref(v, None, OH, OW), c_pad)


def u8_values(x, B, S, F, C, mean, std, div255, diff=False, frames=None):
    """x [B, H, W, S*F*CS] uint8 (CS = C, or C + 3 with diff) -> (values, float32 error bound) [B, S, Fk, C, H, W]:
    `t = (float)q; t = t / 255.f; (t - m) / sd`: division, subtraction, division -> 3 u (|t / 255| + |m|) / |sd| (2 u without div255);
    diff: t = floor((next - cur + 255) * 0.5) (exact in float32)"""
    H, W = x.shape[1:3]
    CS = C + 3 if diff else C
    q = x.reshape(B, H, W, S, F, CS).permute(0, 3, 4, 5, 1, 2).double()[:, :, frames]
    t = q[:, :, :, :C]
    if diff:
        t = torch.floor((q[:, :, :, 3:3 + C] - q[:, :, :, :C] + 255.0) * 0.5)
    n = len(mean)
    m = torch.tensor([h32(mean[c % n]) for c in range(C)], dtype=torch.float64).reshape(1, 1, 1, C, 1, 1)
    sd = torch.tensor([h32(std[c % n]) for c in range(C)], dtype=torch.float64).reshape(1, 1, 1, C, 1, 1)
    if div255:
        t = t / 255.0
    return (t - m) / sd, (3 if div255 else 2) * U32 * (t.abs() + m.abs()) / sd.abs()


def clip_u8_ref(x, B, S, F, C, OH, OW, frame_step, c_pad, mean, std, div255, diff=False, frame_offset=0):
    """adamml_clip_u8_to_nhwc / adamml_clip_u8_rgbdiff_to_nhwc (diff: C = 3 D) -> (ref, tol) [S, B*Fk, OH, OW, c_pad]"""
    frames = [min(f + frame_offset, F - 1) for f in range(0, F, frame_step)]
    v, verr = u8_values(x, B, S, F, C, mean, std, div255, diff, frames)
    return to_segments(*bilinear_ref(v, verr, OH, OW), c_pad)


# ------------------------------------------------------------------------------------------------------------------------- chain row
# The algebraic BatchNorm backward composed as adamml_amd/runtime.py _conv1x1_backward_alg composes it -- P = g'^T a
# (adamml_conv_bwd_weight_grouped), sum(g' zhat) from adamml_alg_sumfix, the coefficients from adamml_bn_bwd_finalize_affine, adamml_alg_pack,
# adamml_conv_bwd_data_alg, G = a^T a, s = sum a, adamml_alg_wgrad_combine -- against T, the float64 BatchNorm backward of the forward that
# ran: z = bf16(W) a unrounded, dz = A g' + B z + C with the coefficients of the exact sums at the float32 (mean, invstd) the forward
# stored, dx = bf16(W)^T dz, dW = dz^T a.  The kernels read the float32 master W instead of bf16(W).  F is their composition in exact
# arithmetic; with delta = W - bf16(W):  d sum(g' zhat) = invstd (delta . P), dB = -k0 dk2 invstd, dC = k0 dk2 mean invstd and
#     F_dx - T_dx = dz delta + (dB z + B (a delta^T) + dC) bf16(W)            F_dW - T_dW = dB (bf16(W) G) + B (delta G) + dC s^T
# to first order (`chain_first_order`; the remainder F - T - FO is second order in delta and is added as computed).
# Error model: |h - T| <= |FO| + |F - T - FO| + E, E the per-kernel models carried through the composition to first order:
#   eP (weight-gradient model of conv_ref: 2^-22 |P| + C_ACC sqrt(n) u |g'|^T |a|) -> e(sum g' zhat) = the alg_sumfix bound + invstd |W| . eP ->
#   ek2 -> eA, eB, eC (the counted bounds of bn_bwd_finalize_affine, tests/elementwise_ref.py, + |dB / dk2| ek2, |dC / dk2| ek2) -> the pack
#   (its own model + |W|^T eA, |W|^T eB |W|, |W|^T eC) -> the data gradient: its own model at F, + sum_k |x_k| e_k over the systematic part of
#   the pack error, + the bf16 roundings of the K = Cout + Cin pack entries of a row, which are independent errors |eps_k| <= 2^-8 |w_k|:
#   |sum_k x_k eps_k| <= min(sum_k |x_k| 2^-8 |w_k|, C_ACC 2^-8 sqrt(sum_k x_k^2 w_k^2)) (Hoeffding at the project's lambda = C_ACC).
#   dW: the combine model at F + |A| eP + eA |P| + eB |W G| + |B| |W| eG + eC |s| + |C| es (eG, es: the models of their kernels).
def chain_operands(Cout, Cin, G, P, seed):
    from tests.elementwise_ref import act_data, bn_vectors, rand_bf16
    w, _ = alg_operands(Cout, Cin, G, seed)
    return {"w": w, "a_raw": act_data(G * P, Cin, 1, seed + 1), "vin": bn_vectors(G, Cin, seed + 2), "g": rand_bf16(G * P, Cout, seed=seed + 3),
            "gamma": (torch.rand(Cout, generator=gen(seed + 4)) + 0.5).float(), "G": G, "P": P}


def chain_forward(op, eps=1e-5):
    """the forward that ran: a (the lazy operand, bf16-staged), z = bf16(W) a in float64, and the float32 vec [G, 4, Cout] its BatchNorm stored"""
    G, P = op["G"], op["P"]
    Cin = op["w"].shape[1]
    vf = op["vin"].reshape(-1)
    a = lazy_operand(op["a_raw"].reshape(G * P, 1, 1, Cin), vf, vf[Cin:], 1, G, 4 * Cin).reshape(G, P, Cin)
    wb = bf16(d64(op["w"]))
    z = torch.einsum("gpi,oi->gpo", a, wb)
    mu, var = z.mean(1), z.var(1, unbiased=False)
    inv = 1.0 / torch.sqrt(var + eps)
    ga = d64(op["gamma"])
    vec = torch.stack([ga * inv, -mu * ga * inv, mu, inv], 1).float()
    return {"a": a, "wb": wb, "z": z, "vec": vec, "g": d64(op["g"]).reshape(G, P, -1)}


def _coef(fw, op, s1, s2):
    v, n = d64(fw["vec"]), float(op["P"])
    mu, inv = v[:, 2], v[:, 3]
    k0, k1, k2 = d64(op["gamma"]) * inv, s1 / n, s2 / n
    return k0, k1, k2, mu, inv, (k0, -k0 * k2 * inv, k0 * (k2 * mu * inv - k1))


def chain_true(op, fw):
    g, z, a = fw["g"], fw["z"], fw["a"]
    v = d64(fw["vec"])
    s1, s2 = g.sum(1), (g * (z - v[:, 2].unsqueeze(1)) * v[:, 3].unsqueeze(1)).sum(1)
    A, B, C = _coef(fw, op, s1, s2)[5]
    dz = A.unsqueeze(1) * g + B.unsqueeze(1) * z + C.unsqueeze(1)
    return {"dz": dz, "dx": dz @ fw["wb"], "dw": torch.einsum("gpo,gpi->oi", dz, a), "A": A, "B": B, "C": C}


def chain_alg(op, fw):
    """F: the composition in exact arithmetic from the float32 master weight, with every intermediate the error model needs"""
    W, g, a = d64(op["w"]), fw["g"], fw["a"]
    Pm, Gm, sv, s1 = torch.einsum("gpo,gpi->goi", g, a), torch.einsum("gpi,gpj->gij", a, a), a.sum(1), g.sum(1)
    v = d64(fw["vec"])
    s2 = v[:, 3] * ((W.unsqueeze(0) * Pm).sum(2) - v[:, 2] * s1)
    k0, k1, k2, mu, inv, (A, B, C) = _coef(fw, op, s1, s2)
    wa, M, epi = W.t().unsqueeze(0) * A.unsqueeze(1), torch.einsum("oi,go,oj->gij", W, B, W), torch.einsum("oi,go->gi", W, C)
    x = torch.cat([g, a], 2)
    w_alg = torch.cat([wa, M], 2)
    gemm = torch.einsum("gpk,gck->gpc", x, w_alg)
    WG = torch.einsum("oj,gji->goi", W, Gm)
    dw = (A.unsqueeze(2) * Pm + B.unsqueeze(2) * WG + C.unsqueeze(2) * sv.unsqueeze(1)).sum(0)
    return dict(P=Pm, G=Gm, s=sv, s1=s1, s2=s2, k0=k0, k1=k1, k2=k2, mu=mu, inv=inv, A=A, B=B, C=C, wa=wa, M=M, epi=epi, x=x, w_alg=w_alg,
                gemm=gemm, dx=gemm + epi.unsqueeze(1), WG=WG, dw=dw)


def chain_first_order(op, fw, T, Fa):
    W, wb, g, a, z = d64(op["w"]), fw["wb"], fw["g"], fw["a"], fw["z"]
    dl, n = W - wb, float(op["P"])
    dk2 = Fa["inv"] * (dl.unsqueeze(0) * Fa["P"]).sum(2) / n
    dB, dC = -Fa["k0"] * dk2 * Fa["inv"], Fa["k0"] * dk2 * Fa["mu"] * Fa["inv"]
    B = T["B"]
    dx = T["dz"] @ dl + (dB.unsqueeze(1) * z + B.unsqueeze(1) * torch.einsum("gpi,oi->gpo", a, dl) + dC.unsqueeze(1)) @ wb
    dw = (dB.unsqueeze(2) * torch.einsum("oj,gji->goi", wb, Fa["G"]) + B.unsqueeze(2) * torch.einsum("oj,gji->goi", dl, Fa["G"])
          + dC.unsqueeze(2) * Fa["s"].unsqueeze(1)).sum(0)
    return dx, dw


def chain_kernel_tolerance(op, fw, Fa, tile):
    """E of the comment above -> (tol_dx [G, P, Cin], tol_dw [Cout, Cin])"""
    W, g, a = d64(op["w"]).abs(), fw["g"].abs(), fw["a"].abs()
    Cout, Cin = W.shape
    n, Gn = float(op["P"]), op["G"]
    k0, k1, k2, mu, inv = (Fa[k].abs() for k in ("k0", "k1", "k2", "mu", "inv"))
    A, B, C = Fa["A"].abs(), Fa["B"].abs(), Fa["C"].abs()
    wsum = C_ACC * math.sqrt(n) * U32
    eP = RHO_F32 * Fa["P"].abs() + wsum * torch.einsum("gpo,gpi->goi", g, a)
    eG = RHO_F32 * Fa["G"].abs() + wsum * torch.einsum("gpi,gpj->gij", a, a)
    es = RHO_F32 * Fa["s"].abs() + acc(n) * U32 * a.sum(1)
    es2 = (Cin + 3) * U64 * inv * ((W.unsqueeze(0) * Fa["P"].abs()).sum(2) + mu * Fa["s1"].abs()) + inv * (W.unsqueeze(0) * eP).sum(2)
    ek2 = es2 / n + U32 * k2
    eA = U32 * k0
    eB = 4 * U32 * B + k0 * inv * ek2
    eC = 6 * U32 * k0 * (k2 * mu * inv + k1) + k0 * mu * inv * ek2
    wa, M = Fa["wa"].abs(), Fa["M"].abs()
    r_pack = RHO_BF16 * torch.cat([wa, M], 2)                                             # independent bf16 roundings
    s_pack = torch.cat([U32 * wa + W.t().unsqueeze(0) * eA.unsqueeze(1),
                        (acc(Cout) + 1) * U32 * torch.einsum("oi,go,oj->gij", W, B, W) + torch.einsum("oi,go,oj->gij", W, eB, W)], 2)
    e_epi = acc(Cout) * U32 * torch.einsum("oi,go->gi", W, C) + torch.einsum("oi,go->gi", W, eC)
    x = Fa["x"].abs()
    nk = Cout + Cin
    gab = torch.einsum("gpk,gck->gpc", x, Fa["w_alg"].abs())
    model = RHO_BF16 * Fa["dx"].abs() + (C_ACC * math.sqrt(nk) + 1) * U32 * (gab + Fa["epi"].abs().unsqueeze(1))
    if tile:
        model = model + RHO_BF16 * Fa["gemm"].abs()
    rnd = torch.minimum(torch.einsum("gpk,gck->gpc", x, r_pack), C_ACC * torch.sqrt(torch.einsum("gpk,gck->gpc", x * x, r_pack * r_pack)))
    tol_dx = model + rnd + torch.einsum("gpk,gck->gpc", x, s_pack) + e_epi.unsqueeze(1)
    WGab = torch.einsum("oj,gji->goi", W, Fa["G"].abs())
    ab = (A.unsqueeze(2) * Fa["P"].abs() + B.unsqueeze(2) * WGab + C.unsqueeze(2) * Fa["s"].abs().unsqueeze(1)).sum(0)
    tol_dw = (Gn + 4) * U32 * ab + (B.unsqueeze(2) * acc(Cin) * U32 * WGab).sum(0) + (
        A.unsqueeze(2) * eP + eA.unsqueeze(2) * Fa["P"].abs() + eB.unsqueeze(2) * WGab + B.unsqueeze(2) * torch.einsum("oj,gji->goi", W, eG)
        + eC.unsqueeze(2) * Fa["s"].abs().unsqueeze(1) + C.unsqueeze(2) * es.unsqueeze(1)).sum(0)
    return tol_dx, tol_dw


def chain_model(op, tile):
    """-> (T, F, tol_dx, tol_dw, figures): |h - T| <= |FO| + |F - T - FO| + E; figures: max |F - T| / max |T| of dx and dW (how far the
    algebraic backward is from the backward of the forward that ran, before any rounding) and the share of the remainder"""
    fw = chain_forward(op)
    T, Fa = chain_true(op, fw), chain_alg(op, fw)
    fo_dx, fo_dw = chain_first_order(op, fw, T, Fa)
    ex, ew = chain_kernel_tolerance(op, fw, Fa, tile)
    rx, rw = (Fa["dx"] - T["dx"] - fo_dx).abs(), (Fa["dw"] - T["dw"] - fo_dw).abs()
    fig = {"dx": ((Fa["dx"] - T["dx"]).abs().max() / T["dx"].abs().max()).item(), "dw": ((Fa["dw"] - T["dw"]).abs().max() / T["dw"].abs().max()).item(),
           "rem_dx": (rx.max() / fo_dx.abs().max()).item(), "rem_dw": (rw.max() / fo_dw.abs().max()).item()}
    return fw, T, Fa, fo_dx.abs() + rx + ex, fo_dw.abs() + rw + ew, fig
