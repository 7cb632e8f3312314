"""float64 references of the convolution kernels and the per-element error model they are checked with.

Plain CPU module (it never touches torch.cuda): the GPU conformance rows (tests/test_conv_conformance_gpu.py) and the CPU
sensitivity test (tests/test_conv_ref_cpu.py) both import it; tests/elementwise_ref.py builds the references of the BatchNorm, pooling,
depthwise and stem kernels on the same helpers.

Operands.  A reference is built from the exact operand values a kernel multiplies, not from an approximation of them:
`lazy_operand` reproduces the lazily normalised read bf16(clamp(fmaf(z, scale, shift))) -- the fma in float64, rounded once to
float32 (= fmaf up to a double-rounding tie), clamped (NaN-propagating, as csrc/common.h clamp_act), rounded to bf16 to nearest
even -- with per-group vectors read `gstride` elements apart and padded channels zero.  Weights are drawn bf16-representable, so
packing them is exact.

Error model.  Every kernel multiplies bf16 operands exactly and accumulates in float32; the result is then rounded once to the
output type.  Element i of an output with reduction length n is accepted when

    |h_i - ref_i| <= rho * |ref_i| + C_ACC * sqrt(n) * 2^-24 * abs_i  (+ extra_i)

where abs_i is the same contraction over |operands| and rho the output rounding: 2^-8 (half a bf16 ulp, relative) for a bf16 output,
2^-22 for a float32 one (its final rounding plus the few float32 additions of a split reduction).  The second term is the
probabilistic bound of Higham & Mary (SIAM J. Sci. Comput. 41(5), 2019) for float32 recursive or blocked summation: with independent
mean-zero rounding errors it holds with probability at least 1 - 2 exp(-lambda^2 / 2) per element for lambda = C_ACC.  C_ACC = 8 makes
that 2.5e-14, negligible over the ~10^7 checked elements of the suite, and it is still sqrt(n) times tighter than the deterministic
bound n * 2^-24 * abs_i.  In practice the partial sums are far below abs_i and the observed error is a small fraction of this term
(the rows report max err / tol).  `extra_i` carries a second rounding the kernel really performs (the accumulating epilogues round
the GEMM result to bf16 before adding it to the stored tensor: rho * |conv_i|).

Rounding bias.  A per-element bound cannot see truncation where round-to-nearest-even was meant (both stay within one ulp), so
bf16 outputs of >= 10^4 elements also get `bias_check`: over the elements whose accumulation term is below a quarter ulp, the mean
of (h - ref) * sign(ref) / ulp(ref) is ~0 for round-to-nearest-even and ~-0.5 for truncation; it must lie within +-0.1.

Statistics.  The per-channel sums of a conv output are accumulated from the STORED bf16 values in float32 partial sums, combined
exactly across workgroups (csrc/common.h); `stats_check` bounds them against float64 sums of the stored output with the same model,
n = the number of pixels (an upper bound on the length of any float32 partial).
"""
import math

import torch
import torch.nn.functional as F

C_ACC = 8.0
U32 = 2.0 ** -24
RHO_BF16 = 2.0 ** -8
RHO_F32 = 2.0 ** -22
BIAS_LIMIT = 0.1
BIAS_MIN_ELEMENTS = 10000

ACT_BOUNDS = {0: (-math.inf, math.inf), 1: (0.0, math.inf), 2: (0.0, 6.0)}


def bf16(x):
    """float64 -> float32 -> bf16 (round to nearest even) -> float64."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def group_vec(v, g, gstride, c):
    """the c values group g reads from the vector whose first element the kernel is given (v: that element onward, flat;
    gstride = 0: shared by all groups)"""
    v = v.detach().double().cpu().reshape(-1)
    return v[g * gstride: g * gstride + c]


def lazy_operand(z, scale=None, shift=None, act=0, groups=1, gstride=0, cin_true=None, round_bf16=True):
    """Exact operand values of an NHWC bf16 input [groups*N, H, W, C] as a kernel reads it -> float64 NHWC on the CPU.
    round_bf16 = False: the float32 value clamp(fmaf(z, scale, shift)) itself, for the kernels that compare, mask or accumulate it
    without rounding it to bf16 (pools, global average pool, depthwise convs: tests/elementwise_ref.py)."""
    v = z.detach().cpu().double()
    C = v.shape[-1]
    if scale is not None:
        lo, hi = ACT_BOUNDS[act]
        n = v.shape[0] // groups
        out = torch.empty_like(v)
        for g in range(groups):
            s, t = group_vec(scale, g, gstride, C), group_vec(shift, g, gstride, C)
            y = (v[g * n:(g + 1) * n] * s + t).to(torch.float32).double()
            if lo > -math.inf or hi < math.inf:
                y = torch.clamp(y, min=lo if lo > -math.inf else None, max=hi if hi < math.inf else None)
            out[g * n:(g + 1) * n] = bf16(y) if round_bf16 else y
        v = out
    if cin_true is not None and cin_true < C:
        v = v.clone()
        v[..., cin_true:] = 0
    return v


def to_nchw(v):
    return v.permute(0, 3, 1, 2).contiguous()


def to_nhwc(v):
    return v.permute(0, 2, 3, 1).contiguous()


def conv_fwd_ref(a, w, stride, pad):
    """a: float64 NHWC operand, w: [Cout, Cin, KH, KW] -> (ref, abs) float64 NHWC, n = Cin * KH * KW"""
    x, w = to_nchw(a), w.detach().cpu().double()
    x = x[:, :w.shape[1]]
    ref = F.conv2d(x, w, stride=stride, padding=pad)
    ab = F.conv2d(x.abs(), w.abs(), stride=stride, padding=pad)
    return to_nhwc(ref), to_nhwc(ab), w.shape[1] * w.shape[2] * w.shape[3]


def conv_dgrad_ref(g, w, in_hw, stride, pad):
    """g: float64 NHWC [N, OH, OW, Cout] -> (dx, abs) float64 NHWC [N, H, W, Cin], n = Cout * taps (the taps that reach a pixel)"""
    gn, w = to_nchw(g), w.detach().cpu().double()
    size = (gn.shape[0], w.shape[1], in_hw[0], in_hw[1])
    dx = torch.nn.grad.conv2d_input(size, w, gn, stride=stride, padding=pad)
    ab = torch.nn.grad.conv2d_input(size, w.abs(), gn.abs(), stride=stride, padding=pad)
    return to_nhwc(dx), to_nhwc(ab), w.shape[0] * w.shape[2] * w.shape[3]


def conv_wgrad_ref(a, g, w_shape, stride, pad):
    """a: float64 NHWC input operand, g: float64 NHWC dz -> (dw, abs) float64 [Cout, cin, KH, KW], n = pixels"""
    x, gn = to_nchw(a)[:, :w_shape[1]], to_nchw(g)
    dw = torch.nn.grad.conv2d_weight(x, w_shape, gn, stride=stride, padding=pad)
    ab = torch.nn.grad.conv2d_weight(x.abs(), w_shape, gn.abs(), stride=stride, padding=pad)
    return dw, ab, gn.shape[0] * gn.shape[2] * gn.shape[3]


def bn_mask(z, vec, act, groups=1, gstride=None):
    """act'(fmaf(z, scale, shift)) of the BatchNorm-fused data-gradient epilogue (mask_act: strict inequalities, 0 at a bound).
    z: NHWC bf16 [groups*N, H, W, C]; vec: [groups][4][C] (scale, shift, mean, invstd)"""
    zz = z.detach().cpu().double()
    C = zz.shape[-1]
    gs = 4 * C if gstride is None else gstride
    lo, hi = ACT_BOUNDS[act]
    n = zz.shape[0] // groups
    m = torch.empty_like(zz)
    for g in range(groups):
        s, t = group_vec(vec, g, gs, C), group_vec(vec, g, gs, 2 * C)[C:]
        pre = (zz[g * n:(g + 1) * n] * s + t).to(torch.float32).double()
        m[g * n:(g + 1) * n] = ((pre > lo) & (pre < hi)).double()
    return m


def bn_dgrad_sums_ref(gp, z, vec, groups=1):
    """float64 sums (sum g', sum g' * zhat) per group and channel of the STORED g' (float64 NHWC) -> ([G, 2C], abs [G, 2C])"""
    zz = z.detach().cpu().double()
    C = zz.shape[-1]
    n = zz.shape[0] // groups
    out, ab = torch.empty(groups, 2 * C, dtype=torch.float64), torch.empty(groups, 2 * C, dtype=torch.float64)
    for g in range(groups):
        v = vec.detach().cpu().double().reshape(groups, 4, -1)[g, :, :C]
        f = gp[g * n:(g + 1) * n].reshape(-1, C)
        zh = (zz[g * n:(g + 1) * n].reshape(-1, C) - v[2]) * v[3]
        out[g, :C], out[g, C:] = f.sum(0), (f * zh).sum(0)
        ab[g, :C], ab[g, C:] = f.abs().sum(0), (f * zh).abs().sum(0)
    return out, ab


def acc_factor(n, acc=None):
    """coefficient of 2^-24 * abs_i: C_ACC * sqrt(n) (the probabilistic bound of a length-n float32 sum) unless the caller counted the
    float32 roundings of a short expression itself (acc = that count: the deterministic bound, tests/elementwise_ref.py)"""
    return C_ACC * math.sqrt(n) if acc is None else (acc if torch.is_tensor(acc) else float(acc))


def tolerance(ref, ab, n, rho, extra=None, acc=None):
    t = rho * ref.abs() + acc_factor(n, acc) * U32 * ab
    return t if extra is None else t + extra


def err_ratio(h, ref, ab, n, rho, extra=None, acc=None):
    """max over the elements of |h - ref| / tol (NaN anywhere in h where ref is finite -> inf)"""
    h = h.detach().cpu().double()
    err = (h - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    tol = tolerance(ref, ab, n, rho, extra, acc)
    # (tol == 0 only where ref and abs are exactly 0: padding rows; any non-zero h there is an error)
    r = err / torch.where(tol > 0, tol, torch.full_like(tol, 1e-300))
    return r.max().item() if r.numel() else 0.0


def ulp_bf16(x):
    """bf16 ulp at |x| (normal range)"""
    e = torch.floor(torch.log2(x.abs()))
    return torch.pow(2.0, e - 7)


def rounding_bias(h, ref, ab, n, extra=None, acc=None):
    """mean of (h - ref) * sign(ref) / ulp(ref) over the elements whose accumulation term is below 1/4 ulp -> (bias, count)"""
    h = h.detach().cpu().double().reshape(-1)
    af = acc_factor(n, acc)
    if torch.is_tensor(af):
        af = af.expand(ref.shape).reshape(-1)
    ref, ab = ref.reshape(-1), ab.reshape(-1)
    nz = ref != 0
    u = torch.ones_like(ref)
    u[nz] = ulp_bf16(ref[nz])
    at = af * U32 * ab + (0 if extra is None else extra.reshape(-1))
    sel = nz & (at <= 0.25 * u) & torch.isfinite(h)
    if int(sel.sum()) == 0:
        return 0.0, 0
    d = ((h[sel] - ref[sel]) * torch.sign(ref[sel]) / u[sel]).clamp(-1, 1)
    return d.mean().item(), int(sel.sum())


def check(h, ref, ab, n, rho=RHO_BF16, extra=None, what="", bias=None, acc=None):
    """Assert the per-element bound (and, for bf16 outputs of >= 10^4 elements, the rounding bias); returns max err / tol."""
    r = err_ratio(h, ref, ab, n, rho, extra, acc)
    assert r <= 1.0, "%s: max err/tol %.3g (n = %d)" % (what, r, n)
    if bias is None:
        bias = rho == RHO_BF16 and ref.numel() >= BIAS_MIN_ELEMENTS and extra is None
    if bias:
        b, cnt = rounding_bias(h, ref, ab, n, extra, acc)
        assert cnt >= 1000, "%s: only %d elements qualify for the rounding-bias check" % (what, cnt)
        assert abs(b) <= BIAS_LIMIT, "%s: rounding bias %.3f ulp over %d elements" % (what, b, cnt)
    return r


def stats_ref(y):
    """float64 per-channel sum / sum of squares of a STORED NHWC output (float64) of one group -> (ref [2C], abs [2C])"""
    f = y.reshape(-1, y.shape[-1])
    ref = torch.cat([f.sum(0), (f * f).sum(0)])
    ab = torch.cat([f.abs().sum(0), (f * f).sum(0)])
    return ref, ab


def stats_check(s, y, what="stats", groups=1):
    """s: [groups, 2C] (adamml_stats_collapse) against float64 sums of the stored y [groups*N, ..., C]"""
    s = s.detach().cpu().double().reshape(groups, -1)
    yy = y.detach().cpu().double()
    n = yy.shape[0] // groups
    worst = 0.0
    for g in range(groups):
        ref, ab = stats_ref(yy[g * n:(g + 1) * n])
        npix = yy[g * n:(g + 1) * n].numel() // yy.shape[-1]
        # (sum of squares: each square is rounded once in float32 before it is added -> rho = 2^-23 on top)
        r = err_ratio(s[g], ref, ab, npix, 2.0 ** -23)
        assert r <= 1.0, "%s (group %d): max err/tol %.3g" % (what, g, r)
        worst = max(worst, r)
    return worst
