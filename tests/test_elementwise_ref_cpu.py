"""The checkers of tests/elementwise_ref.py have teeth (CPU only): a correctly rounded float32 emulation of each kernel's arithmetic, in the
operation order of the source, is accepted (err / tol <= 1), and every planted defect is rejected by at least twice the tolerance -- or by
the rounding-bias check or an exact comparison where that is the detector.  The float64 references themselves are tied to torch's own
F.batch_norm / F.max_pool2d / MaxPool3d / AvgPool3d / F.conv2d (autograd in float64)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as R
from tests import elementwise_ref as E

f = torch.float32


def truncate_bf16(x):
    """float -> float32 -> bf16 by dropping the low 16 bits (round toward zero)"""
    b = x.to(torch.float32).contiguous().view(torch.int32) & ~0xFFFF
    return b.view(torch.float32).double()


def emu_fma(a, b, c):
    """fmaf on float32 tensors"""
    return (a.double() * b.double() + c.double()).to(f)


def emu_clamp(v, act, ignore_hi=False):
    lo, hi = R.ACT_BOUNDS[act]
    if ignore_hi:
        hi = math.inf
    return torch.clamp(v, min=None if lo == -math.inf else lo, max=None if hi == math.inf else hi) if (lo > -math.inf or hi < math.inf) else v


def emu_mask(v, act, ge=False, ignore_hi=False):
    lo, hi = R.ACT_BOUNDS[act]
    if ignore_hi:
        hi = math.inf
    return (((v >= lo) & (v <= hi)) if ge else ((v > lo) & (v < hi))).to(f)


# ------------------------------------------------------------------------------------------------------------------------ bn_act_add
def emu_bn_act_add(z, vz, idn, vi, act, ignore_hi=False):
    """bn_act_add_kernel row(): float32 result before the bf16 store"""
    v = emu_fma(z.to(f), vz[0], vz[1])
    if idn is not None:
        v = v + (emu_fma(idn.to(f), vi[0], vi[1]) if vi is not None else idn.to(f))
    return emu_clamp(v, act, ignore_hi)


def act_add_case(act, lazy_idn, P=2000, C=64):
    z, idn = E.act_data(P, C, act, 1), E.rand_bf16(P, C, seed=2)
    vz, vi = E.bn_vectors(1, C, 3, act)[0], E.bn_vectors(1, C, 4, act)[0]
    if not lazy_idn:
        vi = None
    # channel 0 of the identity is zero so that the planted pre-activations stay on the bounds
    idn[:, 0] = 0
    if vi is not None:
        vi[1, 0] = 0.0
    ref, ab, k = E.bn_act_add_ref(z, vz[0], vz[1], 0, act, idn, None if vi is None else vi[0], None if vi is None else vi[1])
    return z, idn, vz, vi, ref, ab, k


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("lazy_idn", [False, True])
def test_bn_act_add_accepts_clean_rejects_truncation(act, lazy_idn):
    z, idn, vz, vi, ref, ab, k = act_add_case(act, lazy_idn)
    assert k == (3 if lazy_idn else 2)
    out32 = emu_bn_act_add(z, vz, idn, vi, act)
    E.point_check(R.bf16(out32.double()), ref, ab, k, what="clean")
    b, cnt = R.rounding_bias(truncate_bf16(out32), ref, ab, 1, acc=k)
    assert cnt >= R.BIAS_MIN_ELEMENTS // 10 and b <= -2 * R.BIAS_LIMIT, (b, cnt)
    with pytest.raises(AssertionError):
        E.point_check(truncate_bf16(out32), ref, ab, k)


def test_bn_act_add_rejects_ignored_relu6_bound_and_mask_at_bounds():
    z, idn, vz, vi, ref, ab, k = act_add_case(2, True)
    bad = R.bf16(emu_bn_act_add(z, vz, idn, vi, 2, ignore_hi=True).double())
    assert R.err_ratio(bad, ref, ab, 1, R.RHO_BF16, acc=k) >= 2
    out = R.bf16(emu_bn_act_add(z, vz, idn, vi, 2).double())
    assert (out[:, 0] == 0).any() and (out[:, 0] == 6).any()           # the planted bounds arrive exactly
    good = E.mask_bits_ref(out, 2)
    ge = (emu_mask(out.to(f), 2, ge=True).reshape(-1, 8).to(torch.int64) << torch.arange(8)).sum(1).to(torch.uint8)
    nohi = (emu_mask(out.to(f), 2, ignore_hi=True).reshape(-1, 8).to(torch.int64) << torch.arange(8)).sum(1).to(torch.uint8)
    assert not torch.equal(ge, good) and not torch.equal(nohi, good)
    # and the exact backward from the stored output
    g = E.rand_bf16(*out.shape, seed=9)
    ref_g = E.act_bwd_ref(g, out, 2)
    assert not torch.equal(g.double() * emu_mask(out.to(f), 2, ge=True).double(), ref_g)
    assert torch.equal(g.double() * emu_mask(out.to(f), 2).double(), ref_g)


# ----------------------------------------------------------------------------------------------------------------------- bn_bwd_apply
def emu_bn_bwd_apply(g, z, vec, coef, act, groups=1, drop_k1=False, drop_k2=False, mean_group_shift=0, ge=False):
    """bn_bwd_apply_kernel one(): float32 ops in source order -> float32 [groups*P, C]"""
    n = z.shape[0] // groups
    out = torch.empty(z.shape, dtype=f)
    for gi in range(groups):
        v, cf = vec[gi], coef[gi]
        mu = vec[(gi + mean_group_shift) % groups][2]
        gv, zv = g[gi * n:(gi + 1) * n].to(f), z[gi * n:(gi + 1) * n].to(f)
        gp = gv * emu_mask(emu_fma(zv, v[0], v[1]), act, ge=ge)
        zh = (zv - mu) * v[3]
        t = gp if drop_k1 else gp - cf[1]
        t = t if drop_k2 else t - zh * cf[2]
        out[gi * n:(gi + 1) * n] = cf[0] * t
    return out


def apply_case(act=2, G=3, P=1500, C=64):
    z, g = E.act_data(G * P, C, act, 11), E.rand_bf16(G * P, C, seed=12)
    vec = E.bn_vectors(G, C, 13, act)
    coef = torch.stack([vec[:, 3] * 1.3, torch.randn(G, C, generator=E.gen(14)) * 0.1, torch.randn(G, C, generator=E.gen(15)) * 0.2], 1)
    gp = g.double() * R.bn_mask(z, vec, act, groups=G)
    ref, ab = E.bn_bwd_apply_ref(gp, z, vec, coef, groups=G)
    return z, g, vec, coef, ref, ab


def test_bn_bwd_apply_accepts_clean_rejects_defects():
    act, G = 2, 3
    z, g, vec, coef, ref, ab = apply_case(act, G)
    k = E.K_BN_BWD_APPLY
    out32 = emu_bn_bwd_apply(g, z, vec, coef, act, G)
    E.point_check(R.bf16(out32.double()), ref, ab, k, what="clean")
    b, cnt = R.rounding_bias(truncate_bf16(out32), ref, ab, 1, acc=k)
    assert cnt >= R.BIAS_MIN_ELEMENTS // 10 and b <= -2 * R.BIAS_LIMIT, (b, cnt)
    for kw in ({"drop_k1": True}, {"drop_k2": True}, {"mean_group_shift": 1}, {"ge": True}):
        bad = R.bf16(emu_bn_bwd_apply(g, z, vec, coef, act, G, **kw).double())
        assert R.err_ratio(bad, ref, ab, 1, R.RHO_BF16, acc=k) >= 2, kw


def test_bn_bwd_reduce_accepts_clean_rejects_mask_from_rounded_preactivation():
    act, G, P, C = 2, 2, 6000, 64
    z, g = E.act_data(G * P, C, act, 21), E.rand_bf16(G * P, C, seed=22)
    vec = E.bn_vectors(G, C, 23, act)
    gp = g.double() * R.bn_mask(z, vec, act, groups=G)
    ref, ab = R.bn_dgrad_sums_ref(gp, z, vec, groups=G)

    def emu(rounded, ge=False):
        out = torch.empty(G, 2 * C, dtype=torch.float64)
        differ = 0
        for gi in range(G):
            v = vec[gi]
            gv, zv = g[gi * P:(gi + 1) * P].to(f), z[gi * P:(gi + 1) * P].to(f)
            pre = emu_fma(zv, v[0], v[1])
            m = emu_mask(pre.to(torch.bfloat16).to(f) if rounded else pre, act, ge=ge)
            differ += int((m != emu_mask(pre, act)).sum())
            t = gv * m
            out[gi, :C] = t.sum(0, dtype=f).double()
            out[gi, C:] = (t * (zv - v[2]) * v[3]).sum(0, dtype=f).double()
        return out, differ
    clean, _ = emu(False)
    assert E.sums_check(clean, ref, ab, P) <= 1
    bad, differ = emu(True)
    assert differ > 0                                              # pre-activations in (6 - half a bf16 ulp, 6) exist
    assert R.err_ratio(bad, ref, ab, P, 2.0 ** -23, acc=R.C_ACC * math.sqrt(P) + E.K_REDUCE_TERM) >= 2
    bad, _ = emu(False, ge=True)                                   # the planted 0 and 6 of channel 0
    assert R.err_ratio(bad, ref, ab, P, 2.0 ** -23, acc=R.C_ACC * math.sqrt(P) + E.K_REDUCE_TERM) >= 2


def test_bn_references_equal_torch_batch_norm_autograd():
    """bn_finalize_ref -> bn_act_add_ref -> bn_dgrad_sums_ref -> bn_bwd_finalize_ref -> bn_bwd_apply_ref == F.batch_norm + relu in float64"""
    P, C = 400, 16
    z = E.rand_bf16(P, C, scale=1.5, offset=0.3, seed=31)
    gm, bt = torch.rand(C, generator=E.gen(32)) + 0.5, torch.randn(C, generator=E.gen(33)) * 0.2
    rm, rv = torch.randn(C, generator=E.gen(34)) * 0.1, torch.rand(C, generator=E.gen(35)) + 0.5
    zd = z.double().requires_grad_(True)
    gd, bd = gm.double().requires_grad_(True), bt.double().requires_grad_(True)
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    out = F.relu(F.batch_norm(zd.t().reshape(1, C, P), rm64, rv64, gd, bd, True, 0.1, 1e-5).reshape(C, P).t())
    s = torch.cat([z.double().sum(0), (z.double() ** 2).sum(0)]).reshape(1, -1)
    fin = E.bn_finalize_ref(s, float(P), gm, bt, rm, rv, 0.1, 1e-5)
    vec = fin["vec"][0]
    assert torch.allclose(fin["rm"][0], rm64, rtol=1e-7, atol=1e-9) and torch.allclose(fin["rv"][0], rv64, rtol=1e-6, atol=1e-9)
    ref, _, _ = E.bn_act_add_ref(z, vec[0, 0], vec[0, 1], 0, 1)
    assert torch.allclose(ref, out.detach(), rtol=1e-6, atol=1e-7)
    g = E.rand_bf16(P, C, seed=36)
    out.backward(g.double())
    gp = g.double() * R.bn_mask(z, vec, 1)
    sums, _ = R.bn_dgrad_sums_ref(gp, z, vec)
    bf = E.bn_bwd_finalize_ref(sums, float(P), gm, vec, torch.zeros(C), torch.zeros(C), 1.0)
    assert torch.allclose(bf["dgamma"][0], gd.grad, rtol=1e-6, atol=1e-7) and torch.allclose(bf["dbeta"][0], bd.grad, rtol=1e-6, atol=1e-7)
    dz, _ = E.bn_bwd_apply_ref(gp, z, vec, bf["coef"][0])
    assert torch.allclose(dz, zd.grad, rtol=1e-5, atol=1e-6)
    aff = bf["aff"][0][0]
    assert torch.allclose(aff[0] * gp + aff[1] * z.double() + aff[2], zd.grad, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------------------------------ bn_finalize
def emu_bn_finalize(s, count, gamma, beta, rm, rv, momentum, eps, biased=False, once=False, reverse=False):
    """bn_finalize_kernel in numpy: fp64 where the source is fp64, float32 where it is float32"""
    s = s.numpy()
    G, C = s.shape[0], s.shape[1] // 2
    m, e = np.float32(momentum), np.float32(eps)
    ga, be = gamma.numpy(), beta.numpy()
    vec = np.empty((G, 4, C), dtype=np.float32)
    rmean, rvar = rm.numpy().copy(), rv.numpy().copy()
    order = range(G - 1, -1, -1) if reverse else range(G)
    muf, unf = [None] * G, [None] * G
    for g in range(G):
        mu = s[g, :C] / count
        var = np.maximum(s[g, C:] / count - mu * mu, 0.0)
        inv = (1.0 / np.sqrt(var + np.float64(e))).astype(np.float32)
        sc = ga * inv
        vec[g] = np.stack([sc, be - mu.astype(np.float32) * sc, mu.astype(np.float32), inv])
        unb = var if (biased or count <= 1.0) else var * count / (count - 1.0)
        muf[g], unf[g] = mu.astype(np.float32), unb.astype(np.float32)
    for g in (list(order)[:1] if once else order):
        rmean = (np.float32(1) - m) * rmean + m * muf[g]
        rvar = (np.float32(1) - m) * rvar + m * unf[g]
    return torch.from_numpy(vec), torch.from_numpy(rmean), torch.from_numpy(rvar)


@pytest.mark.parametrize("G", [1, 5, 33])
def test_bn_finalize_accepts_clean_rejects_defects(G):
    C, count = 24, 50.0
    g = E.gen(40 + G)
    mean = torch.randn(G, C, generator=g, dtype=torch.float64) * (1.0 + torch.arange(G).double().view(G, 1) * 0.05)
    std = torch.rand(G, C, generator=g, dtype=torch.float64) + 0.5
    mean[:, 1] = 30.0 * std[:, 1]                                   # |mean| / std = 30
    s = torch.cat([mean * count, (std ** 2 + mean ** 2) * count], 1)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    ref = E.bn_finalize_ref(s, count, gamma, beta, rm, rv, 0.1, 1e-5)
    vec, rm1, rv1 = emu_bn_finalize(s, count, gamma, beta, rm, rv, 0.1, 1e-5)
    assert E.vec_ratio(vec, *ref["vec"]) <= 1 and E.vec_ratio(rm1, *ref["rm"]) <= 1 and E.vec_ratio(rv1, *ref["rv"]) <= 1
    _, _, rvb = emu_bn_finalize(s, count, gamma, beta, rm, rv, 0.1, 1e-5, biased=True)
    assert E.vec_ratio(rvb, *ref["rv"]) >= 2
    if G > 1:
        _, rmo, rvo = emu_bn_finalize(s, count, gamma, beta, rm, rv, 0.1, 1e-5, once=True)
        assert E.vec_ratio(rmo, *ref["rm"]) >= 2 and E.vec_ratio(rvo, *ref["rv"]) >= 2
        _, rmr, _ = emu_bn_finalize(s, count, gamma, beta, rm, rv, 0.1, 1e-5, reverse=True)
        assert E.vec_ratio(rmr, *ref["rm"]) >= 2


def test_bn_bwd_finalize_and_eval_affine_accept_clean():
    G, C, count = 5, 24, 300.0
    g = E.gen(50)
    sums = torch.randn(G, 2 * C, generator=g, dtype=torch.float64) * 20
    gamma = torch.rand(C, generator=g) + 0.5
    vec = E.bn_vectors(G, C, 51)
    dg0, db0 = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = E.bn_bwd_finalize_ref(sums, count, gamma, vec, dg0, db0, 0.5)
    k0 = gamma * vec[:, 3]
    k1, k2 = (sums[:, :C] / count).to(f), (sums[:, C:] / count).to(f)
    coef = torch.stack([k0, k1, k2], 1)
    aff = torch.stack([k0, -k0 * k2 * vec[:, 3], k0 * (k2 * vec[:, 2] * vec[:, 3] - k1)], 1)
    dg, db = torch.zeros(C), torch.zeros(C)
    for gi in range(G):
        dg, db = dg + sums[gi, C:].to(f), db + sums[gi, :C].to(f)
    assert E.vec_ratio(coef, *ref["coef"]) <= 1 and E.vec_ratio(aff, *ref["aff"]) <= 1
    assert E.vec_ratio(dg0 + dg * 0.5, *ref["dgamma"]) <= 1 and E.vec_ratio(db0 + db * 0.5, *ref["dbeta"]) <= 1
    assert E.vec_ratio(dg0 + dg, *ref["dgamma"]) >= 2               # grad_scale dropped
    aref, atol = E.bn_bwd_affine_ref(coef, vec)
    assert E.vec_ratio(aff, aref, atol) <= 1
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    (sref, stol), (href, htol) = E.bn_eval_affine_ref(gamma, vec[0, 1], rm, rv, 1e-5)
    sc = gamma / torch.sqrt(rv + np.float32(1e-5))
    assert E.vec_ratio(sc, sref, stol) <= 1 and E.vec_ratio(vec[0, 1] - rm * sc, href, htol) <= 1


def test_stat_bins_round_trip():
    v = torch.randn(3, 40, generator=E.gen(60), dtype=torch.float64) * torch.tensor([1e-6, 1.0, 1e9]).view(3, 1)
    v[0, 0] = 0.0
    val, ab = E.det_decode_host(E.det_encode_host(v))
    assert torch.equal(val, v) and (ab >= v.abs()).all()
    assert E.stats_to_slots(v, E.STAT_SLOTS).shape == (3, 32, 40) and E.stats_to_slots(v, 1).shape == (3, 1, 40)


# ------------------------------------------------------------------------------------------------------------------------------ pools
def tied_pool_input(N, H, W, C, seed):
    """relu(bn(x)) input whose windows tie at 0: half the channels have a shift that sends whole neighbourhoods below 0"""
    x = E.rand_bf16(N, H, W, C, seed=seed)
    vec = E.bn_vectors(1, C, seed + 1)[0]
    vec[1, C // 2:] = -2.5
    return E.plant_bounds(x), vec


def test_maxpool_reference_equals_torch_and_rejects_last_argmax():
    N, H, W, C = 2, 13, 18, 16
    x, vec = tied_pool_input(N, H, W, C, 70)
    y, idx, zsel = E.maxpool2d_fwd_ref(x, vec[0], vec[1], 0, 1)
    v = E.lazy_f32(x, vec[0], vec[1], 1)
    ty, ti = F.max_pool2d(R.to_nchw(v), 3, 2, 1, return_indices=True)
    assert torch.equal(y, R.bf16(R.to_nhwc(ty)))
    OH, OW = y.shape[1:3]
    oh, ow = torch.arange(OH).view(1, OH, 1, 1), torch.arange(OW).view(1, 1, OW, 1)
    flat = (2 * oh - 1 + idx // 3) * W + (2 * ow - 1 + idx % 3)
    assert torch.equal(flat, R.to_nhwc(ti))                        # first arg-max in torch's window order, tied windows included
    taps = E._taps2d(v, OH, OW, -math.inf)
    tied = ((taps == taps.max(0).values) | torch.isinf(taps)).all(0)
    assert tied.double().mean().item() >= 0.01                     # >= 1 % of the windows fully tied
    _, last = E.first_argmax(taps, last=True)
    assert not torch.equal(last, idx)
    # routing: float64 autograd on the continuous channels == maxpool2d_route from idx
    g = E.rand_bf16(N, OH, OW, C, seed=72)
    xx = R.to_nchw(E.lazy_f32(x)).requires_grad_(True)
    F.max_pool2d(xx, 3, 2, 1).backward(R.to_nchw(g.double()))
    _, idx_plain, _ = E.maxpool2d_fwd_ref(x, None, None, 0, 0)
    gx, ab = E.maxpool2d_route(g, idx_plain, H, W)
    assert torch.equal(gx, R.to_nhwc(xx.grad))
    E.point_check(R.bf16(gx.to(f).double()), gx, ab, E.K_MAXPOOL_BWD, what="routed", bias=False)
    gx_last, _ = E.maxpool2d_route(g, last, H, W)
    gx_first, ab1 = E.maxpool2d_route(g, idx, H, W)
    assert R.err_ratio(R.bf16(gx_last), gx_first, ab1, 1, R.RHO_BF16, acc=E.K_MAXPOOL_BWD) >= 2


@pytest.mark.parametrize("T", [8, 5, 3, 2, 1])
def test_temporal_references_equal_torch(T):
    NB, HW, C = 2, 6, 8
    x = E.rand_bf16(NB * T, HW, C, seed=80 + T)
    v = E.lazy_f32(x).reshape(NB, T, HW, C).permute(0, 3, 1, 2).unsqueeze(-1).clone().requires_grad_(True)       # [NB, C, T, HW, 1]
    y, arg = E.temporal_pool_fwd_ref(x, None, None, 0, 0, T, 0)
    ref = torch.nn.MaxPool3d((3, 1, 1), (2, 1, 1), (1, 0, 0))(v)
    To = ref.shape[2]
    assert torch.equal(y.reshape(NB, To, HW, C), ref.detach()[..., 0].permute(0, 2, 3, 1))
    g = E.rand_bf16(NB * To, HW, C, seed=90 + T)
    ref.backward(g.double().reshape(NB, To, HW, C).permute(0, 3, 1, 2).unsqueeze(-1))
    gx, _ = E.temporal_pool_bwd_ref(g, arg, T, 0)
    assert torch.equal(gx.reshape(NB, T, HW, C), v.grad[..., 0].permute(0, 2, 3, 1))
    if T >= 3:
        v.grad = None
        ref = torch.nn.AvgPool3d((3, 1, 1), (2, 1, 1), (1, 0, 0))(v)
        a, _ = E.temporal_pool_fwd_ref(x, None, None, 0, 0, T, 1)
        assert torch.allclose(a.reshape(NB, To, HW, C), ref.detach()[..., 0].permute(0, 2, 3, 1), rtol=1e-14, atol=1e-15)
        ref.backward(g.double().reshape(NB, To, HW, C).permute(0, 3, 1, 2).unsqueeze(-1))
        gx, _ = E.temporal_pool_bwd_ref(g, None, T, 1)
        assert torch.allclose(gx.reshape(NB, T, HW, C), v.grad[..., 0].permute(0, 2, 3, 1), rtol=1e-14, atol=1e-15)


@pytest.mark.parametrize("T", [8, 5, 3])
def test_temporal_avg_accepts_clean_rejects_valid_count_divisor(T):
    NB, HW, C = 3, 40, 32
    x = E.act_data(NB * T * HW, C, 1, 100 + T).reshape(NB * T, HW, C)
    vec = E.bn_vectors(1, C, 101)[0]
    ref, ab = E.temporal_pool_fwd_ref(x, vec[0], vec[1], 0, 1, T, 1)
    v = E.lazy_f32(x, vec[0], vec[1], 1).to(f).reshape(NB, T, -1)
    To, win = E.temporal_windows(T)
    third = torch.tensor(1.0, dtype=f) / 3

    def emu(valid_count):
        out = []
        for w in win:
            acc = torch.zeros(NB, v.shape[2], dtype=f)
            for t in w:
                acc = acc + v[:, t]
            out.append(acc / len(w) if valid_count else acc * third)
        return torch.stack(out, 1)
    E.point_check(R.bf16(emu(False).double()), ref, ab, E.K_TPOOL_AVG_FWD, what="clean", bias=False)
    assert R.err_ratio(R.bf16(emu(True).double()), ref, ab, 1, R.RHO_BF16, acc=E.K_TPOOL_AVG_FWD) >= 2
    # backward
    g = E.rand_bf16(NB * To, HW, C, seed=102)
    gref, gab = E.temporal_pool_bwd_ref(g, None, T, 1)
    gg = g.to(f).reshape(NB, To, -1)

    def emu_b(valid_count):
        gx = torch.zeros(NB, T, gg.shape[2], dtype=f)
        for to, w in enumerate(win):
            for t in w:
                gx[:, t] = gx[:, t] + (gg[:, to] / len(w) if valid_count else gg[:, to] * third)
        return gx
    E.point_check(R.bf16(emu_b(False).double()), gref, gab, E.K_TPOOL_AVG_BWD, what="clean bwd", bias=False)
    assert R.err_ratio(R.bf16(emu_b(True).double()), gref, gab, 1, R.RHO_BF16, acc=E.K_TPOOL_AVG_BWD) >= 2


def test_temporal_max_lazy_ties_and_last_argmax():
    T, NB, HW, C = 8, 2, 30, 16
    x, vec = tied_pool_input(NB * T, HW, 1, C, 110)
    x = x.reshape(NB * T, HW, C)
    y, arg = E.temporal_pool_fwd_ref(x, vec[0], vec[1], 0, 1, T, 0)
    v = E.lazy_f32(x, vec[0], vec[1], 1).reshape(NB, T, -1)
    To, win = E.temporal_windows(T)
    tied = torch.stack([torch.stack([v[:, t] for t in w]).max(0).values == torch.stack([v[:, t] for t in w]).min(0).values for w in win], 1)
    assert tied.double().mean().item() >= 0.01
    g = E.rand_bf16(NB * To, HW, C, seed=111)
    gx, ab = E.temporal_pool_bwd_ref(g, arg, T, 0)
    E.point_check(R.bf16(gx.to(f).double()), gx, ab, E.K_TPOOL_MAX_BWD, what="clean", bias=False)
    last = torch.stack([torch.tensor(w)[E.first_argmax(torch.stack([v[:, t] for t in w]), last=True)[1]] for w in win], 1)
    bad, _ = E.temporal_pool_bwd_ref(g, last, T, 0)
    assert R.err_ratio(R.bf16(bad), gx, ab, 1, R.RHO_BF16, acc=E.K_TPOOL_MAX_BWD) >= 2


def test_gap_accepts_clean():
    N, HW, C = 4, 49, 64
    x = E.act_data(N * HW, C, 2, 120)
    vec = E.bn_vectors(1, C, 121, 2)[0]
    ref, ab, n = E.gap_fwd_ref(x, vec[0], vec[1], 0, 2, N, HW)
    v = E.lazy_f32(x, vec[0], vec[1], 2).to(f).reshape(N, HW, C)
    acc = torch.zeros(N, C, dtype=f)
    for p in range(HW):
        acc = acc + v[:, p]
    inv = torch.tensor(1.0, dtype=f) / HW
    assert R.err_ratio(acc * inv, ref, ab, n, R.RHO_F32) <= 1
    assert R.err_ratio(acc * inv * (HW / (HW - 1.0)), ref, ab, n, R.RHO_F32) >= 2          # one pixel too few in the divisor
    g = torch.randn(N, C, generator=E.gen(122))
    gref = (g.double() / HW).view(N, 1, C).expand(N, HW, C)
    E.point_check(R.bf16((g * inv).double()).view(N, 1, C).expand(N, HW, C), gref, gref.abs(), E.K_GAP_BWD, what="gap bwd", bias=False)


# -------------------------------------------------------------------------------------------------------------------------- depthwise
def emu_dw_fwd(a, w, stride, replicate=False):
    """dwconv_fwd_kernel emit(): nine float32 multiply-adds in tap order -> float32 NHWC"""
    a = a.to(f)
    N, H, W, C = a.shape
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    if replicate:
        p = F.pad(R.to_nchw(a), (1, stride + 1, 1, stride + 1), mode="replicate").permute(0, 2, 3, 1)
    else:
        p = torch.zeros(N, stride * OH + 3, stride * OW + 3, C, dtype=f)
        p[:, 1:H + 1, 1:W + 1] = a
    acc = torch.zeros(N, OH, OW, C, dtype=f)
    for kh in range(3):
        for kw in range(3):
            acc = acc + p[:, kh:kh + stride * OH:stride, kw:kw + stride * OW:stride] * w[:, 0, kh, kw].to(f)
    return acc


@pytest.mark.parametrize("stride,H,W", [(1, 9, 14), (2, 13, 10), (1, 1, 7), (2, 2, 2)])
def test_dwconv_fwd_accepts_clean_rejects_padding_and_border_defects(stride, H, W):
    N, C = 2, 24
    x = E.act_data(N * H * W, C, 2, 130).reshape(N, H, W, C)
    vec = E.bn_vectors(1, C, 131, 2)[0]
    w = torch.randn(C, 1, 3, 3, generator=E.gen(132)) * 0.4
    a = E.lazy_f32(x, vec[0], vec[1], 2)
    ref, ab, nt = E.dwconv_fwd_ref(a, w, stride)
    out = R.bf16(emu_dw_fwd(a, w, stride).double())
    R.check(out, ref, ab, 9, acc=E.dw_acc(nt), what="clean", bias=False)
    bad = R.bf16(emu_dw_fwd(a, w, stride, replicate=True).double())
    assert R.err_ratio(bad, ref, ab, 9, R.RHO_BF16, acc=E.dw_acc(nt)) >= 2
    for sl in ((slice(None), -1), (slice(None), slice(None), -1)):
        unwritten = out.clone()
        unwritten[sl] = math.nan                                    # the NaN pre-fill of a row / column the kernel never stores
        assert R.err_ratio(unwritten, ref, ab, 9, R.RHO_BF16, acc=E.dw_acc(nt)) == math.inf


def test_dwconv_rejects_weights_rounded_to_bf16():
    """single-tap channels (E.single_tap_weights): activation 1.5, centre tap just above 1 + 2^-9 * 4/3 -- the exact product lies above the
    bf16 midpoint 1.50390625 and rounds to 1.5078125; with the tap rounded to bf16 (-> 1.0) the product is 1.5: a full ulp, deterministic.
    Half an ulp from the reference is at most 2/3 of the per-element bound at 1.5, so the detector is the exact comparison: a single-tap
    output is bf16(float32(a * w)) whatever the order or contraction of the other eight (zero) taps."""
    N, H, W, C = 1, 6, 6, 8
    x = torch.full((N, H, W, C), 1.5, dtype=torch.bfloat16)
    w = E.single_tap_weights(torch.randn(C, 1, 3, 3, generator=E.gen(133)), range(C))
    a = E.lazy_f32(x)
    ref, ab, nt = E.dwconv_fwd_ref(a, w, 1)
    want = E.single_tap_expected(a, w, 1)
    good = R.bf16(emu_dw_fwd(a, w, 1).double())
    assert (want == 1.5078125).all() and torch.equal(good, want)
    R.check(good, ref, ab, 9, acc=E.dw_acc(nt), what="clean", bias=False)
    bad = R.bf16(emu_dw_fwd(a, w.to(torch.bfloat16).to(f), 1).double())
    assert (bad == 1.5).all() and not torch.equal(bad, want)


@pytest.mark.parametrize("stride", [1, 2])
def test_dwconv_gradient_references_equal_autograd_and_accept_clean(stride):
    N, H, W, C = 2, 9, 11, 16
    x = E.rand_bf16(N, H, W, C, seed=140)
    w = torch.randn(C, 1, 3, 3, generator=E.gen(141)) * 0.4
    a = E.lazy_f32(x)
    xa, wa = R.to_nchw(a).requires_grad_(True), w.double().requires_grad_(True)
    y = F.conv2d(xa, wa, stride=stride, padding=1, groups=C)
    g = E.rand_bf16(N, y.shape[2], y.shape[3], C, seed=142)
    y.backward(R.to_nchw(g.double()))
    dx, dab, nt = E.dwconv_dgrad_ref(g.double(), w, (H, W), stride)
    assert torch.allclose(dx, R.to_nhwc(xa.grad), rtol=1e-13, atol=1e-14)
    dw, wab, n = E.dwconv_wgrad_ref(a, g.double(), stride)
    assert torch.allclose(dw, wa.grad, rtol=1e-12, atol=1e-13)
    # float32 emulations: the data gradient is the transposed walk, the weight gradient a float32 sum over the pixels
    xf, wf = R.to_nchw(a).to(f).requires_grad_(True), w.clone().requires_grad_(True)
    F.conv2d(xf, wf, stride=stride, padding=1, groups=C).backward(R.to_nchw(g.to(f)))
    R.check(R.bf16(R.to_nhwc(xf.grad).double()), dx, dab, 9, acc=E.dw_acc(nt), what="dgrad", bias=False)
    E.wgrad_check(wf.grad, dw, wab, n, what="wgrad")
    base = E.rand_bf16(N, H, W, C, seed=143)
    R.check(R.bf16((R.to_nhwc(xf.grad) + base.to(f)).double()), dx + base.double(), dab + base.double().abs(), 10, acc=E.dw_acc(nt, 1),
            extra=R.RHO_BF16 * dx.abs(), what="dgrad accumulate")


def test_fused_dz_bound_holds_for_the_kernels_rounding():
    G, N, H, W, C = 2, 1, 5, 6, 16
    g, z = E.rand_bf16(G * N, H, W, C, seed=150), E.rand_bf16(G * N, H, W, C, scale=1.5, seed=151)
    aff = torch.randn(G, 3, C, generator=E.gen(152)) * 0.5
    dz, bound = E.fused_dz_ref(g, z, aff, G)
    a = aff.view(G, 3, 1, 1, 1, C)
    gg, zz = g.to(f).view(G, N, H, W, C), z.to(f).view(G, N, H, W, C)
    emu = emu_fma(a[:, 0], gg, emu_fma(a[:, 1], zz, a[:, 2])).to(torch.bfloat16).double().view_as(dz)
    assert ((emu - dz).abs() <= bound).all()
    assert not ((truncate_bf16(emu_fma(a[:, 0], gg, emu_fma(a[:, 1], zz, a[:, 2]))).view_as(dz) - dz).abs() <= bound).all()


def test_stem_wgrad_rejects_missing_ragged_tile():
    N, H, W, Cin = 1, 30, 50, 3                                     # 15 x 25 = 375 output pixels: the last tile of 64 is ragged
    x = E.rand_bf16(N, H, W, 8, seed=160)
    x[..., Cin:] = 0
    w_shape = (64, Cin, 7, 7)
    OH, OW = 15, 25
    g = E.rand_bf16(N, OH, OW, 64, seed=161)
    ref, ab, n = R.conv_wgrad_ref(x.double(), g.double(), w_shape, 2, 3)
    good = torch.nn.grad.conv2d_weight(R.to_nchw(x.to(f))[:, :Cin], w_shape, R.to_nchw(g.to(f)), stride=2, padding=3)
    E.wgrad_check(good, ref, ab, n, what="clean", products_round=False)
    gcut = g.clone().view(-1, 64)
    gcut[(OH * OW) // 64 * 64:] = 0
    bad = torch.nn.grad.conv2d_weight(R.to_nchw(x.to(f))[:, :Cin], w_shape, R.to_nchw(gcut.view_as(g).to(f)), stride=2, padding=3)
    assert R.err_ratio(bad, ref, ab, n, R.RHO_F32) >= 2
