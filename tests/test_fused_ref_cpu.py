"""tests/fused_ref.py on the CPU: every reference is anchored to an independent statement of the same operation (F.conv2d, F.batch_norm,
MaxPool3d(return_indices) and float64 autograd), every error model is self-tested -- an emulation of the kernel in its own formats (bf16
operands, float32 accumulation in blocks of one MFMA K step, the staged roundings) passes it, each planted error of the issue's list
fails it by name -- and the undecided share of every GPU row's inputs is bounded from the reference alone."""
import math

import pytest
import torch
import torch.nn.functional as Fn

from tests import conv_ref as R
from tests import elementwise_ref as E
from tests import fused_ref as F

T64 = dict(rtol=1e-12, atol=1e-12)


def bf(x):
    """float32 -> bf16 (nearest even) -> float32"""
    return x.to(torch.bfloat16).float()


def trunc_bf16(x):
    """float32 -> bf16 by truncation (the planted rounding error)"""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def emu_gemm(a, w, blk=32):
    """[.., K] x [Co, K]^T with float32 accumulation, one partial product per MFMA K step of 32"""
    acc = torch.zeros(a.shape[:-1] + (w.shape[-2],))
    for k0 in range(0, a.shape[-1], blk):
        acc = acc + a[..., k0:k0 + blk].float() @ w[..., k0:k0 + blk].float().transpose(-1, -2)
    return acc


def small_row(**kw):
    row = dict(id="cpu-row", G=3, P=700, Cin=64, Cout=32, in_act=1, act=2, idn="lazyg")
    row.update(kw)
    return row


def emu_fadd(row, op, r, rnd=bf, vec_group=None, idn_first=False):
    """the forward kernels' expression in their own formats; vec_group: every group reads that group's vectors (gstride ignored);
    idn_first: the identity joins the accumulator BEFORE the bf16 staging"""
    G, Cout = row["G"], row["Cout"]
    z32 = emu_gemm(r["a"], op["w"])
    out = torch.empty_like(z32)
    idn = op["idn"].float().reshape(G, -1, Cout) if op["idn"] is not None else None
    for g in range(G):
        gv = g if vec_group is None else vec_group
        sc, sh = op["vec"][gv, 0], op["vec"][gv, 1]
        t2 = 0.0
        if idn is not None:
            if op["ivec"] is None:
                t2 = idn[g]
            else:
                gi = (gv if op["id_gstride"] else 0)
                t2 = E.fma32(idn[g].double(), op["ivec"][gi, 0].double(), op["ivec"][gi, 1].double()).float()
        if idn_first:
            zb = bf(z32[g] + t2 / sc)
            f = E.fma32(zb.double(), sc.double(), sh.double()).float()
        else:
            zb = bf(z32[g])
            f = E.fma32(zb.double(), sc.double(), sh.double()).float() + t2
        out[g] = rnd(E.clamp(f, row["act"]))
    return out


def pool_emulate(h, T):
    """h [G, clips, T, Q, C] -> (pooled, window tap of the first maximum, of the last maximum) [G, clips, To, Q, C]"""
    pooled, first, last = [], [], []
    for win in F.pool_windows(T):
        vals = torch.stack([h[:, :, t] for _, t in win], -1)
        taps = torch.tensor([k for k, _ in win])
        hit = vals == vals.max(-1, keepdim=True).values
        pooled.append(vals.max(-1).values)
        first.append(taps[hit.double().argmax(-1)])
        last.append(taps[len(win) - 1 - torch.flip(hit, [-1]).double().argmax(-1)])
    return torch.stack(pooled, 2), torch.stack(first, 2), torch.stack(last, 2)


# ------------------------------------------------------------------------------------------------------------------------ anchors, forward
def test_fwd_bn_add_ref_equals_conv2d_affine_add_act():
    row = small_row()
    op = F.fadd_operands(row)
    op["w"] = F.weight(row["Cout"], row["Cin"], 5)                    # (no zero rows: no exactly evaluated element)
    r = F.fadd_reference(row, op)
    assert not r["exact"].any()
    G, P, Cin, Cout = row["G"], row["P"], row["Cin"], row["Cout"]
    xv = op["xvec"].double()
    for g in range(G):
        x = op["x"].double().reshape(G, P, Cin)[g]
        a = R.bf16(torch.clamp(E.f32(x * xv[g, 0] + xv[g, 1]), min=0.0))
        z = Fn.conv2d(a.t().reshape(1, Cin, P, 1), op["w"].double().reshape(Cout, Cin, 1, 1))[0, :, :, 0].t()
        iv = op["ivec"].double()[g]
        pre = z * op["vec"][g, 0].double() + op["vec"][g, 1].double() + op["idn"].double().reshape(G, P, Cout)[g] * iv[0] + iv[1]
        assert torch.allclose(r["pre"][g], pre, **T64) and torch.allclose(r["ref"][g], Fn.relu6(pre), **T64)
    m, und = F.act_mask_ref(r["pre"], r["tol_pre"], 2)
    assert torch.equal(m, (r["pre"] > 0) & (r["pre"] < 6))
    near = ((r["pre"].abs() <= r["tol_pre"]) | ((r["pre"] - 6).abs() <= r["tol_pre"]))
    assert torch.equal(und, near) and 0 < und.double().mean() <= F.UNDECIDED_CAP


def test_exact_elements_are_the_float32_epilogue_and_sit_on_the_bounds():
    row = small_row()
    op = F.fadd_operands(row)
    r = F.fadd_reference(row, op)
    ex = r["exact"]
    assert ex[..., :F.PLANTED].all() and not ex[..., F.PLANTED:].any()
    assert (r["tol"][ex] == 0).all() and (r["pre"][..., 0] == 0).all() and (r["pre"][..., 1] == 6).all()
    p2 = r["pre"][..., 2].reshape(-1)
    assert (p2[0::7] == 0).all() and (p2[3::7] == 6).all()
    m, und = F.act_mask_ref(r["pre"], r["tol_pre"], 2)
    assert not und[ex].any() and not m[..., 0].any() and not m[..., 1].any()          # strict inequalities: 0 at a bound, and decided
    h = emu_fadd(row, op, r)
    assert torch.equal(h.double()[ex], r["ref"][ex])


def test_fwd_bn_add_next_ref_is_a_conv_of_the_stored_output():
    out = E.rand_bf16(2 * 50, 256, seed=1)
    wn = F.weight(64, 256, 2)
    ref, ab, n = F.fwd_bn_add_next_ref(out, wn, 2)
    want = Fn.conv2d(out.double().t().reshape(1, 256, 100, 1), wn.double().reshape(64, 256, 1, 1))[0, :, :, 0].t().reshape(2, 50, 64)
    assert n == 256 and torch.allclose(ref, want, **T64) and (ab >= ref.abs() - 1e-12).all()


@pytest.mark.parametrize("T", [2, 4, 8])
def test_pool_reference_equals_maxpool3d_with_first_maximum_on_ties(T):
    """values on a coarse grid: exact ties in most windows; tolerance 0: the near set is exactly the first maximum"""
    G, clips, Q, C = 2, 3, 5, 16
    v = torch.randint(-2, 3, (G, clips * T * Q, C), generator=F.gen(T)).double()
    out = v.clamp_min(0)
    zero = torch.zeros_like(v)
    r = dict(ref=out, tol=zero, pre=v, tol_pre=zero, Q=Q)
    p = F.fwd_bn_add_tpool_ref(r, T)
    x = out.reshape(G * clips, T, Q, C).permute(0, 3, 1, 2).unsqueeze(-1)              # [N, C, T, Q, 1]
    y, idx = Fn.max_pool3d(x, (3, 1, 1), (2, 1, 1), (1, 0, 0), return_indices=True)
    y, idx = y[..., 0].permute(0, 2, 3, 1), idx[..., 0].permute(0, 2, 3, 1)             # [N, To, Q, C]
    assert torch.equal(p["ref"].reshape(y.shape), y)
    frame = idx // Q                                                                  # flat index over (T, Q, 1) -> frame of the first maximum
    to = torch.arange(T // 2).reshape(1, -1, 1, 1)
    tap = (frame - (2 * to - 1)).reshape(p["ref"].shape)
    assert (p["near"].sum(-1) == 1).all() and torch.equal(p["near"].double().argmax(-1), tap)
    assert torch.equal(p["must3"], p["ref"] <= 0) and not p["und3"].any()
    code = torch.where(p["must3"], torch.full_like(tap, 3), tap)
    F.tpool_check(y.reshape(-1, Q, C).to(torch.bfloat16), E.pack_codes(code), p, "first maximum")
    # planted: the LAST maximum on an exact tie
    _, first, last = pool_emulate(out.reshape(G, clips, T, Q, C), T)
    assert torch.equal(first, tap)
    assert (last != tap).any()
    with pytest.raises(AssertionError, match="near-maximal first tap"):
        F.tpool_check(y.reshape(-1, Q, C).to(torch.bfloat16), E.pack_codes(torch.where(p["must3"], torch.full_like(tap, 3), last)), p, "last maximum")
    # planted: a gradient-carrying code where the maximum is <= 0, and 3 where it is positive
    for wrong in (torch.where(p["must3"], torch.ones_like(tap), tap), torch.where(~p["must3"] & (tap == 1), torch.full_like(tap, 3), code)):
        with pytest.raises(AssertionError):
            F.tpool_check(y.reshape(-1, Q, C).to(torch.bfloat16), E.pack_codes(wrong), p, "code 3")


def test_pool_row_with_duplicated_frames_accepts_only_the_first_copy():
    row = next(r for r in F.TPOOL_ROWS if r["dup"] and r["Q"] <= 200 and r["Cout"] <= 256)
    op = F.tpool_operands(row)
    r, p = F.tpool_reference(row, op)
    G, clips, T, Q, C = row["G"], row["clips"], row["T"], row["Q"], row["Cout"]
    h = emu_fadd(dict(row, act=1, P=clips * T * Q), op, r).reshape(G, clips, T, Q, C)
    pooled, first, last = pool_emulate(h, T)
    dead = pooled <= 0
    q, und = F.tpool_check(pooled.to(torch.bfloat16), E.pack_codes(torch.where(dead, torch.full_like(first, 3), first)), p, "emulation")
    assert q <= 1.0 and und <= F.UNDECIDED_CAP
    assert ((last != first) & ~dead).any(), "the duplicated frames produce no exact tie"
    with pytest.raises(AssertionError, match="near-maximal first tap"):
        F.tpool_check(pooled.to(torch.bfloat16), E.pack_codes(torch.where(dead, torch.full_like(first, 3), last)), p, "last copy")


# ----------------------------------------------------------------------------------------------------------- forward model, planted errors
def test_forward_model_accepts_the_emulation_and_rejects_the_planted_errors():
    row = small_row(P=1701, Cout=64, idn="lazyg")
    op = F.fadd_operands(row)
    r = F.fadd_reference(row, op)
    h = emu_fadd(row, op, r)
    q, und = F.fadd_check(h.to(torch.bfloat16), r, row["act"], F.mask_from_output(h.to(torch.bfloat16), row["act"]), "emulation")
    assert q <= 1.0 and und <= F.UNDECIDED_CAP
    b, cnt = R.rounding_bias(h, r["ref"], r["ab"], r["n"], r["extra"])
    assert cnt >= 1000 and abs(b) <= R.BIAS_LIMIT
    # truncation instead of round-to-nearest-even: most elements stay inside the per-element bound (one ulp against half an ulp plus the
    # other terms); the bias check sees it on its own
    ht = emu_fadd(row, op, r, rnd=trunc_bf16)
    bt, cnt = R.rounding_bias(ht, r["ref"], r["ab"], r["n"], r["extra"])
    assert cnt >= 1000 and bt < -3 * R.BIAS_LIMIT
    with pytest.raises(AssertionError):
        F.fadd_check(ht.to(torch.bfloat16), r, row["act"], None, "truncation")
    # the last partial 32-pixel tile of one group left unwritten
    hp = h.clone()
    hp[1, row["P"] - row["P"] % 32:] = float("nan")
    with pytest.raises(AssertionError, match="max err/tol"):
        F.fadd_check(hp.to(torch.bfloat16), r, row["act"], None, "partial tile")
    # group g reads group 0's vectors (gstride ignored)
    with pytest.raises(AssertionError, match="max err/tol"):
        F.fadd_check(emu_fadd(row, op, r, vec_group=0).to(torch.bfloat16), r, row["act"], None, "gstride")
    # mask bit order reversed within a byte
    good = F.mask_from_output(h.to(torch.bfloat16), row["act"])
    rev = F.pack_bits(torch.flip(F.unpack_bits(good, (h.numel() // 8, 8)), [1]))
    assert not torch.equal(rev, good)
    with pytest.raises(AssertionError, match="mask"):
        F.fadd_check(h.to(torch.bfloat16), r, row["act"], rev, "bit order")
    # a mask that follows the float64 pre-activation everywhere but flips one DECIDED bit
    m, und_set = F.act_mask_ref(r["pre"], r["tol_pre"], row["act"])
    assert torch.equal(F.unpack_bits(good, m.shape)[~und_set], m[~und_set])


def test_identity_before_the_staging_is_rejected():
    """the kernels stage z as bf16 and add the identity afterwards; with the identity in the accumulator the staging rounds
    |scale z + idn'| instead of |scale z|: outside the bound when the identity dominates"""
    row = small_row(P=1701, Cout=64, idn="plain", act=0, idn_scale=16.0)
    op = F.fadd_operands(row)
    r = F.fadd_reference(row, op)
    assert F.fadd_check(emu_fadd(row, op, r).to(torch.bfloat16), r, 0, None, "emulation")[0] <= 1.0
    with pytest.raises(AssertionError, match="max err/tol"):
        F.fadd_check(emu_fadd(row, op, r, idn_first=True).to(torch.bfloat16), r, 0, None, "identity first")


# ------------------------------------------------------------------------------------------------------------------------------ backward
def _res_case(G=2, P=333, C=64, K=32, act=1, seed=3):
    dz = E.rand_bf16(G * P, K, scale=0.5, seed=seed)
    w = F.weight(K, C, seed + 1)
    dx_in = E.rand_bf16(G * P, C, seed=seed + 2)
    za, zb = E.act_data(G * P, C, act, seed + 3), E.rand_bf16(G * P, C, seed=seed + 4)
    va, vb = E.bn_vectors(G, C, seed + 5, act), E.bn_vectors(G, C, seed + 6, act)
    return dz, w, dx_in, za, zb, va, vb


@pytest.mark.parametrize("act", [0, 1, 2])
def test_res_ref_equals_autograd_through_the_residual_add_and_the_conv(act):
    """out = act(bn_a(z_a) + bn_b(z_b)), y = conv1x1(out): d loss / d out (+ the identity-path gradient), masked by act'(out), and the
    BatchNorm-backward sums of both operands"""
    G, P, C, K = 2, 333, 64, 32
    dz, w, dx_in, za, zb, va, vb = _res_case(G, P, C, K, act)
    vad, vbd = va.double().unsqueeze(2), vb.double().unsqueeze(2)                       # [G, 4, 1, C]
    zad, zbd = F.gview(za.double(), G), F.gview(zb.double(), G)
    pre = zad * vad[:, 0] + vad[:, 1] + zbd * vbd[:, 0] + vbd[:, 1]
    out = E.clamp(pre, act).requires_grad_(True)
    y = out @ w.double().t()
    (y * F.gview(dz.double(), G)).sum().backward()
    res_out = out.detach()
    m = F.res_mask(res_out=res_out, res_act=act, shape=(G, P, C))
    ref, ab, n, extra = F.res_ref(F.gview(dz.double(), G), w, m, F.gview(dx_in, G))
    want = (out.grad + F.gview(dx_in.double(), G)) * E.act_mask(res_out, act)
    assert n == K and torch.allclose(ref, want, **T64)
    ref0 = F.res_ref(F.gview(dz.double(), G), w, m)
    assert ref0[3] is None and torch.allclose(ref0[0], out.grad * E.act_mask(res_out, act), **T64)
    assert torch.equal(F.res_mask(bits=F.pack_bits(m.bool()), shape=(G, P, C)), m)
    # sums of the stored g' for both operands = the reductions of F.batch_norm's backward
    gp = R.bf16(ref)
    for z, v in ((za, va), (zb, vb)):
        zh = (F.gview(z.double(), G) - v.double()[:, 2].unsqueeze(1)) * v.double()[:, 3].unsqueeze(1)
        got = torch.cat([gp.sum(1), (gp * zh).sum(1)], 1)
        F.res_sums_check(got, gp, z, v, G, "sums")
        with pytest.raises(AssertionError):
            F.res_sums_check(torch.cat([gp.sum(1), (gp * zh).sum(1) - gp[:, -1] * zh[:, -1]], 1), gp, z, v, G, "last pixel dropped")
    F.res_sums_check(torch.cat([gp.sum(1), torch.zeros(G, C, dtype=torch.float64)], 1), gp, None, None, G, "z_a NULL")
    with pytest.raises(AssertionError):
        F.res_sums_check(torch.cat([gp.sum(1), gp.sum(1)], 1), gp, None, None, G, "z_a NULL, second half written")


def emu_res(dz, w, dx_in, m, G, rnd=bf):
    conv = rnd(emu_gemm(F.gview(dz.float(), G), w.t().contiguous()))             # (the staged tile; a truncating kernel truncates here too)
    f = conv + F.gview(dx_in.float(), G) if dx_in is not None else conv
    return rnd(f * m.float())


def test_res_model_accepts_the_emulation_and_rejects_the_planted_errors():
    G, P, C, K = 2, 1333, 64, 128
    dz, w, dx_in, za, zb, va, vb = _res_case(G, P, C, K)
    m = (torch.rand(G, P, C, generator=F.gen(9)) > 0.4).double()
    for base in (dx_in, None):
        ref, ab, n, extra = F.res_ref(F.gview(dz.double(), G), w, m, None if base is None else F.gview(base, G))
        h = emu_res(dz, w, base, m, G)
        assert R.check(h, ref, ab, n, extra=extra, what="emulation", bias=True) <= 1.0
        bt, cnt = R.rounding_bias(emu_res(dz, w, base, m, G, rnd=trunc_bf16), ref, ab, n, extra)
        assert cnt >= 1000 and bt < -3 * R.BIAS_LIMIT, "truncation must show in the rounding bias"
        hp = h.clone()
        hp[1, P - P % 32:] = float("nan")
        with pytest.raises(AssertionError, match="max err/tol"):
            R.check(hp, ref, ab, n, extra=extra, what="partial tile")
        # mask bit order reversed within a byte
        mrev = torch.flip(m.reshape(-1, 8), [1]).reshape(m.shape)
        with pytest.raises(AssertionError, match="max err/tol"):
            R.check(emu_res(dz, w, base, mrev, G), ref, ab, n, extra=extra, what="bit order")


def emu_prod(gp, a, chunk, drop=None):
    """float32 partial products per workgroup (chunk pixels), summed in order; drop: the partial left out"""
    acc = torch.zeros(gp.shape[0], gp.shape[2], a.shape[2])
    for i, p0 in enumerate(range(0, gp.shape[1], chunk)):
        if i != drop:
            acc = acc + emu_gemm(gp[:, p0:p0 + chunk].float().transpose(1, 2), a[:, p0:p0 + chunk].float().transpose(1, 2))
    return acc


def test_res_prod_model_is_per_element_and_sees_a_missing_partial():
    G, P, C = 2, 4205, 64
    gp = E.rand_bf16(G * P, C, seed=1).double().reshape(G, P, C) * (torch.rand(G, P, C, generator=F.gen(2)) > 0.5)
    x, v = E.act_data(G * P, 64, 1, 3), E.bn_vectors(G, 64, 4).reshape(-1)
    a = F.operand(x, v, v[64:], 1, G, 4 * 64)
    ref, ab, n = F.res_prod_ref(gp, a)
    assert n == P and torch.allclose(ref, torch.einsum("gpc,gpk->gck", gp, a), **T64)
    assert F.prod_check(emu_prod(gp, a, 544), ref, ab, n, "emulation") <= 1.0
    with pytest.raises(AssertionError, match="per element"):
        F.prod_check(emu_prod(gp, a, 544, drop=3), ref, ab, n, "one workgroup's partial missing")
    with pytest.raises(AssertionError, match="per element"):                       # group 1 with group 0's vectors
        F.prod_check(emu_prod(gp, F.operand(x, v, v[64:], 1, G, 0), 544), ref, ab, n, "gstride")
    small = emu_prod(gp, a, 544)
    k = ref.abs().reshape(-1).argmin()
    small.view(-1)[k] = small.view(-1)[k] + 3e-4 * ref.abs().max().float()         # far inside any max-norm bound, outside the element's own
    with pytest.raises(AssertionError, match="per element"):
        F.prod_check(small, ref, ab, n, "small entry")


def test_dual_ref_equals_autograd_through_train_mode_batchnorm():
    """z = W a, y = BN_train(z): dz from float64 autograd == A g + B z + C with the coefficients adamml_bn_bwd_finalize / _affine document
    (coef = gamma invstd, sum g / n, sum g zhat / n), dx == W^T dz; then the stored dz_side through the three epilogues"""
    G, P, Cin, Cout, eps = 2, 200, 16, 32, 1e-5
    a = E.rand_bf16(G * P, Cin, seed=1).double().reshape(G, P, Cin).requires_grad_(True)
    w = F.weight(Cout, Cin, 2)
    gamma = (torch.rand(Cout, generator=F.gen(3)) + 0.5).double()
    g = E.rand_bf16(G * P, Cout, seed=4)
    z = a @ w.double().t()
    y = torch.stack([Fn.batch_norm(z[i], None, None, gamma, None, True, 0.1, eps) for i in range(G)])
    (y * F.gview(g.double(), G)).sum().backward()
    zd = z.detach()
    mu, inv = zd.mean(1), 1.0 / torch.sqrt(zd.var(1, unbiased=False) + eps)
    gg = F.gview(g.double(), G)
    zh = (zd - mu.unsqueeze(1)) * inv.unsqueeze(1)
    coef = torch.stack([gamma * inv, gg.sum(1) / P, (gg * zh).sum(1) / P], 1)
    vec = torch.stack([gamma * inv, -mu * gamma * inv, mu, inv], 1)
    aff = E.bn_bwd_affine_ref(coef, vec)[0]
    dz, dza = F.dual_dz_ref(gg, zd, aff, G)
    dx, ab, n, extra = F.dual_ref(dz, w)
    assert n == Cout and extra is None and torch.allclose(dx, a.grad, rtol=1e-9, atol=1e-10)
    # the loader in float32, and the planted error: the B z term dropped
    zb16 = zd.to(torch.bfloat16).double()
    dzr, dza = F.dual_dz_ref(gg, zb16, aff.float(), G)
    af = aff.float().double().unsqueeze(2)
    h = bf(E.fma32(af[:, 0], gg, E.fma32(af[:, 1], zb16, af[:, 2])).float())
    assert R.check(h, dzr, dza, 1, acc=F.DUAL_OPS, what="dz emulation") <= 1.0
    with pytest.raises(AssertionError, match="max err/tol"):
        R.check(bf(E.fma32(af[:, 0], gg, af[:, 2].expand_as(gg)).float()), dzr, dza, 1, acc=F.DUAL_OPS, what="B z dropped")
    with pytest.raises(AssertionError, match="max err/tol"):                         # group 1 with group 0's coefficients
        R.check(bf(E.fma32(af[:1, 0], gg, E.fma32(af[:1, 1], zb16, af[:1, 2])).float()), dzr, dza, 1, acc=F.DUAL_OPS, what="gstride")
    # epilogues on the STORED dz: accumulate, BatchNorm-fused
    base = E.rand_bf16(G * P, Cin, seed=5)
    ref, ab, n, extra = F.dual_ref(h.double(), w, base=base, groups=G)
    assert torch.allclose(ref, h.double() @ w.double() + F.gview(base.double(), G), **T64) and extra is not None
    hx = bf(bf(emu_gemm(h, w.t().contiguous())) + F.gview(base.float(), G))
    assert R.check(hx, ref, ab, n, extra=extra, what="accumulate emulation") <= 1.0
    zin, vin = E.act_data(G * P, Cin, 2, 6), E.bn_vectors(G, Cin, 7, 2)
    ref, ab, n, extra = F.dual_ref(h.double(), w, z_in=zin, bn_vec=vin, act=2, groups=G)
    m = F.gview(R.bn_mask(zin.reshape(G * P, 1, 1, Cin), vin, 2, G), G)
    assert extra is None and torch.allclose(ref, (h.double() @ w.double()) * m, **T64) and (m == 0).any() and (m == 1).any()


def test_gram_models():
    G, P, C = 2, 3000, 256
    x, v = E.act_data(G * P, C, 1, 1), E.bn_vectors(G, C, 2).reshape(-1)
    a = F.operand(x, v, v[C:], 1, G, 4 * C)
    Gr, Ga, sr, sa, n = F.gram_ref(a)
    assert n == P and torch.allclose(Gr, torch.einsum("gpi,gpj->gij", a, a), **T64) and torch.allclose(sr, a.sum(1), **T64)
    # emulation: float32 partials per split of 256 pixels, the splits summed in float64 and rounded once
    parts = [emu_gemm(a[:, p0:p0 + 256].transpose(1, 2), a[:, p0:p0 + 256].transpose(1, 2)).double() for p0 in range(0, P, 256)]
    Gh = torch.stack(parts).sum(0).float()
    Gh = torch.triu(Gh) + torch.triu(Gh, 1).transpose(1, 2)                         # (each unordered block pair computed once and mirrored)
    sh = torch.stack([a[:, p0:p0 + 256].float().sum(1).double() for p0 in range(0, P, 256)]).sum(0).float()
    assert F.gram_check(Gh, sh, a, "emulation") <= 1.0
    # one mirrored 64 x 64 block left unwritten (stale zeros) / holding the untransposed block
    for bad in (torch.zeros(G, 64, 64), Gh[:, 64:128, 0:64].clone()):
        Gb = Gh.clone()
        Gb[:, 0:64, 64:128] = bad
        with pytest.raises(AssertionError):
            F.gram_check(Gb, sh, a, "mirrored block")
    # a partial of one split missing; group 1 with group 0's vectors
    with pytest.raises(AssertionError, match="per element"):
        F.gram_check(Gh, (sh.double() - a[:, -100:].sum(1)).float(), a, "tail of s dropped")
    with pytest.raises(AssertionError, match="per element"):
        F.gram_check(Gh, sh, F.operand(x, v, v[C:], 1, G, 0), "gstride")


def test_gram_stats_ref_equals_the_statistics_of_z():
    G, P, Cin, Cout = 2, 500, 64, 96
    a = E.rand_bf16(G * P, Cin, seed=1).double().reshape(G, P, Cin) + 1.0
    w = F.weight(Cout, Cin, 2)
    Gm, sv = torch.einsum("gpi,gpj->gij", a, a), a.sum(1)
    ref, tol = F.gram_stats_ref(w, Gm, sv)
    z = a @ w.double().t()
    assert torch.allclose(ref, torch.cat([z.sum(1), (z * z).sum(1)], 1), rtol=1e-11, atol=1e-9) and (tol > 0).all()
    assert F.ratio(ref, ref, tol) == 0.0
    f32 = torch.cat([sv.float() @ w.t(), torch.einsum("oi,gij,oj->go", w, Gm.float(), w)], 1)
    ref32, tol32 = F.gram_stats_ref(w, Gm.float(), sv.float())
    assert F.ratio(f32, ref32, tol32) > 1.0, "float32 accumulation must not pass a float64 model"


def test_tpool_bwd_code_prod_ref_equals_maxpool3d_autograd():
    G, clips, T, Q, C, Cin = 2, 2, 8, 7, 16, 8
    To = T // 2
    x = torch.randint(-3, 4, (G * clips, C, T, Q, 1), generator=F.gen(1)).double().requires_grad_(True)
    y, idx = Fn.max_pool3d(Fn.relu(x), (3, 1, 1), (2, 1, 1), (1, 0, 0), return_indices=True)
    gy = E.rand_bf16(G * clips * To, Q, C, seed=2)
    gyn = gy.double().reshape(G * clips, To, Q, C).permute(0, 3, 1, 2).unsqueeze(-1)
    (y * gyn).sum().backward()
    frame = (idx[..., 0] // Q).permute(0, 2, 3, 1)                                      # [N, To, Q, C]
    tap = frame - (2 * torch.arange(To).reshape(1, -1, 1, 1) - 1)
    code = torch.where(y[..., 0].permute(0, 2, 3, 1) <= 0, torch.full_like(tap, 3), tap).reshape(G * clips * To, Q, C)
    a = E.rand_bf16(G * clips * T * Q, Cin, seed=3).double().reshape(G, -1, Cin)
    g2, pr, pa, n = F.tpool_bwd_code_prod_ref(gy, code, a, T, G)
    want = x.grad[..., 0].permute(0, 2, 3, 1).reshape(G, clips * T * Q, C)              # (ReLU of x: zero gradient where the maximum is 0)
    assert torch.equal(g2, R.bf16(want)) and n == clips * T * Q
    assert torch.allclose(pr, torch.einsum("gpc,gpk->gck", g2, a), **T64)
    assert torch.equal(F.unpack_codes(E.pack_codes(code), code.shape), code)


def test_pack_references_are_the_documented_layouts():
    w = torch.randn(24, 10, 3, 3, generator=F.gen(1))
    f, d, dw = F.pack_ref(w, 16, 0), F.pack_ref(w, 16, 1), F.pack_ref(torch.randn(12, 1, 3, 3, generator=F.gen(2)), 1, 2)
    wb = w.to(torch.bfloat16)
    assert f.shape == (24, 9, 16) and torch.equal(f[:, :, :10], wb.reshape(24, 10, 9).permute(0, 2, 1)) and (f[:, :, 10:] == 0).all()
    assert d.shape == (16, 9, 24) and torch.equal(d[:10], torch.flip(wb.reshape(24, 10, 9), [2]).permute(1, 2, 0)) and (d[10:] == 0).all()
    assert dw.shape == (9, 12) and dw.dtype == torch.float32
    rows, blk = F.pack_table([(24, 10, 3, 3, 0, 16), (12, 1, 3, 3, 2, 1), (24, 10, 3, 3, 1, 16)], [(1, 2), (3, 4), (5, 6)], 2048)
    assert [r[5] for r in rows] == [0, 2, 3] and blk == 5 and rows[1][2] == 12 | (1 << 32) and rows[2][4] == 3 | (1 << 32)


# -------------------------------------------------------------------------------------------------------------------------------- chain
def test_chain_reference_is_train_mode_batchnorm_and_its_bound_is_first_order():
    G, P, Cin, Cout, eps = 2, 600, 64, 32, 1e-5
    row = dict(id="cpu-chain", G=G, P=P, Cin=Cin, Cout=Cout, in_act=1, act=1, idn="plain")
    op = F.fadd_operands(row)
    op["w"] = F.weight(Cout, Cin, 4)
    gamma, beta = (torch.rand(Cout, generator=F.gen(5)) + 0.5).float(), (torch.randn(Cout, generator=F.gen(6)) * 0.3).float()
    ch = F.chain_reference(row, op, gamma, beta, eps)
    r = F.fadd_reference(row, op)
    z = r["a"] @ op["w"].double().t()
    bn = torch.stack([Fn.batch_norm(z[g], None, None, gamma.double(), beta.double(), True, 0.1, eps) for g in range(G)])
    want = Fn.relu(bn + F.gview(op["idn"].double(), G))
    assert torch.allclose(ch["ref"], want, rtol=1e-9, atol=1e-9)
    # the vectors of an emulated chain (float32 Gram sums -> float64 statistics -> float32 vectors) lie inside the propagated bound, a
    # variance computed from the Gram matrix of the wrong group does not
    a32 = r["a"].float()
    Gm, sv = torch.einsum("gpi,gpj->gij", a32, a32), a32.sum(1)
    wd = op["w"].double()
    s1, s2 = sv.double() @ wd.t(), torch.einsum("oi,gij,oj->go", wd, Gm.double(), wd)
    mu, var = s1 / P, s2 / P - (s1 / P) ** 2
    inv = 1 / torch.sqrt(var + eps)
    vec = torch.stack([gamma.double() * inv, beta.double() - mu * gamma.double() * inv, mu, inv], 1).float()
    assert F.ratio(vec, ch["vec"], ch["vec_tol"]) <= 1.0
    assert F.ratio(torch.flip(vec, [0]), ch["vec"], ch["vec_tol"]) > 1.0
    assert (ch["tol"] >= r["tol"] * 0).all() and (ch["vec_tol"] > 0).all()


# --------------------------------------------------------------------------------------------------------------------- undecided share
@pytest.mark.parametrize("row", F.FORWARD_ROWS, ids=[r["id"] for r in F.FORWARD_ROWS])
def test_undecided_share_of_every_gpu_row_is_at_most_one_percent(row):
    share = F.undecided_share(row)
    assert 0.0 <= share <= F.UNDECIDED_CAP, "%s: %.4f of the elements are undecided" % (row["id"], share)
    assert F.UNDECIDED_CAP == 0.01 and not math.isnan(share)
