"""tests/abi_ref.py on the CPU: every reference is anchored to an independent statement of the same operation (torch.optim stepped in
float64, F.linear / adaptive_avg_pool2d, F.interpolate, nn.LSTMCell and the arithmetic of F.gumbel_softmax in float64, the explicit
dz = A g + B z + C BatchNorm backward through float64 autograd), the tie share of every policy row's seed is asserted, and every error
model is self-tested: a float32 emulation of the kernel's own expression passes it, the planted error of the same row fails it."""
import pytest
import torch
import torch.nn.functional as F

from tests import abi_ref as A
from tests import conv_ref as R
from tests import elementwise_ref as E

T64 = dict(rtol=1e-12, atol=1e-13)


# ------------------------------------------------------------------------------------------------------------- algebraic BatchNorm backward
def _alg_case(Cout=64, Cin=16, G=2, P=50, seed=3):
    w, aff = A.alg_operands(Cout, Cin, G, seed)
    g = E.rand_bf16(G * P, Cout, seed=seed + 1)
    a = E.rand_bf16(G * P, Cin, seed=seed + 2)
    return w, aff, g, a


def test_alg_references_equal_the_explicit_batchnorm_backward():
    """dx and dW of z = W a, dz = A g' + B z + C through float64 autograd == the algebraic formulas the references restate"""
    Cout, Cin, G, P = 64, 16, 2, 50
    w, aff, g, a = _alg_case(Cout, Cin, G, P)
    W = w.double().requires_grad_(True)
    av = a.double().reshape(G, P, Cin).requires_grad_(True)
    gv = g.double().reshape(G, P, Cout)
    z = torch.einsum("gpi,oi->gpo", av, W)
    af = aff.double()
    dz = af[:, 0].unsqueeze(1) * gv + af[:, 1].unsqueeze(1) * z.detach() + af[:, 2].unsqueeze(1)
    (z * dz).sum().backward()
    pk = A.alg_pack_ref(w, aff)
    x = torch.cat([gv, av.detach()], 2)
    w_alg = torch.cat([pk["wa"][0], pk["m"][0]], 2)
    dx = torch.einsum("gpk,gck->gpc", x, w_alg) + pk["epi"][0].unsqueeze(1)
    assert torch.allclose(dx, av.grad, **T64)
    Pm = torch.einsum("gpo,gpi->goi", gv, av.detach())
    Gm = torch.einsum("gpi,gpj->gij", av.detach(), av.detach())
    sv = av.detach().sum(1)
    dw, _ = A.alg_wgrad_combine_ref(w, aff, Pm, G=Gm, s=sv)
    assert torch.allclose(dw, W.grad, **T64)
    # the wg_pre form reads W G_g laid out [Cout][groups * Cin]
    wg = torch.einsum("oj,gji->ogi", w.double(), Gm).reshape(Cout, G * Cin)
    base = A.randn32(Cout, Cin, seed=9)
    dw2, _ = A.alg_wgrad_combine_ref(w, aff, Pm, wg_pre=wg, s=sv, dw0=base)
    assert torch.allclose(dw2, W.grad + base.double(), **T64)
    # sum(g' zhat) = invstd (W . P - mean sum g')
    vec = E.bn_vectors(G, Cout, 5)
    zh = (z.detach() - vec[:, 2].double().unsqueeze(1)) * vec[:, 3].double().unsqueeze(1)
    ref, tol = A.alg_sumfix_ref(w, Pm, vec, gv.sum(1))
    assert torch.allclose(ref, (gv * zh).sum(1), rtol=1e-10, atol=1e-10)
    assert (tol > 0).all()


def _pack_f32(w, aff, use_a_for_b=False):
    """alg_pack_kernel in float32 on the CPU (sequential accumulation instead of four split accumulators: same model)"""
    Cout, Cin = w.shape
    Gn = aff.shape[0]
    wa = (w.t().unsqueeze(0) * aff[:, 0].unsqueeze(1)).to(torch.bfloat16)
    B = aff[:, 0 if use_a_for_b else 1]
    m = torch.zeros(Gn, Cin, Cin)
    epi = torch.zeros(Gn, Cin)
    for co in range(Cout):
        m = m + (w[co].unsqueeze(0).unsqueeze(2) * B[:, co].reshape(Gn, 1, 1)) * w[co].reshape(1, 1, Cin)
        epi = epi + w[co].unsqueeze(0) * aff[:, 2, co].unsqueeze(1)
    return wa, m.to(torch.bfloat16), epi


def test_alg_pack_model_passes_fp32_and_fails_planted():
    w, aff, _, _ = _alg_case()
    pk = A.alg_pack_ref(w, aff)
    wa, m, epi = _pack_f32(w, aff)
    assert A.ratio(wa, *pk["wa"]) <= 1.0 and A.ratio(m, *pk["m"]) <= 1.0 and A.ratio(epi, *pk["epi"]) <= 1.0
    _, m_bad, _ = _pack_f32(w, aff, use_a_for_b=True)                      # A where B belongs
    assert A.ratio(m_bad, *pk["m"]) > 1.0
    # one rounding too many on the large term: W * A rounded to bf16 BEFORE the product with A
    wa_bad = (w.to(torch.bfloat16).float().t().unsqueeze(0) * aff[:, 0].unsqueeze(1)).to(torch.bfloat16)
    assert A.ratio(wa_bad, *pk["wa"]) > 1.0
    # m_pre is read [g][ci][cj]: a transposed read fails the exact comparison
    mp = A.randn32(2, 16, 16, seed=4)
    pm = A.alg_pack_ref(w, aff, m_pre=mp)
    assert A.ratio(mp.to(torch.bfloat16), *pm["m"]) == 0.0
    assert A.ratio(mp.transpose(1, 2).to(torch.bfloat16), *pm["m"]) > 1.0


def test_alg_wgrad_combine_model():
    Cout, Cin, G, P = 64, 16, 3, 40
    w, aff, g, a = _alg_case(Cout, Cin, G, P, seed=7)
    gv, av = g.float().reshape(G, P, Cout), a.float().reshape(G, P, Cin)
    Pm, Gm, sv = torch.einsum("gpo,gpi->goi", gv, av), torch.einsum("gpi,gpj->gij", av, av), av.sum(1)
    base = A.randn32(Cout, Cin, seed=8)
    ref, tol = A.alg_wgrad_combine_ref(w, aff, Pm, G=Gm, s=sv, dw0=base)
    accum = torch.zeros(Cout, Cin)
    for gi in range(G):
        accum = accum + (aff[gi, 0].unsqueeze(1) * Pm[gi] + aff[gi, 1].unsqueeze(1) * (w @ Gm[gi]) + aff[gi, 2].unsqueeze(1) * sv[gi].unsqueeze(0))
    assert A.ratio(base + accum, ref, tol) <= 1.0
    bad = base + accum - aff[G - 1, 2].unsqueeze(1) * sv[G - 1].unsqueeze(0) + aff[G - 1, 2].unsqueeze(1) * sv[0].unsqueeze(0)   # s of the wrong group
    assert A.ratio(bad, ref, tol) > 1.0
    assert A.ratio(accum, ref, tol) > 1.0                                  # the base dW dropped


def test_alg_sumfix_model_is_absolute_and_sees_the_mean_term():
    """|mean| / std = 40 and a small sum(g' zhat): an fp64 evaluation passes, float32 does not, nor does the formula without mean * s1"""
    Cout, Cin, G, P = 32, 16, 2, 400
    w, _ = A.alg_operands(Cout, Cin, G, 11)
    a = E.rand_bf16(G * P, Cin, seed=12).double().reshape(G, P, Cin) + 1.0
    z = torch.einsum("gpi,oi->gpo", a, w.double())
    mean, std = z.mean(1), z.std(1)
    shift = 40.0 * std - mean.abs()
    gp = E.rand_bf16(G * P, Cout, seed=13).double().reshape(G, P, Cout)
    vec = torch.zeros(G, 4, Cout)
    vec[:, 2], vec[:, 3] = (mean + torch.sign(mean) * shift).float(), (1.0 / std).float()
    Pm = torch.einsum("gpo,gpi->goi", gp, a).float()
    s1 = gp.sum(1)
    ref, tol = A.alg_sumfix_ref(w, Pm, vec, s1)
    v = vec.double()
    h64 = v[:, 3] * ((w.double().unsqueeze(0) * Pm.double()).sum(2) - v[:, 2] * s1)
    assert A.ratio(h64, ref, tol) <= 1.0
    assert ((v[:, 2].abs() * v[:, 3]).min() >= 30.0)
    h32_ = vec[:, 3] * ((w.unsqueeze(0) * Pm).sum(2) - vec[:, 2] * s1.float())
    assert A.ratio(h32_, ref, tol) > 1.0
    assert A.ratio(v[:, 3] * (w.double().unsqueeze(0) * Pm.double()).sum(2), ref, tol) > 1.0


def test_dgrad_alg_model():
    Cout, Cin, G, P = 64, 16, 2, 37
    _, _, g, a = _alg_case(Cout, Cin, G, P, seed=21)
    w_alg = E.rand_bf16(G, Cin, Cout + Cin, scale=0.2, seed=22)
    epi = A.randn32(G, Cin, seed=23, scale=0.1)
    vec = E.bn_vectors(G, Cin, 24)
    vf = vec.reshape(-1)
    base = E.rand_bf16(G * P, Cin, seed=25)
    av = R.lazy_operand(a.reshape(G * P, 1, 1, Cin), vf, vf[Cin:], 1, G, 4 * Cin).reshape(G, P, Cin).float()
    x = torch.cat([g.float().reshape(G, P, Cout), av], 2)
    gemm = torch.einsum("gpk,gck->gpc", x, w_alg.float())
    for tile in (True, False):
        for b in (None, base):
            ref, ab, n, extra, k = A.dgrad_alg_ref(g, a, vf, vf[Cin:], 1, 4 * Cin, w_alg, epi, G, tile, base=b)
            f = gemm.to(torch.bfloat16).float() if tile else gemm
            f = f + epi.unsqueeze(1)
            if b is not None:
                f = f.to(torch.bfloat16).float() + b.float().reshape(G, P, Cin)
            assert A.dgrad_alg_check(f.to(torch.bfloat16).reshape(G * P, Cin), ref, ab, n, extra, k) <= 1.0
    ref, ab, n, extra, k = A.dgrad_alg_ref(g, a, vf, vf[Cin:], 1, 4 * Cin, w_alg, epi, G, False)
    with pytest.raises(AssertionError):                                    # epi_add of the other group
        A.dgrad_alg_check((gemm + epi.flip(0).unsqueeze(1)).to(torch.bfloat16).reshape(G * P, Cin), ref, ab, n, extra, k)
    with pytest.raises(AssertionError):                                    # the lazy transform of a skipped
        x0 = torch.cat([g.float().reshape(G, P, Cout), a.float().reshape(G, P, Cin)], 2)
        A.dgrad_alg_check((torch.einsum("gpk,gck->gpc", x0, w_alg.float()) + epi.unsqueeze(1)).to(torch.bfloat16).reshape(G * P, Cin), ref, ab, n, extra, k)


# ----------------------------------------------------------------------------------------------------------------------------- gemm_f32
@pytest.mark.parametrize("K", [0, 3, 65, 2560])
def test_gemm_model(K):
    a, b = A.randn32(37, K, seed=K + 1), A.randn32(70, K, seed=K + 2)
    bias, c0 = A.randn32(70, seed=K + 3), A.randn32(37, 70, seed=K + 4)
    ref, tol = A.gemm_f32_ref(a, b, bias, 1, c0)
    assert torch.allclose(ref, F.relu(F.linear(a.double(), b.double(), bias.double())) + c0.double(), **T64)
    h = F.relu(F.linear(a, b, bias)) + c0
    assert A.ratio(h, ref, tol) <= 1.0
    if K >= 16:
        hb = F.relu(F.linear(a[:, :K - 1], b[:, :K - 1], bias)) + c0       # the last K column dropped (a tail predicate always false)
        assert A.ratio(hb, ref, tol) > 1.0
        hr = F.relu(F.linear(a, b, bias).to(torch.bfloat16).float()) + c0  # one rounding too many on the large term
        assert A.ratio(hr, ref, tol) > 1.0
    else:
        assert A.ratio(F.relu(F.linear(a, b)) + c0, ref, tol) > 1.0        # bias dropped


# --------------------------------------------------------------------------------------------------------------------------------- head
def test_head_references_and_models():
    clips, T, HW, C, K, G = 6, 3, 49, 32, 10, 3
    x = E.act_data(clips * T * HW, C, 2, 31).reshape(clips * T, HW, C)
    vec = E.bn_vectors(G, C, 32, 2)
    vf = vec.reshape(-1)
    keep = (torch.rand(clips * T, C, generator=E.gen(33)) > 0.5).to(torch.uint8)
    keep[4] = 0
    W, bias = A.randn32(K, C, seed=34, scale=0.1), A.randn32(K, seed=35)
    ref, tol = A.head_feat_ref(x, vf, vf[C:], 4 * C, 2, keep, 2.0, T, HW, G)
    # independent statement: adaptive_avg_pool2d of the clamped affine, dropout as a mask, linear, mean over the frames
    xs = x.double().reshape(G, -1, HW, C)
    act = torch.clamp((xs * vec[:, 0].double().reshape(G, 1, 1, C) + vec[:, 1].double().reshape(G, 1, 1, C)).float().double(), 0, 6)
    pooled = F.adaptive_avg_pool2d(act.reshape(clips * T, 7, 7, C).permute(0, 3, 1, 2), 1).reshape(clips * T, C) * keep.double() * 2.0
    assert torch.allclose(ref, pooled, **T64)
    v32 = E.lazy_f32(x.reshape(clips * T, HW, 1, C), vf, vf[C:], 2, G, 4 * C).reshape(clips * T, HW, C).float()
    f32_ = v32.sum(1) * (1.0 / HW) * keep.float() * 2.0
    assert A.ratio(f32_, ref, tol) <= 1.0
    assert A.ratio(v32.to(torch.bfloat16).float().sum(1) * (1.0 / HW) * keep.float() * 2.0, ref, tol) > 1.0     # operand rounded to bf16
    lref, ltol = A.head_logits_ref(f32_, W, bias, T)
    assert torch.allclose(lref, F.linear(f32_.double(), W.double(), bias.double()).reshape(clips, T, K).mean(1), **T64)
    assert A.ratio(F.linear(f32_, W).reshape(clips, T, K).sum(1) / T + bias, lref, ltol) <= 1.0
    assert A.ratio((F.linear(f32_, W).reshape(clips, T, K).sum(1) + bias) / T, lref, ltol) > 1.0                  # the bias divided by T too
    # backward: autograd of the same float64 head
    g = A.randn32(clips, K, seed=36)
    xa = act.reshape(clips * T, HW, C).clone().requires_grad_(True)
    lg = F.linear(xa.mean(1) * keep.double() * 2.0, W.double(), bias.double()).reshape(clips, T, K).mean(1)
    (lg * g.double()).sum().backward()
    gx, gab, k, grows = A.head_bwd_ref(g, keep, 2.0, W, T, HW)
    assert torch.allclose(gx, xa.grad, **T64)
    h = ((g @ W) * (1.0 / (T * HW))).repeat_interleave(T, 0) * keep.float() * 2.0
    hx = h.to(torch.bfloat16).unsqueeze(1).expand(-1, HW, -1)
    assert R.check(hx, gx, gab, 1, acc=k) <= 1.0
    with pytest.raises(AssertionError):                                    # scaled by 1 / HW instead of 1 / (T HW)
        R.check((h * T).to(torch.bfloat16).unsqueeze(1).expand(-1, HW, -1), gx, gab, 1, acc=k)
    assert (gx[4] == 0).all()
    assert A.ratio(g.repeat_interleave(T, 0) / T, grows, A.U32 * grows.abs()) <= 1.0


def test_colsum_model():
    a, o = A.randn32(300, 17, seed=41), A.randn32(17, seed=42)
    ref, tol = A.colsum_ref(a, o)
    s = torch.zeros(17)
    for r in range(300):
        s = s + a[r]
    assert A.ratio(o + s, ref, tol) <= 1.0
    assert A.ratio(s, ref, tol) > 1.0
    ref0, tol0 = A.colsum_ref(a[:0])
    assert (ref0 == 0).all() and (tol0 == 0).all()
    ref1, tol1 = A.colsum_ref(a[:1])
    assert torch.equal(ref1, a[0].double())


# --------------------------------------------------------------------------------------------------------------------------- optimizers
SGD_CASES = [(mu, nes, first, wd) for mu in (0.0, 0.9) for nes in (0, 1) for first in (1, 0) for wd in (0.0, 5e-4) if not (nes and mu == 0.0)]


def _sgd_f32(p, g, mom, lr, mu, wd, nes, first, stale_nesterov=False):
    lr, mu, wd = (torch.tensor(x, dtype=torch.float32) for x in (lr, mu, wd))
    d = g + wd * p
    b = mom
    if mu != 0:
        b = d if first else mu * mom + d
        d = (d + mu * (mom if stale_nesterov else b)) if nes else b
    return p - lr * d, b


@pytest.mark.parametrize("mu,nes,first,wd", SGD_CASES)
def test_sgd_reference_is_torch_optim_and_model_holds(mu, nes, first, wd):
    n, lr = 1000, 0.05
    p, g, mom = A.randn32(n, seed=51, scale=0.05), A.randn32(n, seed=52), A.randn32(n, seed=53)
    q = torch.nn.Parameter(p.double())
    opt = torch.optim.SGD([q], lr=A.h32(lr), momentum=A.h32(mu), weight_decay=A.h32(wd), nesterov=bool(nes))
    if mu != 0 and not first:
        opt.state[q]["momentum_buffer"] = mom.double().clone()
    q.grad = g.double()
    opt.step()
    out = A.sgd_ref(p, g, mom, lr, mu, wd, nes, first)
    assert torch.allclose(out["upd"][0], q.detach() - p.double(), rtol=1e-11, atol=1e-14)
    if mu != 0:
        assert torch.allclose(out["mom"][0], opt.state[q]["momentum_buffer"], **T64)
    pn, b = _sgd_f32(p, g, mom, lr, mu, wd, nes, first)
    assert A.ratio(A.update_of(pn, p), *out["upd"]) <= 1.0
    if mu != 0:
        assert A.ratio(b, *out["mom"]) <= 1.0
    if nes and not first:
        pb, _ = _sgd_f32(p, g, mom, lr, mu, wd, nes, first, stale_nesterov=True)     # Nesterov using mom before its update
        assert A.ratio(A.update_of(pb, p), *out["upd"]) > 1.0


def _adam_f32(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2):
    t = lambda x: torch.tensor(x, dtype=torch.float32)      # noqa: E731
    lr, b1, b2, eps, wd, bc1, bc2 = (t(x) for x in (lr, b1, b2, eps, wd, bc1, bc2))
    d = g + wd * p
    mi = b1 * m + (1 - b1) * d
    vi = b2 * v + (1 - b2) * d * d
    return p - (lr / bc1) * mi / (torch.sqrt(vi) / torch.sqrt(bc2) + eps), mi, vi


@pytest.mark.parametrize("step", [1, 2, 3, 10, 1000])
def test_adam_reference_is_torch_optim_and_model_sees_bc2(step):
    n, lr, b1, b2, eps, wd = 1000, 1e-2, 0.9, 0.999, 1e-8, 5e-4
    p, g = A.randn32(n, seed=61, scale=0.02), A.randn32(n, seed=62)
    m, v = A.randn32(n, seed=63, scale=0.3), A.randn32(n, seed=64).abs() * 0.5
    if step == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    q = torch.nn.Parameter(p.double())
    opt = torch.optim.Adam([q], lr=A.h32(lr), betas=(A.h32(b1), A.h32(b2)), eps=A.h32(eps), weight_decay=A.h32(wd))
    opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.double().clone(), "exp_avg_sq": v.double().clone()}
    q.grad = g.double()
    opt.step()
    out = A.adam_ref(p, g, m, v, lr, b1, b2, eps, wd, step)
    assert torch.allclose(out["upd"][0], q.detach() - p.double(), rtol=1e-10, atol=1e-15)
    assert torch.allclose(out["m"][0], opt.state[q]["exp_avg"], **T64) and torch.allclose(out["v"][0], opt.state[q]["exp_avg_sq"], **T64)
    bc1, bc2 = A.adam_bias_corrections(b1, b2, step)
    pn, mi, vi = _adam_f32(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2)
    assert A.ratio(A.update_of(pn, p), *out["upd"]) <= 1.0
    assert A.ratio(mi, *out["m"]) <= 1.0 and A.ratio(vi, *out["v"]) <= 1.0
    pb, _, _ = _adam_f32(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2 * (1 + 2e-5))          # bc2 wrong by 2e-5
    assert A.ratio(A.update_of(pb, p), *out["upd"]) > 1.0
    _, _, vb = _adam_f32(p, g, m, v, lr, b1, b2 * (1 - 1e-6), eps, wd, bc1, bc2)
    assert A.ratio(vb, *out["v"]) > 1.0


def test_lazy_colsum_model():
    G, P, C = 2, 500, 16
    x = E.act_data(G * P, C, 1, 71)
    vec = E.bn_vectors(G, C, 72)
    vf = vec.reshape(-1)
    ref, ab, n = A.lazy_colsum_ref(x, vf, vf[C:], 4 * C, 1, G)
    v = R.lazy_operand(x.reshape(G * P, 1, 1, C), vf, vf[C:], 1, G, 4 * C).reshape(G, P, C).float()
    assert A.f32_sum_check(v.sum(1), ref, ab, n) <= 1.0
    u = R.lazy_operand(x.reshape(G * P, 1, 1, C), vf, vf[C:], 1, G, 4 * C, round_bf16=False).reshape(G, P, C).float()
    with pytest.raises(AssertionError):                                    # the operand not rounded to bf16
        A.f32_sum_check(u.sum(1), ref, ab, n)


# ------------------------------------------------------------------------------------------------------------ policy head, gate, fusion
def test_policy_reference_is_lstmcell_and_gumbel_softmax():
    """policy_run in float64 == nn.LSTMCell (float64) over cat(feat, previous logits) + nn.Linear heads + the arithmetic of
    F.gumbel_softmax(hard=True)[..., -1] with the exponential draw given"""
    M, B, S, tau = 3, 4, 3, 5.0
    op = A.policy_operands(M, B, S, 81)
    g = E.gen(82)
    feat = torch.randn(S, B, A.FEAT, generator=g, dtype=torch.float64)
    b_ih = torch.randn(4 * A.HID, generator=g, dtype=torch.float64) * 0.05
    op["gates_x"] = feat @ op["w_ih"].double()[:, :A.FEAT].t() + b_ih
    ref = A.policy_run(op, tau, torch.float64, True)
    cell = torch.nn.LSTMCell(A.FEAT + 2 * M, A.HID).double()
    with torch.no_grad():
        cell.weight_ih.copy_(op["w_ih"]), cell.weight_hh.copy_(op["w_hh"]), cell.bias_ih.copy_(b_ih), cell.bias_hh.copy_(op["b_hh"])
    h, c = torch.zeros(B, A.HID, dtype=torch.float64), torch.zeros(B, A.HID, dtype=torch.float64)
    prev = torch.zeros(B, 2 * M, dtype=torch.float64)
    decs, lgs = [], []
    for s in range(S):
        h, c = cell(torch.cat([feat[s], prev], 1), (h, c))
        lg = torch.cat([F.linear(h, op["fc_w"][m].double(), op["fc_b"][m].double()) for m in range(M)], 0)      # [M*B, 2]
        gum = -torch.log(op["expo"][s].double().reshape(M * B, 2))
        y = F.softmax((lg + gum) / A.h32(tau), dim=-1)
        hard = torch.zeros_like(y).scatter_(-1, y.argmax(-1, keepdim=True), 1.0)
        decs.append((hard - y.detach() + y)[:, -1].reshape(M, B))
        lgs.append(lg.reshape(M, B, 2))
        prev = lg.reshape(M, B, 2).permute(1, 0, 2).reshape(B, 2 * M)
    loss = (torch.stack(decs) * op["d_dec"].double()).sum() + (torch.stack(lgs) * op["d_logits_in"].double()).sum()
    gw = torch.autograd.grad(loss, [cell.weight_hh, cell.weight_ih])
    assert torch.allclose(ref["decisions"], torch.stack(decs).detach(), **T64) and torch.allclose(ref["logits"], torch.stack(lgs).detach(), **T64)
    assert torch.allclose(ref["h_all"][-1], h.detach(), **T64) and torch.allclose(ref["c_all"][-1], c.detach(), **T64)
    # the weight gradients are GEMMs over d_gates: d W_hh = sum_s d_gates[s]^T h_all[s], d W_ih[:, F:] = sum_s d_gates[s]^T prev_all[s]
    assert torch.allclose(torch.einsum("sbr,sbk->rk", ref["d_gates"], ref["h_all"][:-1]), gw[0], rtol=1e-10, atol=1e-12)
    assert torch.allclose(torch.einsum("sbr,sbk->rk", ref["d_gates"], ref["prev_all"]), gw[1][:, A.FEAT:], rtol=1e-10, atol=1e-12)


def _swap_f_g(op):
    """the operands with the f and g gate blocks exchanged: the reference on them == a kernel that reads the gates in the order i, g, f, o"""
    o = dict(op)
    idx = torch.cat([torch.arange(0, 256), torch.arange(512, 768), torch.arange(256, 512), torch.arange(768, 1024)])
    o["gates_x"], o["w_ih"], o["w_hh"], o["b_hh"] = op["gates_x"][..., idx], op["w_ih"][idx], op["w_hh"][idx], op["b_hh"][idx]
    return o


def test_policy_gate_sees_the_planted_defects():
    """16 E32 against: the logit feedback detached, the feedback laid out [j][m], the gate order swapped"""
    op = A.policy_operands(3, 5, 3, 83)
    r64, r32 = A.policy_run(op, 5.0, torch.float64, True), A.policy_run(op, 5.0, torch.float32, True)
    for k in A.POLICY_TENSORS:
        assert A.e32_ratio(r32[k], r64[k], r32[k])[2] <= 1.0 / A.E32_FACTOR + 1e-12
    worst = {}
    for name, bad in (("detach", A.policy_run(op, 5.0, torch.float64, True, detach_feedback=True)),
                      ("layout", A.policy_run(op, 5.0, torch.float64, True, swap_prev=True)),
                      ("order", A.policy_run(_swap_f_g(op), 5.0, torch.float64, True))):
        worst[name] = max(A.e32_ratio(bad[k], r64[k], r32[k])[2] for k in A.POLICY_TENSORS)
        assert worst[name] > 100.0, (name, worst[name])
    # the forward tensors alone see the layout and the order; the detached feedback only shows in the gradients
    assert A.e32_ratio(A.policy_run(op, 5.0, torch.float64, True, swap_prev=True)["logits"], r64["logits"], r32["logits"])[2] > 100.0


@pytest.mark.parametrize("row", A.POLICY_ROWS, ids=[A.policy_id(r) for r in A.POLICY_ROWS])
def test_policy_rows_have_few_ties(row):
    """the seeds of the GPU rows: the reference alone excludes at most 1 % of a row's decisions as ties, and E32 is measurable (> 0) for
    every compared tensor that is not identically zero"""
    M, B, S, dlin = row
    op = A.policy_operands(M, B, S, A.policy_seed(row))
    r64, r32 = A.policy_run(op, A.POLICY_TAU, torch.float64, dlin), A.policy_run(op, A.POLICY_TAU, torch.float32, dlin)
    assert A.decided(r64["ysoft"], r32["ysoft"])[1] <= 0.01
    A.decision_check(r32["decisions"], r64["ysoft"], r32["ysoft"], A.policy_id(row))
    for k in A.POLICY_TENSORS:
        if r64[k].abs().max() > 0:
            assert A.rel_max(r32[k], r64[k]) > 0, k


def test_gate_references():
    lg, ex, dd = A.gate_operands(37, 84)
    l64 = lg.double().requires_grad_(True)
    d, y = A.gate(l64, ex.double(), A.h32(5.0))
    (d * dd.double()).sum().backward()
    ys32 = A.gate(lg, ex, torch.tensor(5.0))[1]
    ref, tol = A.gate_bwd_ref(dd, ys32, 5.0)
    # from the float32 ysoft the kernel reads: autograd of the float64 gate agrees to the float32 rounding of ysoft
    assert torch.allclose(ref, l64.grad, rtol=1e-5, atol=1e-7)
    y32, dy = ys32, dd
    dot = dy * y32[:, 1]
    h = torch.stack([y32[:, 0] * (0.0 - dot) / 5.0, y32[:, 1] * (dy - dot) / 5.0], 1)
    assert A.ratio(h, ref, tol) <= 1.0
    assert A.ratio(torch.stack([h[:, 1], h[:, 0]], 1), ref, tol) > 1.0
    assert A.decided(y.detach(), ys32.double())[1] <= 0.03        # one row of 37
    assert (ex.min() <= 1e-30) and (ex.max() >= 80.0)


@pytest.mark.parametrize("M,learn,gated", [(1, False, True), (3, True, True), (4, True, False), (2, False, False), (4, False, True)])
def test_fusion_references_and_models(M, learn, gated):
    S, B, C = 3, 5, 31
    xs = [A.randn32(S * B, C, seed=90 + m) for m in range(M)]
    dec = (torch.rand(S, M, B, generator=E.gen(95)) > 0.4).float() if gated else None
    lf = (torch.rand(M - 1, generator=E.gen(96)) * 0.4).float() if learn and M > 1 else None
    g = A.randn32(B, C, seed=97)
    x64 = [t.double().requires_grad_(True) for t in xs]
    d64_ = dec.double().requires_grad_(True) if gated else None
    w64 = (torch.cat([lf.double(), (1 - lf.double().sum()).reshape(1)]) if lf is not None else torch.full((M,), 1.0 / M, dtype=torch.float64)).requires_grad_(True)
    out = sum(w64[m] * x64[m].reshape(S, B, C) * (d64_[:, m].unsqueeze(2) if gated else 1.0) for m in range(M)).mean(0)
    ref, tol = A.fusion_fwd_ref(xs, dec, lf, S, B)
    assert torch.allclose(ref, out.detach(), **T64)
    (out * g.double()).sum().backward()
    b = A.fusion_bwd_ref(xs, dec, lf, g, S, B)
    assert torch.allclose(b["d_x"][0], torch.stack([t.grad for t in x64]), **T64)
    if gated:
        assert torch.allclose(b["d_dec"][0], d64_.grad, **T64)
    assert torch.allclose(b["d_lf"][0].sum(0), w64.grad, **T64)
    # float32 emulation of the kernels' expressions
    w32 = torch.cat([lf, (1 - lf.sum()).reshape(1)]) if lf is not None else torch.full((M,), 1.0) / M
    d32 = dec if gated else torch.ones(S, M, B)
    acc = torch.zeros(B, C)
    for s in range(S):
        v = torch.zeros(B, C)
        for m in range(M):
            v = v + w32[m] * (xs[m].reshape(S, B, C)[s] * d32[s, m].unsqueeze(1))
        acc = acc + v
    assert A.ratio(acc / S, ref, tol) <= 1.0
    gv = g * (torch.tensor(1.0) / S)
    dx = torch.stack([(gv.unsqueeze(0) * w32[m] * d32[:, m].unsqueeze(2)).reshape(S * B, C) for m in range(M)])
    assert A.ratio(dx, *b["d_x"]) <= 1.0
    dot = torch.stack([(gv.unsqueeze(0) * xs[m].reshape(S, B, C)).sum(2) for m in range(M)], 1)
    assert A.ratio(w32.reshape(1, M, 1) * dot, *b["d_dec"]) <= 1.0
    assert A.ratio((d32 * dot).permute(0, 2, 1).reshape(S * B, M), *b["d_lf"]) <= 1.0
    if lf is not None:
        wb = torch.cat([lf, lf[M - 2:]])                                   # fuse_weight returning lf[m] for the last modality
        accb = sum(wb[m] * xs[m].reshape(S, B, C) * d32[:, m].unsqueeze(2) for m in range(M)).sum(0) / S
        assert A.ratio(accb, ref, tol) > 1.0


# ------------------------------------------------------------------------------------------------------------------------ input kernels
@pytest.mark.parametrize("H,W,OH,OW", [(12, 20, 7, 9), (6, 5, 13, 11), (9, 9, 9, 9), (224, 224, 160, 160)])
def test_clip_reference_is_interpolate_and_model_holds(H, W, OH, OW):
    B, S, Fr, C, step, c_pad = 2, 2, 8, 3, 3, 8
    if H == 224:
        B, S, Fr, step = 1, 1, 2, 1
    x = A.randn32(B, S * Fr * C, H, W, seed=H + OW)
    ref, tol = A.clip_ref(x, B, S, Fr, C, OH, OW, step, c_pad)
    frames = list(range(0, Fr, step))
    v = x.reshape(B, S, Fr, C, H, W)[:, :, frames]
    Fk = len(frames)
    want = v.double()
    if (OH, OW) != (H, W):
        want = F.interpolate(want.reshape(-1, C, H, W), size=(OH, OW), mode="bilinear", align_corners=False).reshape(B, S, Fk, C, OH, OW)
    want = want.permute(1, 0, 2, 4, 5, 3).reshape(S, B * Fk, OH, OW, C)
    # (float32 source coordinates against torch's float64 ones: a coordinate is off by <= 3 u max(H, W), on each axis, and the value moves
    # by at most 2 max|x| per unit of it)
    assert torch.allclose(ref[..., :C], want, rtol=0, atol=2 * 3 * A.U32 * max(H, W) * 2 * x.abs().max().item()) and (ref[..., C:] == 0).all()
    assert A.taps_stable(H, OH) and A.taps_stable(W, OW)
    # float32 emulation of the kernel's expression
    h32 = v
    if (OH, OW) != (H, W):
        h0, h1, lh0, lh1, _ = A.resize_taps(H, OH)
        w0, w1, lw0, lw1, _ = A.resize_taps(W, OW)
        lh0, lh1, lw0, lw1 = lh0.float().reshape(-1, 1), lh1.float().reshape(-1, 1), lw0.float(), lw1.float()
        r0, r1 = v[..., h0, :], v[..., h1, :]
        h32 = lh0 * (lw0 * r0[..., w0] + lw1 * r0[..., w1]) + lh1 * (lw0 * r1[..., w0] + lw1 * r1[..., w1])
    h = torch.zeros(S, B * Fk, OH, OW, c_pad)
    h[..., :C] = h32.permute(1, 0, 2, 4, 5, 3).reshape(S, B * Fk, OH, OW, C)
    assert A.ratio(h.to(torch.bfloat16), ref, tol) <= 1.0
    if Fk > 1:
        bad, _ = A.clip_ref(x, B, S, Fr, C, OH, OW, step, c_pad, frame_offset=1)       # an off-by-one frame index
        assert A.ratio(bad.to(torch.bfloat16), ref, tol) > 1.0
    hb = h.clone()
    hb[..., C] = 1e-3                                                                    # a padded channel not zeroed
    assert A.ratio(hb.to(torch.bfloat16), ref, tol) > 1.0


@pytest.mark.parametrize("diff", [False, True])
def test_clip_u8_reference_and_model(diff):
    B, S, Fr, D, H, W, OH, OW = 2, 2, 4, 2, 10, 12, 7, 8
    C = 3 * D if diff else 3
    CS = C + 3 if diff else C
    x = torch.randint(0, 256, (B, H, W, S * Fr * CS), generator=E.gen(5), dtype=torch.uint8)
    x[0, 0, 0, :2], x[0, 0, 0, 3:5] = torch.tensor([0, 255], dtype=torch.uint8), torch.tensor([255, 0], dtype=torch.uint8)
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    ref, tol = A.clip_u8_ref(x, B, S, Fr, C, OH, OW, 2, 8, mean, std, 1, diff=diff)
    # the reference pipeline: Stack -> ToTorchFormatTensor(div) -> GroupNormalize -> data-layer interpolate
    t = x.reshape(B, H, W, S, Fr, CS).permute(0, 3, 4, 5, 1, 2).double()
    if diff:
        t = torch.floor((t[:, :, :, 3:] - t[:, :, :, :C] + 255.0) * 0.5)
        assert t.min() >= 0 and t.max() <= 255
    m = torch.tensor([A.h32(mean[c % 3]) for c in range(C)], dtype=torch.float64).reshape(1, 1, 1, C, 1, 1)
    sd = torch.tensor([A.h32(std[c % 3]) for c in range(C)], dtype=torch.float64).reshape(1, 1, 1, C, 1, 1)
    n = ((t / 255.0 - m) / sd)[:, :, ::2]
    want = F.interpolate(n.reshape(-1, C, H, W), size=(OH, OW), mode="bilinear", align_corners=False).reshape(B, S, 2, C, OH, OW)
    # (float32 source coordinates against torch's float64 ones: a coordinate is off by <= 3 u max(H, W) on each axis, and the value moves by
    # at most 2 max|n| per unit of it -- as in test_clip_reference_is_interpolate_and_model_holds)
    assert torch.allclose(ref[..., :C], want.permute(1, 0, 2, 4, 5, 3).reshape(S, B * 2, OH, OW, C), rtol=0,
                          atol=2 * 3 * A.U32 * max(H, W) * 2 * n.abs().max().item())
    # float32 emulation of the kernel: t / 255.f, (t - m) / sd per tap, then bilerp4 (fmaf(lw1, p01, lw0 * p00), .., fmaf(lh1, bot, lh0 * top):
    # each fmaf = the exact float64 expression rounded once to float32)
    t32 = t.float()[:, :, ::2]
    n32 = (t32 / 255.0 - m.float()) / sd.float()
    h0, h1, lh0, lh1, _ = A.resize_taps(H, OH)
    w0, w1, lw0, lw1, _ = A.resize_taps(W, OW)
    lh0, lh1 = lh0.reshape(-1, 1), lh1.reshape(-1, 1)
    f32 = lambda v: v.float().double()      # noqa: E731
    r0, r1 = n32.double()[..., h0, :], n32.double()[..., h1, :]
    top = f32(lw1 * r0[..., w1] + f32(lw0 * r0[..., w0]))
    bot = f32(lw1 * r1[..., w1] + f32(lw0 * r1[..., w0]))
    v32 = f32(lh1 * bot + f32(lh0 * top))
    h = torch.zeros(S, B * 2, OH, OW, 8)
    h[..., :C] = v32.float().permute(1, 0, 2, 4, 5, 3).reshape(S, B * 2, OH, OW, C)
    assert A.ratio(h.to(torch.bfloat16), ref, tol) <= 1.0
    # the float32 part of the tolerance alone (before the bf16 rounding) holds the float32 result: the counted 3 u / 4 u terms suffice
    assert A.ratio(h, ref, tol - A.RHO_BF16 * ref.abs()) <= 1.0
    hb = h.clone()
    hb[..., :C] = (n32 * 255.0 / 256.0)[..., h0, :][..., w0].permute(1, 0, 2, 4, 5, 3).reshape(S, B * 2, OH, OW, C)    # / 256 and nearest tap
    assert A.ratio(hb.to(torch.bfloat16), ref, tol) > 1.0
    bad, _ = A.clip_u8_ref(x, B, S, Fr, C, OH, OW, 2, 8, mean, std, 1, diff=diff, frame_offset=1)       # reading `off + c + CS`
    assert A.ratio(bad.to(torch.bfloat16), ref, tol) > 1.0


# ----------------------------------------------------------------------------------------------------------------------------- chain row
def _chain_f32(op, fw, tile, drop_cs=False, m_from_a=False):
    """the composition in the kernels' number formats on the CPU: float32 products and coefficients, sum(g' zhat) in float64 from the float32
    P, the pack rounded to bf16, a float32 GEMM over [g' | a], a bf16 data gradient and a float32 weight gradient"""
    G, P = op["G"], op["P"]
    W, g, a, vec, ga = op["w"], fw["g"].float(), fw["a"].float(), fw["vec"], op["gamma"]
    Cout = W.shape[0]
    Pm, Gm, sv = torch.einsum("gpo,gpi->goi", g, a), torch.einsum("gpi,gpj->gij", a, a), a.sum(1)
    s1 = fw["g"].sum(1)
    s2 = vec[:, 3].double() * ((W.double().unsqueeze(0) * Pm.double()).sum(2) - vec[:, 2].double() * s1)
    k0, k1, k2 = ga * vec[:, 3], (s1 / P).float(), (s2 / P).float()
    Aa, Bb, Cc = k0, -k0 * k2 * vec[:, 3], k0 * (k2 * vec[:, 2] * vec[:, 3] - k1)
    wa = (W.t().unsqueeze(0) * Aa.unsqueeze(1)).to(torch.bfloat16)
    M = torch.einsum("oi,go,oj->gij", W, Aa if m_from_a else Bb, W).to(torch.bfloat16)
    epi = torch.einsum("oi,go->gi", W, Cc)
    gemm = torch.einsum("gpk,gck->gpc", torch.cat([g, a], 2), torch.cat([wa, M], 2).float())
    if tile:
        gemm = gemm.to(torch.bfloat16).float()
    dx = (gemm + epi.unsqueeze(1)).to(torch.bfloat16)
    dw = torch.zeros(Cout, W.shape[1])
    for gi in range(G):
        dw = dw + (Aa[gi].unsqueeze(1) * Pm[gi] + Bb[gi].unsqueeze(1) * (W @ Gm[gi]) + (0 if drop_cs else Cc[gi].unsqueeze(1) * sv[gi].unsqueeze(0)))
    return dx, dw


@pytest.mark.parametrize("Cout,Cin,tile", [(64, 16, False), (128, 32, True)])
def test_chain_model(Cout, Cin, tile):
    """The composed algebraic backward against the float64 BatchNorm backward of z = bf16(W) a: the first-order terms in W - bf16(W) explain
    F - T (the remainder is second order), an emulation in the kernels' formats stays inside |FO| + remainder + E, the planted defects do not,
    and the model is far below the 2e-2 of the result's maximum that held the composition before"""
    op = A.chain_operands(Cout, Cin, 2, 150, 3)
    fw, T, Fa, tx, tw, fig = A.chain_model(op, tile)
    assert fig["rem_dx"] < 0.02 and fig["rem_dw"] < 0.02, fig
    assert 0 < fig["dx"] < 1e-2 and 0 < fig["dw"] < 1e-2, fig
    # T is the BatchNorm backward: autograd through y = gamma (z - mean(z)) / sqrt(var(z) + eps) in float64 agrees to the float32 rounding
    # of the stored (mean, invstd)
    a = fw["a"].clone().requires_grad_(True)
    wb = fw["wb"].clone().requires_grad_(True)
    z = torch.einsum("gpi,oi->gpo", a, wb)
    y = op["gamma"].double() * (z - z.mean(1, keepdim=True)) / torch.sqrt(z.var(1, unbiased=False, keepdim=True) + 1e-5)
    (y * fw["g"]).sum().backward()
    assert torch.allclose(T["dx"], a.grad, rtol=0, atol=1e-5 * T["dx"].abs().max().item())
    assert torch.allclose(T["dw"], wb.grad, rtol=0, atol=1e-5 * T["dw"].abs().max().item())
    dx, dw = _chain_f32(op, fw, tile)
    assert A.ratio(dx.double(), T["dx"], tx) <= 1.0 and A.ratio(dw.double(), T["dw"], tw) <= 1.0
    assert tx.max() < 2e-2 * T["dx"].abs().max() and tw.max() < 1e-2 * T["dw"].abs().max()
    dxb, _ = _chain_f32(op, fw, tile, m_from_a=True)
    _, dwb = _chain_f32(op, fw, tile, drop_cs=True)
    assert A.ratio(dxb.double(), T["dx"], tx) > 1.0 and A.ratio(dwb.double(), T["dw"], tw) > 1.0
    # a composition that were consistent with the forward (bf16(W) everywhere) has no first-order term: it must fit E alone
    op2 = dict(op, w=op["w"].to(torch.bfloat16).float())
    _, T2, _, tx2, tw2, fig2 = A.chain_model(op2, tile)
    assert fig2["dx"] < 1e-12 and fig2["dw"] < 1e-12        # (float64 reassociation only)
