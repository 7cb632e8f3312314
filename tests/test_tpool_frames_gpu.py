"""Stage-boundary kernels at 16 and 32 frames per clip: the fused conv3 + bn3 + add + ReLU + temporal max-pool (its three kernels), the pool
backward fused with the residual backward / read from the 2-bit codes / with the product, the plain pool walks, and one ResNet-50 step.
Float64 references and bounds are the ones of the 8-frame rows (tests/fused_ref.py, tests/elementwise_ref.py, tests/executor_ref.py);
every fused result is also compared bit for bit with the unfused launches it replaces."""
import pytest
import torch
from ctypes import byref

from tests import conv_ref as R, elementwise_ref as E, fused_ref as F

pytestmark = pytest.mark.gpu

from adamml_amd import hip  # noqa: E402
from adamml_amd.hip import call, ptr  # noqa: E402
from tests import test_elementwise_conformance_gpu as EC, test_executor_gpu as XG  # noqa: E402
from tests.test_conv_conformance_gpu import DEV, GB, guard, ssum  # noqa: E402,F401  (guard: the autouse check of every row)
from tests.test_fused_conformance_gpu import FwdArgs, Guarded  # noqa: E402

# kernel -> (Cin, Cout, pixels per frame, answer of adamml_conv_fwd_bn_add_tpool_streams): the tile kernel below one ragged pixel tile; the layer-1
# kernel has no pixel threshold (one full 16-pixel block + 1); the wave-slice kernel needs clips * T * pixels >= 4096 per group
FWD = {"tile": (64, 128, lambda T: 15, 0), "l1": (64, 256, lambda T: 17, 1), "l2-slice": (128, 512, lambda T: 4096 // (2 * T), 2)}


def operands(row):
    """F.tpool_operands with its eight per-frame identity factors repeated over T frames; `dup`: frame t := frame t - 1 (exact ties)"""
    T, clips, Q, G, Cout = row["T"], row["clips"], row["Q"], row["G"], row["Cout"]
    op = F.fadd_operands(dict(row, P=clips * T * Q, act=1))
    op["vec"][:, 1, Cout - 8:] = -40.0                                     # block output <= 0 in every frame: code 3
    idn = op["idn"].float().reshape(G, clips, T, Q, Cout)
    idn[..., F.PLANTED:] *= torch.tensor([0.3, 1.7, 0.8, 2.6, 0.5, 2.1, 1.2, 3.0]).repeat(T // 8).reshape(1, 1, T, 1, 1)
    x = op["x"].reshape(G, clips, T, Q, -1).clone()
    dup_of = list(range(T))
    for t in row["dup"]:
        idn[:, :, t], x[:, :, t], dup_of[t] = idn[:, :, t - 1], x[:, :, t - 1], dup_of[t - 1]
    op.update(idn=idn.to(torch.bfloat16).reshape(-1, Cout), x=x.reshape(-1, x.shape[-1]), dup_of=dup_of)
    return op


def codes_of(full, T):
    """[rows * T, HW, C] stored block output -> (pooled bf16 values, code 0..2 = tap of the first maximum, 3 where the maximum is <= 0)"""
    y, arg = E.temporal_pool_fwd_ref(full, None, None, 0, 0, T, 0)
    code = arg - (2 * torch.arange(T // 2).reshape(1, -1, 1) - 1)
    return y, torch.where(y > 0, code, torch.full_like(code, 3))


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("lazy", [True, False], ids=["lazy", "plain"])
@pytest.mark.parametrize("T", [16, 32])
@pytest.mark.parametrize("kern", list(FWD))
def test_conv_fwd_bn_add_tpool(kern, T, lazy, G, monkeypatch):
    monkeypatch.delenv("ADAMML_FADD_TPOOL_SLICE", raising=False)
    Cin, Cout, q_of, probe = FWD[kern]
    clips, Q = 2, q_of(T)
    # frames 7 = 8 = 9: window 4 is one exact tie whose FIRST tap is the frame carried across the 8-frame segment boundary
    row = dict(id="tp%d-%s-%s-g%d" % (T, kern, "lazy" if lazy else "plain", G), T=T, clips=clips, Q=Q, G=G, Cin=Cin, Cout=Cout,
               in_act=1 if lazy else None, act=1, idn="plain", dup=(3, 8, 9, T - 1))
    op = operands(row)
    r, p = F.tpool_reference(row, op)
    ref = r["ref"].reshape(G, clips, T, Q, Cout)
    assert ((ref[:, :, 8] == ref[:, :, 7]) & (ref[:, :, 9] == ref[:, :, 7]) & (ref[:, :, 7] > 0)).any(), "no positive tie in the reference"
    assert p["must3"].any() and (~p["must3"] & ~p["und3"]).any(), "no window <= 0 (or none above) in the reference"
    a = FwdArgs(row, op, clips * T, Q, 1)
    assert hip.load().adamml_conv_fwd_bn_add_tpool_supported(byref(a.d), T, 1, 1 if lazy else 0) == 1
    assert hip.load().adamml_conv_fwd_bn_add_tpool_streams(byref(a.d), T) == probe, "dispatch probe"
    rows = G * clips * (T // 2) * Q
    pooled, code = Guarded(rows, Cout, torch.bfloat16), Guarded(rows, Cout // 8, torch.int16)
    call("adamml_conv_fwd_bn_add_tpool", *a.head, T, ptr(pooled.t), ptr(code.t))
    h, c = pooled.check(row["id"]).cpu(), code.check(row["id"] + " code").cpu()
    q, und = F.tpool_check(h, c, p, row["id"])
    assert und <= F.UNDECIDED_CAP, (q, und)
    # the unfused sequence: the full-rate block output, then the pool; the codes follow from the stored block output exactly
    full = Guarded(G * clips * T * Q, Cout, torch.bfloat16)
    call("adamml_conv_fwd_bn_add", *a.head, ptr(full.t), None)
    y = EC.nan_bf16(rows, Cout)
    call("adamml_temporal_pool_fwd", ptr(full.t), None, None, 0, 0, ptr(y), clips, T, Q * Cout, Cout, 0, G)
    assert torch.equal(h, y.cpu()), "pooled differs from conv_bn_add + temporal_pool_fwd"
    yr, cr = codes_of(full.check(row["id"] + " unfused").cpu().reshape(G * clips * T, Q, Cout), T)
    assert torch.equal(h.double().reshape(yr.shape), yr) and torch.equal(F.unpack_codes(c, cr.shape), cr), "codes differ from the unfused block output's"


@pytest.mark.parametrize("C", [64, 256])
@pytest.mark.parametrize("T", [16, 32])
def test_temporal_pool_bwd_res_and_code(T, C):
    NB, HW, G, act, To = 2, 15, 2, 1, T // 2
    name = "T%d-C%d" % (T, C)
    out = E.rand_bf16(G * NB * T, HW, C, seed=T + C).float().clamp(min=0).to(torch.bfloat16)          # a block output: ties at 0
    out[1::3] = out[0::3][: out[1::3].shape[0]]                                                     # and exact ties between neighbouring frames
    g, z, vec = E.rand_bf16(G * NB * To, HW, C, seed=T + C + 1), E.rand_bf16(G * NB * T, HW, C, seed=T + C + 2), E.bn_vectors(G, C, T + C + 3)
    y, arg = E.temporal_pool_fwd_ref(out, None, None, 0, 0, T, 0)
    routed, rab = E.temporal_pool_bwd_ref(g, arg, T, 0)
    m = E.act_mask(out.double(), act).reshape(routed.shape)
    od, gd, zd, vd = GB.frozen(out), GB.frozen(g), GB.frozen(z), GB.frozen(vec)
    gx, g2u, su = EC.nan_bf16(G * NB * T, HW, C), EC.nan_bf16(G * NB * T, HW, C), EC.zsums(G, C)
    call("adamml_temporal_pool_bwd", ptr(gd), ptr(od), None, None, 0, 0, ptr(gx), NB, T, HW * C, C, 0, G)
    call("adamml_residual_bwd", ptr(gx), ptr(od), act, ptr(g2u), ptr(zd), ptr(vd), ptr(su), None, None, None, NB * T * HW, C, G)
    assert hip.load().adamml_temporal_pool_bwd_res_supported(T, C, 0) == 1
    g2, sums = EC.nan_bf16(G * NB * T, HW, C), EC.zsums(G, C)
    call("adamml_temporal_pool_bwd_res", ptr(gd), ptr(od), act, ptr(g2), ptr(zd), ptr(vd), ptr(sums), NB, T, HW, C, G)
    h = g2.cpu()
    assert torch.equal(h, g2u.cpu()), name + ": g2 differs from temporal_pool_bwd + residual_bwd"
    E.point_check(h.reshape(routed.shape), routed * m, rab * m, E.K_TPOOL_MAX_BWD, what="temporal_pool_bwd_res " + name)
    sref, sab = R.bn_dgrad_sums_ref(h.double().reshape(-1, C), z.reshape(-1, C), vec, groups=G)
    E.sums_check(ssum(sums).cpu(), sref, sab, NB * T * HW, what="temporal_pool_bwd_res sums " + name)
    # the same gradient from the codes the fused forward would have stored for this block output
    _, code = codes_of(out, T)
    cd, g2c, sc = GB.frozen(E.pack_codes(code.reshape(G * NB * To, HW, C))), EC.nan_bf16(G * NB * T, HW, C), EC.zsums(G, C)
    call("adamml_temporal_pool_bwd_code", ptr(gd), ptr(cd), ptr(g2c), ptr(sc), NB, T, HW, C, G)
    assert torch.equal(g2c.cpu(), h), name + ": g2 from the codes differs"
    f = h.double().reshape(G, -1, C)
    E.sums_check(ssum(sc).cpu()[:, :C], f.sum(1), f.abs().sum(1), NB * T * HW, what="temporal_pool_bwd_code sums " + name)


@pytest.mark.parametrize("T", [16, 32])
def test_temporal_pool_bwd_code_prod(T):
    clips, Q, G, C, Cin, To = 2, 17, 2, 256, 64, T // 2
    assert hip.load().adamml_temporal_pool_bwd_code_prod_supported(T, C, Cin) == 1
    rows, P = G * clips * To * Q, clips * T * Q
    gy, code = E.rand_bf16(rows, C, seed=T), torch.randint(0, 4, (rows, C), generator=F.gen(T + 1))
    a, av = E.plant_bounds(E.rand_bf16(G * P, Cin, scale=1.5, seed=T + 2)), E.bn_vectors(G, Cin, T + 3).reshape(-1)
    gyd, cd, ad, avd = GB.frozen(gy), GB.frozen(E.pack_codes(code)), GB.frozen(a), GB.frozen(av)
    g2c, sc = EC.nan_bf16(G * P, C), EC.zsums(G, C)
    call("adamml_temporal_pool_bwd_code", ptr(gyd), ptr(cd), ptr(g2c), ptr(sc), clips, T, Q, C, G)
    g2, prod, sa = Guarded(G * P, C, torch.bfloat16), Guarded(G * C, Cin, torch.float32), EC.zsums(G, C)
    ws = hip.scratch(hip.load().adamml_temporal_pool_bwd_code_prod_workspace(clips, T, Q, C, Cin, G), DEV)
    call("adamml_temporal_pool_bwd_code_prod", ptr(gyd), ptr(cd), ptr(g2.t), ptr(sa), ptr(ad), ptr(avd), ptr(avd[Cin:]), 4 * Cin, 1, ptr(prod.t),
         ptr(ws), ws.numel() * ws.element_size(), clips, T, Q, C, Cin, G)
    h = g2.check("tpb-T%d" % T).cpu()
    assert torch.equal(h, g2c.cpu()), "g2 differs from temporal_pool_bwd_code"
    g2r, pr, pa, n = F.tpool_bwd_code_prod_ref(gy.reshape(-1, Q, C), code.reshape(-1, Q, C), F.operand(a, av, av[Cin:], 1, G, 4 * Cin), T, G)
    assert torch.equal(h.double().reshape(g2r.shape), g2r)
    F.prod_check(prod.check("tpb-T%d prod" % T).cpu().reshape(G, C, Cin), pr, pa, n, "tpb-T%d prod" % T)
    F.res_sums_check(ssum(sa).cpu(), h, None, None, G, "tpb-T%d sums" % T)


@pytest.mark.parametrize("mode", [0, 1], ids=["max", "avg"])
@pytest.mark.parametrize("T", [16, 32])
def test_temporal_pool_walks(T, mode):
    EC.test_temporal_pool(T, mode, 1)              # forward (max: bit-exact) and backward against float64, lazy ReLU input, ragged workgroups


def test_resnet50_16_frames_takes_the_fused_boundaries(monkeypatch):
    """One training step, 2 clips x 16 frames of 32 x 32 (stage 1 ends at 16 frames, stage 2 at 8, stage 3 at 4 with its pool behind add_act): logits,
    BatchNorm state and every gradient against the forced float64 replay under the 8-frame rows' bounds (XG.resnet_row asserts them)."""
    n = XG.resnet_row(XG.resnet(16), 32, 2, 1, monkeypatch, "resnet50-t16")["names"]
    assert n["adamml_conv_fwd_bn_add_tpool"] == 2 and n["adamml_temporal_pool_bwd_code_prod"] == 1 and n["adamml_temporal_pool_bwd_code"] == 1
    assert n["adamml_temporal_pool_fwd"] == 1 and n["adamml_temporal_pool_bwd_res"] == 1 and n["adamml_temporal_pool_bwd"] == 0
