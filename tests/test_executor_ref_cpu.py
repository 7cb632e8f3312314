"""tests/executor_ref.py can fail: its replay is anchored to torch, and a torch emulation of the host executor (bf16 storage at the
runtime's storage points, Gram-matrix statistics for conv_bn_add, the algebraic dW = A.(g'^T a) + B.(W G) + C (x) s and dx forms in
float32) passes the shared bound at K while each of seven planted executor defects misses it by at least a factor 2.  The op-level
graphs of tools/executor_ops.py (the arms no model reaches) get the same three anchors at the end of the file, with six more defects.
The BasicBlock graph of ResNet-18 / -34 (MiniBasicNet) gets them too, in two placements of the residual backward -- every add masks its own
gradient, or the next block's conv1 finishes it in its data-gradient epilogue -- with six defects of the host decisions around it.  No GPU."""
import math
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import executor_ref as X
from tests import elementwise_ref as E
from tests import fused_ref as FR
from adamml_amd.runtime import ConvState
from adamml_amd.mobilenet_common import BlockPlan

ACT_NONE, ACT_RELU, ACT_RELU6 = 0, 1, 2
bf = X.bf


def q(x):
    return x + (bf(x.detach()) - x).detach()


# ------------------------------------------------------------------------------------------------------ torch emulation of the executor
class ELazy:
    """what the recorder and the replay read of a runtime Lazy, + the autograd value the emulation's consumers use"""

    def __init__(self, data, vec=None, act=ACT_NONE, val=None, requires_grad=True):
        self.data, self.vec, self.act = data, vec, act
        self.scale = None if vec is None else vec[0, 0]
        self.shift = None if vec is None else vec[0, 1]
        self.gs = 0 if vec is None else 4 * data.shape[-1]
        self.res, self.alg, self.val, self.requires_grad = None, False, val, requires_grad
        self.hold = None          # an add output: what its backward shares with the conv whose data-gradient epilogue may finish it (Emu.add_act)

    @property
    def shape(self):
        return self.data.shape


class Branch(torch.autograd.Function):
    """one consumer's view of a tensor; drop: this consumer's gradient is lost (the other consumer WROTE where it had to accumulate)"""
    @staticmethod
    def forward(ctx, v, drop):
        ctx.drop = drop
        return v.view_as(v)

    @staticmethod
    def backward(ctx, g):
        return (torch.zeros_like(g) if ctx.drop else g), None


class AddAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, act, drop_idn, no_mask, hold=None):
        out = bf(E.clamp(a + b, act))
        lo, hi = X.R.ACT_BOUNDS[act]
        ctx.m = torch.ones_like(out) if no_mask else ((out > lo) & (out < hi)).to(out.dtype)
        ctx.drop, ctx.hold = drop_idn, hold
        if hold is not None:
            hold.m = ctx.m
        return out

    @staticmethod
    def backward(ctx, g):
        if ctx.hold is not None and ctx.hold.done:
            # the last consumer's data-gradient epilogue already masked g (runtime._add_backward, res_done): both operands take it as it is.
            # planted (e): the epilogue summed the gradient BEFORE the mask for the BatchNorm'd operand's backward
            gz = ctx.hold.unmasked if ctx.hold.sum_unmasked else g
            return gz, (torch.zeros_like(g) if ctx.drop else g), None, None, None, None
        g2 = bf(g * ctx.m)
        return g2, (torch.zeros_like(g2) if ctx.drop else g2), None, None, None, None


class IdnCapture(torch.autograd.Function):
    """the identity operand of the NEXT block's add, where the next block's conv1 finishes this add's backward: its gradient is what sits in
    x.grad (bf16, already masked by the next add) when conv1's data gradient runs -- kept for ResEpilogue, not passed on a second time"""
    @staticmethod
    def forward(ctx, v, hold):
        ctx.hold = hold
        return v.view_as(v)

    @staticmethod
    def backward(ctx, g):
        ctx.hold.idn_grad = g
        return torch.zeros_like(g), None


class ResEpilogue(torch.autograd.Function):
    """conv1's view of an add output x whose backward its data gradient finishes (runtime._dgrad_finish_residual, adamml_conv_bwd_data_res):
    g' = bf16(act'(x) (float32 data gradient + the identity-path gradient stored in x.grad)), written once.  hold.staged: the data gradient
    passes through the kernels' bf16 staging tile in LDS before the identity-path gradient is added (conv_gemm.hip / conv3x3_c64.hip: the
    epilogue reads the GEMM tile back as bf16) -- no storage point, one of the roundings K = 4 is there for"""
    @staticmethod
    def forward(ctx, v, hold):
        ctx.hold = hold
        return v.view_as(v)

    @staticmethod
    def backward(ctx, g):
        hold = ctx.hold
        assert hold.idn_grad is not None, "the add recorded after conv1 has not run its backward: conv1 is not the last consumer"
        total = (bf(g) if hold.staged else g) + hold.idn_grad
        hold.unmasked = bf(total)
        hold.done = True
        return bf(total * hold.m), None


class TPool(torch.autograd.Function):
    """temporal max-pool of relu(a + b) over the T frames of a clip, candidates compared after their bf16 rounding, first maximum"""
    @staticmethod
    def forward(ctx, a, b, T, last):
        full = bf(torch.relu(a + b))
        N, H, W, C = full.shape
        f = full.reshape(N // T, T, H, W, C)
        ys, codes, route = [], [], []
        for win in FR.pool_windows(T):
            cand = torch.stack([f[:, t] for _, t in win])
            taps = torch.tensor([k for k, _ in win])
            frames = torch.tensor([t for _, t in win])
            i = X.first_argmax(cand)
            il = E.first_argmax(cand.double(), last=True)[1]
            best = cand.max(0).values
            ys.append(best)
            codes.append(torch.where(best > 0, taps[i], torch.full_like(i, 3)))
            route.append(torch.where(best > 0, frames[il if last else i], torch.full_like(i, -1)))
        ctx.route, ctx.T, ctx.shape = torch.stack(route, 1), T, full.shape
        ctx.mark_non_differentiable(code := torch.stack(codes, 1))
        return torch.stack(ys, 1).reshape(N // 2, H, W, C), code

    @staticmethod
    def backward(ctx, g, _):
        N, H, W, C = ctx.shape
        T = ctx.T
        gg = g.reshape(N // T, T // 2, H, W, C)
        gx = torch.zeros(N // T, T, H, W, C, dtype=g.dtype)
        for to in range(T // 2):
            for t in range(T):
                gx[:, t] += gg[:, to] * (ctx.route[:, to] == t).to(g.dtype)
        gx = bf(gx).reshape(ctx.shape)
        return gx, gx, None, None


class AlgConvBN(torch.autograd.Function):
    """o = BatchNorm(bf16(bf16(W) a)) of a 1x1 conv, train mode, per group; backward in the algebraic form of _conv1x1_backward_alg:
    it reads g', a and the float32 MASTER weight, never z.  gram: statistics from G = a^T a and s = sum a (conv_bn_add)."""
    @staticmethod
    def forward(ctx, a, w, gamma, beta, gram, hold, no_mean_term, share_vec, gemm_defect=0, direct=False):
        G, P, Cin = a.shape
        wb = bf(w)
        zb = bf(a @ wb.t())
        if gram:
            Gm, s = a.transpose(1, 2) @ a, a.sum(1)
            s1 = s.double() @ wb.double().t()
            s2 = torch.einsum("oi,gij,oj->go", wb.double(), Gm.double(), wb.double())
            mean, var = s1 / P, s2 / P - (s1 / P) ** 2
        else:
            mean, var = zb.double().mean(1), zb.double().var(1, unbiased=False)
        inv = (1.0 / torch.sqrt(var + X.EPS)).float()
        mean = mean.float()
        scale = gamma * inv
        shift = beta - mean * scale
        hold.y, hold.vec, hold.var = zb, torch.stack([scale, shift, mean, inv], 1), var
        ctx.save_for_backward(a, w, gamma, mean, inv)
        ctx.flags = (no_mean_term, share_vec, gemm_defect)
        ctx.zb = zb if direct else None
        return zb * scale.unsqueeze(1) + shift.unsqueeze(1)

    @staticmethod
    def backward(ctx, g):
        a, w, gamma, mean, inv = ctx.saved_tensors
        no_mean_term, share_vec, gemm_defect = ctx.flags
        Cout = w.shape[0]
        G, P, Cin = a.shape
        g = bf(g)
        if share_vec:                                   # planted (e): every group reads group 0's vectors
            mean, inv = mean[:1].expand_as(mean), inv[:1].expand_as(inv)
        s1 = g.sum(1)
        Pm = torch.einsum("gpo,gpi->goi", g, a)
        if ctx.zb is not None:          # the producer of g' left no partial sums: adamml_bn_bwd_reduce / adamml_residual_bwd read the stored (recomputed) z
            s2 = (g * ((ctx.zb - mean.unsqueeze(1)) * inv.unsqueeze(1))).sum(1)
        else:
            s2 = inv * ((w.unsqueeze(0) * Pm).sum(2) - (0.0 if no_mean_term else mean * s1))          # adamml_alg_sumfix
        k0, k1, k2 = gamma * inv, s1 / P, s2 / P
        A, B, C = k0, -k0 * k2 * inv, k0 * (k2 * mean * inv - k1)
        wa = bf(w.t().unsqueeze(0) * A.unsqueeze(1))                                              # adamml_alg_pack: bf16 entries
        if Cin >= 256:
            # the ALG_GEMM_CIN arm: W^T diag(B_g) W for all groups as one product [G*Cin, Cout] x [Cout, Cin], W G_g as [Cout, Cin] x [Cin, G*Cin].
            # planted (6): the operand is laid out [Cout][Cin][G] (1) / [Cin][Cin][G] (2) and read as [..][G][Cin] -- the same bytes at G = 1
            wb = (w.unsqueeze(2) * B.t().unsqueeze(1)) if gemm_defect == 1 else (w.unsqueeze(1) * B.t().unsqueeze(2))
            M = bf((wb.reshape(Cout, G * Cin).t() @ w).reshape(G, Cin, Cin))
        else:
            M = bf(torch.einsum("oi,go,oj->gij", w, B, w))
        epi = torch.einsum("oi,go->gi", w, C)
        dx = bf(torch.einsum("gpo,gco->gpc", g, wa) + torch.einsum("gpj,gcj->gpc", a, M) + epi.unsqueeze(1))
        Gm, sv = a.transpose(1, 2) @ a, a.sum(1)
        if Cin >= 256:
            gm = Gm.permute(1, 2, 0) if gemm_defect == 2 else Gm.permute(1, 0, 2)
            WG = (w @ gm.reshape(Cin, G * Cin)).reshape(Cout, G, Cin).permute(1, 0, 2)
        else:
            WG = torch.einsum("oj,gji->goi", w, Gm)
        dw = (A.unsqueeze(2) * Pm + B.unsqueeze(2) * WG + C.unsqueeze(2) * sv.unsqueeze(1)).sum(0)
        return dx, dw, s2.sum(0), s1.sum(0), None, None, None, None, None, None


class Emu:
    """The executor entry points on torch (CPU, float32).  defects: name -> index of the call of that kind that misbehaves."""

    def __init__(self, module, groups, defects=None):
        self.named = list(module.named_parameters())
        self.p, self.names = X.leaves(self.named, torch.float32)
        self.running = {k: [v[0].float(), v[1].float(), v[2]] for k, v in X.running_of(module).items()}
        self.rt = types.SimpleNamespace(groups=groups, capture={"aux": {}}, training=True, tape=types.SimpleNamespace(need_grad=True))
        self.defects = defects or {}
        self.count = {}
        self.state = {}
        self.logits = None
        # True / "staged": a last_consumer conv of an add output finishes that add's backward in its data-gradient epilogue (ResEpilogue)
        self.fused_residual = False
        self.direct_sums = False      # True: no producer of g' leaves partial sums (the op-level graphs): sum(g' zhat) from the stored z, no sumfix

    def _hit(self, kind):
        i = self.count.get(kind, 0)
        self.count[kind] = i + 1
        return self.defects.get(kind) == i

    def use(self, x, finish=False):
        st = self.state.setdefault(id(x), [getattr(x, "val", None), 0, x, len(self.state)])
        if st[0] is None:
            st[0] = x.data.float()
        k = st[1]
        st[1] += 1
        v = st[0]
        hold = getattr(x, "hold", None)
        if finish:                          # this consumer's data gradient finishes the add that produced x
            hold.claimed = True
            hold.sum_unmasked, hold.staged = self._hit("sum_unmasked"), self.fused_residual == "staged"
            v = ResEpilogue.apply(v, hold)
        elif hold is not None and hold.claimed:
            v = IdnCapture.apply(v, hold)
        # planted (d): the second consumer in tape order (conv1; reversed first) loses its gradient to the downsample's write
        drop = k == 1 and self._hit("two_consumers")
        # planted (1), (2): (t, k) -- the k-th consumer (forward order) of the t-th tensor that got a consumer loses its gradient: the consumer
        # recorded BEFORE it runs its backward AFTER it and overwrote the gradient it had to add to (acc dropped)
        drop = drop or self.defects.get("drop_use") == (st[3], k)
        return Branch.apply(v, drop)

    def _running(self, bn, mean, var, n):
        run = self.running[id(bn)]
        biased = self._hit("running_var")
        for g in range(mean.shape[0]):
            run[0] = (1 - X.MOMENTUM) * run[0] + X.MOMENTUM * mean[g].detach().float()
            run[1] = (1 - X.MOMENTUM) * run[1] + X.MOMENTUM * (var[g].detach().float() * (1.0 if biased else n / (n - 1.0)))
        run[2] += mean.shape[0]

    def _act(self, y, vec, act):
        """the activated value of a lazy conv output: gate from fmaf(scale, y, shift) in float32"""
        G = vec.shape[0]
        sc, sh = vec[:, 0].reshape(G, 1, 1, 1, -1), vec[:, 1].reshape(G, 1, 1, 1, -1)
        yg = y.reshape((G, -1) + tuple(y.shape[1:]))
        v = (yg * sc + sh).reshape(y.shape)
        pre = (yg.detach().double() * sc.detach().double() + sh.detach().double()).float().reshape(y.shape)
        v = v + (pre - v).detach()                          # the loaders' fmaf: one rounding
        if act != ACT_NONE:
            lo, hi = X.R.ACT_BOUNDS[act]
            v = v * ((pre > lo) & (pre < hi)).float() + (6.0 * (pre >= hi).float() if act == ACT_RELU6 else 0.0)
        return v

    def _alg_ok(self, cs, act, x):
        cin = cs.weight.shape[1]
        return (not cs.depthwise and act == ACT_NONE and cs.kh == 1 and cs.stride == 1 and cin in (64, 128, 256)
                and 2 * cin <= cs.cout <= 512 and x.requires_grad)

    def _alg(self, a4, cs, bn, gram):
        G = self.rt.groups
        hold = types.SimpleNamespace()
        a = a4.reshape(G, -1, a4.shape[-1])
        hit_c, hit_e = (self._hit("sumfix"), self._hit("group_vec")) if gram else (False, False)
        o = AlgConvBN.apply(a, self.p[id(cs.weight)].reshape(cs.cout, -1), self.p[id(bn.weight)], self.p[id(bn.bias)], gram, hold, hit_c, hit_e,
                            self.defects.get("gemm_transposed", 0), self.direct_sums)
        self._running(bn, hold.vec[:, 2], hold.var, a.shape[1])
        shp = tuple(a4.shape[:3]) + (cs.cout,)
        return o.reshape(shp), hold.y.reshape(shp), hold.vec.detach()

    def conv_bn(self, rt, x, cs, bn, act, sole_consumer=False, last_consumer=False):
        G = rt.groups
        a = self.use(x, finish=self._residual_fusable(x, cs, last_consumer))
        if self._alg_ok(cs, act, x):
            o, y, vec = self._alg(q(a), cs, bn, False)
            out = ELazy(y.detach().to(torch.bfloat16), vec, act, o.register_hook(bf) and o)
            out.alg = True
            return out
        w = self.p[id(cs.weight)]
        if cs.depthwise:
            y = F.conv2d(a.permute(0, 3, 1, 2), w, stride=cs.stride, padding=cs.pad, groups=cs.cout)
        else:
            y = F.conv2d(q(a)[..., :w.shape[1]].permute(0, 3, 1, 2), q(w), stride=cs.stride, padding=cs.pad)
        return self._bn_out(G, q(y.permute(0, 2, 3, 1)), bn, act)

    def _residual_fusable(self, x, cs, last_consumer):
        """runtime._conv_backward_plain's `c.last_consumer and _residual_fusable(x, d)`: x is the output of an add nobody has finished, the
        add's first operand is a BatchNorm'd conv output, the conv is one adamml_conv_bwd_data_res_supported admits (1x1, or 3x3 / pad 1, stride 1)"""
        hold = getattr(x, "hold", None)
        if not (self.fused_residual and last_consumer and hold is not None and not hold.claimed and x.res[0].vec is not None):
            return False
        return not cs.depthwise and cs.stride == 1 and (cs.kh, cs.pad) in ((1, 0), (3, 1))

    def _bn_out(self, G, y, bn, act):
        """train-mode BatchNorm of the stored raw output y (statistics from the stored values), as one lazy tensor"""
        y.register_hook(bf)
        yg = y.reshape(G, -1, y.shape[-1])
        n = yg.shape[1]
        mean, var = yg.mean(1), yg.var(1, unbiased=False)
        if not bn.weight.requires_grad and self._hit("frozen_bn_constant"):
            # planted (5): a BatchNorm with frozen gamma / beta back-propagated as the constant affine map it is in eval mode
            mean, var = mean.detach(), var.detach()
        inv = (var + X.EPS).rsqrt()
        scale = self.p[id(bn.weight)] * inv
        shift = self.p[id(bn.bias)] - mean * scale
        self._running(bn, mean, var, n)
        vec = torch.stack([scale, shift, mean, inv], 1)
        v = self._act(y, vec, act)
        v.register_hook(bf)
        return ELazy(y.detach().to(torch.bfloat16), vec.detach().clone(), act, v)

    def conv_stem1_bn(self, rt, x1, cs, bn, act):
        B, G, H, W = x1.shape
        a = x1.permute(1, 0, 2, 3).reshape(G * B, 1, H, W)
        y = q(F.conv2d(a, self.p[id(cs.weight)], stride=2, padding=1).permute(0, 2, 3, 1))
        return self._bn_out(rt.groups, y, bn, act)

    def materialize(self, rt, x):
        y = q(self.use(x))
        y.register_hook(bf)
        return ELazy(y.detach().to(torch.bfloat16), None, ACT_NONE, y, requires_grad=x.requires_grad)

    def gap(self, rt, x):
        v = self.use(x)
        self.logits = v.reshape(v.shape[0], -1, v.shape[-1]).mean(1)
        return self.logits.detach(), None

    def add_act(self, rt, z, idn, act, idn_sole=False):
        hold = types.SimpleNamespace(m=None, claimed=False, done=False, idn_grad=None, unmasked=None, sum_unmasked=False, staged=False)
        out = AddAct.apply(self.use(z), self.use(idn), act, self._hit("drop_identity"), self._hit("no_mask"), hold)
        lz = ELazy(out.detach().to(torch.bfloat16), None, ACT_NONE, out)
        lz.res = (z, idn, act, idn_sole, E.mask_bits_ref(lz.data, act) if act != ACT_NONE else None)
        lz.hold = hold
        return lz

    def conv_bn_add(self, rt, x, cs, bn, idn, act, idn_sole=False, tpool=0, next_cs=None):
        o, _, vec = self._alg(q(self.use(x)), cs, bn, True)
        iv = self.use(idn) if idn is not None else torch.zeros_like(o)
        if tpool:
            out, code = TPool.apply(o, iv, tpool, self._hit("tie_last"))
            lz = ELazy(out.detach().to(torch.bfloat16), None, ACT_NONE, out)
            rt.capture["aux"][id(lz)] = (E.pack_codes(code), None, vec)
            return lz
        out = AddAct.apply(o, iv, act, self._hit("drop_identity"), self._hit("no_mask"))
        lz = ELazy(out.detach().to(torch.bfloat16), None, ACT_NONE, out)
        mask = E.mask_bits_ref(lz.data, act) if act != ACT_NONE else None
        lz.res = (None, idn, act, idn_sole, mask)
        rt.capture["aux"][id(lz)] = (None, mask, vec)
        return lz

    def maxpool3x3s2(self, rt, x, sole_consumer=False):
        v = self.use(x)
        N, H, W, C = v.shape
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        taps = X.taps2d(v, OH, OW)
        pad = X.taps2d(torch.ones_like(v.detach()), OH, OW) == 0
        idx = X.first_argmax(torch.where(pad, torch.full_like(taps.detach(), -math.inf), taps.detach()))
        y = torch.gather(taps, 0, idx.unsqueeze(0))[0]
        if self._hit("first_tap"):                # planted (3): the gradient goes to the window's first tap, not to the recorded one
            y = taps[0] + (y - taps[0]).detach()
        y = q(y)
        y.register_hook(bf)
        lz = ELazy(y.detach().to(torch.bfloat16), None, ACT_NONE, y)
        rt.capture["aux"][id(lz)] = idx.to(torch.uint8)
        return lz

    def temporal_pool(self, rt, x, frames, mode, sole_consumer=False):
        v = self.use(x)
        NT, H, W, C = v.shape
        To, win = E.temporal_windows(frames)
        f = v.reshape(NT // frames, frames, H, W, C)
        ys = []
        for w in win:
            arg = torch.tensor(w)[X.first_argmax(torch.stack([f[:, t] for t in w]).detach())]
            ys.append(sum(f[:, t] * (arg == t).float() for t in w) if mode == "max" else sum(f[:, t] for t in w) / 3.0)
        y = q(torch.stack(ys, 1).reshape(NT // frames * To, H, W, C))
        y.register_hook(bf)
        return ELazy(y.detach().to(torch.bfloat16), None, ACT_NONE, y)

    def head(self, rt, x, fc, frames, dropout_p, keep_mask=None):
        v = self.use(x)
        NT, H, W, C = v.shape
        rows = v.reshape(NT, H * W, C).mean(1) @ self.p[id(fc.weight)].t() + self.p[id(fc.bias)]
        self.logits = rows.reshape(NT // frames, frames, -1).mean(1)
        return self.logits.detach(), None

    def grads(self):
        return {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in self.p.items() if v.requires_grad}


# ---------------------------------------------------------------------------------------------------------------------------- mini nets
class Bottleneck(nn.Module):
    def __init__(self, inplanes, planes, down):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(inplanes, planes, 1, bias=False), nn.BatchNorm2d(planes)
        self.conv2, self.bn2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False), nn.BatchNorm2d(planes)
        self.conv3, self.bn3 = nn.Conv2d(planes, planes * 4, 1, bias=False), nn.BatchNorm2d(planes * 4)
        self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, bias=False), nn.BatchNorm2d(planes * 4)) if down else None


class MiniResNet(nn.Module):
    """stem + max-pool + three bottlenecks + temporal pool + head, with the parameter names and the op order of adamml_amd.resnet"""

    def __init__(self, frames=4, classes=7):
        super().__init__()
        self.frames = frames
        self.conv1, self.bn1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64)
        self.layer1 = nn.Sequential(Bottleneck(64, 64, True), Bottleneck(256, 64, False), Bottleneck(256, 64, False))
        self.fc = nn.Linear(256, classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                m.cs = ConvState(m.weight, m.stride[0], m.padding[0])

    def run(self, ops, x, fused):
        """ResNet._run with `ops` as the executor (conv_bn_add where the production code would take it)"""
        rt = ops.rt
        h = ELazy(x, requires_grad=False)
        h = ops.conv_bn(rt, h, self.conv1.cs, self.bn1, ACT_RELU)
        h = ops.maxpool3x3s2(rt, h, sole_consumer=True)
        pooled = False
        for bi, b in enumerate(self.layer1):
            idn = ops.conv_bn(rt, h, b.downsample[0].cs, b.downsample[1], ACT_NONE) if b.downsample is not None else h
            o = ops.conv_bn(rt, h, b.conv1.cs, b.bn1, ACT_RELU, last_consumer=b.downsample is None)
            o = ops.conv_bn(rt, o, b.conv2.cs, b.bn2, ACT_RELU, sole_consumer=True)
            if fused:
                pooled = bi == 2
                h = ops.conv_bn_add(rt, o, b.conv3.cs, b.bn3, idn, ACT_RELU, idn_sole=b.downsample is not None, tpool=self.frames if pooled else 0)
            else:
                o = ops.conv_bn(rt, o, b.conv3.cs, b.bn3, ACT_NONE, sole_consumer=True)
                h = ops.add_act(rt, o, idn, ACT_RELU, idn_sole=b.downsample is not None)
        if not pooled:
            h = ops.temporal_pool(rt, h, self.frames, "max", sole_consumer=True)
        return ops.head(rt, h, self.fc, self.frames // 2, 0.0)

    def torch_forward(self, x, groups):
        """plain torch modules, one call per group (x NCHW double)"""
        outs = []
        for xg in x.chunk(groups):
            h = F.max_pool2d(F.relu(self.bn1(self.conv1(xg))), 3, 2, 1)
            for b in self.layer1:
                idn = b.downsample(h) if b.downsample is not None else h
                o = F.relu(b.bn1(b.conv1(h)))
                o = F.relu(b.bn2(b.conv2(o)))
                h = F.relu(b.bn3(b.conv3(o)) + idn)
            nt, c, hh, ww = h.shape
            v = h.view(nt // self.frames, self.frames, c, hh, ww).transpose(1, 2)
            h = F.max_pool3d(v, (3, 1, 1), (2, 1, 1), (1, 0, 0)).transpose(1, 2).reshape(-1, c, hh, ww)
            f = self.fc(h.mean((2, 3)))
            outs.append(f.view(-1, self.frames // 2, f.shape[1]).mean(1))
        return torch.cat(outs)


class BasicBlock(nn.Module):
    def __init__(self, inplanes, planes, stride):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False), nn.BatchNorm2d(planes)
        self.conv2, self.bn2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False), nn.BatchNorm2d(planes)
        down = stride != 1 or inplanes != planes
        self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes, 1, stride, bias=False), nn.BatchNorm2d(planes)) if down else None


class MiniBasicNet(nn.Module):
    """stem + max-pool + two 64-channel BasicBlocks + temporal max-pool + a stride-2 128-channel BasicBlock with a downsample branch + a plain
    one + head, with the parameter names and the op order of the BasicBlock arm of adamml_amd.resnet.ResNet._run"""
    basic = True

    def __init__(self, frames=4, classes=7):
        super().__init__()
        self.frames = frames
        self.conv1, self.bn1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64)
        self.layer1 = nn.Sequential(BasicBlock(64, 64, 1), BasicBlock(64, 64, 1))
        self.layer2 = nn.Sequential(BasicBlock(64, 128, 2), BasicBlock(128, 128, 1))
        self.fc = nn.Linear(128, classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                m.cs = ConvState(m.weight, m.stride[0], m.padding[0])

    def run(self, ops, x, fused=False):
        """the BasicBlock arm of ResNet._run with `ops` as the executor (which placement the backward takes is the executor's decision)"""
        rt = ops.rt
        frames = self.frames
        h = ELazy(x, requires_grad=False)
        h = ops.conv_bn(rt, h, self.conv1.cs, self.bn1, ACT_RELU)
        h = ops.maxpool3x3s2(rt, h, sole_consumer=True)
        for li, layer in enumerate((self.layer1, self.layer2)):
            for b in layer:
                idn = ops.conv_bn(rt, h, b.downsample[0].cs, b.downsample[1], ACT_NONE) if b.downsample is not None else h
                o = ops.conv_bn(rt, h, b.conv1.cs, b.bn1, ACT_RELU, last_consumer=b.downsample is None)
                o = ops.conv_bn(rt, o, b.conv2.cs, b.bn2, ACT_NONE, sole_consumer=True)
                h = ops.add_act(rt, o, idn, ACT_RELU, idn_sole=b.downsample is not None)
            if li == 0:
                h = ops.temporal_pool(rt, h, frames, "max", sole_consumer=True)
                frames //= 2
        return ops.head(rt, h, self.fc, frames, 0.0)

    def torch_forward(self, x, groups):
        """plain torch modules, one call per group (x NCHW double)"""
        outs = []
        for xg in x.chunk(groups):
            frames = self.frames
            h = F.max_pool2d(F.relu(self.bn1(self.conv1(xg))), 3, 2, 1)
            for li, layer in enumerate((self.layer1, self.layer2)):
                for b in layer:
                    idn = b.downsample(h) if b.downsample is not None else h
                    o = F.relu(b.bn1(b.conv1(h)))
                    h = F.relu(b.bn2(b.conv2(o)) + idn)
                if li == 0:
                    nt, c, hh, ww = h.shape
                    v = h.view(nt // frames, frames, c, hh, ww).transpose(1, 2)
                    h = F.max_pool3d(v, (3, 1, 1), (2, 1, 1), (1, 0, 0)).transpose(1, 2).reshape(-1, c, hh, ww)
                    frames //= 2
            f = self.fc(h.mean((2, 3)))
            outs.append(f.view(-1, frames, f.shape[1]).mean(1))
        return torch.cat(outs)


class Recorded:
    """an Emu whose entry points go through a Recorder (what monkeypatch does to the model modules on the GPU)"""

    def __init__(self, emu, rec):
        self.rt = emu.rt
        for n in X.OPS:
            if hasattr(emu, n):
                setattr(self, n, rec.wrap(n, getattr(emu, n)))


def randomize(module, seed):
    g = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.weight.data = torch.rand(m.weight.shape, generator=g) + 0.5
            m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.2


def resnet_case(dup=False):
    torch.manual_seed(0)
    net = MiniResNet()
    randomize(net, 1)
    G, clips, T = 2, 1, net.frames
    x = torch.randn(G * clips * T, 20, 20, 8, generator=torch.Generator().manual_seed(2))
    x[..., 3:] = 0
    if dup:                      # frame 2 of every clip := frame 1: exact ties between two taps of a window
        xv = x.reshape(G * clips, T, 20, 20, 8)
        xv[:, 2] = xv[:, 1]
    g = bf(torch.randn(G * clips, 7, generator=torch.Generator().manual_seed(3)))
    return net, x.to(torch.bfloat16), g, G


def basic_case():
    """MiniBasicNet on 2 groups of 2 clips of 4 frames 28 x 28 (spatial sizes 7 and 4; 64 values per channel and group at the least)"""
    torch.manual_seed(0)
    net = MiniBasicNet()
    randomize(net, 1)
    G, clips, T = 2, 2, net.frames
    x = torch.randn(G * clips * T, 28, 28, 8, generator=torch.Generator().manual_seed(2))
    x[..., 3:] = 0
    g = bf(torch.randn(G * clips, 7, generator=torch.Generator().manual_seed(3)))
    return net, x.to(torch.bfloat16), g, G


def emulate(net, x, g, G, fused=True, defects=None):
    emu = Emu(net, G, defects)
    emu.fused_residual = fused if getattr(net, "basic", False) else False       # (MiniResNet: `fused` is conv_bn_add, its own graph)
    rec = X.Recorder()
    net.run(Recorded(emu, rec), x, fused)
    emu.logits.backward(g)
    return emu, rec


def judge(net, x, g, G, fused, defects=None):
    """-> (worst err / bound over the parameter gradients, worst running-statistic err / tol, replay)"""
    emu, rec = emulate(net, x, g, G, fused, defects)
    named = list(net.named_parameters())
    p64, names = X.leaves(named, torch.float64)
    rep = X.Replay(rec.calls, G, p64, X.running_of(net))
    ref = rep.backward(g)
    pert = rep.backward_alg(g)
    p32, _ = X.leaves(named, torch.float32)
    em = X.Replay(rec.calls, G, p32, X.running_of(net), dtype=torch.float32, round_grads=True)
    bnd = X.bounds(ref, em.backward(g), X.alg_terms(ref, pert))
    res = X.compare(emu.grads(), ref, bnd)
    k, wr = X.worst(res)
    stat = 0.0
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            trm, trv = rep.stat_tol[id(m)]
            stat = max(stat, E.vec_ratio(emu.running[id(m)][0], rep.running[id(m)][0], trm),
                       E.vec_ratio(emu.running[id(m)][1], rep.running[id(m)][1], trv))
            assert emu.running[id(m)][2] == rep.running[id(m)][2]
    return wr, names[k], stat, rep, res, names, bnd


# -------------------------------------------------------------------------------------------------------------------------------- tests
def test_unforced_replay_is_torch_autograd_resnet():
    net, x, g, G = resnet_case()
    net.double()
    emu, rec = emulate(net.float(), x, g, G, fused=False)
    net.double()
    named = list(net.named_parameters())
    p64, names = X.leaves(named, torch.float64)
    rep = X.Replay(rec.calls, G, p64, X.running_of(net), force=False)
    rep.backward(g)
    net.train()
    net.zero_grad()
    out = net.torch_forward(x.double()[..., :3].permute(0, 3, 1, 2), G)
    out.backward(g.double())
    assert X.rel_l2(rep.logits, out) <= 1e-12
    gmax = max(p.grad.norm().item() for _, p in named)
    for n, p in named:               # (a bias in front of another BatchNorm has an analytically zero gradient: absolute against the largest)
        assert (p64[id(p)].grad - p.grad).norm().item() <= 1e-12 * max(p.grad.norm().item(), X.SMALL * gmax), n
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            assert X.rel_l2(rep.running[id(m)][0], m.running_mean) <= 1e-12 and X.rel_l2(rep.running[id(m)][1], m.running_var) <= 1e-12
            assert rep.running[id(m)][2] == int(m.num_batches_tracked) == G


def test_unforced_replay_is_torch_autograd_basic():
    """the BasicBlock graph: two consumers of every block input, the stride-2 conv1 and the stride-2 downsample sharing one, the max-pool
    output and a temporal pool's output as identity operands"""
    net, x, g, G = basic_case()
    emu, rec = emulate(net, x, g, G, fused=False)
    net.double()
    named = list(net.named_parameters())
    p64, names = X.leaves(named, torch.float64)
    rep = X.Replay(rec.calls, G, p64, X.running_of(net), force=False)
    rep.backward(g)
    net.train()
    net.zero_grad()
    out = net.torch_forward(x.double()[..., :3].permute(0, 3, 1, 2), G)
    out.backward(g.double())
    assert len(rec.calls) == 1 + 1 + 4 * 3 + 1 + 1 + 1 and [c.op for c in rec.calls].count("add_act") == 4
    assert X.rel_l2(rep.logits, out) <= 1e-12
    gmax = max(p.grad.norm().item() for _, p in named)
    for n, p in named:               # (a bias in front of another BatchNorm has an analytically zero gradient: absolute against the largest)
        assert (p64[id(p)].grad - p.grad).norm().item() <= 1e-12 * max(p.grad.norm().item(), X.SMALL * gmax), n
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            assert X.rel_l2(rep.running[id(m)][0], m.running_mean) <= 1e-12 and X.rel_l2(rep.running[id(m)][1], m.running_var) <= 1e-12
            assert rep.running[id(m)][2] == int(m.num_batches_tracked) == G


class IR(nn.Module):
    def __init__(self, cin, cout, stride, t):
        super().__init__()
        hid = cin * t
        self.pw, self.bnp = nn.Conv2d(cin, hid, 1, bias=False), nn.BatchNorm2d(hid)
        self.dw, self.bnd = nn.Conv2d(hid, hid, 3, stride, 1, groups=hid, bias=False), nn.BatchNorm2d(hid)
        self.pwl, self.bnl = nn.Conv2d(hid, cout, 1, bias=False), nn.BatchNorm2d(cout)
        self.residual = stride == 1 and cin == cout

    def forward(self, x):
        y = F.relu6(self.bnp(self.pw(x)))
        y = F.relu6(self.bnd(self.dw(y)))
        y = self.bnl(self.pwl(y))
        return x + y if self.residual else y


def test_unforced_replay_is_torch_autograd_inverted_residuals(monkeypatch):
    """three inverted residuals through the production run_blocks (stride 2, residual, widening), two groups"""
    from adamml_amd import mobilenet_common as MC
    torch.manual_seed(0)
    net = nn.Sequential(IR(16, 24, 2, 6), IR(24, 24, 1, 6), IR(24, 32, 1, 6))
    net.fc = nn.Linear(32, 5)
    randomize(net, 4)
    net.double()
    G = 2
    plans = [BlockPlan((ConvState(b.pw.weight, 1, 0), b.bnp), (ConvState(b.dw.weight, b.dw.stride[0], 1, depthwise=True), b.bnd),
                       (ConvState(b.pwl.weight, 1, 0), b.bnl), b.residual) for b in net[:3]]
    x = bf(torch.randn(G * 3, 9, 9, 16, generator=torch.Generator().manual_seed(5)))
    g = bf(torch.randn(G * 3, 5, generator=torch.Generator().manual_seed(6)))
    net.float()
    emu = Emu(net, G)
    rec = X.Recorder()
    for n in ("conv_bn", "add_act", "temporal_pool"):
        monkeypatch.setattr(MC, n, rec.wrap(n, getattr(emu, n)))
    monkeypatch.setattr(MC, "conv_bn_add_supported", lambda *a, **k: False)
    h = MC.run_blocks(emu.rt, ELazy(x.to(torch.bfloat16)), plans)
    rec.wrap("head", emu.head)(emu.rt, h, net.fc, 1, 0.0)
    net.double()
    named = list(net.named_parameters())
    p64, _ = X.leaves(named, torch.float64)
    rep = X.Replay(rec.calls, G, p64, X.running_of(net), force=False)
    rep.backward(g)
    net.train()
    xs = x.double().permute(0, 3, 1, 2).requires_grad_(False)
    out = torch.cat([net.fc(net[2](net[1](net[0](c))).mean((2, 3))) for c in xs.chunk(G)])
    out.backward(g.double())
    assert X.rel_l2(rep.logits, out) <= 1e-12
    gmax = max(p.grad.norm().item() for _, p in named)
    for n, p in named:               # (a bias in front of another BatchNorm has an analytically zero gradient: absolute against the largest)
        assert (p64[id(p)].grad - p.grad).norm().item() <= 1e-12 * max(p.grad.norm().item(), X.SMALL * gmax), n


@pytest.fixture(scope="module")
def clean():
    net, x, g, G = resnet_case()
    return (net, x, g, G) + judge(net, x, g, G, True)


def test_emulated_executor_passes_the_bound(clean):
    net, x, g, G, wr, name, stat, rep, res, names, bnd = clean
    print("worst err/bound %.3f at %s; running statistics %.3f; worst forward ratio %.3f" % (wr, name, stat, max(v[1] for v in rep.fwd.values())))
    for k, (e, b) in res.items():
        print("  %-28s err %.3e bound %.3e e_emu %.3e" % (names[k], e, b, clean[10][k][0]))
    assert wr <= 1.0, (wr, name)
    assert stat <= 1.0
    assert max(v[1] for v in rep.fwd.values()) <= 1.0, rep.fwd
    assert max(rep.vec_ratio.values()) <= 1.0, rep.vec_ratio


def test_unfused_emulation_passes_the_bound():
    net, x, g, G = resnet_case()
    wr, name, stat, rep, res, names, _ = judge(net, x, g, G, False)
    assert wr <= 1.0 and stat <= 1.0, (wr, name, stat)
    assert max(v[1] for v in rep.fwd.values()) <= 1.0, rep.fwd


DEFECTS = [("a-identity-gradient-dropped", {"drop_identity": 1}), ("b-block-mask-not-applied", {"no_mask": 0}),
           ("c-sumfix-without-mean-term", {"sumfix": 1}), ("d-two-consumer-gradient-overwritten", {"two_consumers": 0}),
           ("e-group-1-reads-group-0-vectors", {"group_vec": 2}), ("f-running-var-biased", {"running_var": 5}),
           ("g-temporal-pool-last-maximum", {"tie_last": 0})]


@pytest.mark.parametrize("name,defect", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_planted_defect_misses_the_bound(clean, name, defect):
    net, x, g, G = clean[:4]
    if "tie_last" in defect:
        # exact ties between two frames of a window at a POSITIVE value (ties at 0 are gated off): the second frame of every clip repeated.
        # The clean emulation passes on this input too.
        net, x, g, G = resnet_case(dup=True)
        wr, where, stat = judge(net, x, g, G, True)[:3]
        assert max(wr, stat) <= 1.0, (wr, where, stat)
    wr, where, stat = judge(net, x, g, G, True, defect)[:3]
    print("%s: worst err/bound %.2f at %s, running statistics %.2f" % (name, wr, where, stat))
    assert max(wr, stat) >= 2.0, (name, wr, where, stat)


def test_forcing_leaves_little_undecided(clean):
    rep = clean[7]
    share = rep.undecided_share()
    print("undecided share %.4f" % share)
    assert rep.und[1] > 0 and share <= FR.UNDECIDED_CAP


# --------------------------------------------------------------------------------------- the BasicBlock graph (ResNet-18 / -34), two placements
PLACEMENTS = ["unfused", "fused-residual-epilogue", "fused-residual-epilogue-staged-tile"]
FUSED = {"unfused": False, "fused-residual-epilogue": True, "fused-residual-epilogue-staged-tile": "staged"}


@pytest.fixture(scope="module")
def basic_clean():
    """placement -> (net, x, g, G) + judge(...) of the clean emulation"""
    out = {}
    for placement in PLACEMENTS:
        net, x, g, G = basic_case()
        out[placement] = (net, x, g, G) + judge(net, x, g, G, FUSED[placement])
    return out


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_emulated_basic_blocks_pass_the_bound(basic_clean, placement):
    """unfused: every add's backward masks its own gradient.  fused-residual-epilogue: where conv1 is the last consumer of an add output
    (layer1.1.conv1, layer2.1.conv1 -- not layer1.0.conv1, which reads the max-pool output) g' is the float32 data gradient plus the stored
    identity-path gradient, masked and rounded to bf16 once, and the add's own backward passes it on."""
    net, x, g, G, wr, name, stat, rep, res, names, bnd = basic_clean[placement]
    fwd = max(v[1] for v in rep.fwd.values())
    print("%s: worst err/bound %.3f at %s; running statistics %.3f; forward %.3f; vectors %.3f; undecided share %.5f"
          % (placement, wr, name, stat, fwd, max(rep.vec_ratio.values()), rep.undecided_share()))
    assert wr <= 1.0 and stat <= 1.0, (wr, name, stat)
    assert fwd <= 1.0, rep.fwd
    assert max(rep.vec_ratio.values()) <= 1.0, rep.vec_ratio
    assert rep.und[1] > 0 and rep.undecided_share() <= FR.UNDECIDED_CAP
    assert len(res) == 3 * 10 + 2 and not rep.alg          # ten convs with their BatchNorms, fc; nothing ran algebraically


def test_fused_residual_epilogue_runs_where_the_executor_takes_it():
    """the emulation claims the epilogue at the two convs the production _residual_fusable admits on this graph, and nowhere else"""
    net, x, g, G = basic_case()
    emu, rec = emulate(net, x, g, G, fused=True)
    adds = [st[2] for st in emu.state.values() if getattr(st[2], "hold", None) is not None]
    assert [(h.hold.claimed, h.hold.done) for h in adds] == [(True, True), (False, False), (True, True), (False, False)]
    emu, rec = emulate(net, x, g, G, fused=False)
    assert not [st for st in emu.state.values() if getattr(st[2], "hold", None) is not None and st[2].hold.claimed]


# Tensor 9 (in order of first use) is the temporal pool's output, the input of layer2.0: its consumers are the downsample (0), recorded first
# and so reversed last, and conv1 (1), whose data gradient is in h.grad when the downsample's must ADD to it.  drop_use (9, 1): it overwrote.
BASIC_DEFECTS = [("a-identity-gradient-of-the-second-add-dropped", {"drop_identity": 1}, PLACEMENTS[:2]),
                 ("b-first-add-mask-not-applied", {"no_mask": 0}, PLACEMENTS[:2]),
                 ("c-two-consumer-gradient-overwritten-without-downsample", {"two_consumers": 0}, PLACEMENTS[:2]),
                 ("d-downsample-data-gradient-overwrites-conv1", {"drop_use": (9, 1)}, PLACEMENTS[:2]),
                 ("e-epilogue-sums-the-unmasked-gradient", {"sum_unmasked": 0}, PLACEMENTS[1:]),
                 ("f-running-var-biased", {"running_var": 5}, PLACEMENTS[:1])]
BASIC_DEFECT_CASES = [(n, d, p) for n, d, ps in BASIC_DEFECTS for p in ps]


@pytest.mark.parametrize("name,defect,placement", BASIC_DEFECT_CASES, ids=["%s-%s" % (c[0], c[2]) for c in BASIC_DEFECT_CASES])
def test_planted_basic_defect_misses_the_bound(basic_clean, name, defect, placement):
    net, x, g, G, wr0, _, stat0 = basic_clean[placement][:7]
    assert max(wr0, stat0) <= 1.0                    # the clean run on the same input
    wr, where, stat = judge(net, x, g, G, FUSED[placement], defect)[:3]
    print("%s (%s): worst err/bound %.2f at %s, running statistics %.2f" % (name, placement, wr, where, stat))
    assert max(wr, stat) >= 2.0, (name, wr, where, stat)


# ------------------------------------------------------------------------------- op-level graphs (tools/executor_ops.py): the new forms
O = X.ops_module()

OPS_ENTRY = ("conv_bn", "conv_bn_add", "add_act", "materialize", "maxpool3x3s2")


def he(module, seed):
    g = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, nn.Conv2d):
            fan = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
            m.weight.data = torch.randn(m.weight.shape, generator=g) * (2.0 / fan) ** 0.5


def one_d(net):
    return [p for p in net.parameters() if p.dim() == 1]


def depthwise(net):
    return [m.weight for m in net.modules() if isinstance(m, nn.Conv2d) and m.groups > 1]


# label of executor_ops.ROWS, frozen set: every new form, and the two partial freezes the model rows take (frozen BatchNorm vectors,
# frozen depthwise weights) on a graph small enough for the CPU
OPS_CASES = [("ops-shared-depthwise-input", None), ("ops-shared-depthwise-input", depthwise), ("ops-alg-gemm-arm", None),
             ("ops-alg-gemm-arm-fused", None), ("ops-unfused-maxpool-pool-first", None), ("ops-unfused-maxpool-conv-first", None),
             ("ops-accumulating-add", None), ("ops-accumulating-add", one_d)]
OPS_IDS = [c[0] + ("-frozen-" + c[1].__name__ if c[1] else "") for c in OPS_CASES]


def ops_case(label, frozen=None):
    net = O.make(label)
    he(net, 7)
    randomize(net, 8)
    for p in (frozen(net) if frozen else ()):
        p.requires_grad_(False)
    return net, net.make_input()


def ops_emulate(monkeypatch, net, x, G, defects=None):
    """the graph of an executor_ops net with the torch emulation as its executor, recorded -> (emu, recorder, output ELazy, g)"""
    emu = Emu(net, G, defects)
    emu.direct_sums = True
    rec = X.Recorder()
    with monkeypatch.context() as mp:
        for n in OPS_ENTRY:
            mp.setattr(O, n, rec.wrap(n, getattr(emu, n)))
        mp.setattr(O, "conv_bn_add_supported", lambda *a, **k: True)
        out = net.graph(emu.rt, ELazy(x, requires_grad=False))
    g = bf(torch.randn(tuple(out.shape), generator=torch.Generator().manual_seed(3)))
    out.val.backward(g)
    return emu, rec, out, g


def ops_judge(monkeypatch, label, frozen=None, defects=None, G=O.GROUPS):
    """-> (worst err / bound, where, worst running-statistic err / tol, replay, emulation)"""
    net, x = ops_case(label, frozen)
    emu, rec, out, g = ops_emulate(monkeypatch, net, x, G, defects)
    named = list(net.named_parameters())
    p64, names = X.leaves(named, torch.float64)
    rep = X.Replay(rec.calls, G, p64, X.running_of(net)).output_of(out)
    ref = rep.backward(g)
    pert = rep.backward_alg(g)
    p32, _ = X.leaves(named, torch.float32)
    em = X.Replay(rec.calls, G, p32, X.running_of(net), dtype=torch.float32, round_grads=True, recomputed_z=label.endswith("-fused")).output_of(out)
    res = X.compare(emu.grads(), ref, X.bounds(ref, em.backward(g), X.alg_terms(ref, pert)))
    k, wr = X.worst(res)
    stat = 0.0
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            trm, trv = rep.stat_tol[id(m)]
            stat = max(stat, E.vec_ratio(emu.running[id(m)][0], rep.running[id(m)][0], trm),
                       E.vec_ratio(emu.running[id(m)][1], rep.running[id(m)][1], trv))
            assert emu.running[id(m)][2] == rep.running[id(m)][2] == G
    return wr, names[k], stat, rep, emu


@pytest.mark.parametrize("label,frozen", OPS_CASES, ids=OPS_IDS)
def test_unforced_replay_is_torch_autograd_ops(monkeypatch, label, frozen):
    """Replay.output_of on a graph without a head; a shared input, a pool that is not the sole consumer, a tensor added twice and the
    frozen sets fall out of autograd: the unforced replay IS float64 torch autograd of the same modules, group by group"""
    net, x = ops_case(label, frozen)
    G = O.GROUPS
    emu, rec, out, g = ops_emulate(monkeypatch, net, x, G)
    net.double()
    named = list(net.named_parameters())
    p64, _ = X.leaves(named, torch.float64)
    rep = X.Replay(rec.calls, G, p64, X.running_of(net), force=False).output_of(out)
    got = rep.backward(g)
    net.train()
    net.zero_grad()
    want = torch.cat([net.torch_forward(c) for c in x.double().permute(0, 3, 1, 2).chunk(G)]).permute(0, 2, 3, 1)
    want.backward(g.double())
    assert X.rel_l2(rep.logits, want) <= 1e-12
    assert set(got) == {id(p) for _, p in named if p.requires_grad} and all(p.grad is None for _, p in named if not p.requires_grad)
    gmax = max(p.grad.norm().item() for _, p in named if p.requires_grad)
    for n, p in named:
        if p.requires_grad:
            assert (got[id(p)] - p.grad).norm().item() <= 1e-12 * max(p.grad.norm().item(), X.SMALL * gmax), n
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            assert X.rel_l2(rep.running[id(m)][0], m.running_mean) <= 1e-12 and X.rel_l2(rep.running[id(m)][1], m.running_var) <= 1e-12
            assert rep.running[id(m)][2] == int(m.num_batches_tracked) == G


@pytest.mark.parametrize("label,frozen", OPS_CASES, ids=OPS_IDS)
def test_emulated_ops_pass_the_bound(monkeypatch, label, frozen):
    wr, where, stat, rep, _ = ops_judge(monkeypatch, label, frozen)
    print("%s: worst err/bound %.3f at %s; running statistics %.3f; forward %.3f" % (label, wr, where, stat, max(v[1] for v in rep.fwd.values())))
    assert wr <= 1.0 and stat <= 1.0, (wr, where, stat)
    assert max(v[1] for v in rep.fwd.values()) <= 1.0, rep.fwd
    assert max(rep.vec_ratio.values()) <= 1.0, rep.vec_ratio
    assert rep.undecided_share() <= FR.UNDECIDED_CAP
    assert len(rep.alg) == (1 if "alg" in label else 0)


# (row, frozen set, defect).  drop_use (t, k): see Emu.use -- in ops-shared-depthwise-input tensor 1 is h (consumers: the depthwise conv, then
# materialize, whose gradient is there first and which the depthwise data gradient must ADD to); in ops-unfused-maxpool-pool-first tensor 1
# is h (consumers: the pool, then the strided conv, whose data gradient is there first and which adamml_maxpool2d_bwd must add to)
OPS_DEFECTS = [("1-depthwise-data-gradient-overwrites", "ops-shared-depthwise-input", None, {"drop_use": (1, 1)}),
               ("2-maxpool-backward-overwrites", "ops-unfused-maxpool-pool-first", None, {"drop_use": (1, 1)}),
               ("3-maxpool-backward-first-tap", "ops-unfused-maxpool-conv-first", None, {"first_tap": 0}),
               ("4-act-bwd-from-output-mask-skipped", "ops-shared-depthwise-input", None, {"no_mask": 0}),
               ("5-frozen-batchnorm-as-constant-affine", "ops-accumulating-add", one_d, {"frozen_bn_constant": 1}),
               ("6-gemm-arm-wtbw-group-channel-transposed", "ops-alg-gemm-arm", None, {"gemm_transposed": 1}),
               ("6-gemm-arm-wg-group-channel-transposed", "ops-alg-gemm-arm", None, {"gemm_transposed": 2}),
               ("6-gemm-arm-wg-transposed-gram-from-forward", "ops-alg-gemm-arm-fused", None, {"gemm_transposed": 2})]


@pytest.mark.parametrize("name,label,frozen,defect", OPS_DEFECTS, ids=[d[0] for d in OPS_DEFECTS])
def test_planted_ops_defect_misses_the_bound(monkeypatch, name, label, frozen, defect):
    wr, where, stat = ops_judge(monkeypatch, label, frozen, defect)[:3]
    print("%s: worst err/bound %.2f at %s, running statistics %.2f" % (name, wr, where, stat))
    assert max(wr, stat) >= 2.0, (name, wr, where, stat)


@pytest.mark.parametrize("which", [1, 2])
def test_gemm_arm_transposition_is_invisible_with_one_group(monkeypatch, which):
    """[Cout][Cin][G] read as [Cout][G][Cin] is the same buffer at G = 1: the defect every G = 1 row passes.  The same graph, input and
    defect as above in ONE BatchNorm group gives bit for bit the clean gradients (and meets the bound)."""
    clean = ops_judge(monkeypatch, "ops-alg-gemm-arm", G=1)
    planted = ops_judge(monkeypatch, "ops-alg-gemm-arm", None, {"gemm_transposed": which}, G=1)
    assert clean[0] <= 1.0 and planted[0] <= 1.0, (clean[:2], planted[:2])
    a, b = clean[4].grads(), planted[4].grads()
    assert len(a) == len(b) == 6 and all(torch.equal(u, v) for u, v in zip(a.values(), b.values()))
