"""Forced float64 replay of what the host executor (adamml_amd/runtime.py) ran, and the bound its parameter gradients are held to.

Plain CPU module (it never touches torch.cuda).  Three parts:

Recorder.  Wraps the executor entry points (OPS; `gap` is the policy net's output op) in the namespaces of the model modules and of the
op-level graphs of tools/executor_ops.py (MODULES) through pytest's monkeypatch and keeps,
for every call in order, the op, its bound arguments (flags included) and a snapshot of the returned Lazy: data, vec (scale, shift, mean,
invstd), act, gs, the 1-bit mask of a residual add, and what NetRT.capture["aux"] filed for it (codes / mask / vec of conv_bn_add, idx of
maxpool3x3s2).  The production `_run` methods are driven unchanged.

Replay.  Rebuilds the network from that record as a torch-autograd graph in NHWC doubles in which every STORED tensor takes the value the
run stored (straight-through: v = ref + (stored - ref).detach()) and every DECISION is the one the run took:
  ReLU / ReLU6 gate of a lazy conv output   fmaf(scale, y, shift) of the recorded raw y and vec in float32, strict inequalities (conv_ref.bn_mask)
  block-output gate                          the recorded mask bits
  spatial max-pool                           the recorded idx;  fused temporal pool: the recorded 2-bit codes (3 = gate closed)
  unfused temporal pool                      first maximum of the float32 values the kernel compares
  conv operands                              the staged bf16 value (conv_ref.lazy_operand), weights bf16(W) (depthwise / 1-channel stem: float32)
  BatchNorm statistics                       float64 from the stored raw tensor; conv_bn_add: float64 from z = bf16(W) a (never stored)
  running mean / var, num_batches_tracked    nn.BatchNorm2d (momentum 0.1, unbiased variance), once per group in group order
Its backward is the exact derivative of the forward that ran.  While it builds the graph it checks the forward op by op, teacher-forced:
each op's float64 result from the recorded inputs against the recorded output with the per-kernel models of conv_ref / fused_ref /
elementwise_ref (`fwd`: op index -> max err / tol), and the BatchNorm vectors against `vec_tolerance`.
force=False: no forcing, own decisions, unrounded weights -- plain float64 autograd of the same modules (the anchor of the CPU test).

Emulator.  The same replay in float32 with a hook that rounds the gradient to bf16 at every tensor whose gradient the runtime stores as
the UNFUSED path places them: every raw conv output (dz) and every activated value.  Its per-tensor distance from the float64 replay is
e_emu, computed from the reference alone.

Bound, per parameter-gradient tensor:   rel-L2(hip, ref) <= K e_emu + alg_term
  K = 4: the fused kernels add at most two further bf16 roundings per layer over the unfused placement (the staged GEMM tile, dz never
  formed on the algebraic path): under 1.8x in quadrature, 4 leaves a factor two.  Shared by the CPU and GPU tests, not tuned on either.
  alg_term: what the algebraic backward computes in exact arithmetic minus the derivative of the forward that ran -- abi_ref's chain row
  (chain_alg - chain_true: first order in W - bf16(W), + the bf16 rounding of the adamml_alg_pack entries), for the convs whose backward
  ran algebraically.  That deviation is constant over the pixels, so it does not average out in the sums over pixels UPSTREAM of the conv
  (bn2's dgamma / dbeta of the same block) as the emulator's independent roundings do: it is carried to every tensor by a second backward
  pass (Replay.backward_alg) instead of being charged to the conv's own weight alone.
  Tensors whose reference norm is below 1e-3 of the largest are compared in absolute terms against that largest norm.  An exact zero of
  the reference (e_emu = 0, alg_term = 0) has a zero bound.
"""
import importlib
import importlib.util
import inspect
import math
import os
import sys

import torch
import torch.nn.functional as F

from tests import conv_ref as R
from tests import elementwise_ref as E
from tests import fused_ref as FR
from tests import abi_ref as AB

K = 4.0
SMALL = 1e-3
EPS, MOMENTUM = 1e-5, 0.1
OPS = ("conv_bn", "conv_stem1_bn", "conv_bn_add", "add_act", "materialize", "maxpool3x3s2", "temporal_pool", "head", "gap")
MODULES = ("adamml_amd.resnet", "adamml_amd.mobilenet_common", "adamml_amd.sound_mobilenet_v2", "adamml_amd.policy_net", "executor_ops")
ACT_NONE, ACT_RELU, ACT_RELU6 = 0, 1, 2


def bf(x):
    """round to bf16 in the tensor's own dtype"""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def st(ref, stored):
    """straight-through: the stored value, the reference's derivative"""
    return ref + (stored.to(ref.dtype) - ref).detach()


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-300)).item()


# ------------------------------------------------------------------------------------------------------------------------------ recorder
def ops_module():
    """tools/executor_ops.py (the op-level graphs, shared with tools/launch_trace.py) as the module `executor_ops`, loaded by path once"""
    mod = sys.modules.get("executor_ops")
    if mod is None:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "executor_ops.py")
        spec = importlib.util.spec_from_file_location("executor_ops", path)
        mod = sys.modules["executor_ops"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    return mod


class Snap:
    """what a Lazy held when its producer returned (tensors by reference: the executor never rewrites them)"""
    __slots__ = ("data", "vec", "scale", "shift", "act", "gs", "mask", "alg", "shape")

    def __init__(self, lz):
        self.data, self.vec, self.act, self.gs = lz.data, lz.vec, lz.act, lz.gs
        self.scale, self.shift = lz.scale, lz.shift
        res = getattr(lz, "res", None)
        self.mask = res[4] if res is not None else None
        self.alg = bool(getattr(lz, "alg", False))
        self.shape = tuple(lz.shape)


class Call:
    __slots__ = ("op", "args", "out", "snap", "aux")


class Recorder:
    def __init__(self):
        self.calls = []
        self.keep = []          # every Lazy seen: ids stay unique for the replay

    def wrap(self, name, fn):
        sig = inspect.signature(fn)

        def wrapped(*a, **k):
            out = fn(*a, **k)
            b = sig.bind(*a, **k)
            b.apply_defaults()
            c = Call()
            c.op, c.args, c.out = name, dict(b.arguments), out
            rt = c.args.pop(next(iter(b.arguments)))
            lz = out[0] if name in ("head", "gap") else out
            c.snap = None if name in ("head", "gap") else Snap(lz)
            cap = getattr(rt, "capture", None)
            c.aux = cap["aux"].get(id(lz)) if cap and "aux" in cap else None
            self.keep.append((out, c.args))
            self.calls.append(c)
            return out
        return wrapped

    def install(self, monkeypatch):
        for m in MODULES:
            mod = ops_module() if m == "executor_ops" else importlib.import_module(m)
            for n in OPS:
                if hasattr(mod, n):
                    monkeypatch.setattr(mod, n, self.wrap(n, getattr(mod, n)))


# -------------------------------------------------------------------------------------------------------------------------------- replay
class Node:
    __slots__ = ("raw", "scale", "shift", "act", "snap", "value")


def _cpu(t):
    return None if t is None else t.detach().cpu()


def _svec(snap):
    """(scale, shift, gstride) as the kernels are given them: flat views from the first element onward"""
    if snap.vec is not None:
        v = _cpu(snap.vec).reshape(-1)
        return v, v[snap.shape[-1]:], 4 * snap.shape[-1]
    if snap.scale is not None:
        return _cpu(snap.scale).reshape(-1), _cpu(snap.shift).reshape(-1), snap.gs
    return None, None, 0


def first_argmax(taps):
    """E.first_argmax on any dtype: scan `t > best` from -inf -> index of the first maximum"""
    best = torch.full_like(taps[0], -math.inf)
    idx = torch.zeros(taps[0].shape, dtype=torch.int64)
    for i in range(taps.shape[0]):
        upd = taps[i] > best
        best = torch.where(upd, taps[i], best)
        idx = torch.where(upd, torch.full_like(idx, i), idx)
    return idx


def taps2d(v, OH, OW):
    """differentiable E._taps2d (zero padding: a selected tap is never a padding position)"""
    p = F.pad(v, (0, 0, 1, 2 * OW + 1 - v.shape[2], 1, 2 * OH + 1 - v.shape[1]))
    return torch.stack([p[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2] for kh in range(3) for kw in range(3)])


class Replay:
    def __init__(self, calls, groups, params, running, dtype=torch.float64, force=True, round_grads=False, check=None, training=True, recomputed_z=False):
        """params: id(Parameter) -> leaf of `dtype`; running: id(BatchNorm module) -> [running_mean, running_var, num_batches_tracked]
        as they were BEFORE the recorded step (updated in place here, in float64).
        recomputed_z (emulator only): the BatchNorm-backward reduction of every conv_bn_add read the raw conv output as Lazy.recompute wrote
        it, rounded to bf16 (no producer of its gradient left partial sums) -- one more storage point of the run the emulator then rounds at."""
        self.recomputed_z = bool(recomputed_z and round_grads)
        self.calls, self.G, self.p, self.running = calls, groups, params, running
        self.dt, self.force, self.round, self.training = dtype, force, round_grads, training
        self.check = (dtype == torch.float64 and force) if check is None else check
        self.nodes = {}
        self.fwd = {}             # op index -> (op, max err / tol)
        self.vec_ratio = {}       # op index -> max err / tol of the recorded BatchNorm vectors
        self.und = [0.0, 0.0]     # undecided gates, gates
        self.alg = {}             # id(weight) -> dict(a, w, vec, gamma, g) of a conv whose backward ran algebraically
        self.stat_tol = {}        # id(bn) -> (tol running_mean, tol running_var)
        self.logits = None
        self.perturb = False
        for i, c in enumerate(calls):
            getattr(self, "_" + c.op)(i, c, **c.args)

    # -- helpers
    def _hook(self, t):
        if self.round and t.requires_grad:
            t.register_hook(bf)
        return t

    def _node(self, lz):
        n = self.nodes.get(id(lz))
        if n is None:                 # a network input
            n = self._new(lz, _cpu(lz.data).to(self.dt), None, None, ACT_NONE, Snap(lz))
        return n

    def _new(self, lz, raw, scale, shift, act, snap):
        n = Node()
        n.raw, n.scale, n.shift, n.act, n.snap, n.value = raw, scale, shift, act, snap, None
        self.nodes[id(lz)] = n
        return n

    def _g(self, t):
        return t.reshape((self.G, -1) + tuple(t.shape[1:]))

    def _affine(self, raw, scale, shift):
        return (self._g(raw) * scale.reshape(self.G, 1, 1, 1, -1) + shift.reshape(self.G, 1, 1, 1, -1)).reshape(raw.shape)

    def _pre32(self, snap):
        """float32 fmaf(scale, y, shift) of the recorded raw tensor and vec: what every loader's gate sees"""
        s, t, gs = _svec(snap)
        return R.lazy_operand(_cpu(snap.data), s, t, 0, self.G, gs, round_bf16=False)

    def _gate(self, v, pre, act):
        lo, hi = R.ACT_BOUNDS[act]
        m = ((pre > lo) & (pre < hi)).to(v.dtype)
        v = v * m
        if act == ACT_RELU6:
            v = v + 6.0 * (pre >= hi).to(v.dtype)
        return v

    def _val(self, lz):
        n = self._node(lz)
        if n.value is None:
            if n.scale is None:
                n.value = n.raw
            else:
                v = self._affine(n.raw, n.scale, n.shift)
                if n.act != ACT_NONE:
                    v = self._gate(v, self._pre32(n.snap) if self.force else v.detach(), n.act)
                n.value = self._hook(v)
        return n.value

    def _operand(self, lz, dense):
        v = self._val(lz)
        if not self.force:
            return v, None
        sn = self._node(lz).snap
        s, t, gs = _svec(sn)
        exact = R.lazy_operand(_cpu(sn.data), s, t, sn.act, self.G, gs, round_bf16=dense)
        return st(v, exact), exact

    def _weight(self, cs, dense):
        w = self.p[id(cs.weight)]
        return st(w, bf(w.detach())) if (self.force and dense) else w

    def _bn(self, i, y, bn, snap=None, stat_err=None):
        """train-mode BatchNorm of y [G*N, H, W, C] (graph) per group -> (scale, shift) [G, C]; running statistics updated"""
        C = y.shape[-1]
        if not self.training:
            # eval mode: the affine of the module's running statistics AS THEY ARE NOW (`running`), one pair for all groups
            rm, rv = self.running[id(bn)][0].to(self.dt), self.running[id(bn)][1].to(self.dt)
            scale = self.p[id(bn.weight)] * (rv + EPS).rsqrt()
            shift = self.p[id(bn.bias)] - rm * scale
            if self.check and snap is not None:
                got = _cpu(snap.vec).reshape(self.G, 4, C)[0, :2] if snap.vec is not None else torch.stack([_cpu(snap.scale), _cpu(snap.shift)])
                ref = torch.stack([scale, shift]).detach().double()
                tol = K_FINALIZE * R.U32 * torch.stack([scale.abs(), shift.abs() + (rm * scale).abs()]).detach().double()
                self.vec_ratio[i] = E.vec_ratio(got, ref, tol)
            return scale.expand(self.G, C), shift.expand(self.G, C)
        yg = y.reshape(self.G, -1, C)
        n = yg.shape[1]
        mean, var = yg.mean(1), yg.var(1, unbiased=False)
        inv = (var + EPS).rsqrt()
        scale = self.p[id(bn.weight)] * inv
        shift = self.p[id(bn.bias)] - mean * scale
        run = self.running.get(id(bn))
        mag = None
        if run is not None:
            mag = [run[0].abs(), run[1].abs()]          # the running values the float32 update rounds: before, and after every group
            for g in range(self.G):
                run[0] = (1 - MOMENTUM) * run[0] + MOMENTUM * mean[g].detach().double()
                run[1] = (1 - MOMENTUM) * run[1] + MOMENTUM * var[g].detach().double() * n / max(n - 1, 1)
                mag = [torch.maximum(mag[0], run[0].abs()), torch.maximum(mag[1], run[1].abs())]
            run[2] += self.G
        if self.check and snap is not None and snap.vec is not None:
            ref = torch.stack([scale, shift, mean, inv], 1).detach().double()
            tol, trm, trv = vec_tolerance(ref, self.p[id(bn.weight)].detach().double(), n, stat_err(yg.detach()), self.G)
            self.vec_ratio[i] = E.vec_ratio(_cpu(snap.vec).reshape(ref.shape), ref, tol)
            if mag is not None:
                u = K_FINALIZE * R.U32 * self.G
                self.stat_tol[id(bn)] = (trm + u * mag[0], trv + u * mag[1])
        return scale, shift

    def _undecided(self, pre, tol):
        self.und[0] += float((pre.abs() <= tol).sum())
        self.und[1] += pre.numel()

    # -- ops
    def _conv(self, i, x_val, exact, w, cs, bn, act, snap, lz, groups_conv, stride, pad):
        cin = w.shape[1] * groups_conv
        y = F.conv2d(x_val[..., :cin].permute(0, 3, 1, 2), w, stride=stride, padding=pad, groups=groups_conv).permute(0, 2, 3, 1)
        tol = None
        if self.check:
            with torch.no_grad():
                ab = F.conv2d(exact[..., :cin].permute(0, 3, 1, 2).abs(), w.detach().abs(), stride=stride, padding=pad,
                              groups=groups_conv).permute(0, 2, 3, 1)
                nred = w.shape[1] * w.shape[2] * w.shape[3]
                tol = R.tolerance(y.detach(), ab, nred, R.RHO_BF16)
                self.fwd[i] = ("conv", R.err_ratio(_cpu(snap.data), y.detach(), ab, nred, R.RHO_BF16))
        raw = self._hook(st(y, _cpu(snap.data)) if self.force else y)
        scale, shift = self._bn(i, raw, bn, snap, stat_err=stored_stat_err)
        n = self._new(lz, raw, scale, shift, act, snap)
        if self.check and act != ACT_NONE and snap.vec is not None:
            sc = _cpu(snap.vec).double()[:, 0].reshape(self.G, 1, 1, 1, -1).abs()
            pre = self._pre32(snap)
            t = (self._g(tol) * sc).reshape(pre.shape)
            self._undecided(pre, t)
            if act == ACT_RELU6:
                self._undecided(pre - 6.0, t)
        return n

    def _conv_bn(self, i, c, x, cs, bn, act, sole_consumer=False, last_consumer=False):
        dense = not cs.depthwise
        a, exact = self._operand(x, dense)
        w = self._weight(cs, dense)
        self._conv(i, a, exact, w, cs, bn, act, c.snap, c.out, cs.cout if cs.depthwise else 1, cs.stride, cs.pad)
        if c.snap.alg and self.check:
            self._file_alg(c.out, cs, bn, exact, c.snap.vec, a)

    def _conv_stem1_bn(self, i, c, x1, cs, bn, act):
        B, G, H, W = x1.shape
        v = _cpu(x1).to(self.dt).permute(1, 0, 2, 3).reshape(G * B, H, W, 1)
        self._conv(i, v, v, self.p[id(cs.weight)], cs, bn, act, c.snap, c.out, 1, 2, 1)

    def _alg_entry(self, cs, bn, exact, vec, a_t, lin):
        """file what abi_ref's chain row needs of a conv whose backward ran algebraically, and hook its graph: g' (the gradient arriving at
        the linear BatchNorm output `lin`) is kept; in the perturbed pass the gradient of the operand a_t gets the chain row's F - T added"""
        ent = dict(a=exact.reshape(self.G, -1, exact.shape[-1]).double(), w=cs.weight.detach().cpu().float().reshape(cs.cout, -1),
                   vec=_cpu(vec).float().reshape(self.G, 4, -1), gamma=bn.weight.detach().cpu().float())
        self.alg[id(cs.weight)] = ent
        if lin.requires_grad:
            lin.register_hook(lambda g: ent.__setitem__("g", g.detach().double().reshape(self.G, -1, g.shape[-1])))
        if a_t.requires_grad:
            a_t.register_hook(lambda ga: ga + alg_delta(ent).reshape(ga.shape) if self.perturb else ga)

    def _file_alg(self, lz, cs, bn, exact, vec, a_t):
        self._alg_entry(cs, bn, exact, vec, a_t, self._val(lz))

    def _conv_bn_add(self, i, c, x, cs, bn, idn, act, idn_sole=False, tpool=0, next_cs=None):
        G = self.G
        a, exact = self._operand(x, True)
        w = self._weight(cs, True)
        z = self._hook(a @ w.reshape(cs.cout, -1).t())                              # never stored: no forcing
        if self.recomputed_z:
            z = st(z, bf(z.detach()))
        code_t, mask_t, vec = c.aux if c.aux is not None else (None, None, None)
        scale, shift = self._bn(i, z, bn, None if vec is None else _VecOnly(vec, z.shape),
                                stat_err=lambda zg: gram_stat_err(exact.reshape(G, -1, exact.shape[-1]), w.detach().double().reshape(cs.cout, -1)))
        lin = self._affine(z, scale, shift)
        if self.check and vec is not None and self.training:
            self._alg_entry(cs, bn, exact, vec, a, lin)
        pre = lin + self._val(idn) if idn is not None else lin
        r = None
        if self.check:
            isn = None if idn is None else self._node(idn).snap
            s, t, gs = (None, None, 0) if isn is None else _svec(isn)
            r = FR.fwd_bn_add_ref(exact.reshape(G, -1, exact.shape[-1]).double(), bf(cs.weight.detach().cpu().float()).reshape(cs.cout, -1),
                                  _cpu(vec), act, None if idn is None else _cpu(isn.data), s, t, gs)
        if not tpool:
            if act != ACT_NONE:
                if self.force and mask_t is not None:
                    pre = pre * FR.unpack_bits(_cpu(mask_t), pre.shape).to(pre.dtype)
                elif self.force:                 # (no gradient was asked for: no mask stored; the gate of the stored output)
                    pre = self._gate(pre, _cpu(c.snap.data).double(), act)
                else:
                    pre = self._gate(pre, pre.detach(), act)
            if self.check:
                q, und = FR.fadd_check(_cpu(c.snap.data), r, act, None if mask_t is None else _cpu(mask_t), what="op %d conv_bn_add" % i, bias=False)
                self.fwd[i] = ("conv_bn_add", q)
                self.und[0] += und * pre.numel()
                self.und[1] += pre.numel()
            out = pre
        else:
            T = tpool
            blk = self._hook(pre)                                                     # the full-rate block output (its gate is in the codes)
            N, H, W, C = blk.shape
            f = blk.reshape(N // T, T, H, W, C)
            wins = FR.pool_windows(T)
            if self.force and code_t is not None:
                code = FR.unpack_codes(_cpu(code_t), (N // T, T // 2, H, W, C))
            else:
                cs_ = []
                for win in wins:
                    cand = torch.stack([f[:, t] for _, t in win]).detach()
                    tap = torch.tensor([k for k, _ in win])[first_argmax(cand)]
                    cs_.append(torch.where(cand.max(0).values > 0, tap, torch.full_like(tap, 3)))
                code = torch.stack(cs_, 1)
            out = torch.stack([sum(f[:, t] * (code[:, to] == k).to(f.dtype) for k, t in win) for to, win in enumerate(wins)], 1)
            out = out.reshape(N // 2, H, W, C)
            if self.check:
                r["Q"] = H * W
                p = FR.fwd_bn_add_tpool_ref(r, T)
                q, und = FR.tpool_check(_cpu(c.snap.data), None if code_t is None else _cpu(code_t), p, what="op %d conv_bn_add tpool" % i)
                self.fwd[i] = ("conv_bn_add_tpool", q)
                self.und[0] += und * out.numel()
                self.und[1] += out.numel()
        out = self._hook(st(out, _cpu(c.snap.data)) if self.force else out)
        self._new(c.out, out, None, None, ACT_NONE, c.snap)

    def _add_act(self, i, c, z, idn, act, idn_sole=False):
        pre = self._val(z) + (self._val(idn) if idn is not None else 0)
        if act != ACT_NONE:
            if self.force and c.snap.mask is not None:
                pre = pre * FR.unpack_bits(_cpu(c.snap.mask), pre.shape).to(pre.dtype)
            elif self.force:
                pre = self._gate(pre, _cpu(c.snap.data).double(), act)
            else:
                pre = self._gate(pre, pre.detach(), act)
        if self.check:
            zs, ids = self._node(z).snap, (None if idn is None else self._node(idn).snap)
            C = zs.shape[-1]
            s, t, gs = _svec(zs)
            s2, t2, gs2 = (None, None, 0) if ids is None else _svec(ids)
            ref, ab, k = E.bn_act_add_ref(_cpu(zs.data).reshape(-1, C), s, t, gs, act, None if ids is None else _cpu(ids.data).reshape(-1, C),
                                          s2, t2, gs2, self.G)
            self.fwd[i] = ("add_act", R.err_ratio(_cpu(c.snap.data).reshape(-1, C), ref, ab, 1, R.RHO_BF16, acc=k))
            if act != ACT_NONE and c.snap.mask is not None:
                assert torch.equal(_cpu(c.snap.mask).reshape(-1), E.mask_bits_ref(_cpu(c.snap.data), act)), "op %d: mask is not act'(stored out)" % i
        out = self._hook(st(pre, _cpu(c.snap.data)) if self.force else pre)
        self._new(c.out, out, None, None, ACT_NONE, c.snap)

    def _materialize(self, i, c, x):
        v = self._val(x)
        if self.check:
            sn = self._node(x).snap
            C = sn.shape[-1]
            s, t, gs = _svec(sn)
            ref, ab, k = E.bn_act_add_ref(_cpu(sn.data).reshape(-1, C), s, t, gs, sn.act, groups=self.G)
            self.fwd[i] = ("materialize", R.err_ratio(_cpu(c.snap.data).reshape(-1, C), ref, ab, 1, R.RHO_BF16, acc=k))
        out = self._hook(st(v, _cpu(c.snap.data)) if self.force else v)
        self._new(c.out, out, None, None, ACT_NONE, c.snap)

    def _maxpool3x3s2(self, i, c, x, sole_consumer=False):
        v = self._val(x)
        N, H, W, C = v.shape
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        taps = taps2d(v, OH, OW)
        if self.force:
            idx = _cpu(c.aux).to(torch.int64)
        else:
            neg = taps2d(torch.ones_like(v.detach()), OH, OW) == 0
            idx = first_argmax(torch.where(neg, torch.full_like(taps.detach(), -math.inf), taps.detach()))
        y = torch.gather(taps, 0, idx.unsqueeze(0))[0]
        if self.check:
            sn = self._node(x).snap
            s, t, gs = _svec(sn)
            # the kernel compares the float32 values fmaf(scale, x, shift) and stores the winner rounded once: the recorded tap must hold
            # the maximum (to the two float32 roundings by which an fmaf can differ from this evaluation) and the stored value be its bf16
            v32 = E.lazy_f32(_cpu(sn.data), s, t, sn.act, self.G, gs)
            ab = v32.abs() if s is None else E.lazy_f32(_cpu(sn.data).double().abs(), s.abs(), t.abs(), 0, self.G, gs)
            t32 = E._taps2d(v32, OH, OW, -math.inf)
            sel = torch.gather(t32, 0, idx.unsqueeze(0))[0]
            sab = torch.gather(E._taps2d(ab, OH, OW, 0.0), 0, idx.unsqueeze(0))[0]
            short = ((t32.max(0).values - sel) / (4 * R.U32 * sab + 1e-300)).max().item()
            self.fwd[i] = ("maxpool3x3s2", max(short, R.err_ratio(_cpu(c.snap.data), sel, sab, 1, R.RHO_BF16, acc=2)))
        out = self._hook(st(y, _cpu(c.snap.data)) if self.force else y)
        self._new(c.out, out, None, None, ACT_NONE, c.snap)

    def _temporal_pool(self, i, c, x, frames, mode, sole_consumer=False):
        v = self._val(x)
        NT, H, W, C = v.shape
        T = frames
        To, win = E.temporal_windows(T)
        f = v.reshape(NT // T, T, H, W, C)
        sn = self._node(x).snap
        s, t, gs = _svec(sn) if sn is not None else (None, None, 0)
        if mode == "max":
            if self.force:
                dec = E.lazy_f32(_cpu(sn.data), s, t, sn.act, self.G, gs).reshape(f.shape)
            else:
                dec = f.detach()
            ys = []
            for w in win:
                arg = torch.tensor(w)[first_argmax(torch.stack([dec[:, tt] for tt in w]))]
                ys.append(sum(f[:, tt] * (arg == tt).to(f.dtype) for tt in w))
            y = torch.stack(ys, 1)
        else:
            y = torch.stack([sum(f[:, tt] for tt in w) / 3.0 for w in win], 1)
        y = y.reshape(NT // T * To, H, W, C)
        if self.check:
            xr = _cpu(sn.data).reshape(NT, H * W, C)
            if mode == "max":
                yr, _ = E.temporal_pool_fwd_ref(xr, s, t, gs, sn.act, T, 0, self.G)
                self.fwd[i] = ("temporal_pool", 0.0 if torch.equal(_cpu(c.snap.data).double().reshape(yr.shape), yr) else math.inf)
            else:
                ref, ab = E.temporal_pool_fwd_ref(xr, s, t, gs, sn.act, T, 1, self.G)
                self.fwd[i] = ("temporal_pool_avg", R.err_ratio(_cpu(c.snap.data).reshape(ref.shape), ref, ab, 1, R.RHO_BF16, acc=E.K_TPOOL_AVG_FWD))
        out = self._hook(st(y, _cpu(c.snap.data)) if self.force else y)
        self._new(c.out, out, None, None, ACT_NONE, c.snap)

    def _head(self, i, c, x, fc, frames, dropout_p, keep_mask=None):
        if keep_mask is not None or (dropout_p and dropout_p > 0):
            raise RuntimeError("executor_ref: the replay runs with dropout 0")
        v = self._val(x)
        NT, H, W, C = v.shape
        feat = v.reshape(NT, H * W, C).mean(1)
        wt, b = self.p[id(fc.weight)], self.p[id(fc.bias)]
        rows = feat @ wt.t() + b
        self.logits = rows.reshape(NT // frames, frames, -1).mean(1)
        if self.check:
            sn = self._node(x).snap
            sc, sh, gs = _svec(sn)
            fr, fa, _ = E.gap_fwd_ref(_cpu(sn.data), sc, sh, gs, sn.act, NT // self.G, H * W, self.G)      # teacher-forced: the recorded vec
            wd, bd = wt.detach().double(), b.detach().double()
            ref = (fr @ wd.t() + bd).reshape(NT // frames, frames, -1).mean(1)
            ab = (fa @ wd.abs().t() + bd.abs()).reshape(NT // frames, frames, -1).mean(1)
            # float32 throughout: the average pool (H W terms), the dot product (C), the bias and the mean over the frames
            self.fwd[i] = ("head", R.err_ratio(_cpu(c.out[0]), ref, ab, H * W + C + frames + 1, R.RHO_F32))

    def _gap(self, i, c, x):
        """the policy net's output: the spatial mean, float32 [N, C]"""
        v = self._val(x)
        NT, H, W, C = v.shape
        self.logits = v.reshape(NT, H * W, C).mean(1)
        if self.check:
            sn = self._node(x).snap
            sc, sh, gs = _svec(sn)
            ref, ab, n = E.gap_fwd_ref(_cpu(sn.data), sc, sh, gs, sn.act, NT // self.G, H * W, self.G)
            self.fwd[i] = ("gap", R.err_ratio(_cpu(c.out[0]), ref, ab, n, R.RHO_F32))

    def output_of(self, lz):
        """Designates the output of a graph that ends in neither `head` nor `gap` (tools/executor_ops.py): the value of the Lazy `lz`, a
        tensor one of the recorded calls returned.  backward / backward_alg then take the gradient w.r.t. that value [G*N, H, W, C]."""
        self.logits = self._val(lz)
        return self

    def backward(self, g):
        """-> id(Parameter) -> gradient"""
        self.logits.backward(_cpu(g).to(self.dt), retain_graph=bool(self.alg))
        return {k: (v.grad.clone() if v.grad is not None else torch.zeros_like(v)) for k, v in self.p.items() if v.requires_grad}

    def backward_alg(self, g):
        """The same backward with every algebraically-run conv replaced by what the algebraic form computes in exact arithmetic (abi_ref's
        chain row: F instead of T, its weight pack rounded to bf16 as adamml_alg_pack stores it) -> id(Parameter) -> gradient.  Its distance
        from backward() is the alg_term of the bound: first order in W - bf16(W) and in the pack rounding, both constant over the pixels,
        so they do NOT average out in the sums over pixels upstream (bn2's dgamma / dbeta) the way the emulator's independent roundings do."""
        if not self.alg:                 # nothing ran algebraically: the same gradients
            return {k: (v.grad.clone() if v.grad is not None else torch.zeros_like(v)) for k, v in self.p.items() if v.requires_grad}
        for v in self.p.values():
            v.grad = None
        self.perturb = True
        try:
            self.logits.backward(_cpu(g).to(self.dt))
        finally:
            self.perturb = False
        out = {k: (v.grad.clone() if v.grad is not None else torch.zeros_like(v)) for k, v in self.p.items() if v.requires_grad}
        for wid, e in self.alg.items():
            if "ddw" in e and wid in out:
                out[wid] = out[wid] + e["ddw"].reshape(out[wid].shape)
        return out

    def undecided_share(self):
        return self.und[0] / max(self.und[1], 1.0)


class _VecOnly:
    def __init__(self, vec, shape):
        self.vec, self.shape = vec, tuple(shape)


# ------------------------------------------------------------------------------------------------------- BatchNorm vectors and statistics
def stored_stat_err(yg):
    """errors of (sum y, sum y^2) accumulated from the STORED output [G, n, C] in float32 partials (conv_ref.stats_check's model)"""
    n = yg.shape[1]
    w = R.C_ACC * math.sqrt(n) * R.U32
    yy = yg.double()
    s1a, s2 = yy.abs().sum(1), (yy * yy).sum(1)
    return 2.0 ** -23 * yy.sum(1).abs() + w * s1a, (2.0 ** -23 + w) * s2


def gram_stat_err(a, w):
    """errors of (W s, diag(W G W^T)) from the float32 Gram matrix and column sums of the operand a [G, P, Cin] (fused_ref.chain_reference)"""
    Gr, Ga, sr, sa, P = FR.gram_ref(a.double())
    wacc = R.C_ACC * math.sqrt(P) * R.U32
    eG, es = R.RHO_F32 * Gr.abs() + wacc * Ga, R.RHO_F32 * sr.abs() + wacc * sa
    _, gst = FR.gram_stats_ref(w, Gr, sr)
    Cout = w.shape[0]
    return es @ w.abs().t() + gst[:, :Cout], torch.einsum("oi,gij,oj->go", w.abs(), eG, w.abs()) + gst[:, Cout:]


K_FINALIZE = 8     # float32 roundings adamml_bn_finalize spends on one output (mean, variance, rsqrt, two products, the running update)


def vec_tolerance(ref, gamma, n, stat_err, groups):
    """ref [G, 4, C] float64 (scale, shift, mean, invstd) -> (tol [G, 4, C], tol running_mean [C], tol running_var [C]): the statistics'
    errors carried to first order as fused_ref.chain_reference does, + K_FINALIZE float32 roundings of the finalize kernel itself.  The
    running tolerances cover what the batch statistics contribute; the caller adds the roundings of the running values themselves."""
    e_s1, e_s2 = stat_err
    sc, sh, mu, inv = ref[:, 0], ref[:, 1], ref[:, 2], ref[:, 3]
    var = 1.0 / (inv * inv)
    u = K_FINALIZE * R.U32
    e_mu = e_s1 / n + u * mu.abs()
    e_var = e_s2 / n + 2 * mu.abs() * e_mu + u * (var + mu * mu)
    e_inv = 0.5 * inv ** 3 * e_var + u * inv
    e_sc = gamma.abs() * e_inv + u * sc.abs()
    e_sh = mu.abs() * e_sc + sc.abs() * e_mu + u * (sh.abs() + (mu * sc).abs())
    tol = torch.stack([e_sc, e_sh, e_mu, e_inv], 1)
    k = n / max(n - 1.0, 1.0)
    return tol, MOMENTUM * e_mu.sum(0) + groups * u * mu.abs().max(0).values, MOMENTUM * k * e_var.sum(0) + groups * u * (k * var).max(0).values


# --------------------------------------------------------------------------------------------------------------------------------- bound
def alg_delta(e):
    """F - T of abi_ref's chain row for one conv (e: Replay._alg_entry, with the g' of the running backward pass) -> dx difference
    [G, P, Cin]; the dW difference is left in e["ddw"]"""
    G, P = e["a"].shape[0], e["a"].shape[1]
    op = {"w": e["w"], "G": G, "P": P, "gamma": e["gamma"]}
    wb = R.bf16(e["w"].double())
    fw = {"a": e["a"], "wb": wb, "z": torch.einsum("gpi,oi->gpo", e["a"], wb), "vec": e["vec"], "g": e["g"]}
    T, Fa = AB.chain_true(op, fw), AB.chain_alg(op, fw)
    e["ddw"] = Fa["dw"] - T["dw"]
    dx = torch.einsum("gpk,gck->gpc", Fa["x"], R.bf16(Fa["w_alg"])) + Fa["epi"].unsqueeze(1)
    return dx - T["dx"]


def alg_terms(ref, pert):
    """key -> |gradient of the perturbed pass - gradient| (absolute; `bounds` divides by its denominator)"""
    return {k: (pert[k].double() - ref[k].double()).norm().item() for k in ref}


def bounds(ref, emu, alg=None):
    """ref, emu: key -> gradient tensor of the float64 replay / the float32 emulator -> key -> (e_emu, bound, denominator)"""
    alg = alg or {}
    gmax = max(v.double().norm().item() for v in ref.values())
    out = {}
    for k, r in ref.items():
        nr = r.double().norm().item()
        small = nr < SMALL * gmax
        den = gmax if small else nr
        e = (emu[k].double() - r.double()).norm().item() / den if den > 0 else 0.0
        out[k] = (e, K * e + (alg.get(k, 0.0) / den if den > 0 else 0.0), den)
    return out


def compare(got, ref, bnd):
    """-> key -> (err, bound): err = |got - ref| / denominator of `bounds`"""
    res = {}
    for k, (e, b, den) in bnd.items():
        d = (got[k].detach().cpu().double() - ref[k].double()).norm().item()
        res[k] = (d / den if den > 0 else (0.0 if d == 0 else math.inf), b)
    return res


def worst(res):
    k = max(res, key=lambda n: res[n][0] / res[n][1] if res[n][1] > 0 else (0.0 if res[n][0] == 0 else math.inf))
    e, b = res[k]
    return k, (e / b if b > 0 else (0.0 if e == 0 else math.inf))


def leaves(named_params, dtype):
    """id(Parameter) -> detached CPU leaf of `dtype` (requires_grad as the parameter), and the id -> name map"""
    p = {id(v): v.detach().cpu().to(dtype).clone().requires_grad_(v.requires_grad) for _, v in named_params}
    return p, {id(v): k for k, v in named_params}


def running_of(module):
    """id(BatchNorm module) -> [running_mean, running_var, num_batches_tracked] (float64 CPU copies)"""
    return {id(m): [m.running_mean.detach().cpu().double().clone(), m.running_var.detach().cpu().double().clone(), int(m.num_batches_tracked)]
            for m in module.modules() if isinstance(m, torch.nn.BatchNorm2d)}
