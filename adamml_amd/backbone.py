"""Shared machinery of the HIP backbones: parameter containers with reference-identical state_dict names,
flat fp32 parameter / gradient buffers, weight re-packing, and the autograd bridge that runs one backbone
call as a single node (forward = fused HIP launches, backward = the recorded tape in reverse)."""
import warnings
import weakref

import torch
import torch.nn as nn

from . import hip, interleave, ops, plan
from .runtime import NetRT, ConvState, Tape


class FlatBuffers:
    """Re-homes every parameter of `module` into one flat fp32 buffer and pre-assigns .grad as views of a
    second flat buffer: one memset zeroes all gradients, one RCCL all-reduce synchronises them, and the fused
    optimizer kernels update the whole sub-network in one launch."""

    RECHECK_EVERY = 32

    def __init__(self, module):
        self.module = module
        self.flat = None
        self.flat_grad = None
        self.params = []
        self.detached = False       # True: .grad belongs to autograd / torch.optim (enable_autograd_param_grads)
        # every backbone below `module` reports an assigned / deleted parameter or sub-module (HipBackbone.__setattr__): a swapped `fc`
        # is re-homed by the NEXT ensure(), not by the every-32nd-call walk (round-4 advisor finding)
        for m in module.modules():
            if isinstance(m, HipBackbone):
                m.__dict__.setdefault("_flat_watchers", []).append(weakref.ref(self))

    def invalidate(self):
        """The next ensure() walks the module's parameters again (a parameter object may have been replaced)."""
        self._calls = -1

    def set_detached(self, on):
        """on: stop managing .grad (drop the flat views so that AccumulateGrad creates ordinary gradient tensors)."""
        if on and not self.detached and self.flat_grad is not None:
            lo, hi = self.flat_grad.data_ptr(), self.flat_grad.data_ptr() + self.flat_grad.numel() * 4
            for p in self.params:
                if p.grad is not None and lo <= p.grad.data_ptr() < hi:
                    p.grad = None
            self.flat_grad = None
        self.detached = on

    def ensure(self, device):
        # fast path (every forward): the parameter objects found at the last re-homing still sit in the flat buffer.  (Walking
        # module.parameters() -- ~1400 modules for AdaMML -- costs ~1 ms per sub-network per step, which matters at the per-GPU batch
        # of the reference recipe where the step is host-bound; a parameter REPLACED by the caller is caught by the data_ptr probes of
        # the first and the last one and by the optimizers / load_state_dict going through .data, which keeps the objects.)
        # A parameter OBJECT swapped by the caller in the middle of the list (a new `fc` for another class count) is not seen by those two
        # probes: every RECHECK_EVERY-th call takes the full walk anyway (round-3 advisor finding), and so does the first call after invalidate().
        self._calls = getattr(self, "_calls", 0) + 1
        if self.flat is not None and self.flat.device == device and self.params and self._calls % self.RECHECK_EVERY and \
                self.params[0].data_ptr() == self.views[0].data_ptr() and self.params[-1].data_ptr() == self.views[-1].data_ptr():
            return
        params = [p for p in self.module.parameters()]
        for m in self.module.modules():             # (the backbones cache their parameter lists too)
            m.__dict__.pop("_plist", None)
        if self.flat is not None and self.flat.device == device and len(params) == len(self.params) and \
                all(p.data_ptr() == v.data_ptr() for p, v in zip(params, self.views)):
            self.params = params
            return
        total = sum(p.numel() for p in params)
        flat = torch.empty(total, dtype=torch.float32, device=device)
        views = []
        off = 0
        for p in params:
            n = p.numel()
            v = flat[off:off + n].view(p.shape)
            v.copy_(p.data.to(device=device, dtype=torch.float32))
            p.data = v
            views.append(v)
            off += n
        self.flat, self.views, self.params = flat, views, params
        self.flat_grad = None

    def ensure_grads(self):
        """(Re)attach zeroed gradient views when the optimizer dropped them (zero_grad(set_to_none=True))."""
        if self.detached:
            return
        params = self.params
        if self.flat_grad is None:
            self.flat_grad = torch.zeros_like(self.flat)
            attached = False
        else:
            attached = all((p.grad is not None) for p in params if p.requires_grad)
        if attached:
            return
        self.flat_grad.zero_()
        off = 0
        for p in params:
            n = p.numel()
            p.grad = self.flat_grad[off:off + n].view(p.shape) if p.requires_grad else None
            off += n


def queue_end_of_backward(fn):
    """Run fn() once the current autograd backward pass has executed all its nodes.  torch exposes this only as
    `Variable._execution_engine.queue_callback` -- the hook torch's own DistributedDataParallel reducer and FSDP finalise their
    backward with, unchanged since torch 1.0, but not part of the documented API: it is reached through this ONE function, which fails
    with a clear message when a torch build moves it (tests/test_host_cpu.py::test_autograd_end_of_backward_callback pins the behaviour
    this package relies on)."""
    eng = getattr(torch.autograd.Variable, "_execution_engine", None)
    q = getattr(eng, "queue_callback", None)
    if q is None:
        raise RuntimeError("torch %s has no autograd end-of-backward callback (Variable._execution_engine.queue_callback): adamml_amd "
                           "defers the SyncBatchNorm backward rounds and the side-stream join to it" % torch.__version__)
    q(fn)


def run_backward(net, tape, g, params):
    """Backward of one backbone invocation (autograd formula of adamml::backbone_call, ops.py): the recorded tape in reverse.
    params empty  -> the weight-gradient kernels accumulate into the pre-attached flat .grad views; returns [].
    params given  -> their gradients are delivered THROUGH autograd (stock DistributedDataParallel hooks, torch.optim): the
                     kernels write into a fresh scratch buffer bound to .grad for the duration of the tape, the views of that
                     buffer are returned and AccumulateGrad adds them to whatever .grad held before."""
    if not params and net.rt.sync.enabled and interleave.ENABLED:
        # SyncBatchNorm: the backward passes of the backbones are issued round-robin (interleave.py) once autograd has
        # handed every backbone its output gradient -- nothing upstream waits for a backbone's input gradient
        _deferred.append((tape, g.contiguous(), net, torch.cuda.current_stream()))
        if len(_deferred) == 1:
            queue_end_of_backward(_run_deferred)
        return []
    if not params:
        run_tape(tape, g, net)
        return []
    total = sum(p.numel() for p in params)
    scratch = torch.zeros(total, dtype=torch.float32, device=g.device)
    views, saved, off = [], [], 0
    for p in params:
        views.append(scratch[off:off + p.numel()].view(p.shape))
        off += p.numel()
        saved.append(p.grad)
    try:
        for p, v in zip(params, views):
            p.grad = v
        run_tape(tape, g, net)
    finally:
        for p, s_ in zip(params, saved):
            p.grad = s_
    return views


def run_tape(tape, g, net):
    if isinstance(tape, plan.PlanTape):
        # replayed call: the recorded reverse tape as one C call per segment (arena memset, launches and stream waits included)
        tape.grad_out = g
        tape.backward()
        _queue_default_stream_join(net, g.device, torch.cuda.current_stream())
        return
    rec = getattr(tape, "recorder", None)
    if rec is not None:                       # this call is being recorded into a launch plan: its backward too
        g = g.contiguous()
        rec.begin_backward(g)
        hip.recorder = rec
    try:
        net.rt.bwd_arena.reset(g.device)
        tape.grad_out = g.contiguous()
        tape.backward()
        side = torch.cuda.current_stream()
        if net.rt.wgrad_stream is not None:
            side.wait_stream(net.rt.wgrad_stream)      # the weight gradients are complete before anyone reads .grad
            if hip.recorder is not None:
                hip.recorder.wait(side.cuda_stream, net.rt.wgrad_stream.cuda_stream)
            net.rt.wgrad_pending.clear()               # later allocations on this stream are ordered behind that wait
    finally:
        if rec is not None:
            hip.recorder = None
    if rec is not None:
        rec.end_backward()
        net._finish_recording(tape, rec)
    _queue_default_stream_join(net, g.device, side)


def _queue_default_stream_join(net, device, side):
    if side != torch.cuda.default_stream(device) and not getattr(net, "_join_queued", False):
        # the HIP weight-gradient kernels wrote .grad on a side stream without going through AccumulateGrad: make
        # the default stream wait for them once, when the whole backward pass has been enqueued
        net._join_queued = True

        def _join():
            net._join_queued = False
            torch.cuda.default_stream(device).wait_stream(side)
        if _in_deferred_run[0]:
            _join()                     # already past the engine's callbacks: join right away
        else:
            queue_end_of_backward(_join)


_deferred = []
_in_deferred_run = [False]


def _run_deferred():
    """End-of-backward callback under SyncBatchNorm: run the recorded tapes of all backbones interleaved."""
    pend = list(_deferred)
    del _deferred[:]
    if not pend:
        return
    dev = pend[0][1].device
    _in_deferred_run[0] = True
    try:
        jobs = [((lambda t=t, g=g, n=n: run_tape(t, g, n)), s) for (t, g, n, s) in pend]
        interleave.run_interleaved(jobs, dev, phase="bwd")
    finally:
        _in_deferred_run[0] = False


def enable_autograd_param_grads(module, on=True):
    """Deliver the backbones' parameter gradients through autograd instead of writing them into the flat .grad views behind
    its back: what stock torch.nn.parallel.DistributedDataParallel (its hooks sit on the AccumulateGrad nodes) and
    torch.optim on `model.module.*.parameters()` need -- the reference's own loop (train_adamml.py:126-129, 250-257).  Switched
    on by the first forward that arrives through a DistributedDataParallel wrapper (StockDDPAware), or explicitly by the caller."""
    for m in module.modules():
        if isinstance(m, HipBackbone):
            m.expose_param_grads = on
        for fb in (getattr(m, "_flat_policy", None), getattr(m, "_flat_main", None), getattr(m, "flat_owner", None)):
            if isinstance(fb, FlatBuffers):
                fb.set_detached(on)


class StockDDPAware:
    """Mixin of the modules a caller may wrap in torch's DistributedDataParallel (train_adamml.py:129).  Stock DDP hangs its
    reduction hooks on the parameters' AccumulateGrad nodes, so the parameter gradients have to travel through autograd instead
    of being written into the flat .grad views behind its back.  The switch is made where the wrap becomes a FACT, not where it is
    probed: the first forward that arrives through a DistributedDataParallel parent (`_adopt_stock_ddp`, called from `forward`
    via the module's `_ddp_parent_probe` forward-pre-hook) calls enable_autograd_param_grads(self, True).  Attribute probes
    (hasattr / inspect.getmembers / dir()-based tools) have no side effect."""

    def _install_ddp_probe(self):
        self._under_stock_ddp = False
        self.register_forward_pre_hook(StockDDPAware._ddp_parent_probe)

    @staticmethod
    def _ddp_parent_probe(module, args):
        if module._under_stock_ddp:
            return
        # DistributedDataParallel.forward runs `self.module(*inputs)` from inside its own forward: look for it on the call stack
        # (a dozen frames per forward until the wrap is seen; nothing afterwards)
        import sys
        from torch.nn.parallel import DistributedDataParallel
        f = sys._getframe(1)
        while f is not None:
            owner = f.f_locals.get("self")
            if isinstance(owner, DistributedDataParallel) and getattr(owner, "module", None) is module:
                module._under_stock_ddp = True
                enable_autograd_param_grads(module, True)
                return
            f = f.f_back


def _check_groups(x, groups):
    """x: NHWC bf16 frames [groups * N, H, W, C] (group-major), or -- one-channel fp32 input of the MobileNetV2 stems, handed over as the
    caller has it -- [B, groups, H, W] fp32 (group = dim 1, runtime.conv_stem1_bn)."""
    if x.dtype == torch.float32:
        if x.dim() != 4 or x.shape[1] != groups:
            raise RuntimeError("backbone call: fp32 input must be [B, groups, H, W] (got %s for %d groups)" % (tuple(x.shape), groups))
    elif groups < 1 or x.shape[0] % groups:
        raise RuntimeError("backbone call: %d images do not split into %d groups" % (x.shape[0], groups))


class NotifyingSequential(nn.Sequential):
    """nn.Sequential whose item edits (`net.classifier[1] = nn.Linear(...)`, del / append / insert / extend) are reported to the backbone
    that owns it, exactly as an attribute assignment on the backbone is (HipBackbone.__setattr__): the flat parameter buffers and the
    optimizers re-home the new parameters at the NEXT call instead of at the every-32nd-call walk (round-5 advisor finding).  Same
    state_dict names as a plain nn.Sequential."""

    def _notify(self):
        owner = self.__dict__.get("_owner_ref")
        owner = owner() if owner is not None else None
        if owner is not None:
            owner._params_changed()

    def bind_owner(self, owner):
        self.__dict__["_owner_ref"] = weakref.ref(owner)
        return self

    def __setitem__(self, idx, module):
        super().__setitem__(idx, module)
        self._notify()

    def __delitem__(self, idx):
        super().__delitem__(idx)
        self._notify()

    def append(self, module):
        r = super().append(module)
        self._notify()
        return r

    def insert(self, index, module):
        r = super().insert(index, module)
        self._notify()
        return r

    def extend(self, sequential):
        r = super().extend(sequential)
        self._notify()
        return r


class HipBackbone(nn.Module):
    """Base of ResNet / MobileNetV2 backbones executed by libadamml_hip."""

    def __init__(self):
        super().__init__()
        self.rt = NetRT()
        self._conv_states = []
        self._anchor = None
        self._packed_version = None
        self.flat_owner = None       # FlatBuffers managing this net's parameters (self or the enclosing sub-network)
        self.grad_hook = None        # HipDDP: callable(params) fired in backward once the gradients of `params` are final
        self.expose_param_grads = False      # deliver parameter gradients through autograd (enable_autograd_param_grads)
        self._handle = ops.register_net(self)
        self._pending_tape = None
        self._precomputed = None
        self._bn_probe = None

    # -- a parameter or sub-module assigned / removed after construction (e.g. a new `fc` for another class count) ---------------
    def _params_changed(self):
        self.__dict__.pop("_plist", None)
        self.__dict__["_packed_version"] = None
        for ref in self.__dict__.get("_flat_watchers", ()):
            fb = ref()
            if fb is not None:
                fb.invalidate()
        fo = self.__dict__.get("flat_owner")
        if fo is not None:
            fo.invalidate()

    def __setattr__(self, name, value):
        super().__setattr__(name, value)
        if isinstance(value, (nn.Parameter, nn.Module)):
            self._params_changed()

    def __delattr__(self, name):
        watched = name in self._parameters or name in self._modules
        super().__delattr__(name)
        if watched:
            self._params_changed()

    def register_parameter(self, name, param):
        super().register_parameter(name, param)
        self._params_changed()

    # -- weight packs ------------------------------------------------------------------------------
    def _register_conv(self, conv, depthwise=False):
        cs = ConvState(conv.weight, conv.stride[0], conv.padding[0], depthwise)
        self._conv_states.append(cs)
        return cs

    def mark_weights_dirty(self):
        """Parameters were rewritten through raw pointers (fused optimizer step, checkpoint load into the flat buffer):
        re-pack the bf16 GEMM operands and drop the cached eval-mode BatchNorm affines."""
        self._packed_version = None
        self.rt.state_gen += 1

    def _repack(self, need_dgrad):
        ver = tuple(cs.weight._version for cs in self._conv_states[:4]) + (self._conv_states[0].weight.data_ptr(), need_dgrad)
        if self._packed_version == ver:
            return
        # one launch refreshes every bf16 GEMM pack of this backbone (table rebuilt only when a buffer moved)
        rows = [r for cs in self._conv_states for r in cs.pack_rows(need_dgrad)]
        key = tuple((r[0].data_ptr(), r[1].data_ptr()) for r in rows)
        if getattr(self, "_pack_key", None) != key:
            epb = hip.load().adamml_pack_block_elems()
            tab, blk = [], 0
            for w, out, cout, cin_true, cin_pad, kh, kw, mode, n in rows:
                tab.append([w.data_ptr(), out.data_ptr(), cout | (cin_true << 32), cin_pad | (kh << 32), kw | (mode << 32), blk])
                blk += (n + epb - 1) // epb
            self._pack_table = torch.tensor(tab, dtype=torch.int64).to(rows[0][0].device)
            self._pack_blocks = blk
            self._pack_key = key
        hip.call("adamml_pack_conv_weights_batched", hip.ptr(self._pack_table), len(rows), self._pack_blocks)
        for cs in self._conv_states:
            cs.repack_stem()
        self._packed_version = ver

    def _mark_grads_ready_after(self, tape, modules):
        """Record a tape marker BEFORE the forward ops of `modules`: in the reversed tape it fires right after their last
        backward closure, i.e. when every weight gradient of those modules has been enqueued -- the data-parallel wrapper
        starts their all-reduce there, overlapping it with the rest of the backward pass."""
        if not tape.need_grad or self.grad_hook is None:
            return
        params = [p for m in modules for p in m.parameters() if p.requires_grad]
        if params:
            def fire():
                if self.grad_hook is None:
                    return
                rec = hip.recorder
                if self.rt.wgrad_stream is not None:       # this bucket's weight gradients run on the side stream
                    cur = torch.cuda.current_stream()
                    cur.wait_stream(self.rt.wgrad_stream)
                    if rec is not None:
                        rec.wait(cur.cuda_stream, self.rt.wgrad_stream.cuda_stream)
                if rec is not None:                        # a launch plan calls the hook between two of its segments
                    hook = self.grad_hook
                    rec.boundary(lambda: hook(params))
                    hip.recorder = None
                try:
                    self.grad_hook(params)
                finally:
                    if rec is not None:
                        hip.recorder = rec
            tape.record(fire)

    def _params(self):
        plist = self.__dict__.get("_plist")
        if plist is None:                # (parameter OBJECTS are fixed after construction; only their .data / .requires_grad change)
            plist = self.__dict__["_plist"] = list(self.parameters())
        return plist

    def _trainable(self):
        return any(p.requires_grad for p in self._params())

    def call(self, x, groups=1, precomputed=None):
        """x: NHWC bf16 frames tensor on the GPU, `groups` independent module calls stacked along dim 0 (group-major):
        each group gets its own train-mode BatchNorm statistics and running-stat update, exactly as `groups` successive
        calls of the reference module would (models/adamml.py:151-160 loops the segments).  Returns the fp32 head output
        of all groups stacked the same way.  precomputed: the (output, tape) of run_raw() on the same x -- the launch sequence has
        already been issued (as a coroutine of interleave.run_interleaved) and is only attached to autograd here."""
        hip.require_gpu(x)
        _check_groups(x, groups)
        need_grad = torch.is_grad_enabled() and self._trainable()
        self._adopt_sync_batchnorm()
        if self._anchor is None or self._anchor.device != x.device:
            self._anchor = torch.zeros(1, device=x.device)
        anchor = self._anchor.detach().requires_grad_(need_grad)
        params = [p for p in self._params() if p.requires_grad] if (need_grad and self.expose_param_grads) else []
        self._precomputed = precomputed
        try:
            return torch.ops.adamml.backbone_call(anchor, x, params, self._handle, groups, need_grad)
        finally:
            self._precomputed = None

    def run_raw(self, x, groups=1):
        """The launch sequence of call() WITHOUT the operator around it: returns (output, tape) for call(x, groups, precomputed=...).
        What a job of interleave.run_interleaved runs: a coroutine must not park inside a torch dispatcher call."""
        hip.require_gpu(x)
        _check_groups(x, groups)
        self._adopt_sync_batchnorm()
        return self.run_planned(x, groups, torch.is_grad_enabled() and self._trainable())

    def _adopt_sync_batchnorm(self):
        """nn.SyncBatchNorm.convert_sync_batchnorm(model) (train_adamml.py:126-127) replaces the BatchNorm2d containers by
        SyncBatchNorm ones holding the same tensors: the statistics exchange of this runtime is switched on from their
        process group, so the reference's two wrapping lines keep their meaning."""
        if self._bn_probe is None:
            self._bn_probe = next((n for n, m in self.named_modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)), "")
        if not self._bn_probe or self.rt.sync.enabled:
            return
        m = self.get_submodule(self._bn_probe)
        if isinstance(m, nn.SyncBatchNorm):
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                from .runtime import SyncCtx
                self.rt.sync = SyncCtx(m.process_group, True)

    def out_shape(self, x_shape, groups):
        """Shape of the fp32 head output for an input of shape x_shape (fake / meta implementation of adamml::backbone_call)."""
        raise NotImplementedError

    # -- the surface distributed.HipDDP queries on the module it wraps: a bare backbone is wrapped by adamml_amd.train_unimodal ---------
    def backbones(self):
        return [self]

    def enable_sync_bn(self, group=None, force=False):
        """SyncBatchNorm (train_unimodal.py:155-157): this backbone's BN statistic sums are all-reduced over `group`."""
        from .runtime import SyncCtx
        self.rt.sync = SyncCtx(group, True, force)

    def flat_grad_buffers(self):
        """The flat fp32 gradient buffer of this backbone when it owns one (inside AdaMML the enclosing sub-network does)."""
        fb = self.flat_owner
        return [fb.flat_grad] if fb is not None and fb.flat_grad is not None else []

    # -- launch plans (plan.py) ----------------------------------------------------------------------------------------
    def _plan_key(self, x, groups, need_grad):
        """Everything the launch sequence of a call depends on; None: this call is not plannable."""
        rt = self.rt
        if not plan.ENABLED or hip.profiler is not None or rt.capture is not None or self.expose_param_grads \
                or getattr(self, "_dropout_keep_mask", None) is not None or (rt.sync.enabled and self.training and not interleave.active()):
            return None
        if not self.training and (not plan.EVAL_ENABLED or need_grad or x.numel() > plan.MAX_EVAL_ELEMENTS):
            # inference: a plan pins the activations of its call shape, and the shapes of policy-gated inference vary with the decisions --
            # worth it for serving-sized calls only
            return None
        ws = rt.wgrad_stream.cuda_stream if rt.wgrad_stream is not None else 0
        if not x.is_contiguous():
            return None            # (a launch sequence that first copies its input would bake the copy's address into the plan: round-3 advisor finding)
        return (tuple(x.shape), x.dtype, groups, need_grad, self.training, rt.sync.enabled, ws, hip._stream(),
                tuple(p.requires_grad for p in self._params()), self.flat_owner.flat.data_ptr() if (self.flat_owner is not None and
                self.flat_owner.flat is not None) else self._params()[0].data_ptr(), self.grad_hook is not None)

    def run_planned(self, x, groups, need_grad):
        """_run(), or the replay of its launch plan once the same call has been seen WARMUP_CALLS times."""
        key = self._plan_key(x, groups, need_grad)
        if key is None:
            return self._run(x, groups, need_grad=need_grad)
        plans = self.__dict__.setdefault("_launch_plans", {})
        entry = plans.get(key)
        if isinstance(entry, plan.Plan):
            if entry.busy():                       # an earlier replay still waits for its backward: this call runs eagerly (plan.Plan.busy)
                plan.stats["busy_fallbacks"] = plan.stats.get("busy_fallbacks", 0) + 1
                entry.busy_streak = getattr(entry, "busy_streak", 0) + 1
                if entry.busy_streak == 8:         # (a replayed forward whose graph is kept alive without a backward pins its plan forever)
                    warnings.warn("adamml launch plan: %d consecutive calls of %s ran eagerly because an earlier replayed forward of the same "
                                  "call still waits for its backward (outputs kept without detach()?); the plan is bypassed until that "
                                  "graph is released" % (entry.busy_streak, type(self).__name__))
                return self._run(x, groups, need_grad=need_grad)
            entry.busy_streak = 0
            return entry.forward(x)
        seen = entry or 0
        if seen < plan.WARMUP_CALLS or hip.recorder is not None:
            plans[key] = seen + 1
            return self._run(x, groups, need_grad=need_grad)
        # record this (ordinary, eager) call
        rec = plan.Recorder(x)
        self._packed_version = None                # the plan re-packs the bf16 operands every step (the weights change every step)
        hip.recorder = rec
        try:
            out, tape = self._run(x, groups, need_grad=need_grad)
        finally:
            hip.recorder = None
        rec.end_forward()
        rec.key = key
        if need_grad:
            tape.recorder = rec                    # the reverse tape is recorded when autograd runs it (run_tape)
            rec.out = out
        else:
            self._finish_recording(None, rec, out)
        return out, tape

    def _finish_recording(self, tape, rec, out=None):
        plans = self.__dict__.setdefault("_launch_plans", {})
        if rec.failed:
            plans[rec.key] = 0 if rec.retry else -(10 ** 9)      # warm up and record again / never try again for this key
            plan.stats["failed_recordings"] = plan.stats.get("failed_recordings", 0) + 1
            return
        plans[rec.key] = plan.Plan(rec, out if out is not None else rec.out)
        plan.stats["recorded"] += 1
        # a plan pins the activations of its call: keep the most recent few (a ragged last batch, a stage switch), drop the oldest
        for mode, cap in ((True, plan.MAX_PLANS_PER_NET), (False, plan.MAX_EVAL_PLANS_PER_NET)):
            live = [k for k, v in plans.items() if isinstance(v, plan.Plan) and k[4] == mode]
            for k in live[:-cap]:
                del plans[k]

    def _run(self, x, groups, need_grad):
        raise NotImplementedError
