"""Helpers of the launch-plan tests (tests/test_launch_plan_cpu.py, tests/test_launch_plan_rows_gpu.py): a decoder of the records
adamml_plan_run replays (include/adamml_hip.h: adamml_plan_op_t) and a host-only harness that drives HipBackbone.run_planned and the
backward of backbone.run_tape on CPU tensors with nothing launched.

The harness follows tools/launch_trace.py: `call`, `ptr` and hip._stream are replaced in every loaded adamml_amd module, so the executor
logs its launches instead of issuing them (the host logic never reads a tensor value).  On top of that every logged launch is forwarded to
the plan.Recorder that listens (as hip.call does), `ptr` hands the recorder the tensor (as hip.ptr does), and hip.load() answers with a
proxy of the built library whose adamml_plan_run DECODES the records it is given instead of running them.  A replayed call then yields
the launch list the C replay would issue, in the form of the eager log, and the two can be compared entry by entry.

Pointers are compared after normalisation: one inside a tensor the model owns (parameter, its .grad, buffer) becomes (kind, name, byte
offset) and has to match by identity, the call's input and incoming gradient become ("input" | "grad_out", offset), every other pointer
the ordinal of its first appearance within the call."""
import bisect
import contextlib
import importlib.util
import os
import struct
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK64 = 0xFFFFFFFFFFFFFFFF
ZERO, WAIT = "<zero>", "<wait>"          # the entries decode() makes of KIND_ZERO / KIND_WAIT records (no entry point has such a name)


def launch_trace():
    """tools/launch_trace.py as the module `launch_trace` (its ROWS are the rows of the plan tests too)"""
    mod = sys.modules.get("launch_trace")
    if mod is None:
        spec = importlib.util.spec_from_file_location("launch_trace", os.path.join(ROOT, "tools", "launch_trace.py"))
        mod = sys.modules["launch_trace"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    return mod


def model_rows():
    """[(label, make)] of launch_trace.ROWS that are models (HipBackbone: they have run_planned); the op-level graphs are not"""
    return [(label, make) for label, make in launch_trace().ROWS if not label.startswith("ops-")]


class Ptr(int):
    """a device address among the arguments of a launch (eager log and decoded record alike)"""

    def __repr__(self):
        return "Ptr(0x%x)" % int(self)


# ------------------------------------------------------------------------------------------------------------------------ decoder
def _names():
    from adamml_amd import hip
    return sorted(hip.SIGNATURES)            # plan.fn_id numbers the entry points in this order


def ops_of(segment):
    """the records of a plan.Segment (or of an (array, n) pair), as the ctypes structures themselves"""
    ops, n = (segment.ops, segment.n) if hasattr(segment, "ops") else segment
    return [ops[i] for i in range(n)]


def decode(segment, slots):
    """-> [(entry point, args)]: what adamml_plan_run issues for these records when the caller's pointer slots are `slots`.
    A ConvDesc is its sixteen fields, a pointer a Ptr (None when null; slots[a[j]] where its slot_mask bit is set), a float / double the
    value of its double bits, everything else the integer modulo 2^64.  (ZERO, (Ptr, bytes)) and (WAIT, (waiting stream slot, stream slot
    waited for, event)) stand for the records that are no launch."""
    from adamml_amd import hip, plan
    names, out = _names(), []
    for op in ops_of(segment):
        if op.kind == plan.KIND_ZERO:
            out.append((ZERO, (Ptr(op.a[0]), int(op.a[1]))))
        elif op.kind == plan.KIND_WAIT:
            out.append((WAIT, (int(op.stream), int(op.a[0]), int(op.a[1]))))
        else:
            assert op.kind == plan.KIND_CALL and 0 <= op.fn < len(names), (op.kind, op.fn)
            name = names[op.fn]
            kinds = hip.SIGNATURES[name][:-1]
            assert op.nargs == len(kinds), (name, op.nargs)
            args = []
            for j, k in enumerate(kinds):
                v = int(op.a[j])
                if (op.slot_mask >> j) & 1:
                    assert k is hip._P and v < len(slots), (name, j, v)
                    args.append(Ptr(slots[v]))
                elif k is hip._DESC:
                    d = hip.ConvDesc.from_address(v)
                    args.append(tuple(getattr(d, f[0]) for f in d._fields_))
                elif k is hip._P:
                    args.append(Ptr(v) if v else None)
                elif k in (hip._F, hip._D):
                    args.append(struct.unpack("<d", struct.pack("<Q", v))[0])
                else:
                    args.append(v)
            out.append((name, tuple(args)))
    return out


def canonical(name, args):
    """an eager launch in the form decode() gives"""
    from adamml_amd import hip
    kinds = hip.SIGNATURES[name][:-1]
    assert len(kinds) == len(args), (name, len(args))
    out = []
    for v, k in zip(args, kinds):
        if k is hip._DESC:
            d = v._obj
            out.append(tuple(getattr(d, f[0]) for f in d._fields_))
        elif k is hip._P:
            assert v is None or isinstance(v, Ptr), (name, v)          # every pointer of the executor goes through ptr()
            out.append(v if v else None)
        elif k in (hip._F, hip._D):
            out.append(float(v))
        else:
            out.append(int(v) & MASK64)
    return name, tuple(out)


def pointer_args(segment):
    """-> [(record index, argument index, value, True where the value is a slot index)] of every pointer argument of the CALL records,
    and of the target of every ZERO record (argument index 0)"""
    from adamml_amd import hip, plan
    names, out = _names(), []
    for i, op in enumerate(ops_of(segment)):
        if op.kind == plan.KIND_ZERO:
            out.append((i, 0, int(op.a[0]), False))
        elif op.kind == plan.KIND_CALL:
            for j, k in enumerate(hip.SIGNATURES[names[op.fn]][:-1]):
                if k is hip._P:
                    out.append((i, j, int(op.a[j]), bool((op.slot_mask >> j) & 1)))
    return out


def segments(p):
    """every Segment of a plan.Plan, forward first"""
    return list(p.rec.fwd) + list(p.rec.bwd or [])


def counts(p):
    """-> (records per forward segment, per backward segment, {CALL, WAIT, ZERO: n})"""
    from adamml_amd import plan
    n = {plan.KIND_CALL: 0, plan.KIND_WAIT: 0, plan.KIND_ZERO: 0}
    for s in segments(p):
        for op in ops_of(s):
            n[op.kind] += 1
    return [s.n for s in p.rec.fwd], [s.n for s in (p.rec.bwd or [])], {"CALL": n[plan.KIND_CALL], "WAIT": n[plan.KIND_WAIT], "ZERO": n[plan.KIND_ZERO]}


# ------------------------------------------------------------------------------------------------------------------ normalisation
def extent(t):
    """[lo, hi) of the bytes a tensor's storage occupies: what stays allocated while the tensor is alive"""
    s = t.untyped_storage()
    return s.data_ptr(), s.data_ptr() + s.nbytes()


class Owners:
    """the address ranges of the tensors a model owns, by name"""

    def __init__(self, net):
        iv = []
        for name, p in net.named_parameters():
            iv.append((p, "param", name))
            if p.grad is not None:
                iv.append((p.grad, "grad", name))
        for name, b in net.named_buffers():
            iv.append((b, "buf", name))
        rows = sorted((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), kind, name) for t, kind, name in iv if t.numel())
        assert all(a[1] <= b[0] for a, b in zip(rows, rows[1:])), "two model-owned tensors overlap"
        self.rows, self.los = rows, [r[0] for r in rows]

    def find(self, addr):
        i = bisect.bisect_right(self.los, addr) - 1
        if i >= 0 and addr < self.rows[i][1]:
            return self.rows[i][2], self.rows[i][3], addr - self.rows[i][0]
        return None


def normalise(entries, owners, x=None, g=None):
    """the launches with every Ptr replaced: (kind, name, offset) inside a model-owned tensor, ("input" | "grad_out", offset) inside the
    call's input / incoming gradient, else ("p", ordinal of first appearance among these entries)"""
    ids = {}
    special = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), what) for t, what in ((x, "input"), (g, "grad_out")) if t is not None]

    def n(a):
        if not isinstance(a, Ptr):
            return a
        o = owners.find(a)
        if o is not None:
            return o
        for lo, hi, what in special:
            if lo <= a < hi:
                return what, a - lo
        return "p", ids.setdefault(int(a), len(ids))
    return [(name, tuple(n(a) for a in args)) for name, args in entries]


def calls_only(entries):
    return [e for e in entries if e[0] not in (ZERO, WAIT)]


# ------------------------------------------------------------------------------------------- the static checks of a recorded plan
def inside(addr, ranges):
    return any(lo <= addr < hi for lo, hi in ranges)


def check_plan(net, pl, x_rec, g_rec, mode):
    """the static checks of a recorded plan"""
    from adamml_amd import plan
    rt = net.rt
    own = [extent(t) for t in list(net.parameters()) + [p.grad for p in net.parameters() if p.grad is not None] + list(net.buffers())]
    kept = [extent(t) for t in pl.rec.keep if isinstance(t, torch.Tensor)]
    baked = [extent(t) for t in (x_rec, g_rec) if t is not None]
    for phase, segs in (("forward", pl.rec.fwd), ("backward", pl.rec.bwd or [])):
        for s in segs:
            for i, j, v, slot in pointer_args(s):
                if slot:
                    assert v in (0, 1) and (v == 0 or phase == "backward"), "%s record %d: slot %d" % (phase, i, v)
                elif v:
                    assert not inside(v, baked), "%s record %d argument %d holds the address of the recorded input / gradient" % (phase, i, j)
                    assert inside(v, kept) or inside(v, own), "%s record %d argument %d points into nothing the plan keeps alive" % (phase, i, j)
    # the statistic accumulators are zeroed by the plan exactly where the eager call zeroes them (Arena.reset): one memset of the whole
    # arena in front of a train-mode forward, one in front of the backward
    for phase, segs, arena, on in (("forward", pl.rec.fwd, rt.fwd_arena, mode != "eval"), ("backward", pl.rec.bwd or [], rt.bwd_arena, mode == "grad")):
        ops = [op for s in segs for op in ops_of(s)]
        zeros = [(i, int(op.a[0]), int(op.a[1])) for i, op in enumerate(ops) if op.kind == plan.KIND_ZERO]
        arenas = [(a.buf.data_ptr(), a.buf.data_ptr() + a.buf.numel() * 8) for a in (rt.fwd_arena, rt.bwd_arena) if a.buf is not None]
        for i, lo, n in zeros:
            assert any(a <= lo and lo + n <= b for a, b in arenas), "%s record %d zeroes memory outside the statistics arenas" % (phase, i)
        if on:
            want = [(0, arena.buf.data_ptr(), max(arena.high, 1) * 8)]
            assert zeros == want, "%s: the arena memset is %s, the eager call's is %s" % (phase, zeros, want)
        else:
            assert not zeros, "%s: a memset the eager call does not issue" % phase
    # every wait names two different streams of the plan and an event of its own (adamml_plan_run records the event, then waits for it)
    waits = [(int(op.stream), int(op.a[0]), int(op.a[1])) for s in segments(pl) for op in ops_of(s) if op.kind == plan.KIND_WAIT]
    assert [w[2] for w in waits] == list(range(pl.n_events)) and all(w[0] != w[1] and max(w[:2]) < pl.n_streams for w in waits), waits
    assert all(0 <= op.stream < pl.n_streams for s in segments(pl) for op in ops_of(s))


# ------------------------------------------------------------------------------------------------------------------ host harness
class Host:
    """what the patches collect: .log the eager launches (canonical form), .replays [(records decoded with the slots given, slots)] per
    adamml_plan_run call, .recorders every plan.Recorder made, .keep the tensors whose addresses were handed out (no address is reused
    while a call's launches are compared)"""

    def __init__(self):
        self.log, self.replays, self.recorders, self.keep = [], [], [], []


@contextlib.contextmanager
def host():
    """The executor and the launch plans run on the host alone inside this context (see the module text); plan.ENABLED and
    plan.EVAL_ENABLED are the caller's to set and are put back, like everything else, on exit."""
    import adamml_amd.resnet, adamml_amd.sound_mobilenet_v2, adamml_amd.policy_net  # noqa: F401,E401  (loaded before `call` is replaced)
    from adamml_amd import hip, plan
    h = Host()
    lib = hip.load()

    def ptr(t):
        if t is None:
            return None
        h.keep.append(t)
        if hip.recorder is not None:
            hip.recorder.keep.append(t)          # (hip.ptr: the plan owns every tensor whose address one of its records holds)
        return Ptr(t.data_ptr())

    def call(name, *args):
        h.log.append(canonical(name, args))
        hip.next_meta = (0.0, 0.0)
        if hip.recorder is not None:
            hip.recorder.call(name, args, 0)     # (hip.call: after the launch, with the stream it went to)

    class Library:
        """the built library, except that adamml_plan_run decodes"""

        def __getattr__(self, name):
            return getattr(lib, name)

        def adamml_plan_run(self, ops, n, streams, n_streams, events, n_events, slot_arr, n_slots):
            slots = [int(slot_arr[i]) for i in range(n_slots)]
            h.replays.append((decode((ops, n), slots), tuple(slots)))
            return 0

    class Recorder(plan.Recorder):
        def __init__(self, x):
            super().__init__(x)
            self.x = x
            h.recorders.append(self)

    mods = [m for n, m in list(sys.modules.items()) if m is not None and (n == "adamml_amd" or n.startswith("adamml_amd."))]
    saved = [(m, n, getattr(m, n)) for m in mods for n, real in (("call", hip.call), ("ptr", hip.ptr)) if getattr(m, n, None) is real]
    n_fns = len(saved)
    saved += [(hip, "_stream", hip._stream), (hip, "_wgrad_ws", hip._wgrad_ws), (hip, "load", hip.load), (hip, "recorder", hip.recorder),
              (hip, "next_meta", hip.next_meta), (plan, "Recorder", plan.Recorder), (plan, "ENABLED", plan.ENABLED),
              (plan, "EVAL_ENABLED", plan.EVAL_ENABLED), (plan, "MAX_PLANS_PER_NET", plan.MAX_PLANS_PER_NET)]
    stats = dict(plan.stats)
    try:
        for m, n, _ in saved[:n_fns]:
            setattr(m, n, call if n == "call" else ptr)
        hip._stream = lambda: 0
        hip._wgrad_ws = {}                       # (a scratch buffer grown by an earlier run would change the workspace sizes passed)
        library = Library()
        hip.load = lambda: library
        hip.recorder = None
        plan.Recorder = Recorder
        yield h
    finally:
        for m, n, v in saved:
            setattr(m, n, v)
        plan.stats.clear()
        plan.stats.update(stats)


def patches_undone():
    """what tests/test_launch_trace_cpu.py::test_the_patches_are_undone asserts, and the same for what host() adds"""
    from adamml_amd import backbone, hip, plan, runtime
    assert runtime.call is hip.call and runtime.ptr is hip.ptr and hip.call.__module__ == "adamml_amd.hip" and hip.ptr.__module__ == "adamml_amd.hip"
    assert hip.load.__module__ == "adamml_amd.hip" and hip._stream.__module__ == "adamml_amd.hip" and hip.recorder is None
    assert plan.Recorder.__module__ == "adamml_amd.plan" and backbone.plan is plan
    assert runtime._on_wgrad_stream.__enter__.__qualname__ == "_on_wgrad_stream.__enter__"


def prepare(net, frozen, mode):
    """a row's model as tools/launch_trace.py prepares it: the frozen set, zeroed gradient tensors for what trains, the mode"""
    for p in frozen:
        p.requires_grad_(False)
    net.train(mode != "eval")
    net.__dict__.pop("_plist", None)
    if mode == "grad":
        for p in net.parameters():
            p.grad = torch.zeros_like(p) if p.requires_grad else None


def plans_of(net):
    from adamml_amd import plan
    return [v for v in net.__dict__.get("_launch_plans", {}).values() if isinstance(v, plan.Plan)]


def step(h, net, x, groups, mode, planned, g=None, backward=True):
    """One call of `net` through run_planned and (mode "grad") its backward, as ops.backbone_call and backbone.run_tape drive them minus
    the torch.cuda stream joins (there is no weight-gradient stream on the host, so no WAIT record either).
    -> namespace: kind ("eager" | "record" | "replay"), out, tape, g, launches (the eager launches of this call, normalised), replayed (the
    CALL entries the replay decodes to, normalised), decoded (every decoded entry, raw), slots [(slot 0, slot 1) per adamml_plan_run call],
    rec (the Recorder this call made, or None), plan (the Plan replayed, or None), backward() where it was deferred"""
    from adamml_amd import hip, plan
    r = types.SimpleNamespace(rec=None, plan=None, g=g)
    del h.log[:], h.replays[:], h.keep[:]
    n_rec = len(h.recorders)
    need_grad = mode == "grad"
    # a scratch buffer of its own per net, as in a process of its own: the twin's calls do not grow the workspace the planned net is handed
    hip._wgrad_ws = net.__dict__.setdefault("_host_scratch", {})
    saved = plan.ENABLED
    plan.ENABLED = planned
    try:
        with torch.set_grad_enabled(need_grad):
            r.out, r.tape = net.run_planned(x, groups, need_grad)
    finally:
        plan.ENABLED = saved

    def run_backward():
        tape = r.tape
        if r.g is None:
            r.g = torch.zeros(tuple(r.out.shape))
        if isinstance(tape, plan.PlanTape):
            tape.grad_out = r.g
            tape.backward()
            return
        rec = getattr(tape, "recorder", None)
        gg = r.g
        if rec is not None:
            gg = gg.contiguous()
            rec.begin_backward(gg)
            hip.recorder = rec
        try:
            net.rt.bwd_arena.reset(gg.device)
            tape.grad_out = gg.contiguous()
            tape.backward()
        finally:
            if rec is not None:
                hip.recorder = None
        if rec is not None:
            rec.end_backward()
            net._finish_recording(tape, rec)

    def finish():
        if len(h.recorders) > n_rec:
            r.rec = h.recorders[-1]
        r.kind = "replay" if isinstance(r.tape, plan.PlanTape) else "record" if r.rec is not None else "eager"
        if r.kind == "replay":
            r.plan = r.tape.plan
        owners = Owners(net)
        r.launches = normalise(list(h.log), owners, x, r.g)
        r.decoded = [e for d, _ in h.replays for e in d]
        r.replayed = normalise(calls_only(r.decoded), owners, x, r.g)
        r.slots = [s for _, s in h.replays]
        return r

    if need_grad and backward:
        run_backward()
    elif need_grad:
        r.backward = lambda: (run_backward(), finish())[1]
    return finish()
