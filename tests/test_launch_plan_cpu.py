"""What a launch plan (adamml_amd/plan.py) replays, checked without a GPU: every model row of tools/launch_trace.py is driven through
HipBackbone.run_planned and its backward on CPU tensors with the launches logged instead of issued (tests/plan_ref.py), five calls with
plans on -- eager, eager, recorded, replayed, replayed -- beside an eager twin of the same construction.  The records adamml_plan_run
is handed on calls 4 and 5 are decoded and must be, entry for entry, the launches the twin issues on the same call: same entry points,
descriptors and scalars, model-owned pointers at the same parameter / gradient / buffer and offset, the call's own input and incoming
gradient through the pointer slots, every other pointer in the same aliasing pattern.  The host logic around the plans (the key, the
retry bookkeeping, the eviction, the busy fallback) has its scenarios below, and eight planted defects show that the per-row check
fails when a plan bakes, drops, reorders or shifts something.

The weight-gradient stream does not exist on the host, so no WAIT record is made here: tests/test_launch_plan_rows_gpu.py covers it."""
import types

import pytest
import torch

import __graft_entry__ as ge
from tests import plan_ref as P

KINDS = ["eager", "eager", "record", "replay", "replay"]
# the op-level rows of launch_trace.ROWS are OpsNet graphs without run_planned (tools/executor_ops.py): nothing of theirs can be planned
LABELS = [label for label, _ in P.model_rows()]
ROWS = dict(P.model_rows())
R18 = "resnet18-c64-g3"


@pytest.fixture(scope="module")
def built():
    ge.build()
    return ge.LIB


def first_difference(a, b):
    for i, (ea, eb) in enumerate(zip(a, b)):
        if ea != eb:
            return "entry %d: %r != %r" % (i, ea, eb)
    return "%d entries != %d entries" % (len(a), len(b))


def tracked(net):
    return [int(m.num_batches_tracked) for m in net.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]


class Pair:
    """a row's model twice, same construction: `twin` runs every call eagerly, `net` with plans on"""

    def __init__(self, h, make):
        self.h = h
        torch.manual_seed(0)
        self.twin, self.x0, self.groups, self.mode, frozen = make()
        P.prepare(self.twin, frozen, self.mode)
        torch.manual_seed(0)
        self.net, _, _, _, frozen = make()
        P.prepare(self.net, frozen, self.mode)
        self.hold = []                  # every input and gradient stays alive: each call sees addresses no earlier call had

    def both(self, fn):
        fn(self.twin)
        fn(self.net)

    def call(self, kind, x_like=None, mode=None):
        """one call of both nets (fresh input, fresh output gradient, the weights marked rewritten as FlatSGD.step does) -> the planned
        net's step, checked: its kind, its launches against the twin's, the slots, num_batches_tracked"""
        h, mode = self.h, mode or self.mode
        x_like = self.x0 if x_like is None else x_like
        xt, xp = torch.zeros_like(x_like), torch.zeros_like(x_like)
        self.hold += [xt, xp]
        self.both(lambda n: n.mark_weights_dirty())
        t = P.step(h, self.twin, xt, self.groups, mode, planned=False)
        p = P.step(h, self.net, xp, self.groups, mode, planned=True)
        self.hold += [t.g, p.g]
        assert t.kind == "eager" and t.launches and not t.replayed
        assert p.kind == kind, "call is %s, expected %s" % (p.kind, kind)
        if p.kind == "replay":
            assert not p.launches, "a replayed call launched %d times from Python" % len(p.launches)
            assert p.replayed == t.launches, "replay differs from the eager twin: " + first_difference(p.replayed, t.launches)
            nf = sum(1 for s in p.plan.rec.fwd if s.n)
            nb = sum(1 for s in (p.plan.rec.bwd or []) if s.n)
            want = [(xp.data_ptr(), 0)] * nf + [(xp.data_ptr(), p.g.data_ptr())] * nb if mode == "grad" else [(xp.data_ptr(), 0)] * nf
            assert p.slots == want, "pointer slots are not this call's input / gradient"
        else:
            assert not p.replayed
            assert p.launches == t.launches, "eager call differs from the eager twin: " + first_difference(p.launches, t.launches)
        if p.kind == "record" and not p.rec.failed:
            # what was recorded is what this very call launched
            pl = P.plans_of(self.net)[-1]
            assert pl.rec is p.rec
            slots = [xp.data_ptr(), p.g.data_ptr() if p.g is not None else 0]
            dec = [e for s in P.segments(pl) for e in P.decode(s, slots)]
            dec = P.normalise(P.calls_only(dec), P.Owners(self.net), xp, p.g)
            assert dec == p.launches, "the records differ from the launches they were made from: " + first_difference(dec, p.launches)
            p.recorded_x, p.recorded_g, p.made = xp, p.g, pl
        assert tracked(self.net) == tracked(self.twin), "num_batches_tracked differs from the eager twin"
        return p


def report(label, pl):
    fwd, bwd, n = P.counts(pl)
    print("PLANROW %-40s fwd segments %s bwd segments %s CALL %d WAIT %d ZERO %d" % (label, fwd, bwd, n["CALL"], n["WAIT"], n["ZERO"]))


def check_row(make, tamper=None, label=None):
    """the per-row check; tamper(namespace of the recording call) is applied to the plan once it is recorded"""
    from adamml_amd import plan
    with P.host() as h:
        plan.EVAL_ENABLED = True
        failed = plan.stats.get("failed_recordings", 0)
        recorded = plan.stats["recorded"]
        pair = Pair(h, make)
        made = None
        for kind in KINDS:
            p = pair.call(kind)
            if kind == "record":
                made = p
                assert p.rec.failed is None, p.rec.failed
                if tamper is not None:
                    tamper(types.SimpleNamespace(plan=p.made, net=pair.net, x=p.recorded_x, g=p.recorded_g))
        assert plan.stats.get("failed_recordings", 0) == failed and plan.stats["recorded"] == recorded + 1
        assert P.plans_of(pair.net) == [made.made]
        P.check_plan(pair.net, made.made, made.recorded_x, made.recorded_g, pair.mode)
        if label:
            report(label, made.made)
    P.patches_undone()


@pytest.mark.parametrize("label", LABELS)
def test_replay_decodes_to_the_eager_launches(built, label):
    check_row(ROWS[label], label=label)


def test_the_rows_left_out_cannot_be_planned(built):
    lt = P.launch_trace()
    left = [(label, make) for label, make in lt.ROWS if label not in ROWS]
    assert [label for label, _ in left] == list(lt._OPS_ROWS) and len(LABELS) == 26
    assert not [label for label, make in left if hasattr(make()[0], "run_planned")]


def test_the_patches_are_undone(built):
    from adamml_amd import plan
    before = (plan.ENABLED, plan.EVAL_ENABLED, dict(plan.stats))
    with pytest.raises(ZeroDivisionError):
        with P.host() as h:
            plan.ENABLED = plan.EVAL_ENABLED = True
            pair = Pair(h, ROWS[R18])
            pair.call("eager")
            1 / 0
    P.patches_undone()
    assert (plan.ENABLED, plan.EVAL_ENABLED, dict(plan.stats)) == before


# ---------------------------------------------------------------------------------------------------- the key and the bookkeeping
def r18_input(net, clips, hw=44, groups=3):
    return P.launch_trace()._frames(net, groups * clips * 4, hw)


def test_a_non_contiguous_input_is_never_planned(built):
    with P.host() as h:
        pair = Pair(h, ROWS[R18])
        x = r18_input(pair.net, 4)[::2]
        assert not x.is_contiguous() and x.shape == pair.x0.shape
        for _ in range(5):
            xt, xp = torch.zeros_like(r18_input(pair.net, 4))[::2], torch.zeros_like(r18_input(pair.net, 4))[::2]
            pair.hold += [xt, xp]
            pair.both(lambda n: n.mark_weights_dirty())
            t = P.step(h, pair.twin, xt, 3, "grad", planned=False)
            p = P.step(h, pair.net, xp, 3, "grad", planned=True)
            assert not xp.is_contiguous() and p.kind == "eager" and p.launches == t.launches and p.launches
        assert not h.recorders and not pair.net.__dict__.get("_launch_plans")


def test_two_alternating_shapes_have_a_plan_each(built):
    from adamml_amd import plan
    with P.host() as h:
        failed = plan.stats.get("failed_recordings", 0)
        pair = Pair(h, ROWS[R18])
        a, b = r18_input(pair.net, 2), r18_input(pair.net, 1, hw=28)
        made = {}
        for kind in KINDS + ["replay"]:
            for name, x in (("a", a), ("b", b)):
                p = pair.call(kind, x)
                if kind == "record":
                    made[name] = p.made
                elif kind == "replay":
                    assert p.plan is made[name]
        assert P.plans_of(pair.net) == [made["a"], made["b"]] and plan.stats.get("failed_recordings", 0) == failed
        assert made["a"] is not made["b"] and min(P.counts(made[k])[2]["CALL"] for k in "ab") > 100
        for name in "ab":
            P.check_plan(pair.net, made[name], None, None, "grad")


def test_the_oldest_plan_is_dropped_and_recorded_again(built):
    from adamml_amd import plan
    with P.host() as h:
        failed = plan.stats.get("failed_recordings", 0)
        pair = Pair(h, ROWS[R18])
        shapes = [r18_input(pair.net, c) for c in range(1, plan.MAX_PLANS_PER_NET + 2)]
        made = []
        for x in shapes:
            for kind in KINDS[:3]:
                p = pair.call(kind, x)
            made.append(p.made)
        assert P.plans_of(pair.net) == made[1:]                          # the first shape's plan went when the fifth was recorded
        for x, pl in list(zip(shapes, made))[1:]:
            assert pair.call("replay", x).plan is pl
        for kind in KINDS[:4]:                                           # the dropped shape starts over: warm-up, recording, replay
            p = pair.call(kind, shapes[0])
        assert p.plan is not made[0] and P.plans_of(pair.net) == made[2:] + [p.plan]
        assert pair.call("eager", shapes[1]).kind == "eager"             # ... and that recording dropped the second shape's
        assert plan.stats.get("failed_recordings", 0) == failed


def test_a_freeze_flip_is_a_new_key_and_the_way_back_finds_the_first_plan(built):
    with P.host() as h:
        pair = Pair(h, ROWS[R18])

        def freeze(on):
            pair.both(lambda n: [p.requires_grad_(not on) for p in n.layer1.parameters()])
        for kind in KINDS[:4]:
            first = pair.call(kind)
        freeze(True)
        for kind in KINDS[:4]:
            second = pair.call(kind)
        assert second.plan is not first.plan and len(second.replayed) < len(first.replayed)        # no weight gradient of layer 1
        assert not [e for e in second.replayed for a in e[1] if isinstance(a, tuple) and a[:1] == ("grad",) and a[1].startswith("layer1.")]
        freeze(False)
        assert pair.call("replay").plan is first.plan
        freeze(True)
        assert pair.call("replay").plan is second.plan
        assert P.plans_of(pair.net) == [first.plan, second.plan]


def test_an_arena_sized_inside_the_recording_fails_it_once_and_retries(built):
    from adamml_amd import plan
    with P.host() as h:
        failed = plan.stats.get("failed_recordings", 0)
        pair = Pair(h, ROWS[R18])
        pair.call("eager")
        pair.call("eager")
        pair.net.rt.fwd_arena.buf = None
        p = pair.call("record")
        assert p.rec.failed and p.rec.retry and plan.stats["failed_recordings"] == failed + 1
        assert not P.plans_of(pair.net) and list(pair.net._launch_plans.values()) == [0]
        for kind in KINDS:
            p = pair.call(kind)
        assert plan.stats["failed_recordings"] == failed + 1 and len(h.recorders) == 2
        P.check_plan(pair.net, p.plan, None, None, "grad")


def test_a_second_forward_before_the_first_backward_runs_eagerly(built):
    from adamml_amd import plan
    with P.host() as h:
        pair = Pair(h, ROWS[R18])
        for kind in KINDS[:4]:
            pair.call(kind)
        busy = plan.stats.get("busy_fallbacks", 0)
        net = pair.net
        x1, x2 = torch.zeros_like(pair.x0), torch.zeros_like(pair.x0)
        net.mark_weights_dirty()
        a = P.step(h, net, x1, 3, "grad", planned=True, backward=False)
        assert a.kind == "replay" and plan.stats.get("busy_fallbacks", 0) == busy
        b = P.step(h, net, x2, 3, "grad", planned=True, backward=False)
        assert b.kind == "eager" and plan.stats["busy_fallbacks"] == busy + 1 and b.launches and not b.replayed
        b.backward()
        a.backward()
        assert not a.plan.busy()
        for _ in range(2):                                               # (the twin takes the same two steps)
            P.step(h, pair.twin, torch.zeros_like(pair.x0), 3, "grad", planned=False)
        assert pair.call("replay").plan is a.plan


# ------------------------------------------------------------------------------------------------------------------ planted defects
def _records(t, phase=None):
    """[(segment, index, record)] of the plan's CALL records"""
    from adamml_amd import plan
    segs = P.segments(t.plan) if phase is None else (t.plan.rec.fwd if phase == "fwd" else t.plan.rec.bwd)
    return [(s, i, op) for s in segs for i, op in enumerate(P.ops_of(s)) if op.kind == plan.KIND_CALL]


def _rebuild(seg, ops):
    from adamml_amd import plan
    seg.ops = (plan.PlanOp * max(len(ops), 1))(*ops)
    seg.n = len(ops)


def _bake_slot(t, slot, addr):
    for s, i, op in _records(t):
        for j in range(op.nargs):
            if (op.slot_mask >> j) & 1 and op.a[j] == slot:
                s.ops[i].slot_mask &= ~(1 << j)
                s.ops[i].a[j] = addr
                return
    raise RuntimeError("no record uses slot %d" % slot)


def bake_input(t):
    _bake_slot(t, 0, t.x.data_ptr())


def bake_gradient(t):
    _bake_slot(t, 1, t.g.data_ptr())


def shift_integer(t):
    from adamml_amd import hip
    names = sorted(hip.SIGNATURES)
    recs = _records(t, "fwd")
    for s, i, op in recs[len(recs) // 2:]:
        for j, k in enumerate(hip.SIGNATURES[names[op.fn]][:-1]):
            if k is hip._I:
                s.ops[i].a[j] += 1
                return
    raise RuntimeError("no integer argument")


def drop_record(t):
    s = t.plan.rec.bwd[0]
    ops = P.ops_of(s)
    _rebuild(s, ops[:len(ops) // 2] + ops[len(ops) // 2 + 1:])


def swap_records(t):
    s = t.plan.rec.fwd[0]
    ops = P.ops_of(s)
    i = next(i for i in range(len(ops) // 2, len(ops) - 1) if ops[i].fn != ops[i + 1].fn)
    _rebuild(s, ops[:i] + [ops[i + 1], ops[i]] + ops[i + 2:])


def drop_zero(t):
    from adamml_amd import plan
    for s in P.segments(t.plan):
        _rebuild(s, [op for op in P.ops_of(s) if op.kind != plan.KIND_ZERO])


def drop_post_forward_hooks(t):
    assert t.plan.rec.post_fwd
    del t.plan.rec.post_fwd[:]


def move_gradient_pointer(t):
    own = P.Owners(t.net)
    for s in t.plan.rec.bwd:
        for i, j, v, slot in P.pointer_args(s):
            o = None if slot or not v else own.find(v)
            if o is not None and o[0] == "grad":
                s.ops[i].a[j] = v + 4
                return
    raise RuntimeError("no gradient pointer")


DEFECTS = [
    (bake_input, "replay differs|pointer slots"),
    (bake_gradient, "replay differs|pointer slots"),
    (shift_integer, "replay differs from the eager twin"),
    (drop_record, "replay differs from the eager twin"),
    (swap_records, "replay differs from the eager twin"),
    (drop_zero, "the arena memset is"),
    (drop_post_forward_hooks, "num_batches_tracked differs"),
    (move_gradient_pointer, "replay differs from the eager twin"),
]


@pytest.mark.parametrize("defect,caught_by", DEFECTS, ids=[d.__name__ for d, _ in DEFECTS])
def test_a_planted_defect_fails_the_row_check(built, defect, caught_by):
    with pytest.raises(AssertionError, match=caught_by):
        check_row(ROWS[R18], tamper=defect)
    P.patches_undone()


@pytest.mark.parametrize("defect", [bake_input, bake_gradient], ids=["bake_input", "bake_gradient"])
def test_a_baked_address_is_seen_in_the_records_alone(built, defect):
    """... without the comparison of the launches: the static check of the plan finds the recorded input's (gradient's) address"""
    with P.host() as h:
        pair = Pair(h, ROWS[R18])
        for kind in KINDS[:3]:
            p = pair.call(kind)
        P.check_plan(pair.net, p.made, p.recorded_x, p.recorded_g, "grad")
        defect(types.SimpleNamespace(plan=p.made, net=pair.net, x=p.recorded_x, g=p.recorded_g))
        with pytest.raises(AssertionError, match="holds the address of the recorded input / gradient"):
            P.check_plan(pair.net, p.made, p.recorded_x, p.recorded_g, "grad")
