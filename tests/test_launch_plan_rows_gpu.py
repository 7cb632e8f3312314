"""Every executor row replayed from a launch plan (adamml_amd/plan.py, csrc/plan.hip), bit for bit against the eager executor.

The rows are those of tests/test_executor_gpu.py (its builders, its shapes: the smallest that reach each branch of the host executor),
both gradient-buffer variants of the partial freezes included.  Each row builds three nets of identical construction -- eager A, eager B,
planned -- and takes five training calls through HipBackbone.run_planned and backbone.run_tape with, per call, an input of other values
at a new address and another output gradient; between calls a plain torch update  p -= lr * p.grad , mark_weights_dirty() (what the fused
optimizers do) and the gradients zeroed in place.  A must equal B (so that a later mismatch is the plan's); the planned net's calls must
be eager, eager, recorded, replayed, replayed, and its output, every gradient, every parameter and every BatchNorm buffer after every call
must be the bits of A.  The gradient rows run with a weight-gradient stream (the configuration AdaMML trains in), so their plans hold the
WAIT records the host-only test (tests/test_launch_plan_cpu.py) cannot make; the scenarios at the end run without one.

No tolerance anywhere: every comparison is equality of bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from adamml_amd import plan  # noqa: E402
from adamml_amd.backbone import run_tape  # noqa: E402
from tests import plan_ref as P  # noqa: E402
from tests.test_executor_gpu import (BUFFERS, Params, all_but, batchnorm_params, depthwise_weights, frames_input, gen, policy_net,  # noqa: E402
                                     resnet, sound_net)

DEV = "cuda"
LR = 1e-3
KINDS = ["eager", "eager", "record", "replay", "replay"]


def bits(t):
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64, 1: torch.int8}[t.element_size()])


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


class Run:
    """one net on the GPU, prepared as tests/test_executor_gpu.py::run_row prepares it, stepped through run_planned / run_tape"""

    def __init__(self, net, groups, frozen=(), frozen_buffers=True, planned=False, side_stream=False, training=True):
        self.net, self.groups, self.planned = net, groups, planned
        net.to(DEV)
        net.train(training)
        if not frozen_buffers:                         # frozen BEFORE the gradient views are attached: their .grad is None, as in a real run
            for m in frozen:
                for p in m.parameters():
                    p.requires_grad_(False)
        if getattr(net, "flat_owner", None) is not None:
            net.flat_owner.ensure(torch.device(DEV, torch.cuda.current_device()))
            net.flat_owner.ensure_grads()
        else:                                          # (the policy trunk's flat buffers belong to the joint net around it)
            for p in net.parameters():
                p.grad = torch.zeros_like(p) if p.requires_grad else None
        self.sentinel = []
        for m in (frozen if frozen_buffers else ()):
            for p in m.parameters():
                p.grad.fill_(0.25)
                self.sentinel.append((p, p.grad))      # the buffer itself: must stay bit for bit what it was
                p.requires_grad_(False)
        self.none = [p for m in (() if frozen_buffers else frozen) for p in m.parameters()]
        net.__dict__.pop("_plist", None)
        if side_stream:
            net.rt.wgrad_stream = torch.cuda.Stream()
        self.tape = None

    def forward(self, x, need_grad=True, eval_plans=False):
        """-> (output, kind); the backward of a gradient call is backward()"""
        before = dict(plan.stats)
        plan.ENABLED, plan.EVAL_ENABLED = self.planned, self.planned and eval_plans
        try:
            with torch.set_grad_enabled(need_grad):
                out, self.tape = self.net.run_planned(x.to(DEV), self.groups, need_grad)
        finally:
            plan.ENABLED = plan.EVAL_ENABLED = False
        self.before = before
        self.kind = "replay" if isinstance(self.tape, plan.PlanTape) else "record" if getattr(self.tape, "recorder", None) is not None or \
            plan.stats["recorded"] > before["recorded"] else "eager"
        return out, self.kind

    def backward(self, g, tape=None):
        run_tape(tape or self.tape, g.to(DEV), self.net)

    def replayed_ops(self):
        return plan.stats["replayed_ops"] - self.before["replayed_ops"]

    def update(self):
        for p in self.net.parameters():
            if p.requires_grad:
                p.data.add_(p.grad, alpha=-LR)
        self.net.mark_weights_dirty()
        for p in self.net.parameters():
            if p.requires_grad:
                p.grad.zero_()

    def perturb(self):
        """other weights without a gradient (the forward-only rows): elementwise, so the same bits on every net"""
        for p in self.net.parameters():
            p.data.add_(p.data.flip(0), alpha=0.05)
        self.net.mark_weights_dirty()

    def check_frozen(self):
        for p, buf in self.sentinel:
            assert p.grad is buf and bool((buf == 0.25).all()), "a frozen parameter's gradient buffer was touched"
        assert all(p.grad is None for p in self.none)


def differences(a, b, grads=True):
    """names of the state tensors (parameters, their gradients, buffers) of two nets that differ in a bit"""
    out = []
    for (name, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        if not same(p.data, q.data):
            out.append(name)
        if grads and p.requires_grad and not same(p.grad, q.grad):
            out.append(name + ".grad")
        assert p.requires_grad == q.requires_grad
    for (name, p), (_, q) in zip(a.named_buffers(), b.named_buffers()):
        if not same(p, q):
            out.append(name)
    return out


def compare(what, out_a, out_b, a, b, grads=True):
    assert same(out_a, out_b), "%s: outputs differ" % what
    diff = differences(a.net, b.net, grads)
    assert not diff, "%s: %d state tensors differ, e.g. %s" % (what, len(diff), diff[:4])


def report(label, pl, recorded):
    fwd, bwd, n = P.counts(pl)
    print("PLANROW %-48s fwd segments %s bwd segments %s CALL %d WAIT %d ZERO %d plans %d" % (label, fwd, bwd, n["CALL"], n["WAIT"], n["ZERO"], recorded))


def five_calls(label, build, make_x, groups, frozen=None, frozen_buffers=True, mode="grad", prime=False):
    """build() -> net; make_x(net, seed) -> the CPU input; frozen(net) -> the frozen set; mode "grad" | "train-nograd" | "eval";
    prime: one train-mode forward first (non-trivial running statistics in front of an eval row)"""
    stats = dict(plan.stats)
    runs = []
    for i in range(3):
        net = build()
        runs.append(Run(net, groups, frozen(net) if frozen else (), frozen_buffers, planned=i == 2, side_stream=mode == "grad", training=True))
    a, b, p = runs
    hold = []                                  # inputs and gradients stay alive: every call sees addresses no earlier call had
    if prime:
        x = make_x(a.net, 50)
        for r in runs:
            plan.ENABLED = False
            with torch.no_grad():
                r.net._run(x.to(DEV), groups, False)
    for r in runs:
        r.net.train(mode != "eval")
    the_plan = previous = None
    for call, kind in enumerate(KINDS):
        x = make_x(a.net, call)
        outs = []
        for r in runs:
            xd = x.to(DEV)
            hold.append(xd)
            out, k = r.forward(xd, need_grad=mode == "grad", eval_plans=mode == "eval")
            if mode == "grad":
                g = torch.randn(tuple(out.shape), generator=gen(100 + call)).to(DEV)
                hold.append(g)
                r.backward(g)
            if r is p:
                assert k == kind, "%s call %d is %s, expected %s" % (label, call + 1, k, kind)
            else:
                assert k == "eager"
            torch.cuda.synchronize()
            outs.append(out.detach().clone())
        assert bool(torch.isfinite(outs[0]).all()), "%s call %d: the eager output is not finite" % (label, call + 1)
        # the calls are told apart by what they compute: another output than the call before, a gradient at the far end of the backward
        assert previous is None or not same(previous, outs[0]), "%s call %d: the output of the call before" % (label, call + 1)
        previous = outs[0]
        if mode == "grad":
            trainable = [q for q in a.net.parameters() if q.requires_grad]
            assert bool(trainable[0].grad.any())
        compare("%s call %d, eager A against eager B" % (label, call + 1), outs[0], outs[1], a, b, mode == "grad")
        compare("%s call %d (%s), planned against eager" % (label, call + 1, kind), outs[0], outs[2], a, p, mode == "grad")
        if kind == "record":
            (the_plan,) = P.plans_of(p.net)
            # the recorded input and output gradient are those of the planned net (the last of `runs`): the newest entries of `hold`
            recorded = (hold[-2], hold[-1]) if mode == "grad" else (hold[-1], None)
        if kind == "replay":
            assert p.tape.plan is the_plan and p.replayed_ops() == sum(s.n for s in P.segments(the_plan))
        for r in runs:
            r.check_frozen()
            r.update() if mode == "grad" else r.perturb()
        torch.cuda.synchronize()
    assert plan.stats.get("failed_recordings", 0) == stats.get("failed_recordings", 0)
    assert plan.stats["recorded"] == stats["recorded"] + 1
    n = P.counts(the_plan)[2]
    assert n["ZERO"] == {"grad": 2, "train-nograd": 1, "eval": 0}[mode]
    assert (n["WAIT"] >= 1) == (mode == "grad"), n        # at least the join of the weight-gradient stream behind the backward
    # what the host-only test asserts of the records, here of records with WAITs and a second stream: nothing baked of the recorded input
    # and gradient, every pointer inside what the plan or the model keeps alive, the memsets those of Arena.reset, an event per wait
    P.check_plan(p.net, the_plan, recorded[0], recorded[1], mode)
    report(label, the_plan, plan.stats["recorded"] - stats["recorded"])
    return runs


# ------------------------------------------------------------------------------------------------------------------- the model rows
def frames(hw, clips, groups):
    def make_x(net, seed):
        return frames_input(groups * clips * net.orig_num_frames, hw, 3, net.input_cpad(hw, hw), seed)
    return make_x


def stem_layer1(n):
    return [n.conv1, n.bn1, n.layer1]


def conv_weights(n):
    return [Params([p for p in n.parameters() if p.dim() == 4])]


# label -> (build, hw, clips, groups, frozen set or None)
RESNET_ROWS = {
    "resnet50-streaming": (lambda: resnet(8), 92, 8, 1, None),
    "resnet50-tile-g3": (lambda: resnet(4), 44, 2, 3, None),
    "resnet50-without-t-stride": (lambda: resnet(4, without_t_stride=True), 44, 2, 1, None),
    "resnet50-avg": (lambda: resnet(12, pooling_method="avg"), 44, 1, 1, None),
    "resnet18-c64-g3": (lambda: resnet(4, depth=18), 44, 2, 3, None),
    "resnet18-tile-7x7-no-t-stride": (lambda: resnet(4, depth=18, without_t_stride=True), 28, 2, 2, None),
    "resnet18-avg": (lambda: resnet(12, depth=18, pooling_method="avg"), 44, 1, 1, None),
    "resnet18-t8-23x23": (lambda: resnet(8, depth=18), 92, 2, 1, None),
    "resnet34-g1": (lambda: resnet(4, depth=34), 44, 2, 1, None),
}
FROZEN_RESNET_ROWS = {
    "resnet50-frozen-stem-layer1": (lambda: resnet(4), 44, 2, 3, stem_layer1),
    "resnet50-frozen-conv-weights": (lambda: resnet(4), 44, 2, 1, conv_weights),
    "resnet18-frozen-stem-layer1": (lambda: resnet(4, depth=18), 44, 2, 3, stem_layer1),
    "resnet18-frozen-batchnorm": (lambda: resnet(4, depth=18), 44, 2, 3, lambda n: [Params(batchnorm_params(n))]),
    "resnet18-frozen-conv-weights": (lambda: resnet(4, depth=18), 44, 2, 3, conv_weights),
}


@pytest.mark.parametrize("label", list(RESNET_ROWS))
def test_resnet_row(label):
    build, hw, clips, groups, _ = RESNET_ROWS[label]
    five_calls(label, build, frames(hw, clips, groups), groups)


@pytest.mark.parametrize("buffers", BUFFERS)
@pytest.mark.parametrize("label", list(FROZEN_RESNET_ROWS))
def test_partly_frozen_resnet_row(label, buffers):
    build, hw, clips, groups, frozen = FROZEN_RESNET_ROWS[label]
    five_calls(label + "-" + buffers, build, frames(hw, clips, groups), groups, frozen=frozen, frozen_buffers=buffers == BUFFERS[0])


def sound_x(net, seed):
    return torch.randn(4, 2, 64, 64, generator=gen(seed))


def policy_x(net, seed):
    return frames_input(2 * 4 * 4, 64, 3, 8, seed)


MOBILENETS = {"sound": (lambda: sound_net()[0], sound_x), "policy": (lambda: policy_net()[0], policy_x)}
# label -> (which net, frozen set or None)
MOBILENET_ROWS = {
    "sound-mobilenetv2-g2": ("sound", None),
    "policy-mobilenetv2-g2": ("policy", None),
}
FROZEN_MOBILENET_ROWS = {
    "policy-mobilenetv2-frozen-depthwise": ("policy", lambda n: [Params(depthwise_weights(n))]),
    "policy-mobilenetv2-depthwise-only": ("policy", lambda n: [Params(all_but(n, depthwise_weights(n)))]),
    "sound-mobilenetv2-frozen-batchnorm": ("sound", lambda n: [Params([p for p in n.parameters() if p.dim() == 1])]),
}


@pytest.mark.parametrize("label", list(MOBILENET_ROWS))
def test_mobilenet_row(label):
    build, make_x = MOBILENETS[MOBILENET_ROWS[label][0]]
    five_calls(label, build, make_x, 2)


@pytest.mark.parametrize("buffers", BUFFERS)
@pytest.mark.parametrize("label", list(FROZEN_MOBILENET_ROWS))
def test_partly_frozen_mobilenet_row(label, buffers):
    which, frozen = FROZEN_MOBILENET_ROWS[label]
    build, make_x = MOBILENETS[which]
    five_calls(label + "-" + buffers, build, make_x, 2, frozen=frozen, frozen_buffers=buffers == BUFFERS[0])


def test_every_model_row_of_the_launch_trace_is_a_row_here():
    here = set(RESNET_ROWS) | set(FROZEN_RESNET_ROWS) | set(MOBILENET_ROWS) | set(FROZEN_MOBILENET_ROWS) | set(FORWARD_ONLY_ROWS)
    assert here == {label for label, _ in P.model_rows()}


# ------------------------------------------------------------------------------------------------------------------- forward-only rows
# label -> (build, make_x, groups, mode)
FORWARD_ONLY_ROWS = {
    "resnet50-train-nograd": (lambda: resnet(4), frames(44, 2, 3), 3, "train-nograd"),
    "resnet50-eval": (lambda: resnet(4), frames(44, 2, 3), 3, "eval"),
    "policy-mobilenetv2-train-nograd": (MOBILENETS["policy"][0], policy_x, 2, "train-nograd"),
    "sound-mobilenetv2-eval": (MOBILENETS["sound"][0], sound_x, 2, "eval"),
    "policy-mobilenetv2-eval": (MOBILENETS["policy"][0], policy_x, 2, "eval"),
    "resnet18-train-nograd": (lambda: resnet(4, depth=18), frames(44, 2, 3), 3, "train-nograd"),
    "resnet18-eval": (lambda: resnet(4, depth=18), frames(44, 2, 3), 3, "eval"),
}


@pytest.mark.parametrize("label", list(FORWARD_ONLY_ROWS))
def test_forward_only_row(label):
    """train mode under no_grad, and eval mode with plan.EVAL_ENABLED: outputs and buffers over five calls, the weights changed in between"""
    build, make_x, groups, mode = FORWARD_ONLY_ROWS[label]
    runs = five_calls(label, build, make_x, groups, mode=mode, prime=mode == "eval")
    tracked = [int(m.num_batches_tracked) for m in runs[2].net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert set(tracked) == ({groups} if mode == "eval" else {5 * groups})


# --------------------------------------------------------------------------------------------------------------------------- scenarios
class Pair:
    """a ResNet-18 (the c64-g3 row) twice: an eager twin and the planned net, no weight-gradient stream"""

    def __init__(self):
        self.stats = dict(plan.stats)
        self.twin, self.run = (Run(resnet(4, depth=18), 3, planned=i == 1) for i in range(2))
        self.hold, self.calls = [], 0

    def both(self, fn):
        fn(self.twin)
        fn(self.run)

    def call(self, kind, clips=2, hw=44, update=True, what=""):
        """one training call of both nets at this shape, compared; -> the planned net's plan where it replayed"""
        self.calls += 1
        x = frames(hw, clips, 3)(self.run.net, self.calls)
        outs = []
        for r in (self.twin, self.run):
            xd = x.to(DEV)
            out, k = r.forward(xd)
            g = torch.randn(tuple(out.shape), generator=gen(100 + self.calls)).to(DEV)
            self.hold += [xd, g]
            r.backward(g)
            torch.cuda.synchronize()
            outs.append(out.detach().clone())
            if r is self.run:
                assert k == kind, "%s call %d is %s, expected %s" % (what, self.calls, k, kind)
                if k == "replay":
                    assert r.replayed_ops() == sum(s.n for s in P.segments(r.tape.plan))
            else:
                assert k == "eager"
        assert bool(torch.isfinite(outs[0]).all())
        compare("%s call %d (%s)" % (what, self.calls, kind), outs[0], outs[1], self.twin, self.run)
        if update:
            self.both(Run.update)
        torch.cuda.synchronize()
        return self.run.tape.plan if kind == "replay" else None

    def failed(self):
        return plan.stats.get("failed_recordings", 0) - self.stats.get("failed_recordings", 0)


def test_alternating_shapes_and_the_eviction_round_trip():
    pair = Pair()
    seen = {}
    for kind in KINDS[:4]:                            # two shapes in turn: a plan each, each replayed with its own records
        for clips in (1, 2):
            seen[clips] = pair.call(kind, clips=clips, what="alternating")
    assert seen[1] is not None and seen[2] is not None and seen[1] is not seen[2]
    for clips in range(3, plan.MAX_PLANS_PER_NET + 2):
        for kind in KINDS[:3]:
            pair.call(kind, clips=clips, what="filling")
    assert len(P.plans_of(pair.run.net)) == plan.MAX_PLANS_PER_NET and seen[1] not in P.plans_of(pair.run.net)
    assert pair.call("replay", clips=2, what="after the eviction") is seen[2]
    for kind in KINDS[:4]:                            # the dropped shape: warm-up, recording, replay
        again = pair.call(kind, clips=1, what="the evicted shape again")
    assert again is not seen[1] and pair.failed() == 0


def test_freeze_flip_and_return():
    pair = Pair()

    def freeze(on):
        pair.both(lambda r: [p.requires_grad_(not on) for p in r.net.layer1.parameters()])
    for kind in KINDS[:4]:
        first = pair.call(kind, what="all trainable")
    freeze(True)
    layer1 = [[p.grad.clone() for p in r.net.layer1.parameters()] for r in (pair.twin, pair.run)]
    for kind in KINDS[:4]:
        second = pair.call(kind, what="layer 1 frozen")
    for r, kept in zip((pair.twin, pair.run), layer1):
        assert all(same(p.grad, k) for p, k in zip(r.net.layer1.parameters(), kept)), "a frozen layer's gradient buffer was written"
    assert second is not first
    freeze(False)
    assert pair.call("replay", what="trainable again") is first
    freeze(True)
    assert pair.call("replay", what="frozen again") is second
    assert pair.failed() == 0 and len(P.plans_of(pair.run.net)) == 2


def test_train_then_eval_then_train():
    pair = Pair()
    for kind in KINDS[:4]:
        first = pair.call(kind, what="train")
    x = frames(44, 2, 3)(pair.run.net, 77)
    outs = []
    for r in (pair.twin, pair.run):
        r.net.eval()
        out, k = r.forward(x, need_grad=False)        # inference is not planned unless plan.EVAL_ENABLED
        assert k == "eager"
        torch.cuda.synchronize()
        outs.append(out.detach().clone())
        r.net.train()
    compare("eval between two training calls", outs[0], outs[1], pair.twin, pair.run)
    assert pair.call("replay", what="train after eval") is first
    assert pair.call("replay", what="train after eval") is first and pair.failed() == 0


def test_two_forward_backward_pairs_before_one_update():
    pair = Pair()
    kinds = iter(KINDS + ["replay"])
    for it in range(3):                               # gradient accumulation: the weight gradients of two calls add up in .grad
        pair.call(next(kinds), update=False, what="accumulation, first half")
        pair.call(next(kinds), update=True, what="accumulation, second half")
    assert pair.failed() == 0 and len(P.plans_of(pair.run.net)) == 1


def test_forced_retry():
    """the statistics arena is (re)allocated inside the call that would record: that recording is given up (once), the key warms up again"""
    pair = Pair()
    pair.call("eager", what="retry")
    pair.call("eager", what="retry")
    pair.run.net.rt.fwd_arena.buf = None
    pair.call("record", what="the recording that fails")
    assert pair.failed() == 1 and not P.plans_of(pair.run.net)
    for kind in KINDS:
        pair.call(kind, what="after the failed recording")
    assert pair.failed() == 1 and plan.stats["recorded"] == pair.stats["recorded"] + 1
