"""Each HIP stream of a step held back in turn: the step must stay bit-identical (tests/stream_delay.py has the helper and the why).

A row is one model and one stage.  It runs, on fresh inputs every step (seed 100 + k):
  1. the reference: the steps with `model.use_side_stream = False` -- every launch on ONE stream (asserted), so FIFO order makes it
     race-free by construction; it also leaves `rt.wgrad_stream` None;
  2. the default multi-stream configuration undelayed, which must equal the reference bit for bit (stream choice must not change
     kernel choice), whose warm-up step names the streams in play (discovery) and whose measured steps give the step time (the
     shortest of them; SD.step_time says why not the warm-up step's);
  3. one fresh model per discovered stream, that stream held for 2x the step time (250 ms at most) in front of the forward and again
     in front of `backward()` of both measured steps, which must equal the reference: logits, decisions, policy logits, every gradient,
     every parameter after one fused SGD step, every BatchNorm buffer.  The second measured step reuses the arenas, the per-stream
     scratch, `wgrad_pending` and `_live_inputs` of the first.
Nothing is read back between issuing a forward and the end of its step; a hold measured below 1.5x the step time fails the row as
"hold too short"; every discovered stream is held in a run of its own, the caller's included.  One control at the end shows that the
harness can fail: with the caller's wait for the held sound stream skipped, the logits differ.

Hardware queues.  A process has 4 hardware queues by default (GPU_MAX_HW_QUEUES; the tests leave it alone), so with more than four
streams some share a queue and a held stream also holds its queue-mates.  That can only HIDE a race in that pairing (the mate is late as
well); it can never produce a difference that is not a race.  The stream count of every row is printed.

The module prints the table that profiles/stream_order_rows.md keeps: row, stage, held stream, measured hold, step time, differing tensors."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from adamml_amd import synth  # noqa: E402
from adamml_amd.optim import FlatSGD  # noqa: E402
from adamml_amd.prefetch import Prefetcher  # noqa: E402
from tests import stream_delay as SD  # noqa: E402
from tests.golden_cases import CASES, CH  # noqa: E402
from tests.test_prefetch_gpu import rgb_sound, _objects  # noqa: E402,F401  (the dataset fixture of the Prefetcher tests)

DEV = "cuda"
_cache = {}


# ---- models and inputs (built once per module where they do not change) -------------------------------------------------------------------
def _adamml50(modality, S):
    from adamml_amd import adamml
    return adamml(groups=8, modality=modality, input_channels=[CH[m] for m in modality], num_segments=S, rng_policy=False,
                  rng_threshold=0.5, causality_modeling="lstm", num_classes=31, depth=50, without_t_stride=False, dropout=0.0,
                  pooling_method="max", fusion_point="logits", unimodality_pretrained=[], learnable_lf_weights=True)


def _adamml18():
    from tests.test_resnet_basic_gpu import build_adamml18
    return build_adamml18(dropout=0.0)[0]


FOUR = CASES["adamml_4mod"]
ARCH = {
    # name: (constructor, modality, B, S, size, sound size)
    "rgb_sound": (lambda: _adamml50(["rgb", "sound"], 2), ["rgb", "sound"], 2, 2, 64, 64),
    "four_mod": (lambda: _adamml50(FOUR["modality"], FOUR["S"]), FOUR["modality"], FOUR["B"], FOUR["S"], FOUR["size"], FOUR["sound_size"]),
    "basic18": (_adamml18, ["rgb", "sound"], 2, 2, 64, 64),
}


def _fresh(arch):
    """A fresh model of `arch` on the device, from the same synthetic state_dict every time."""
    model = ARCH[arch][0]()
    if ("sd", arch) not in _cache:
        _cache[("sd", arch)] = synth.synth_state_dict(model.state_dict(), seed=1234)
    model.load_state_dict(_cache[("sd", arch)])
    return model.to(DEV)


def _batches(arch, steps):
    key = ("batches", arch)
    if key not in _cache or len(_cache[key]) < steps:
        _, modality, B, S, size, sound = ARCH[arch]
        _cache[key] = SD.step_batches(modality, B, S, 8, size, sound, steps, DEV)
        torch.cuda.synchronize()
    return _cache[key][:steps]


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\n" + SD.report_table())


# ---- one row ---------------------------------------------------------------------------------------------------------------------------
def _single_stream(model):
    model.use_side_stream = False
    return model


def drive(row, stage, arch, min_streams, steps=3, first_held=1, wrap=None, extra=(), setup=None):
    """Reference, undelayed run, one held run per discovered stream (the module's text).  wrap(model) -> keyword arguments of SD.run for a
    multi-stream run (a data-parallel wrapper's forward and gradient reduction); extra / setup: SD.run's `extra`, and a context manager
    factory the multi-stream runs are issued under (launch plans enabled).  Returns the undelayed run."""
    import contextlib
    batches = _batches(arch, steps)
    wrap = wrap or (lambda model: {})
    setup = setup or contextlib.nullcontext
    measured = range(first_held, steps)
    ref = SD.run(_single_stream(_fresh(arch)), stage, batches, first_held=first_held)
    assert len(ref.found) == 1, "the single-stream reference launched on %d streams: %s" % (len(ref.found), ref.found.role_list())
    assert all(torch.isfinite(s["logits"]).all() for s in ref.steps)
    assert SD.compare(ref.steps[first_held], ref.steps[first_held + 1]), "two steps on different inputs gave the same bits"
    with setup():
        model = _fresh(arch)
        base = SD.run(model, stage, batches, first_held=first_held, **{"extra": extra, **wrap(model)})
    for k in measured:
        SD.assert_same(ref.steps[k], base.steps[k], "%s [%s] undelayed" % (row, stage), k)
    n = len(base.found)
    step_ms = SD.step_time(base.step_ms[first_held:])
    print("%s [%s]: %d streams %s; undelayed step %s ms in the warm-up, %s ms measured; holds of %.1f ms"
          % (row, stage, n, base.found.role_list(), ", ".join("%.1f" % t for t in base.step_ms[:first_held]),
             ", ".join("%.1f" % t for t in base.step_ms[first_held:]), SD.hold_ms_for(step_ms)))
    SD.report_line(row, stage, "nobody (undelayed)", "-", step_ms, 0)
    assert n >= min_streams, "%s [%s]: %d streams discovered (%s), at least %d expected" % (row, stage, n, base.found.role_list(), min_streams)
    held_roles = []
    for i in range(n):
        with setup():
            model = _fresh(arch)
            r = SD.run(model, stage, batches, pick=lambda found: found.entry(i), step_ms=step_ms, first_held=first_held,
                       **{"extra": extra, **wrap(model)})
        assert r.found.role_list() == base.found.role_list(), (r.found.role_list(), base.found.role_list())
        role = "%d: %s" % (i, r.held[1])
        diff = []
        for k in measured:
            diff += SD.compare(ref.steps[k], r.steps[k])
        hold_ms = min(h.measured_ms() for h in r.holds)
        SD.report_line(row, stage, role, hold_ms, step_ms, len(diff))
        assert len(r.holds) == len(SD.schedule(stage)) * len(measured)
        for h in r.holds:
            SD.check_hold(h.measured_ms(), step_ms, "%s [%s] stream %s, in front of the %s," % (row, stage, role, h.point))
        for k in measured:
            SD.assert_same(ref.steps[k], r.steps[k], "%s [%s]" % (row, stage), k, role)
        assert r.held[0] == r.found.handles()[i]
        held_roles.append(i)
    assert held_roles == list(range(n))                                # every discovered stream was held, in a run of its own
    return base


# Streams a stage reaches at the least.  train_main: the caller's (ResNet), the sound side stream, the policy stream and one weight-gradient
# stream per main net (use_wgrad_stream "all").  With the main net frozen (train_policy) or no backward at all, no weight gradient is
# launched: the caller's, the sound and the policy stream are left.  The skipping forward runs on the caller's stream alone.
@pytest.mark.parametrize("row,stage,arch,min_streams", [
    ("rgb_sound", "train_main", "rgb_sound", 4),
    ("rgb_sound", "train_policy", "rgb_sound", 3),
    ("four_mod", "train_main", "four_mod", 6),
    ("four_mod", "train_policy", "four_mod", 3),
    ("basic18", "train_main", "basic18", 4),
    ("forward_only", "nograd_train", "rgb_sound", 3),
    ("forward_only", "eval_masked", "rgb_sound", 3),
    ("forward_only", "eval_skipping", "rgb_sound", 1),
])
def test_every_stream_held_in_turn(row, stage, arch, min_streams):
    drive(row, stage, arch, min_streams)


def test_user_stream_row():
    """The rgb_sound main-net step issued under a user stream: the consumers run there, and the default stream -- which
    `_queue_default_stream_join` orders behind the side streams although nobody of this step launches on it -- is held as well."""
    user = torch.cuda.Stream()
    _batches("rgb_sound", 3)
    with torch.cuda.stream(user):
        base = drive("user_stream", "train_main", "rgb_sound", 5, extra=[(0, "default stream")])
    assert user.cuda_stream in base.found.handles() and base.found.handles()[0] == user.cuda_stream


@pytest.mark.parametrize("stage", ["train_main", "train_policy"])
def test_planned_row(stage):
    """Launch plans: calls 1-2 eager, call 3 recorded, calls 4-5 replayed with the holds on the handles of Plan.streams; the reference is
    the eager single-stream sequence."""
    import contextlib
    from adamml_amd import plan
    seen = []
    NOT_MET = "plan stream the eager calls never launched on"

    @contextlib.contextmanager
    def planned():
        plan.ENABLED = True
        try:
            yield
        finally:
            plan.ENABLED = False

    class PlanStreams:
        """SD.run's `extra`, read when the warm-up is over: the stream handles of every recorded plan of the model"""

        def __init__(self, model):
            self.model = model

        def __iter__(self):
            handles = [h or 0 for net in self.model.backbones() for p in net.__dict__.get("_launch_plans", {}).values()
                       if isinstance(p, plan.Plan) for h in list(p.streams)]          # (ctypes gives None for the null stream)
            seen.append(set(handles))
            return iter([(h, NOT_MET) for h in handles])

    before = dict(plan.stats)
    base = drive("planned", stage, "rgb_sound", 4 if stage == "train_main" else 3, steps=5, first_held=3, setup=planned,
                 wrap=lambda model: {"extra": PlanStreams(model)})
    assert plan.stats["recorded"] > before["recorded"] and plan.stats["replayed_ops"] > before["replayed_ops"]
    assert plan.stats.get("failed_recordings", 0) == before.get("failed_recordings", 0)
    # every model had recorded plans when its holds began, and discovery had met every stream of theirs in the eager calls: all are held
    assert seen and all(seen) and NOT_MET not in base.found.role_list()


@pytest.fixture()
def rccl_one_rank():
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    try:
        yield
    finally:
        dist.destroy_process_group()


def test_one_rank_rccl_row(rccl_one_rank):
    """HipDDP with SyncBatchNorm and the bucketed gradient all-reduce forced on a one-rank RCCL communicator: the lock-step interleaver, the
    deferred tapes and the bucket hooks, `reduce_gradients` between backward and the consumers.  Every collective is an identity, so the
    step must equal the plain single-stream step.  Only streams that carry the project's launches are held, not RCCL's."""
    from adamml_amd.distributed import HipDDP
    made = []

    def wrap(model):
        ddp = HipDDP(model, sync_bn=True, force_collectives=True)
        assert ddp.active and all(n.rt.sync.enabled for n in model.backbones())
        made.append(ddp)
        return {"forward": ddp, "after_backward": ddp.reduce_gradients}

    drive("one_rank_rccl", "train_main", "rgb_sound", 4, wrap=wrap)
    assert all(d.stats["bucket_all_reduces"] >= 2 for d in made)


# ---- the Prefetcher --------------------------------------------------------------------------------------------------------------------
def _prefetch_steps(model, feed, expo, before_step=None, found=None):
    """SGD steps over `feed`; the logits of every step as clones enqueued on the caller's stream, read at the end.  before_step() runs between a batch's
    hand-over and its step; found: discovery during the first step."""
    import contextlib
    model.freeze_policy_net()
    model.train()
    opt = FlatSGD(model._flat_main, 0.01, 0.9, 1e-4, False)
    outs = []
    it = iter(feed)
    k = 0
    while True:
        with SD.discover(found) if (found is not None and k == 0) else contextlib.nullcontext():
            try:
                inputs, target = next(it)
            except StopIteration:
                break
            if before_step is not None:
                before_step()
            logits, _ = model(inputs, gumbel_exponential=expo)
            outs.append(logits.detach().clone())
            F.cross_entropy(logits, target.to(DEV, non_blocking=True)).backward()
            opt.step()
            opt.zero_grad()
        k += 1
    torch.cuda.synchronize()
    return [o.cpu() for o in outs]


@pytest.fixture(scope="module")
def prefetch_reference(rgb_sound):  # noqa: F811
    """Logits of the four steps on the loader's own objects, without a Prefetcher, and the longest step's wall time."""
    import time
    from tests.test_data_gpu import _model
    expo = synth.synth_gumbel_exponential(2, 2, 2, seed=11).to(DEV)
    model = _model(["rgb", "sound"], 2)
    times = []

    def clock():
        torch.cuda.synchronize()
        times.append(time.perf_counter())

    want = _prefetch_steps(model, _objects(rgb_sound), expo, before_step=clock)
    times.append(time.perf_counter())
    assert len(want) == 4 and all(torch.isfinite(w).all() for w in want) and not torch.equal(want[0], want[1])
    return want, SD.step_time([(b - a) * 1e3 for a, b in zip(times, times[1:])][1:]), expo


@pytest.mark.parametrize("which", ["prefetch_stream", "caller_stream"])
def test_prefetcher_rows(rgb_sound, prefetch_reference, which):  # noqa: F811
    """Steps through Prefetcher(loader, device, depth=1) with (a) the prefetch stream held in front of every `_prepare`, (b) the caller's
    stream held in front of every step, so that batches N + 1 and N + 2 are prepared while step N is still pending."""
    from tests.test_data_gpu import _model
    want, step_ms, expo = prefetch_reference
    model = _model(["rgb", "sound"], 2)
    pf = Prefetcher(rgb_sound, DEV, depth=1)
    found, holds = SD.Found(), []
    ms = SD.hold_ms_for(step_ms)
    if which == "prefetch_stream":
        prepare = pf._prepare

        def held_prepare(source):
            holds.append(SD.hold(pf.stream, ms, "prefetch", "prepare"))
            return prepare(source)

        pf._prepare = held_prepare
        got = _prefetch_steps(model, pf, expo, found=found)
        held = pf.stream.cuda_stream
    else:
        caller = torch.cuda.current_stream()
        got = _prefetch_steps(model, pf, expo, before_step=lambda: holds.append(SD.hold(caller, ms, "caller", "step")), found=found)
        held = caller.cuda_stream
    found.add(pf.stream.cuda_stream, "prefetch stream")
    diff = [k for k, (w, g) in enumerate(zip(want, got)) if not SD._same_bits(w, g)]
    hold_ms = min(h.measured_ms() for h in holds)
    print("prefetcher [%s]: %d streams %s; step %.1f ms, holds of %.1f ms measured; late hand-overs %d"
          % (which, len(found), found.role_list(), step_ms, hold_ms, pf.stats.late))
    SD.report_line("prefetcher", "train_main, " + which, found.role(held), hold_ms, step_ms, len(diff))
    assert len(got) == len(want) == 4 and len(holds) == 4
    for h in holds:
        SD.check_hold(h.measured_ms(), step_ms, "prefetcher [%s]" % which)
    assert not diff, "prefetcher [%s]: the logits of steps %s differ from the steps without a Prefetcher" % (which, diff)
    if which == "prefetch_stream":
        assert pf.stats.late > 0, "the held prefetch stream was never found late at a hand-over: the hold did not take effect"


# ---- the control -----------------------------------------------------------------------------------------------------------------------
def test_control_a_skipped_wait_is_detected(monkeypatch):
    """The harness has teeth: rgb_sound in train mode under no_grad, the sound side stream held, and `Stream.wait_stream` made to skip the
    caller's wait for that one stream during the forward -- `adamml_fusion_fwd` then reads the sound logits before they are written, and
    the logits differ from the reference.  The consumer is arithmetic on tensors that stay allocated; nothing is indexed by what is read
    early, and no backward runs."""
    stage = "nograd_train"
    batches = _batches("rgb_sound", 2)
    ref = SD.run(_single_stream(_fresh("rgb_sound")), stage, batches)
    model = _fresh("rgb_sound")
    opt = SD.prepare(model, stage)
    found = SD.Found()
    with SD.discover(found):
        warm = SD.one_step(model, stage, opt, batches[0])
    assert not SD.compare(ref.steps[0], warm)
    caller, sound = torch.cuda.current_stream().cuda_stream, model._side_stream(torch.device(DEV, torch.cuda.current_device()), 0).cuda_stream
    assert sound in found.handles() and sound != caller
    step_ms = ref.step_ms[1]
    real, skipped = torch.cuda.Stream.wait_stream, []

    def wait_stream(self, other):
        if self.cuda_stream == caller and other.cuda_stream == sound:
            skipped.append(1)
            return None
        return real(self, other)

    holds = []

    def forward(xs, gumbel_exponential=None):
        monkeypatch.setattr(torch.cuda.Stream, "wait_stream", wait_stream)
        try:
            return model(xs, gumbel_exponential=gumbel_exponential)
        finally:
            monkeypatch.setattr(torch.cuda.Stream, "wait_stream", real)

    got = SD.one_step(model, stage, opt, batches[1], SD.as_stream(sound), SD.hold_ms_for(step_ms), holds, forward, None, found.role(sound))
    assert skipped == [1] and len(holds) == 1
    SD.check_hold(holds[0].measured_ms(), step_ms, "control")
    diff = SD.compare(ref.steps[1], got)
    SD.report_line("control: wait skipped", stage, found.role(sound), holds[0].measured_ms(), step_ms, len(diff))
    assert "logits" in diff, "the caller's wait for the held sound stream was skipped and the logits are still the reference's"
