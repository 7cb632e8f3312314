"""Holding one HIP stream back at a time (tests/test_stream_order_gpu.py, tests/test_stream_delay_cpu.py).

A training step of AdaMML is spread over several HIP streams (the ResNet on the caller's stream, the sound net and the policy nets on
side streams, every weight gradient on a stream of its own, the Prefetcher's input work on another) that are joined by
`wait_stream` / events, in launch plans by `KIND_WAIT` records.  Every per-channel reduction is order-fixed (csrc/common.h), so a
step is reproducible to the bit: whichever of its streams runs last, the results must be the same bits.  This module makes one chosen
stream run last -- bounded device work enqueued on it in front of the forward and in front of the backward -- and compares everything
the step produced with the same step issued on ONE stream, where FIFO order leaves no room for a race.

discovery   `discover()` replaces `hip._stream` (looked up as a module global by `hip.call` and `hip.scratch` at every launch) for
            the duration of a warm-up step and records each distinct raw handle with the first entry point launched on it: that name
            is the stream's role in the reports.  No list of known streams is kept anywhere.
delay       `hold(stream, ms)` enqueues `torch.cuda._sleep` (a counted loop of `torch.mm` on a private buffer where a build has
            none) on that stream and nothing else; the cycle count comes from one event-timed calibration per process, every hold
            is event-timed itself, and a hold that came out shorter than 1.5x the step it was to outlast fails its row.
consumers   `one_step` reads nothing back between issuing the forward and the end of the step: logits, decisions, policy logits,
            every gradient, one fused-optimizer step and every parameter and buffer are cloned ON THE CALLER'S STREAM, as a training
            loop consumes them; one `torch.cuda.synchronize()` follows.  An earlier synchronisation would close the window under test.
inputs      step k uses seed 100 + k for inputs, labels and Gumbel draws: a buffer read too early or too late holds other numbers."""
import contextlib
import sys
import time

import torch
import torch.nn.functional as F

HOLD_FACTOR = 2.0          # a hold lasts this many undelayed steps: the held stream is then certainly the last to run anything
MIN_FACTOR = 1.5           # ... and a measured hold below this many fails its row ("hold too short")
MAX_HOLD_MS = 250.0
TRAIN_STAGES = ("train_main", "train_policy")
FORWARD_STAGES = ("nograd_train", "eval_masked", "eval_skipping")
SEED0 = 100


# ---- discovery -----------------------------------------------------------------------------------------------------------------------
class Found:
    """The raw stream handles a step launched on, in order of first appearance, each with its role (first entry point launched on
    it; None for a handle only `hip.scratch` / a plan replay asked for so far)."""

    def __init__(self):
        self.roles = {}

    def see(self, handle, name=None):
        if handle not in self.roles:
            self.roles[handle] = name
        elif self.roles[handle] is None and name is not None:
            self.roles[handle] = name

    def add(self, handle, role):
        """A stream the caller knows to be in play although no entry point is launched on it (Prefetcher.stream with plain tensors, the
        default stream under a user stream)."""
        self.roles.setdefault(handle, role)

    def __len__(self):
        return len(self.roles)

    def handles(self):
        return list(self.roles)

    def entry(self, i):
        h = self.handles()[i]
        return h, self.role(h)

    def role(self, handle):
        r = self.roles[handle]
        return r if r is not None else "(no launch)"

    def role_list(self):
        return [self.role(h) for h in self.roles]


@contextlib.contextmanager
def discover(found=None):
    """`hip._stream` wrapped for the duration of the block: every handle it returns is recorded in `found`, with the entry point where the
    caller is `hip.call`.  Whatever `hip._stream` was on entry (the real accessor, the host-only stand-in of tools/launch_trace.py) is called
    through and put back on exit, on an exception too."""
    from adamml_amd import hip
    found = Found() if found is None else found
    inner = hip._stream

    def _stream():
        handle = inner()
        frame = sys._getframe(1)
        found.see(handle, frame.f_locals.get("name") if frame.f_code.co_name == "call" else None)
        return handle

    hip._stream = _stream
    try:
        yield found
    finally:
        hip._stream = inner


def as_stream(handle, device=None):
    """torch stream object of a raw handle (0, or the None a ctypes pointer array gives for it: the device's default stream)."""
    if not handle:
        return torch.cuda.default_stream(device)
    return torch.cuda.ExternalStream(handle, device=device)


# ---- delay ---------------------------------------------------------------------------------------------------------------------------
def step_time(measured_ms):
    """The time of a step undelayed, from the wall times (host synchronisation to host synchronisation, consumers included) of the
    measured steps of the undelayed multi-stream run: the shortest of them.  Not the warm-up step's: on the MI355X that one carries
    one-time costs of up to seconds (RCCL communicator set-up 4.1 s, the first JPEG decode 2.0 s, weight packs, arenas and scratch
    buffers growing: 1.2x - 4x a later step), and with the 250 ms clamp every hold would be "too short" against it.  Not the longest
    either: single steps were measured 2x - 3x longer than their neighbours (311.9 against 134.3 ms in the four-modality row;
    presumably a host stall while the caching allocator grows, which would delay the issue of all streams alike), and the shortest is
    the nearest to the work of the step itself, which is what the held stream has to outlast."""
    if not measured_ms:
        raise ValueError("stream_delay: no measured step")
    return min(measured_ms)


def hold_ms_for(step_ms):
    """Length of a hold for a step that takes step_ms undelayed."""
    if not step_ms > 0.0:
        raise ValueError("stream_delay: step time %r ms" % (step_ms,))
    return min(HOLD_FACTOR * step_ms, MAX_HOLD_MS)


def rate_from(units, measured_ms):
    """Delay units (sleep cycles, mm launches) per millisecond, from one event-timed delay of `units`."""
    if units <= 0 or not measured_ms > 0.0:
        raise ValueError("stream_delay: calibration measured %r ms for %r units" % (measured_ms, units))
    return units / measured_ms


def units_for(ms, rate):
    """Delay units of a hold of `ms` (clamped to MAX_HOLD_MS: a hold is bounded device work, whatever the caller asks for)."""
    if not rate > 0.0:
        raise ValueError("stream_delay: rate %r" % (rate,))
    return max(1, int(round(min(max(ms, 0.0), MAX_HOLD_MS) * rate)))


def check_hold(measured_ms, step_ms, what=""):
    """A hold shorter than MIN_FACTOR steps may have let the held stream finish before the others: the row proves nothing then."""
    if not measured_ms >= MIN_FACTOR * step_ms:
        raise AssertionError("hold too short: %s measured %.2f ms, the undelayed step takes %.2f ms (at least %.1fx = %.2f ms needed)"
                             % (what, measured_ms, step_ms, MIN_FACTOR, MIN_FACTOR * step_ms))


class Hold:
    """One enqueued hold: the events around it, what was asked for and on which stream."""

    def __init__(self, start, end, asked_ms, role, point):
        self.start, self.end, self.asked_ms, self.role, self.point = start, end, asked_ms, role, point

    def measured_ms(self):
        """(after the step's synchronisation)"""
        return self.start.elapsed_time(self.end)


_calibrated = {}


def _sleep_units(units):
    torch.cuda._sleep(units)


def _mm_units(units, _buf={}):
    dev = torch.cuda.current_device()
    a = _buf.get(dev)
    if a is None:
        a = _buf[dev] = torch.full((512, 512), 1.0 / 512, device="cuda")          # private: no other launch reads or writes it
    for _ in range(units):
        torch.mm(a, a)


def _delay_fn():
    return _sleep_units if hasattr(torch.cuda, "_sleep") else _mm_units


def _timed(fn, units, stream):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        s.record()
        fn(units)
        e.record()
    return s, e


def calibrate():
    """Delay units per millisecond, measured once per process and device: the unit count is raised until one delay takes at least 2 ms
    (at most six event-timed delays, each a fraction of a second)."""
    key = (torch.cuda.current_device(), _delay_fn().__name__)
    if key not in _calibrated:
        fn = _delay_fn()
        stream = torch.cuda.current_stream()
        units = 1000000 if fn is _sleep_units else 16
        _timed(fn, units, stream)[1].synchronize()                                # (first launch: module load)
        for _ in range(6):
            s, e = _timed(fn, units, stream)
            e.synchronize()
            ms = s.elapsed_time(e)
            if ms >= 2.0:
                break
            units *= 8
        _calibrated[key] = rate_from(units, ms)
    return _calibrated[key]


def hold(stream, ms, role="", point=""):
    """Enqueues `ms` milliseconds of device work on `stream` (and nothing else, anywhere); returns the Hold."""
    fn = _delay_fn()
    s, e = _timed(fn, units_for(ms, calibrate()), stream)
    return Hold(s, e, min(ms, MAX_HOLD_MS), role, point)


# ---- schedule ------------------------------------------------------------------------------------------------------------------------
def schedule(stage):
    """The points of a step at which the held stream gets a hold: in front of the forward, and -- where a backward runs -- again in front
    of `backward()` (the forward hold has drained by then: the forward's consumers waited for it)."""
    if stage in TRAIN_STAGES:
        return ("forward", "backward")
    if stage in FORWARD_STAGES:
        return ("forward",)
    raise ValueError("stream_delay: unknown stage %r" % (stage,))


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def step_batches(modality, B, S, groups, size, sound_size, steps, device="cuda"):
    """[(inputs, labels, Gumbel exponentials)] for steps 0 .. steps - 1, on the device; step k is drawn from seed 100 + k."""
    from adamml_amd import synth
    both = "rgbdiff" in modality and "flow" in modality
    out = []
    for k in range(steps):
        xs = [t.to(device) for t in synth.synth_inputs(modality, B, S, groups, size, sound_size, seed=SEED0 + k)]
        target = synth.synth_labels(B, 31, seed=SEED0 + k).to(device)
        expo = synth.synth_gumbel_exponential(S, len(modality) - (1 if both else 0), B, seed=SEED0 + k).to(device)
        out.append((xs, target, expo))
    return out


# ---- one step ------------------------------------------------------------------------------------------------------------------------
def prepare(model, stage):
    """Mode and frozen sub-network of a stage; returns the fused optimizer of the trainable sub-network (None: forward only)."""
    from adamml_amd.optim import FlatSGD
    model.unfreeze_policy_net()
    model.unfreeze_main_net()
    if stage == "train_main":
        model.freeze_policy_net()
    elif stage == "train_policy":
        model.freeze_main_net()
    model.train(stage in TRAIN_STAGES or stage == "nograd_train")
    if stage in ("eval_masked", "eval_skipping"):
        model.skip_unselected = stage == "eval_skipping"
    if stage not in TRAIN_STAGES:
        return None
    return FlatSGD(model._flat_main if stage == "train_main" else model._flat_policy, lr=0.01, momentum=0.9, weight_decay=1e-4)


class Clones:
    """Clones of many tensors enqueued on the current stream, read back later.  `add` queues a tensor under a key; `enqueue` copies what
    is queued -- every tensor read through its own view, one `torch.cat` per dtype instead of a launch per tensor: a model has ~1500
    parameters, gradients and buffers, and a launch and a device-to-host copy for each would make the consumers most of the step; `read`,
    after the step's synchronisation, gives {key: CPU tensor} in the order of `add`."""

    def __init__(self):
        self.queued, self.done = [], []

    def add(self, key, t):
        self.queued.append((key, t.detach()))

    def enqueue(self):
        by_dtype = {}
        for key, t in self.queued:
            by_dtype.setdefault(t.dtype, []).append((key, t))
        for items in by_dtype.values():
            flat = torch.cat([t.reshape(-1) for _, t in items]) if len(items) > 1 else items[0][1].clone().reshape(-1)
            self.done.append(([(key, t.shape) for key, t in items], flat))
        order = [key for key, _ in self.queued]
        self.queued = []
        return order

    def read(self):
        assert not self.queued
        out = {}
        for layout, flat in self.done:
            flat, off = flat.cpu(), 0
            for key, shape in layout:
                n = shape.numel()
                out[key] = flat[off:off + n].view(shape)
                off += n
        return out


def one_step(model, stage, opt, batch, held=None, hold_ms=0.0, holds=None, forward=None, after_backward=None, role=""):
    """One step with its consumers on the caller's stream and ONE synchronisation at its end; `held` (a stream) gets a hold at every point of
    schedule(stage).  Returns {key: CPU tensor}: logits, decisions, policy_logits, g.<parameter>, g.flat<i>, p.<parameter>, s.<buffer>."""
    xs, target, expo = batch
    points = schedule(stage) if held is not None else ()
    forward = model if forward is None else forward
    keep, order = Clones(), []
    if "forward" in points:
        holds.append(hold(held, hold_ms, role, "forward"))
    with contextlib.nullcontext() if stage in TRAIN_STAGES else torch.no_grad():
        logits, sel = forward(xs, gumbel_exponential=expo)
    keep.add("logits", logits)
    keep.add("decisions", sel)
    if stage in TRAIN_STAGES:
        keep.add("policy_logits", model.last_policy_logits)
    order += keep.enqueue()
    if stage in TRAIN_STAGES:
        loss = F.cross_entropy(logits, target)
        if stage == "train_policy":
            loss = loss + (sel.mean(dim=1) ** 2).mean()
        if "backward" in points:
            holds.append(hold(held, hold_ms, role, "backward"))
        loss.backward()
        if after_backward is not None:
            after_backward()
        for k, p in model.named_parameters():
            if p.grad is not None:
                keep.add("g." + k, p.grad)
        for i, fg in enumerate(model.flat_grad_buffers()):
            keep.add("g.flat%d" % i, fg)
        order += keep.enqueue()
        opt.step()
        params = set(k for k, _ in model.named_parameters())
        for k, v in model.state_dict().items():
            keep.add(("p." if k in params else "s.") + k, v)
        order += keep.enqueue()
        opt.zero_grad()
    torch.cuda.synchronize()
    out = keep.read()
    return {k: out[k] for k in order}


class Result:
    __slots__ = ("steps", "found", "holds", "step_ms", "held")


def run(model, stage, batches, pick=None, step_ms=None, first_held=1, forward=None, after_backward=None, extra=()):
    """Steps `model` through `batches` (steps 0 .. first_held - 1: warm-up, under discovery; the others measured).
    pick(found) -> (handle, role), the stream to hold in the measured steps for hold_ms_for(step_ms), or None: nobody is held.
    extra: (handle, role) pairs added to what discovery found.  Returns a Result: the per-step outputs of `one_step`, what was found,
    the holds, the wall time of every step (host synchronisation to host synchronisation) and the held (handle, role)."""
    opt = prepare(model, stage)
    r = Result()
    r.steps, r.found, r.holds, r.step_ms, r.held = [], Found(), [], [], None
    held = None
    for k, batch in enumerate(batches):
        if k == first_held:
            for h, role in extra:
                r.found.add(h, role)
            if pick is not None:
                r.held = pick(r.found)
                held = as_stream(r.held[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if k < first_held:
            with discover(r.found):
                out = one_step(model, stage, opt, batch, forward=forward, after_backward=after_backward)
        else:
            out = one_step(model, stage, opt, batch, held, hold_ms_for(step_ms) if held is not None else 0.0, r.holds, forward,
                           after_backward, r.held[1] if r.held else "")
        r.step_ms.append((time.perf_counter() - t0) * 1e3)
        r.steps.append(out)
    return r


# ---- comparison ----------------------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def compare(ref, got):
    """The keys at which two outputs of `one_step` differ, in the reference's order: "<key>" for other bits (a NaN compares by its bits
    too), "missing:<key>" / "extra:<key>" for a tensor only one of them has."""
    diff = []
    for k, v in ref.items():
        if k not in got:
            diff.append("missing:" + k)
        elif not _same_bits(v, got[k]):
            diff.append(k)
    diff += ["extra:" + k for k in got if k not in ref]
    return diff


def assert_same(ref, got, what, step, role="nobody"):
    diff = compare(ref, got)
    assert not diff, "%s: with the stream of %s held, step %d differs from the single-stream step in %d tensors: %s" % (
        what, role, step, len(diff), ", ".join(diff[:6]))
    return diff


# ---- report --------------------------------------------------------------------------------------------------------------------------
REPORT = []          # (row, stage, stream role, hold measured ms, step measured ms, differing tensors)


def report_line(row, stage, role, hold_ms, step_ms, differing):
    REPORT.append((row, stage, role, hold_ms, step_ms, differing))


def report_table(rows=None):
    rows = REPORT if rows is None else rows
    lines = ["| row | stage | held stream (first entry point) | hold measured, ms | step measured, ms | differing tensors |", "|---|---|---|---|---|---|"]
    for row, stage, role, hold_ms, step_ms, differing in rows:
        lines.append("| %s | %s | %s | %s | %.1f | %d |" % (row, stage, role, hold_ms if isinstance(hold_ms, str) else "%.1f" % hold_ms,
                                                         step_ms, differing))
    return "\n".join(lines)
