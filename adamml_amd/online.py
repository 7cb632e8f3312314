"""Online inference: AdaMML one segment at a time.

    model.eval()
    with torch.no_grad():
        session = model.online(num_segments=10, batch_size=1)          # draws the policy's noise, as one forward would
        for x_t in stream:                                             # x_t: ONE segment per modality, in any form forward takes
            out = session.step(x_t)                                    # out.decisions [N, M], out.logits [N, classes] so far
        logits, decisions = session.result()                          # what forward returns for the segments seen

`AdaMML.forward` needs all S segments of a video before it returns anything.  The policy is causal (an LSTM over the segments
seen), so the decision for segment t can be taken when segment t arrives, the main nets can run on exactly the clips it selects
(`run_selected` of adamml_amd/adamml.py, the runner of the whole-video eval forward, with S = 1), and a running prediction exists
after every segment.

No state is carried between the steps on the device side and nothing was added to the C ABI: the head is ONE tiny launch
(adamml_policy_head_fwd) whose per-video recurrence runs inside the kernel.  The session keeps the joint policy features of the
segments seen so far ([t, N, 2048]) and, at step t, runs `PolicyNet.decide` on all t + 1 of them with the first t + 1 rows of the
noise and reads the last row: the first t rows of that call are, bit for bit, what the earlier steps computed
(tests/test_online_gpu.py pins this prefix property).  With S <= 10 that is at most 55 head launches per batch instead of 10.

`split_segments` turns what a loader hands `forward` (one entry per modality, all S segments) into S per-step inputs.

A `Session` serves its N videos in lock-step.  Streams that start and end independently go through a `Pool` (`model.online_pool`):
every tick names the streams that have a segment and runs ONE batched step for them, whatever their positions -- one head launch
again, on the per-slot features the pool keeps.  `gather_videos` assembles such a tick's input from rows of `split_segments`
pieces, `stagger_schedule` is the schedule `-e --online --online_stagger K` serves a validation batch by, and `batch_noise` cuts
one session's noise draw into the per-stream noise that makes a pool decide what that session decides."""
import copy
import time

import torch

from . import audio, jpeg, video
from .adamml import run_selected

__all__ = ['Session', 'Pool', 'Step', 'split_segments', 'gather_videos', 'augmented', 'stagger_schedule', 'batch_noise']


class Step:
    """What `Session.step` returns: decisions [N, M] (this segment), policy_logits [M, N, 2] (this segment; None when the decisions
    were forced or drawn by rng_policy), logits [N, classes] (mean of the fused logits over the segments seen so far: what `forward`
    returns for a video that ended here), executed (clips run per main net in this step) and decision_seconds (host time from
    entering `step` until the decisions were known on the host: the main nets' launch sizes wait for them)."""
    __slots__ = ('decisions', 'policy_logits', 'logits', 'executed', 'decision_seconds')

    def __init__(self, decisions, policy_logits, logits, executed, decision_seconds):
        self.decisions, self.policy_logits, self.logits, self.executed = decisions, policy_logits, logits, executed
        self.decision_seconds = decision_seconds

    def __repr__(self):
        return "Step(decisions %s, logits %s, executed %s)" % (tuple(self.decisions.shape), tuple(self.logits.shape), self.executed)


def _draw_noise(who, model, S, N, gumbel_exponential=None):
    """The policy's noise for N videos of S segments, drawn exactly as one `forward` call draws it, from the same generator state
    (Gumbel policy: torch.empty(S*M*N, 2).exponential_(); rng_policy: torch.rand((S, M, N))); gumbel_exponential [S, M*N, 2]
    replaces the Gumbel draw, as in `forward`.  Returned segment-major for both head variants, [S, M, N, 2] (or [S, M, N] for the
    rng_policy): the rows of the draw are segment-major for the LSTM head and modality-major for the FC heads (`PolicyNet.decide`)."""
    M, dev = model.num_modality, next(model.parameters()).device
    if model.rng_policy:
        return torch.rand((S, M, N), dtype=torch.float32, device=dev)
    if gumbel_exponential is None:
        expo = torch.empty(S * M * N, 2, dtype=torch.float32, device=dev).exponential_()
    else:
        if gumbel_exponential.numel() != S * M * N * 2:
            raise ValueError("%s: gumbel_exponential holds %d values, [S, M*N, 2] = [%d, %d, 2] needs %d"
                             % (who, gumbel_exponential.numel(), S, M * N, S * M * N * 2))
        expo = gumbel_exponential.to(device=dev, dtype=torch.float32).contiguous()
    if model.policy_net.causality_modeling is not None:
        return expo.reshape(S, M, N, 2)
    return expo.reshape(M, S, N, 2).transpose(0, 1)


def _accept(who, model, x, n, held, decisions):
    """The refusals the two `step` methods share, before anything is launched.  x: the step's input; n: the videos it must hold
    (`held` says why, for the message); decisions: the forced decisions or None, returned as an fp32 [n, M] tensor."""
    if not isinstance(x, (list, tuple)) or len(x) != len(model.modality):
        raise ValueError("%s: %d inputs for the model's %d modalities (%s)"
                         % (who, len(x) if isinstance(x, (list, tuple)) else 1, len(model.modality), " ".join(model.modality)))
    for x_, m in zip(x, model.modality):
        if x_.size(0) != n:
            raise ValueError("%s: the %s input holds %d videos, %s" % (who, m, x_.size(0), held))
    if decisions is not None:
        decisions = torch.as_tensor(decisions, dtype=torch.float32)
        if tuple(decisions.shape) != (n, model.num_modality):
            raise ValueError("%s: forced decisions of shape %s, expected [N, M] = [%d, %d]"
                             % (who, tuple(decisions.shape), n, model.num_modality))
    if model.training:
        raise RuntimeError("%s: the model was put into training mode; call model.eval() before the next step" % who)
    return decisions


def _segment(model, x, n, forced, policy, start):
    """ONE segment of n videos through the model, the body of both `step` methods.  x: an accepted input (`_accept`); forced: its
    decisions [n, M] or None; policy(cur, decide): the caller's state -- it keeps the joint policy features cur [n, F] of this
    segment (None for an rng_policy model) and, if `decide`, returns this segment's (decisions [M, n], policy logits [M, n, 2] or
    None); start: time.perf_counter() on entering `step`.  Returns the decisions [M, n], the policy logits, the fused logits
    [n, classes] of this segment, the clips run per main net, the per-video flags behind those counts (M lists of n, on the host)
    and the seconds from `start` until the decisions were known on the host."""
    M, dev = model.num_modality, next(model.parameters()).device
    model._flat_policy.ensure(dev)
    model._flat_main.ensure(dev)
    p_x, m_x, _ = model.data_layer(x, 1)
    cur = None
    if not model.rng_policy:
        # the policy backbones on this segment, one BatchNorm group; kept also when the decisions are forced
        cur = model.policy_net.joint_net.features([p if p.dtype == torch.float32 else p.flatten(0, 1) for p in p_x], groups=1)
    dec, policy_logits = policy(cur, forced is None)
    if forced is not None:
        dec = forced.to(dev).t().contiguous()                                 # [M, n]
    chosen = (dec > 0.5).tolist()                                             # host sync: the launch sizes depend on the decisions
    decided = time.perf_counter() - start
    stacked, ran = [], []
    for m_i in range(M):
        out, k = run_selected(model.main_net.nets[m_i], m_x[m_i], dec[m_i], 1, n, nsel=sum(chosen[m_i]))
        stacked.append(out)
        ran.append(k)
    return dec, policy_logits, model.main_net.fuse_segments(stacked, dec.reshape(1, M, n), 1), ran, chosen, decided


class Session:
    """One batch of N = batch_size videos, served for at most num_segments steps.  `model`: an AdaMML in eval mode, under
    torch.no_grad().

    The constructor draws the policy's randomness exactly as one `forward` call would, from the same generator state
    (`_draw_noise`): a session and a forward started from the same seed see the same noise.  gumbel_exponential [S, M*N, 2]
    replaces the draw, as in `forward`.

    Everything runs on the current stream.  `step(x, decisions=...)` forces this step's decisions (an external policy, a test); the
    policy features of the segment are still recorded, but forced decisions do not enter the LSTM's recurrence: a later unforced
    step sees the decisions the policy itself would have taken."""

    def __init__(self, model, num_segments, batch_size, gumbel_exponential=None):
        if model.training:
            raise RuntimeError("online.Session: the model is in training mode; call model.eval() first")
        if torch.is_grad_enabled():
            raise RuntimeError("online.Session: gradients are enabled; create and step the session under torch.no_grad()")
        S, N = int(num_segments), int(batch_size)
        if S < 1 or N < 1:
            raise ValueError("online.Session: num_segments %d and batch_size %d must both be >= 1" % (S, N))
        self.model, self.num_segments, self.batch_size, self.t = model, S, N, 0
        M = self.num_modality = model.num_modality
        self.device = next(model.parameters()).device
        noise = _draw_noise("online.Session", model, S, N, gumbel_exponential)
        self._rand, self._expo = (noise, None) if model.rng_policy else (None, noise)
        self._lstm = not model.rng_policy and model.policy_net.causality_modeling is not None
        self._feats, self._decisions, self._sum, self._ran = [], [], None, [0] * M
        model.last_skip_stats = None

    # -- one segment --------------------------------------------------------------------------------------------
    def _policy(self, cur, decide):
        """Keeps this segment's features; this step's (decisions [M, N], policy logits [M, N, 2]) from the features seen so far."""
        model, t = self.model, self.t
        if cur is not None:
            self._feats.append(cur)
        if not decide:
            return None, None
        if model.rng_policy:
            return (self._rand[t] > model.rng_threshold).float(), None
        feats = torch.stack(self._feats, 0)                                   # [t + 1, N, F]
        expo = self._expo[:t + 1] if self._lstm else self._expo[:t + 1].transpose(0, 1)      # the FC heads read it modality-major
        dec, logits = model.policy_net.decide(feats, expo.contiguous())
        model.last_policy_logits = logits                                    # [t + 1, M, N, 2], as forward leaves it
        return dec[t], logits[t]

    @torch.no_grad()
    def step(self, x, decisions=None):
        """x: ONE segment per modality, in every form `forward` accepts with num_segments = 1.  Returns a `Step`."""
        start = time.perf_counter()
        model, N = self.model, self.batch_size
        if self.t >= self.num_segments:
            raise RuntimeError("online.Session: step %d of a session created for num_segments = %d" % (self.t + 1, self.num_segments))
        forced = _accept("online.Session", model, x, N, "the session was created for batch_size = %d" % N, decisions)
        dec, policy_logits, fused, ran, _, decided = _segment(model, x, N, forced, self._policy, start)
        self._sum = fused if self._sum is None else self._sum + fused
        self._decisions.append(dec.t())
        self._ran = [a + b for a, b in zip(self._ran, ran)]
        self.t += 1
        model.last_skip_stats = {"clips": self.t * N, "executed_per_modality": list(self._ran)}
        return Step(dec.t(), policy_logits, self._sum / self.t, ran, decided)

    def result(self):
        """(logits [N, classes], decisions [N, t, M]) over the t segments seen, in the shapes `forward` returns."""
        if self.t == 0:
            raise RuntimeError("online.Session: result() before the first step")
        return self._sum / self.t, torch.stack(self._decisions, 1)


class _Stream:
    """One open stream of a `Pool`: its slot, its position and the clips run for it per main net (host side)."""
    __slots__ = ('slot', 't', 'ran')

    def __init__(self, slot, M):
        self.slot, self.t, self.ran = slot, 0, [0] * M


class Pool:
    """Up to `capacity` streams that open, step and close independently, served in batched ticks.  `model`: an AdaMML in eval mode,
    under torch.no_grad().

        pool = model.online_pool(num_segments=10, capacity=8)
        a = pool.open()                                       # draws the stream's noise as Session(model, S, 1) would
        st = pool.step([a, b], x)                             # x: ONE segment per modality, row i the next segment of ids[i]
        logits, decisions = pool.result(a)                    # [classes], [t, M]
        pool.close(a)

    A tick is `Session.step` over the n streams named, which may be at different positions t_i: the data layer and the policy
    backbones on n rows, ONE `PolicyNet.decide`, each main net on the selected rows, the fusion and a per-stream running sum.  The
    LSTM head is one workgroup per video from segment 0, so streams at different positions share its one launch: the pool keeps the
    joint policy features and the noise rows of every slot ([S, capacity, ...]; the rows a stream has not reached hold zeros and
    ones), hands `decide` the first max(t_i) + 1 rows of the n columns and reads row t_i of column i.  The FC heads have no
    recurrence: they see the current row only.  Nothing was added to the C ABI.

    Forced decisions behave as in `Session`: the segment's features are recorded, the decisions do not enter the recurrence."""

    def __init__(self, model, num_segments, capacity=8):
        if model.training:
            raise RuntimeError("online.Pool: the model is in training mode; call model.eval() first")
        if torch.is_grad_enabled():
            raise RuntimeError("online.Pool: gradients are enabled; create and step the pool under torch.no_grad()")
        S, C = int(num_segments), int(capacity)
        if S < 1 or C < 1:
            raise ValueError("online.Pool: num_segments %d and capacity %d must both be >= 1" % (S, C))
        self.model, self.num_segments, self.capacity = model, S, C
        M = self.num_modality = model.num_modality
        dev = self.device = next(model.parameters()).device
        self._lstm = not model.rng_policy and model.policy_net.causality_modeling is not None
        # every slot's noise, segment-major: Exponential(1) rows [S, capacity, M, 2], or the rng_policy's uniforms [S, capacity, M]
        self._noise = torch.ones((S, C, M) if model.rng_policy else (S, C, M, 2), dtype=torch.float32, device=dev)
        self._decisions = torch.zeros(C, S, M, dtype=torch.float32, device=dev)
        # allocated by the first tick, which knows their widths: the LSTM head's input (features [S, capacity, F], exactly 0 and
        # noise [S, capacity, M, 2], exactly 1 in the rows a slot's stream has not reached) and the running sums [capacity, classes]
        self._feats = self._live = self._sum = None
        self._slots, self._streams, self._next_id = [None] * C, {}, 0
        self._clips, self._ran, self.ticks = 0, [0] * M, 0
        model.last_skip_stats = None

    # -- streams ------------------------------------------------------------------------------------------------
    def open(self, gumbel_exponential=None, rand=None):
        """Takes a free slot and returns the new stream's id (ids are never reused, slots are).  The stream's noise is drawn as
        `Session(model, S, 1)` draws it, from the same generator state; gumbel_exponential [S, M, 2] (segment-major for both head
        variants) or, for an rng_policy model, rand [S, M] replaces the draw."""
        model, S, M, dev = self.model, self.num_segments, self.num_modality, self.device
        if None not in self._slots:
            raise RuntimeError("online.Pool: all %d slots are in use (capacity = %d); close a stream first" % (self.capacity, self.capacity))
        given, name, other = (rand, "rand", gumbel_exponential) if model.rng_policy else (gumbel_exponential, "gumbel_exponential", rand)
        shape = (S, M) if model.rng_policy else (S, M, 2)
        if other is not None:
            raise ValueError("online.Pool: a model with rng_policy = %s takes %s, not %s"
                             % (model.rng_policy, name, "gumbel_exponential" if model.rng_policy else "rand"))
        if given is not None:
            if tuple(given.shape) != shape:
                raise ValueError("online.Pool: %s of shape %s, expected %s = %s"
                                 % (name, tuple(given.shape), "[S, M]" if model.rng_policy else "[S, M, 2]", list(shape)))
            noise = given.to(device=dev, dtype=torch.float32)
        else:
            noise = _draw_noise("online.Pool", model, S, 1)[:, :, 0]
        slot = self._slots.index(None)
        self._noise[:, slot] = noise
        if self._sum is not None:
            self._sum[slot].zero_()
        if self._feats is not None:
            self._feats[:, slot].zero_()
            self._live[:, slot].fill_(1.0)
        sid, self._next_id = self._next_id, self._next_id + 1
        self._slots[slot] = sid
        self._streams[sid] = _Stream(slot, M)
        return sid

    def _stream(self, sid):
        try:
            return self._streams[sid]
        except (KeyError, TypeError):
            raise KeyError("online.Pool: no open stream with id %r" % (sid,)) from None

    def close(self, sid):
        """Frees the stream's slot for the next `open`; the id is unknown from here on."""
        self._slots[self._stream(sid).slot] = None
        del self._streams[sid]

    def position(self, sid):
        """The number of segments the stream has been stepped through."""
        return self._stream(sid).t

    def executed(self, sid):
        """Clips run for this stream so far, per main net."""
        return list(self._stream(sid).ran)

    def result(self, sid):
        """(logits [classes], decisions [t, M]) over the t segments of this stream seen: row `sid` of what `Session.result` returns."""
        st = self._stream(sid)
        if st.t == 0:
            raise RuntimeError("online.Pool: result() of stream %r before its first step" % (sid,))
        return self._sum[st.slot] / st.t, self._decisions[st.slot, :st.t].clone()

    # -- one tick -----------------------------------------------------------------------------------------------
    def _record(self, cur, slots, tpos):
        """Keeps the joint features [n, F] of the segments that arrived, and their noise rows, for the LSTM head's calls."""
        if not self._lstm:
            return
        if self._feats is None:
            S, C, M = self.num_segments, self.capacity, self.num_modality
            self._feats = torch.zeros(S, C, cur.size(1), dtype=torch.float32, device=self.device)
            self._live = torch.ones(S, C, M, 2, dtype=torch.float32, device=self.device)
        self._feats.index_put_((tpos, slots), cur)
        self._live.index_put_((tpos, slots), self._noise[tpos, slots])

    def _decide(self, cur, slots, tpos, T):
        """This tick's (decisions [M, n], policy logits [M, n, 2]): ONE `decide` for all positions.  cur: the joint features [n, F]
        of the segments that arrived, recorded already; slots, tpos: [n] int64 on the device; T = max(tpos) on the host."""
        pol, n = self.model.policy_net, cur.size(0)
        if not self._lstm:
            # FC heads: no recurrence, the current row only -- noise modality-major, as their `decide` reads it
            dec, logits = pol.decide(cur[None], self._noise[tpos, slots].transpose(0, 1).reshape(self.num_modality, 1, n, 2).contiguous())
            return dec[0].contiguous(), logits[0]
        feats = self._feats[:T + 1].index_select(1, slots)                    # [T + 1, n, F]: column i is stream i from segment 0
        expo = self._live[:T + 1].index_select(1, slots).transpose(1, 2)      # [T + 1, M, n, 2]
        dec, logits = pol.decide(feats, expo.contiguous())
        cols = torch.arange(n, device=self.device)
        return dec[tpos, :, cols].t().contiguous(), logits[tpos, :, cols].transpose(0, 1)       # row t_i of column i

    @torch.no_grad()
    def step(self, ids, x, decisions=None):
        """ids: n distinct open streams; x: ONE segment per modality holding n videos, row i the next segment of ids[i], in every
        form `forward` accepts with num_segments = 1.  Returns a `Step` whose rows follow `ids`; `logits` row i is stream i's own
        running mean.  A refused step launches nothing and leaves every stream where it was."""
        start = time.perf_counter()
        model, dev, ids = self.model, self.device, list(ids)
        n = len(ids)
        if n < 1:
            raise ValueError("online.Pool: a step needs at least one stream")
        streams = [self._stream(sid) for sid in ids]
        if len(set(ids)) != n:
            raise ValueError("online.Pool: a stream id occurs more than once in one step (%s)" % (ids,))
        for sid, st in zip(ids, streams):
            if st.t >= self.num_segments:
                raise RuntimeError("online.Pool: step %d of stream %r in a pool created for num_segments = %d"
                                   % (st.t + 1, sid, self.num_segments))
        forced = _accept("online.Pool", model, x, n, "the step names %d streams" % n, decisions)
        index = torch.tensor([[st.slot for st in streams], [st.t for st in streams]], dtype=torch.int64).to(dev, non_blocking=True)
        slots, tpos = index[0], index[1]

        def policy(cur, decide):
            if cur is not None:
                self._record(cur, slots, tpos)                                # also when the decisions are forced, as in Session
            if not decide:
                return None, None
            if model.rng_policy:
                return (self._noise[tpos, slots] > model.rng_threshold).float().t().contiguous(), None
            return self._decide(cur, slots, tpos, max(st.t for st in streams))

        dec, policy_logits, fused, ran, chosen, decided = _segment(model, x, n, forced, policy, start)
        if self._sum is None:
            self._sum = torch.zeros(self.capacity, fused.size(1), dtype=torch.float32, device=dev)
        self._sum.index_add_(0, slots, fused)
        self._decisions.index_put_((slots, tpos), dec.t())
        for i, st in enumerate(streams):
            st.t += 1
            st.ran = [a + int(chosen[m_i][i]) for m_i, a in enumerate(st.ran)]
        self._clips, self._ran, self.ticks = self._clips + n, [a + b for a, b in zip(self._ran, ran)], self.ticks + 1
        model.last_skip_stats = {"clips": self._clips, "executed_per_modality": list(self._ran)}
        logits = self._sum.index_select(0, slots) / (tpos + 1).to(torch.float32)[:, None]
        return Step(dec.t(), policy_logits, logits, ran, decided)


def batch_noise(model, num_segments, batch_size, gumbel_exponential=None):
    """The noise of ONE `Session(model, S, N)`, cut into what `Pool.open` takes: a list of N keyword dicts, entry j holding column j.
    Drawn in one draw exactly as the session draws it (gumbel_exponential [S, M*N, 2] replaces the draw, read as the session reads
    it), so N pool streams opened with these decide as the lock-step session from the same generator state decides."""
    noise = _draw_noise("online.batch_noise", model, int(num_segments), int(batch_size), gumbel_exponential)
    name = "rand" if model.rng_policy else "gumbel_exponential"
    return [{name: noise[:, :, j]} for j in range(noise.size(2))]


def stagger_schedule(n, num_segments, k):
    """Which streams step when, for n streams of S = num_segments segments each, stream j opening at tick j * k: a list over the
    ticks of [(stream, t), ...], stream j being at segment t at tick j * k + t.  k = 0 is lock-step (S ticks of all n streams), with
    k >= S no two streams overlap; ticks in which no stream steps (k > S) are left out."""
    n, S, k = int(n), int(num_segments), int(k)
    if n < 1 or S < 1 or k < 0:
        raise ValueError("stagger_schedule: n = %d and num_segments = %d must be >= 1, k = %d >= 0" % (n, S, k))
    ticks = [[(j, tick - j * k) for j in range(n) if 0 <= tick - j * k < S] for tick in range((n - 1) * k + S)]
    return [tick for tick in ticks if tick]


# ---------------------------------------------------------------------------------------------------- gather_videos
def augmented(piece):
    """A step's per-modality input with every video.Frames / video.EncodedFrames entry turned into the video.Augmented it decodes
    to (`video.augment`, on the device the entry is on); the other entries as they are.  What `gather_videos` does with such
    entries on every call: a caller that takes rows of one piece in several ticks passes this instead, and decodes once."""
    return [video.Augmented(video.augment(x), x.modality, x.k_out) if isinstance(x, (video.Frames, video.EncodedFrames)) else x
            for x in piece]


def _gather_one(entries):
    """entries: [(x, row), ...] of ONE modality -> the input holding those rows, in the form of x."""
    first = entries[0][0]
    if isinstance(first, audio.Waveforms):
        form, same = "Waveforms", lambda x: isinstance(x, audio.Waveforms)
    elif isinstance(first, video.Augmented):
        form, same = "Augmented", lambda x: isinstance(x, video.Augmented) and x.modality == first.modality and x.k_out == first.k_out
    elif torch.is_tensor(first) and first.dtype in (torch.float32, torch.uint8):
        form, same = "%s tensor" % str(first.dtype)[6:], lambda x: torch.is_tensor(x) and x.dtype == first.dtype
    else:
        what = "%s tensor" % str(first.dtype)[6:] if torch.is_tensor(first) else type(first).__name__
        raise TypeError("gather_videos: expected float32 or uint8 tensors, Waveforms, Frames, EncodedFrames or Augmented, got a %s" % what)
    for x, _ in entries:
        if not same(x):
            raise TypeError("gather_videos: the pieces of one modality differ in form: %s and %s"
                            % (form, "%s tensor" % str(x.dtype)[6:] if torch.is_tensor(x) else type(x).__name__))
    if form == "Waveforms":
        return audio.Waveforms(torch.stack([x.wave[r] for x, r in entries]), torch.stack([x.missing[r] for x, r in entries]))
    if form == "Augmented":
        return video.Augmented(torch.stack([x.u8[r] for x, r in entries]), first.modality, first.k_out)
    return torch.stack([x[r] for x, r in entries])


def gather_videos(parts):
    """parts: [(piece, row), ...], `piece` one element of `split_segments(...)` (ONE segment per modality of a batch of videos), row
    a video of it.  Returns the per-modality input of a step made of those rows, in that order: what `Pool.step` takes when its
    streams come from one loader's batches at different positions.  fp32 and uint8 frame tensors, audio.Waveforms (waves and missing
    flags) and video.Augmented keep their form; video.Frames / video.EncodedFrames pieces are first turned into Augmented (`augmented`:
    one decode per distinct piece and call -- pass `augmented(piece)` to decode once for several calls)."""
    parts = list(parts)
    if not parts:
        raise ValueError("gather_videos: no (piece, row) given")
    M = len(parts[0][0])
    if any(len(piece) != M for piece, _ in parts):
        raise ValueError("gather_videos: the pieces hold different numbers of modalities (%s)" % sorted({len(p) for p, _ in parts}))
    decoded = {}
    for piece, _ in parts:
        if id(piece) not in decoded:
            decoded[id(piece)] = augmented(piece)
    return [_gather_one([(decoded[id(piece)][m], int(row)) for piece, row in parts]) for m in range(M)]


# ---------------------------------------------------------------------------------------------------- split_segments
def _split_channels(k, S, what):
    if S < 1 or k % S:
        raise ValueError("split_segments: %s has %d channels, which num_segments = %d does not divide" % (what, k, S))
    return k // S


def _split_frames(fr, S):
    """A video.Frames of S segments -> S Frames of one: each video's source window cut along its channel axis, its Geometry (one
    augmentation per video, as the reference draws it) and its tables kept."""
    kp = _split_channels(fr.k_in, S, "the %s Frames" % fr.modality)
    if fr.modality == 'rgbdiff' and kp % (3 * (fr.diffs + 1)):
        raise ValueError("split_segments: %d rgbdiff channels per segment are no whole frame groups of %d RGB frames" % (kp, fr.diffs + 1))
    meta0 = fr.meta.cpu().numpy()
    wins, offset = [], 0
    for i in range(fr.n):
        d = meta0[i * video.DESC:(i + 1) * video.DESC]
        off = (int(d[0]) & 0xffffffff) | (int(d[1]) << 32)
        h, w = int(d[2]), int(d[3])
        wins.append((off, h, w, offset))
        offset += video._align(h * w * kp)
    pinned = fr.data.device.type == 'cpu' and fr.data.is_pinned()
    pieces = []
    for t in range(S):
        meta = meta0.copy()
        data = torch.empty(max(offset, 16), dtype=torch.uint8, device=fr.data.device, pin_memory=pinned)
        for i, (off, h, w, new) in enumerate(wins):
            src = fr.data[off:off + h * w * fr.k_in].view(h, w, fr.k_in)[:, :, t * kp:(t + 1) * kp]
            data[new:new + h * w * kp].view(h, w, kp).copy_(src)
            d = meta[i * video.DESC:(i + 1) * video.DESC]
            d[0], d[1] = video.split_offset(new)
            d[4] = w * kp
        p = copy.copy(fr)
        p.data, p.k_in = data, kp
        p.k_out = kp // (fr.diffs + 1) * fr.diffs if fr.modality == 'rgbdiff' else kp
        p.read_bytes = sum(h * w * kp for _, h, w, _ in wins)
        p.meta = torch.from_numpy(meta)
        if pinned:
            p.meta = p.meta.pin_memory()
        p.meta = p.meta.to(fr.meta.device)
        pieces.append(p)
    return pieces


def _split_encoded(ef, S):
    """A video.EncodedFrames of S segments -> S EncodedFrames of one: each video's files of that segment (rgb: one file per frame;
    flow: the x then y files; rgbdiff: diffs + 1 files per frame group), its Geometry and tables kept.  No file is parsed again:
    a piece's jpeg.Batch is packed from the whole's entropy-coded bytes and the `jpeg.Info` its constructor kept.  The pieces are
    built on the host (pinned when the whole was) and moved with `.to(device)` like the whole."""
    ch = 1 if ef.modality == 'flow' else 3
    kp = _split_channels(ef.k_in, S, "the %s EncodedFrames" % ef.modality)
    unit = ch * (ef.diffs + 1) if ef.modality == 'rgbdiff' else (2 if ef.modality == 'flow' else ch)
    if kp % unit:
        raise ValueError("split_segments: %d %s channels per segment are no whole number of %d-channel units" % (kp, ef.modality, unit))
    nf_all, nf = ef.k_in // ch, kp // ch
    pinned = ef.meta.device.type == 'cpu' and ef.meta.is_pinned()
    coded, bmeta, meta0 = ef.batch.data.cpu().numpy(), ef.batch.meta.cpu().numpy(), ef.meta.cpu().numpy()
    # every file as (the whole's coded buffer, an Info whose segments are its byte ranges in that buffer)
    infos = []
    for f, inf in enumerate(ef.batch.infos):
        seg_at, nseg = int(bmeta[f * jpeg.DESC + 4]), int(bmeta[f * jpeg.DESC + 5])
        rec = bmeta[seg_at:seg_at + nseg * jpeg.SEG].reshape(nseg, jpeg.SEG)
        inf = copy.copy(inf)
        inf.segments = [(int(o), int(o) + int(n)) for o, n in rec[:, :2]]
        infos.append(inf)
    pieces = []
    for t in range(S):
        meta, places, sel, file_of, offset = meta0.copy(), [], [], [], 0
        for i, g in enumerate(ef.geometries):
            for j in range(nf):
                sel.append(i * nf_all + t * nf + j)
                places.append(jpeg.Placement(offset, g.width * kp, kp, j * ch))
                file_of.append((i, j))
            d = meta[i * video.DESC:(i + 1) * video.DESC]
            d[0], d[1] = video.split_offset(offset)
            d[4] = g.width * kp
            offset += video._align(g.height * g.width * kp)
        p = copy.copy(ef)
        p.k_in, p.file_of = kp, file_of
        p.k_out = kp // (ef.diffs + 1) * ef.diffs if ef.modality == 'rgbdiff' else kp
        p.batch = jpeg.Batch([coded] * len(sel), places, offset, pin_memory=pinned, infos=[infos[f] for f in sel])
        p.meta = torch.from_numpy(meta)
        if pinned:
            p.meta = p.meta.pin_memory()
        pieces.append(p)
    return pieces


def _split_one(x, S):
    if isinstance(x, audio.Waveforms):
        if x.wave.shape[1] != S:
            raise ValueError("split_segments: Waveforms of %d segments, num_segments = %d" % (x.wave.shape[1], S))
        return [audio.Waveforms(x.wave[:, t:t + 1], x.missing[:, t:t + 1]) for t in range(S)]
    if isinstance(x, video.EncodedFrames):
        return _split_encoded(x, S)
    if isinstance(x, video.Frames):
        return _split_frames(x, S)
    if isinstance(x, video.Augmented):
        kp = _split_channels(x.k_out, S, "the %s Augmented" % x.modality)
        return [video.Augmented(x.u8[..., t * kp:(t + 1) * kp], x.modality, kp) for t in range(S)]
    if not torch.is_tensor(x):
        raise TypeError("split_segments: expected tensors, Waveforms, Frames, EncodedFrames or Augmented, got %s" % type(x).__name__)
    if x.dtype == torch.uint8 and x.dim() == 4:                               # decoded frames [N, H, W, S*F*C] (Stack's arrays)
        kp = _split_channels(x.size(3), S, "the uint8 frame tensor")
        return [x[..., t * kp:(t + 1) * kp] for t in range(S)]
    if x.dim() not in (3, 4):
        raise ValueError("split_segments: expected [N, S*F*C, H, W] or sound waveforms [N, S, L], got shape %s" % (tuple(x.shape),))
    kp = _split_channels(x.size(1), S, "the input tensor")                    # segment-major channel axis; sound: [N, S, ...]
    return [x[:, t * kp:(t + 1) * kp] for t in range(S)]


def split_segments(x, num_segments):
    """x: what a loader hands `forward` -- one entry per modality, each holding all S = num_segments segments of its N videos
    (fp32 tensors [N, S*F*C, H, W], sound [N, S, 256, 256] or waveforms [N, S, L], audio.Waveforms, video.Frames,
    video.EncodedFrames, video.Augmented).  Returns S lists, one per step, each what `Session.step` (or `forward` with
    num_segments = 1) takes: tensors and Augmented are sliced along their segment-major channel axis (views), Waveforms along S with
    their `missing` flags, Frames / EncodedFrames take that segment's frames or files and keep each video's one Geometry."""
    S = int(num_segments)
    per_modality = [_split_one(x_, S) for x_ in x]
    return [[pm[t] for pm in per_modality] for t in range(S)]
