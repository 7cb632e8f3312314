"""Online inference: AdaMML one segment at a time.

    model.eval()
    with torch.no_grad():
        session = model.online(num_segments=10, batch_size=1)          # draws the policy's noise, as one forward would
        for x_t in stream:                                             # x_t: ONE segment per modality, in any form forward takes
            out = session.step(x_t)                                    # out.decisions [N, M], out.logits [N, classes] so far
        logits, decisions = session.result()                          # what forward returns for the segments seen

`AdaMML.forward` needs all S segments of a video before it returns anything.  The policy is causal (an LSTM over the segments
seen), so the decision for segment t can be taken when segment t arrives, the main nets can run on exactly the clips it selects,
and a running prediction exists after every segment.

No state is carried between the steps on the device side and nothing was added to the C ABI: the head is ONE tiny launch
(adamml_policy_head_fwd) whose per-video recurrence runs inside the kernel.  The session keeps the joint policy features of the
segments seen so far ([t, N, 2048]) and, at step t, runs `PolicyNet.decide` on all t + 1 of them with the first t + 1 rows of the
noise and reads the last row: the first t rows of that call are, bit for bit, what the earlier steps computed
(tests/test_online_gpu.py pins this prefix property).  With S <= 10 that is at most 55 head launches per batch instead of 10.

`split_segments` turns what a loader hands `forward` (one entry per modality, all S segments) into S per-step inputs."""
import copy
import time

import torch

from . import audio, jpeg, video

__all__ = ['Session', 'Step', 'split_segments']


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


class Session:
    """One batch of N = batch_size videos, served for at most num_segments steps.  `model`: an AdaMML in eval mode, under
    torch.no_grad().

    The constructor draws the policy's randomness exactly as one `forward` call would, from the same generator state (Gumbel
    policy: torch.empty(S*M*N, 2).exponential_(); rng_policy: torch.rand((S, M, N))): a session and a forward started from the same
    seed see the same noise.  gumbel_exponential [S, M*N, 2] replaces the draw, as in `forward`.

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
        dev = self.device = next(model.parameters()).device
        self._rand = self._expo = None
        if model.rng_policy:
            self._rand = torch.rand((S, M, N), dtype=torch.float32, device=dev)
            self._lstm = False
        else:
            if gumbel_exponential is None:
                expo = torch.empty(S * M * N, 2, dtype=torch.float32, device=dev).exponential_()
            else:
                if gumbel_exponential.numel() != S * M * N * 2:
                    raise ValueError("online.Session: gumbel_exponential holds %d values, [S, M*N, 2] = [%d, %d, 2] needs %d"
                                     % (gumbel_exponential.numel(), S, M * N, S * M * N * 2))
                expo = gumbel_exponential.to(device=dev, dtype=torch.float32).contiguous()
            # the row order `PolicyNet.decide` reads: segment-major for the LSTM head, modality-major for the FC heads
            self._lstm = model.policy_net.causality_modeling is not None
            self._expo = expo.reshape(S, M, N, 2) if self._lstm else expo.reshape(M, S, N, 2)
        self._feats, self._decisions, self._sum, self._ran = [], [], None, [0] * M
        model.last_skip_stats = None

    # -- one segment --------------------------------------------------------------------------------------------
    def _check(self, x, decisions):
        model, N, M = self.model, self.batch_size, self.num_modality
        if self.t >= self.num_segments:
            raise RuntimeError("online.Session: step %d of a session created for num_segments = %d" % (self.t + 1, self.num_segments))
        if not isinstance(x, (list, tuple)) or len(x) != len(model.modality):
            raise ValueError("online.Session: %d inputs for the model's %d modalities (%s)"
                             % (len(x) if isinstance(x, (list, tuple)) else 1, len(model.modality), " ".join(model.modality)))
        for x_, m in zip(x, model.modality):
            if x_.size(0) != N:
                raise ValueError("online.Session: the %s input holds %d videos, the session was created for batch_size = %d"
                                 % (m, x_.size(0), N))
        if decisions is not None:
            decisions = torch.as_tensor(decisions, dtype=torch.float32)
            if tuple(decisions.shape) != (N, M):
                raise ValueError("online.Session: forced decisions of shape %s, expected [N, M] = [%d, %d]" % (tuple(decisions.shape), N, M))
        return decisions

    def _decide(self):
        """This step's (decisions [M, N], policy logits [M, N, 2]) from the features seen so far."""
        model, t = self.model, self.t
        feats = torch.stack(self._feats, 0)                                   # [t + 1, N, F]
        expo = self._expo[:t + 1] if self._lstm else self._expo[:, :t + 1]
        dec, logits = model.policy_net.decide(feats, expo.contiguous())
        model.last_policy_logits = logits                                    # [t + 1, M, N, 2], as forward leaves it
        return dec[t], logits[t]

    @torch.no_grad()
    def step(self, x, decisions=None):
        """x: ONE segment per modality, in every form `forward` accepts with num_segments = 1.  Returns a `Step`."""
        start = time.perf_counter()
        forced = self._check(x, decisions)
        model, N, M, dev = self.model, self.batch_size, self.num_modality, self.device
        if model.training:
            raise RuntimeError("online.Session: the model was put into training mode during the session")
        model._flat_policy.ensure(dev)
        model._flat_main.ensure(dev)
        p_x, m_x, _ = model.data_layer(x, 1)
        policy_logits = None
        if not model.rng_policy:
            # the policy backbones on this segment, one BatchNorm group; the joint feature is kept for the later steps' head calls
            pol = model.policy_net
            self._feats.append(pol.joint_net.features([p if p.dtype == torch.float32 else p.flatten(0, 1) for p in p_x], groups=1))
        if forced is not None:
            dec = forced.to(dev).t().contiguous()                             # [M, N]
        elif model.rng_policy:
            dec = (self._rand[self.t] > model.rng_threshold).float()
        else:
            dec, policy_logits = self._decide()
        counts = (dec > 0.5).sum(1).tolist()                                  # host sync: the launch sizes depend on the decisions
        decided = time.perf_counter() - start
        stacked, ran = [], []
        for m_i in range(M):
            out, n = _run_selected(model.main_net.nets[m_i], m_x[m_i], dec[m_i], counts[m_i], N)
            stacked.append(out)
            ran.append(n)
        fused = model.main_net.fuse_segments(stacked, dec.reshape(1, M, N), 1)
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


def _run_selected(net, m_x, decisions, nsel, B):
    """One main net on the videos of this segment whose decision is 1, gathered as `AdaMML._forward_skipping` gathers them.  m_x: the
    data layer's tensor of ONE segment for this net; decisions: [B], nsel of them 1.  Returns ([B, classes] fp32 logits, exactly 0
    for the videos not run, and the number run).  Nothing is launched on the net when no video is selected, and the selected clips
    are never padded: the pad-to-8 of the whole-video forward (few call shapes for its launch plans) would make a stream of one
    video run 8 clips per segment, and with B small the distinct shapes are few anyway."""
    raw32 = m_x.dtype == torch.float32                                        # one-channel fp32 input [B, 1, H, W] (data_layer)
    frames = m_x if raw32 else m_x.flatten(0, 1)                              # [B*F, H, W, C], clips contiguous
    if nsel == B:
        return net.forward_nhwc(frames, 1), nsel
    ncls = net.fc.out_features if hasattr(net, "fc") else net.classifier[1].out_features
    out = torch.zeros(B, ncls, dtype=torch.float32, device=m_x.device)
    if nsel > 0:
        idx = (decisions > 0.5).nonzero().flatten()
        if raw32:
            sel = frames.index_select(0, idx)                                 # [n, 1, H, W]: one group
        else:
            sel = frames.view(B, frames.shape[0] // B, *frames.shape[1:]).index_select(0, idx).flatten(0, 1)
        out.index_copy_(0, idx, net.forward_nhwc(sel, 1))
    return out, nsel


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
