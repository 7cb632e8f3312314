"""`online.Pool` on the GPU: streams that open at different ticks, served in batched steps, against the lock-step `Session` on the same
videos (itself pinned to `forward` by tests/test_online_gpu.py, whose shapes, seeds, model and gate these tests share).

Stream j of a pool takes column j of the session's noise (`online.batch_noise`).  Decisions must be equal; logits and policy logits
are held to that file's GATE, allclose(rtol=1e-5, atol=1e-5) -- the same clip in another launch composition.  As there, decisions are
only compared where none sits on the fence: every reference first asserts that its smallest Gumbel margin is >= 100 x the gate.
Every comparison prints the largest difference it saw (on an MI355X: logits 9.3e-10 for the ResNet-50 + LSTM model, 3.7e-9 for the
depth-18 FC-head and rng_policy models, policy logits and results 0)."""
import collections
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from adamml_amd import hip, online, synth  # noqa: E402
from tests.test_online_gpu import DEV, GATE, MARGIN, build_model, run_session, smallest_margin  # noqa: E402

S, B, M = 3, 4, 2


class Case:
    """A model, four videos, their noise, and what the lock-step Session makes of them: steps[t] = (decisions [B, M], logits
    [B, classes], policy logits [M, B, 2] or None, executed), result = (logits [B, classes], decisions [B, S, M])."""

    def __init__(self, model, expo_for_margin=None):
        self.model = model
        self.xs = [t.to(DEV) for t in synth.synth_inputs(["rgb", "sound"], B, S, 8, 64, seed=5)]
        self.pieces = online.split_segments(self.xs, S)
        with torch.no_grad():
            if model.rng_policy:
                torch.manual_seed(4)
                self.noise = online.batch_noise(model, S, B)
                torch.manual_seed(4)
                session = model.online(S, B)
                self.steps = []
                for piece in self.pieces:
                    st = session.step(piece)
                    self.steps.append((st.decisions.clone(), st.logits.clone(), None, list(st.executed)))
            else:
                expo = synth.synth_gumbel_exponential(S, M, B, seed=11).to(DEV)
                self.noise = online.batch_noise(model, S, B, expo)
                self.steps, session = run_session(model, self.xs, S, B, expo)
                lstm = model.policy_net.causality_modeling is not None
                margin = smallest_margin(model.last_policy_logits, expo if lstm else expo.reshape(M, S, B, 2).transpose(0, 1))
                print("  smallest decision margin of the session %.3e (needs >= %.0e)" % (margin, MARGIN))
                assert margin >= MARGIN, "pick another noise seed: a decision of the reference sits on the fence (%g)" % margin
        self.result = tuple(t.clone() for t in session.result())
        dec = self.result[1]
        assert 0 < dec.sum().item() < dec.numel()                             # both decisions occur


@pytest.fixture(scope="module")
def case():
    return Case(build_model(["rgb", "sound"]))


def serve(case, schedule, capacity=B, permute=None):
    """The case's videos through one Pool by `schedule`; stream j opens when its segment 0 is due.  Returns the pool, the stream ids
    and, per tick, (its [(stream, t), ...] in the order stepped, the Step).  permute(tick) reorders a tick's rows."""
    with torch.no_grad():
        pool = case.model.online_pool(S, capacity)
        sids, served = {}, []
        for tick in schedule:
            tick = permute(tick) if permute else tick
            for j, t in tick:
                if t == 0:
                    sids[j] = pool.open(**case.noise[j])
                assert pool.position(sids[j]) == t
            st = pool.step([sids[j] for j, _ in tick], online.gather_videos([(case.pieces[t], j) for j, t in tick]))
            served.append((tick, st))
    return pool, sids, served


def assert_equals_session(case, pool, sids, served, what):
    """Every tick's rows against the session's step t_i rows, and every stream's result against the session's."""
    worst = collections.defaultdict(float)
    for tick, st in served:
        n = len(tick)
        assert st.decisions.shape == (n, M) and st.logits.shape == (n, 31)
        assert st.executed == [int(v) for v in st.decisions.sum(0).tolist()]
        assert st.decision_seconds > 0
        if case.model.rng_policy:
            assert st.policy_logits is None
        else:
            assert st.policy_logits.shape == (M, n, 2)
        for i, (j, t) in enumerate(tick):
            dec, logits, pol, _ = case.steps[t]
            assert torch.equal(st.decisions[i], dec[j]), (what, tick, i)
            worst["logits"] = max(worst["logits"], (st.logits[i] - logits[j]).abs().max().item())
            assert torch.allclose(st.logits[i], logits[j], **GATE), (what, tick, i, (st.logits[i] - logits[j]).abs().max().item())
            if pol is not None:
                worst["policy logits"] = max(worst["policy logits"], (st.policy_logits[:, i] - pol[:, j]).abs().max().item())
                assert torch.allclose(st.policy_logits[:, i], pol[:, j], **GATE), (what, tick, i)
    ref_logits, ref_dec = case.result
    for j, sid in sids.items():
        logits, dec = pool.result(sid)
        t = pool.position(sid)
        assert dec.shape == (t, M) and torch.equal(dec, ref_dec[j, :t])
        assert pool.executed(sid) == [int(v) for v in dec.sum(0).tolist()]     # a stream's clips run are its decisions summed
        if t == S:
            worst["result"] = max(worst["result"], (logits - ref_logits[j]).abs().max().item())
            assert logits.shape == (31,) and torch.allclose(logits, ref_logits[j], **GATE), (what, j)
    print("  %s: max |pool - session| %s" % (what, ", ".join("%s %.3e" % kv for kv in sorted(worst.items()))))


# ---- staggered == lock-step -------------------------------------------------------------------------------------------------------------

def test_staggered_streams_equal_the_lockstep_session(case):
    """Four streams, stream j opening at tick j: ticks of 1, 2, 3, 3, 2, 1 streams at up to three different positions."""
    schedule = online.stagger_schedule(B, S, 1)
    assert [len(t) for t in schedule] == [1, 2, 3, 3, 2, 1] and [t for _, t in schedule[2]] == [2, 1, 0]
    pool, sids, served = serve(case, schedule)
    assert_equals_session(case, pool, sids, served, "k = 1")
    stats = case.model.last_skip_stats
    assert stats == {"clips": S * B, "executed_per_modality": [int(v) for v in case.result[1].sum((0, 1)).tolist()]}
    assert pool.ticks == 6


def test_one_head_launch_for_a_tick_of_three_positions(case):
    schedule = online.stagger_schedule(B, S, 1)
    pool, sids, _ = serve(case, schedule[:2])
    tick = schedule[2]
    assert sorted(t for _, t in tick) == [0, 1, 2]
    with torch.no_grad():
        sids[2] = pool.open(**case.noise[2])
        x = online.gather_videos([(case.pieces[t], j) for j, t in tick])
        hip.profiler = hip.LaunchProfiler()
        try:
            st = pool.step([sids[j] for j, _ in tick], x)
            torch.cuda.synchronize()
            names = collections.Counter(r[0] for r in hip.profiler.records)
        finally:
            hip.profiler = None
    assert names["adamml_policy_head_fwd"] == 1, names
    assert names["adamml_fusion_fwd"] == 1, names
    for i, (j, t) in enumerate(tick):
        assert torch.equal(st.decisions[i], case.steps[t][0][j])


# ---- lock-step pool, and the order of a tick's rows -------------------------------------------------------------------------------------

def test_lockstep_pool_and_permuted_rows_equal_the_session(case):
    pool, sids, served = serve(case, online.stagger_schedule(B, S, 0))
    assert [len(t) for t, _ in served] == [B] * S
    assert_equals_session(case, pool, sids, served, "k = 0")
    orders = [[2, 0, 3, 1], [3, 2, 1, 0], [1, 3, 0, 2]]
    pool2, sids2, served2 = serve(case, online.stagger_schedule(B, S, 0), permute=lambda tick: [tick[i] for i in orders[tick[0][1]]])
    assert [[j for j, _ in t] for t, _ in served2] == orders
    assert_equals_session(case, pool2, sids2, served2, "k = 0, rows permuted")
    # the same tick in another order: the same rows, moved
    for (tick, a), (tick2, b) in zip(served, served2):
        back = [tick2.index(e) for e in tick]
        assert torch.equal(a.decisions, b.decisions[back]) and torch.allclose(a.logits, b.logits[back], **GATE)
        assert torch.allclose(a.policy_logits, b.policy_logits[:, back], **GATE)


# ---- capacity, slot reuse and the refusals ----------------------------------------------------------------------------------------------

def test_capacity_slot_reuse_and_refusals(case):
    model = case.model
    one = [[x[:1] for x in piece] for piece in case.pieces]                    # video 0 alone
    with torch.no_grad():
        session = model.online(S, 1, gumbel_exponential=case.noise[2]["gumbel_exponential"].reshape(S, M, 2))
        for piece in one:
            ref = session.step(piece)
        ref_logits, ref_dec = session.result()
        pool = model.online_pool(S, capacity=2)
        a, b = pool.open(**case.noise[0]), pool.open(**case.noise[1])
        with pytest.raises(RuntimeError, match=r"capacity = 2"):
            pool.open()
        pool.step([a, b], online.gather_videos([(case.pieces[0], 0), (case.pieces[0], 1)]))
        for t in (1, 2):
            pool.step([a], online.gather_videos([(case.pieces[t], 0)]))        # a runs to its end beside b
        assert pool.position(a) == S and pool.position(b) == 1
        with pytest.raises(RuntimeError, match=r"step 4 of stream 0 .*num_segments = 3"):
            pool.step([a], one[0])
        logits_a, dec_a = pool.result(a)
        assert torch.equal(dec_a, case.result[1][0]) and torch.allclose(logits_a, case.result[0][0], **GATE)
        slot = pool._stream(a).slot
        pool.close(a)
        # the refusals, none of which launches or moves anything
        with pytest.raises(KeyError, match="no open stream with id 0"):
            pool.step([a], one[0])
        with pytest.raises(KeyError):
            pool.result(a)
        with pytest.raises(KeyError):
            pool.step([b, 99], online.gather_videos([(case.pieces[1], 1), (case.pieces[1], 0)]))
        with pytest.raises(ValueError, match="more than once"):
            pool.step([b, b], online.gather_videos([(case.pieces[1], 1), (case.pieces[1], 1)]))
        with pytest.raises(ValueError, match=r"holds 2 videos, the step names 1 streams"):
            pool.step([b], online.gather_videos([(case.pieces[1], 1), (case.pieces[1], 0)]))
        assert pool.position(b) == 1 and pool.ticks == 3
        # video 0 again in the freed slot, with stream 2's noise, beside b's later segments: its one-video Session
        c = pool.open(**case.noise[2])
        assert pool._stream(c).slot == slot and c not in (a, b)
        with pytest.raises(RuntimeError, match=r"capacity = 2"):
            pool.open()
        for t in range(S):
            ids, parts = ([c, b], [(case.pieces[t], 0), (case.pieces[t + 1], 1)]) if t + 1 < S else ([c], [(case.pieces[t], 0)])
            st = pool.step(ids, online.gather_videos(parts))
        logits_c, dec_c = pool.result(c)
        print("  reused slot: max |pool - one-video session| %.3e" % (logits_c - ref_logits[0]).abs().max().item())
        assert torch.equal(dec_c, ref_dec[0]) and torch.allclose(logits_c, ref_logits[0], **GATE)
        assert torch.equal(st.decisions[0], ref.decisions[0]) and torch.allclose(st.logits[0], ref.logits[0], **GATE)
        logits_b, dec_b = pool.result(b)
        assert torch.equal(dec_b, case.result[1][1]) and torch.allclose(logits_b, case.result[0][1], **GATE)


# ---- forced decisions -------------------------------------------------------------------------------------------------------------------

def test_forced_decisions_run_only_what_they_select_and_stay_out_of_the_recurrence(case):
    """Streams 0 and 1 one tick apart.  Stream 1's first two steps are forced to (sound only), (nothing) while stream 0 decides
    for itself beside it; stream 1's third step, unforced, is the unforced reference's: its features were recorded, the forced
    decisions were not."""
    with torch.no_grad():
        pool = case.model.online_pool(S, capacity=2)
        s0, s1 = pool.open(**case.noise[0]), pool.open(**case.noise[1])
        pool.step([s0], online.gather_videos([(case.pieces[0], 0)]))
        own = case.steps[1][0][0]                                              # what stream 0 decides at its segment 1
        st = pool.step([s0, s1], online.gather_videos([(case.pieces[1], 0), (case.pieces[0], 1)]),
                       decisions=torch.stack([own.cpu(), torch.tensor([0., 1.])]))
        assert st.policy_logits is None and st.decisions.tolist() == [own.tolist(), [0., 1.]]
        assert st.executed == [int(own[0].item()), int(own[1].item()) + 1]
        hip.profiler = hip.LaunchProfiler()
        try:
            st = pool.step([s1], online.gather_videos([(case.pieces[1], 1)]), decisions=[[0, 0]])
            torch.cuda.synchronize()
            names = collections.Counter(r[0] for r in hip.profiler.records)
        finally:
            hip.profiler = None
        assert st.executed == [0, 0] and names["adamml_conv_stem_fwd"] == 0 and names["adamml_policy_head_fwd"] == 0, names
        assert pool.executed(s1) == [0, 1] and pool.result(s1)[1].tolist() == [[0., 1.], [0., 0.]]
        st = pool.step([s1, s0], online.gather_videos([(case.pieces[2], 1), (case.pieces[2], 0)]))
        for i, j in enumerate((1, 0)):
            dec, _, pol, _ = case.steps[2]
            assert torch.equal(st.decisions[i], dec[j]), j
            print("  stream %d: max |policy logits - session| %.3e" % (j, (st.policy_logits[:, i] - pol[:, j]).abs().max().item()))
            assert torch.allclose(st.policy_logits[:, i], pol[:, j], **GATE)
        # stream 0 was forced to its own decisions: all of it is the reference
        assert torch.equal(pool.result(s0)[1], case.result[1][0]) and torch.allclose(pool.result(s0)[0], case.result[0][0], **GATE)


# ---- the other policy variants ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["fc_heads", "rng_policy"])
def test_other_policies_staggered_equal_lockstep(variant):
    model = build_model(["rgb", "sound"], depth=18, causality=None) if variant == "fc_heads" else \
        build_model(["rgb", "sound"], depth=18, rng_policy=True)
    other = Case(model)
    pool, sids, served = serve(other, online.stagger_schedule(B, S, 1))
    assert_equals_session(other, pool, sids, served, variant + ", k = 1")
    if variant == "fc_heads":
        with torch.no_grad(), pytest.raises(ValueError, match="takes gumbel_exponential, not rand"):
            model.online_pool(S).open(rand=torch.ones(S, M))


# ---- the launcher's flag ----------------------------------------------------------------------------------------------------------------

def test_launcher_online_stagger_reports_what_online_reports(tmp_path):
    from adamml_amd import train
    from tests.test_validation_report_gpu import ARGS, REPORT, SEED, val_loader
    runs = {}
    for name, extra in (("online", ["--online"]), ("stagger", ["--online", "--online_stagger", "1"])):
        lines = []
        torch.manual_seed(SEED)
        res = train.main(ARGS + ["-e", "--logdir", str(tmp_path / name)] + extra, val_loader=val_loader(), log=lines.append)
        folder = os.path.join(str(tmp_path / name), os.listdir(str(tmp_path / name))[0])
        report = [l for l in lines if isinstance(l, str) and re.match(r"^Val@64@2" + REPORT, l)]
        assert len(report) == 1, lines
        runs[name] = (res, lines, report[0], np.load(os.path.join(folder, "all_selection.npz"))["selections"],
                      np.load(os.path.join(folder, "val_1crops_2clips_64_details_.npy")))
    (a, a_lines, a_rep, a_sel, a_out), (b, b_lines, b_rep, b_sel, b_out) = runs["online"], runs["stagger"]
    assert np.array_equal(a_sel, b_sel) and a_sel.shape == (3, 2, 2)
    assert (a["top1"], a["top5"], a["mAP"], a["selection"], a["flops"], a["executed"]) == \
        (b["top1"], b["top5"], b["mAP"], b["selection"], b["flops"], b["executed"])
    ga, gb = re.match(r"^Val@64@2" + REPORT, a_rep).groups(), re.match(r"^Val@64@2" + REPORT, b_rep).groups()
    assert ga[1:4] == gb[1:4] and ga[5:] == gb[5:]                             # Top@1, Top@5, mAP; flops and the selection figures
    print("  max |outputs - lock-step| %.3e" % np.abs(a_out - b_out).max())
    assert a_out.shape == b_out.shape == (3, 31) and np.allclose(b_out, a_out, **GATE)
    # batches of 2 and 1 videos, S = 2, one tick apart: 3 + 2 steps for 6 video segments, against 2 + 2 in lock-step
    assert "streams_per_step_mean" not in a["online"] and a["online"]["steps"] == 4
    assert b["online"]["steps"] == 5 and b["online"]["streams_per_step_mean"] == pytest.approx(6 / 5)
    pat = (r"^Val@64@2: \tOnline: (\d+\.\d+) ms/segment \(max (\d+\.\d+)\) over 5 steps\tFirst decision: (\d+\.\d+) ms"
           r"\tStreams/step: 1\.20$")
    m = re.match(pat, b_lines[b_lines.index(b_rep) + 1])
    assert m, b_lines
    mean, worst, first = (float(v) for v in m.groups())
    assert 0 < mean <= worst and 0 < first
