#!/usr/bin/env python3
"""What serving a stream costs: AdaMML (rgb + sound, ResNet-50, 224 x 224, S = 10 segments, LSTM policy) fed one segment at a time
through adamml_amd/online.py, against the one-shot eval forward of the same videos (the policy-gated `AdaMML._forward_skipping`,
which needs all 10 segments before it returns anything), at B = 1 and B = 8 videos, with launch plans off and on.

Per arm, over --windows windows of --videos video batches each (the arms alternate in ONE process; inputs resident on the device):

    forward   total_ms       one forward call, its logits waited for
    session   step_ms        one `Session.step`, its running logits waited for (what a streaming caller reads)
              first_decision_ms   from entering the first step to its decisions on the host
              total_ms       the 10 steps of a video batch

The session re-runs the policy head over the features seen so far at every step (55 head launches per batch instead of 10) and
runs each main net on one segment's selected clips at a time: its total is expected ABOVE the one-shot forward's; what it buys is
the first decision after one segment instead of ten, and a prediction after every segment.  Writes one JSON document (--out,
default profiles/online_latency.json) and prints it.  Needs a GPU.

    python tools/bench_online.py [--batches 1 8] [--segments 10] [--videos 10] [--windows 3] [--distinct 3] [--size 224]

--pool measures serving CONCURRENT streams instead: --streams (8) videos, video j starting --stagger (1) ticks after video j - 1
(online.stagger_schedule), so that a tick finds 1 to 8 streams at different positions.  Two arms on the same inputs and noise:

    pool      one `online.Pool`: a tick is ONE batched step over the streams that are due (the rows gathered by online.gather_videos)
    sessions  one `Session(batch_size=1)` per stream: a tick steps the due streams one after another

Per arm: tick_ms (a tick, the running logits of all its streams waited for), tick_ms_by_streams (the same, by how many streams the
tick held), total_ms of the schedule and streams_per_second = stream steps / total.  Writes profiles/online_pool_latency.json.

    python tools/bench_online.py --pool [--streams 8] [--stagger 1] [--segments 10] [--videos 10] [--windows 3]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(ms):
    s = sorted(ms)
    return dict(n=len(s), min=round(s[0], 3), median=round(statistics.median(s), 3), p90=round(s[min(len(s) - 1, int(0.9 * len(s)))], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--segments", type=int, default=10)
    ap.add_argument("--videos", type=int, default=10, help="video batches per window")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=3, help="distinct synthetic video batches cycled through")
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--out", default=None, help="default: profiles/online_latency.json, with --pool profiles/online_pool_latency.json")
    ap.add_argument("--pool", action="store_true", help="measure concurrent streams: one Pool against one-video Sessions")
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--stagger", type=int, default=1)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "online_pool_latency.json" if a.pool else "online_latency.json")

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_online: needs a GPU (a CPU run says nothing about a latency)")
    from adamml_amd import adamml, online, plan, synth
    dev = torch.device("cuda", 0)
    S, mod = a.segments, ["rgb", "sound"]
    model = adamml(groups=8, modality=mod, input_channels=[3, 1], num_segments=S, rng_policy=False, rng_threshold=0.5,
                   causality_modeling="lstm", num_classes=31, depth=50, without_t_stride=False, dropout=0.5, pooling_method="max",
                   fusion_point="logits", unimodality_pretrained=[], learnable_lf_weights=True)
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=1234))
    model.to(dev).eval()

    def forward(xs, pieces):
        t0 = time.perf_counter()
        logits, dec = model(xs, num_segments=S)
        logits.cpu()
        return dict(total_ms=(time.perf_counter() - t0) * 1e3, selected=dec.mean((0, 1)).tolist())

    def session(xs, pieces):
        steps, t0 = [], time.perf_counter()
        sess = model.online(S, xs[0].size(0))
        first = None
        for piece in pieces:
            t1 = time.perf_counter()
            st = sess.step(piece)
            st.logits.cpu()
            steps.append((time.perf_counter() - t1) * 1e3)
            first = st.decision_seconds * 1e3 if first is None else first
        return dict(total_ms=(time.perf_counter() - t0) * 1e3, step_ms=steps, first_decision_ms=first,
                    selected=sess.result()[1].mean((0, 1)).tolist())

    doc = dict(segments=S, size=a.size, modality=mod, depth=50, videos_per_window=a.videos, windows=a.windows, distinct_batches=a.distinct,
               device=torch.cuda.get_device_name(0), hw_queues_env=os.environ.get("GPU_MAX_HW_QUEUES"), batches={})
    before = (plan.ENABLED, plan.EVAL_ENABLED)

    def pool_arm(pieces, schedule, noise):
        pool, sids, ticks, t0 = model.online_pool(S, capacity=a.streams), {}, [], time.perf_counter()
        for tick in schedule:
            t1 = time.perf_counter()
            for j, t in tick:
                if t == 0:
                    sids[j] = pool.open(**noise[j])
            st = pool.step([sids[j] for j, _ in tick], online.gather_videos([(pieces[t], j) for j, t in tick]))
            st.logits.cpu()
            ticks.append((len(tick), (time.perf_counter() - t1) * 1e3))
        return dict(total_ms=(time.perf_counter() - t0) * 1e3, ticks=ticks,
                    selected=torch.stack([pool.result(sids[j])[1] for j in sorted(sids)]).mean((0, 1)).tolist())

    def sessions_arm(pieces, schedule, noise):
        sessions, ticks, t0 = {}, [], time.perf_counter()
        for tick in schedule:
            t1 = time.perf_counter()
            for j, t in tick:
                if t == 0:
                    sessions[j] = model.online(S, 1, gumbel_exponential=noise[j]["gumbel_exponential"])
                sessions[j].step([x[j:j + 1] for x in pieces[t]]).logits.cpu()
            ticks.append((len(tick), (time.perf_counter() - t1) * 1e3))
        return dict(total_ms=(time.perf_counter() - t0) * 1e3, ticks=ticks,
                    selected=torch.cat([sessions[j].result()[1] for j in sorted(sessions)]).mean((0, 1)).tolist())

    if a.pool:
        n, schedule = a.streams, online.stagger_schedule(a.streams, S, a.stagger)
        stream_steps = sum(len(t) for t in schedule)
        doc.pop("batches")
        doc.update(streams=n, stagger=a.stagger, ticks=len(schedule), stream_steps=stream_steps, arms={})
        with torch.no_grad():
            videos = []
            for k in range(a.distinct):
                xs = [t.to(dev) for t in synth.synth_inputs(mod, n, S, 8, a.size, seed=70 + k)]
                videos.append(online.split_segments(xs, S))
            arms = [(name, fn, planned) for planned in (False, True) for name, fn in (("pool", pool_arm), ("sessions", sessions_arm))]
            runs = {(name, planned): [] for name, _, planned in arms}

            def pool_window(name, fn, planned, count, keep):
                plan.ENABLED = plan.EVAL_ENABLED = planned
                torch.manual_seed(1000 + n)                                    # every arm and window draws the same policy noise
                for k in range(count):
                    noise = online.batch_noise(model, S, n)
                    torch.cuda.synchronize()
                    r = fn(videos[k % len(videos)], schedule, noise)
                    if keep:
                        runs[(name, planned)].append(r)

            for arm in arms:                                                   # warm every arm: shapes, arenas, recorded plans
                pool_window(*arm, count=max(2 * len(videos), plan.WARMUP_CALLS + 2), keep=False)
            for _ in range(a.windows):
                for arm in arms:
                    pool_window(*arm, count=a.videos, keep=True)
            for (name, planned), rs in runs.items():
                by = {}
                for r in rs:
                    for k, ms in r["ticks"]:
                        by.setdefault(k, []).append(ms)
                total = summary([r["total_ms"] for r in rs])
                doc["arms"]["%s%s" % (name, "_launch_plans" if planned else "")] = dict(
                    total_ms=total, tick_ms=summary([ms for r in rs for _, ms in r["ticks"]]),
                    tick_ms_by_streams={str(k): summary(v) for k, v in sorted(by.items())},
                    streams_per_second=round(stream_steps / (total["median"] * 1e-3), 1),
                    selected_share=[round(statistics.mean(r["selected"][m] for r in rs), 3) for m in range(len(mod))])
        a.batches = []
    with torch.no_grad():
        for B in a.batches:
            videos = []
            for k in range(a.distinct):
                xs = [t.to(dev) for t in synth.synth_inputs(mod, B, S, 8, a.size, seed=70 + k)]
                videos.append((xs, online.split_segments(xs, S)))
            arms = [(name, fn, planned) for planned in (False, True) for name, fn in (("forward", forward), ("session", session))]
            runs = {(name, planned): [] for name, _, planned in arms}

            def window(name, fn, planned, n, keep):
                plan.ENABLED = plan.EVAL_ENABLED = planned
                torch.manual_seed(1000 + B)                                # every arm and window draws the same policy noise
                for k in range(n):
                    torch.cuda.synchronize()
                    r = fn(*videos[k % len(videos)])
                    if keep:
                        runs[(name, planned)].append(r)

            for arm in arms:                                               # warm every arm: shapes, arenas, recorded plans
                window(*arm, n=max(2 * len(videos), plan.WARMUP_CALLS + 2), keep=False)
            for _ in range(a.windows):
                for arm in arms:
                    window(*arm, n=a.videos, keep=True)
            res = {}
            for (name, planned), rs in runs.items():
                d = dict(total_ms=summary([r["total_ms"] for r in rs]),
                         selected_share=[round(statistics.mean(r["selected"][m] for r in rs), 3) for m in range(len(mod))])
                if name == "session":
                    d["step_ms"] = summary([t for r in rs for t in r["step_ms"]])
                    d["first_step_ms"] = summary([r["step_ms"][0] for r in rs])
                    d["first_decision_ms"] = summary([r["first_decision_ms"] for r in rs])
                res["%s%s" % (name, "_launch_plans" if planned else "")] = d
            doc["batches"]["B%d" % B] = res
            del videos
    plan.ENABLED, plan.EVAL_ENABLED = before
    text = json.dumps(doc, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
