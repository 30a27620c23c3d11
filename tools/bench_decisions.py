"""Latency of one 30 fps tick of ``DecisionStream`` (one new logit row per stream, then ``decide()``) against what a caller can
do without it: keep each stream's logits in a device tensor and run ``DeviceEvalAccumulator(keep_video_predictions=True).add``
over the whole history on every tick.

    python tools/bench_decisions.py [--reps 200] [--rounds 5] [--out profiles/decision_latency.json]

Settings: S in {1, 32} streams, C = 7, the stream in whole-stream mode and with a window of W = 90 frames (three seconds); the
alternative at history lengths 90 and 9000 frames per stream (three seconds and five minutes).  The stream's tick is timed
as the push alone, as ``decide()`` alone and as both; the alternative's tick is one ``add`` over S videos of the history
length (new accumulator, offsets upload, two launches), without the cost of appending the new row to the history.  Each
figure is the median over ``rounds * reps`` = 1000 single calls of the time between two HIP events around ONE call, after
warm-up, with p10 - p90 and the host-clock median (call + synchronise) next to it; the methods alternate round by round in
the same process.  No bar is set: what comes out is written down.  Prints one JSON line and writes it to ``--out``.  Needs
the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

sys.modules.setdefault("triton", None)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

C, WINDOW, HISTORIES = 7, 90, (90, 9000)


def timed(fn, reps):
    """Per-call (HIP-event ms, host ms incl. synchronise) lists."""
    ev, host = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        host.append((time.perf_counter() - t) * 1e3)
        ev.append(e0.elapsed_time(e1))
    return ev, host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decision_latency.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_decisions.py measures on the GPU; none is visible")
    from feature_vs_text_compound_emotion_amd.decisions import DecisionStream
    from feature_vs_text_compound_emotion_amd.eval_device import DeviceEvalAccumulator
    g = torch.Generator(device="cuda").manual_seed(1)
    result = {"classes": C, "window": WINDOW, "reps": a.reps, "rounds": a.rounds, "stream": {}, "offline": {}}
    cases = {}
    for s in (1, 32):
        rows = torch.randn(s, C, device="cuda", generator=g)
        for mode, window in (("whole", None), (f"W{WINDOW}", WINDOW)):
            ds = DecisionStream(C, s, window=window, max_new=1)
            for _ in range(WINDOW):                      # a full window before timing
                ds.push_ragged(rows, [1] * s)
            name = f"stream_S{s}_{mode}"
            cases[name + "_push"] = (lambda ds=ds, rows=rows, s=s: ds.push_ragged(rows, [1] * s))
            cases[name + "_decide"] = ds.decide
            cases[name + "_tick"] = (lambda ds=ds, rows=rows, s=s: (ds.push_ragged(rows, [1] * s), ds.decide()))
        for n in HISTORIES:
            history = torch.randn(s * n, C, device="cuda", generator=g)
            labels = torch.zeros(s * n, device="cuda")
            offsets = [v * n for v in range(s + 1)]

            def offline(history=history, labels=labels, offsets=offsets):
                acc = DeviceEvalAccumulator(C, keep_video_predictions=True)
                acc.add(history, labels, video_offsets=offsets)
                return acc.video_predictions[0][1]
            cases[f"offline_S{s}_n{n}"] = offline
    # the two methods agree where both are defined: whole-stream decisions over a 90-frame history
    z = torch.randn(WINDOW, C, device="cuda", generator=g)
    ds = DecisionStream(C, 1, max_new=WINDOW)
    ds.push_rows(z)
    acc = DeviceEvalAccumulator(C, keep_video_predictions=True)
    acc.add(z, torch.zeros(WINDOW, device="cuda"))
    result["decisions_agree_on_a_90_frame_history"] = bool(torch.equal(ds.decide()[0], acc.video_predictions[0][1]))

    samples = {name: ([], []) for name in cases}
    for fn in cases.values():
        for _ in range(a.warmup):
            fn()
    for _ in range(a.rounds):       # alternate the methods: a drift of the machine hits all of them alike
        for name, fn in cases.items():
            ev, host = timed(fn, a.reps)
            samples[name][0].extend(ev)
            samples[name][1].extend(host)
    for name in cases:
        ev, host = samples[name]
        q = statistics.quantiles(ev, n=10)
        kind, key = name.split("_", 1)
        result[kind][key] = {"event_ms_median": round(statistics.median(ev), 4), "event_ms_p10": round(q[0], 4),
                             "event_ms_p90": round(q[-1], 4), "host_ms_median": round(statistics.median(host), 4)}
    for s in (1, 32):
        for n in HISTORIES:
            off = result["offline"][f"S{s}_n{n}"]["event_ms_median"]
            for mode in ("whole", f"W{WINDOW}"):
                tick = result["stream"][f"S{s}_{mode}_tick"]["event_ms_median"]
                result[f"offline_n{n}_over_stream_{mode}_S{s}"] = round(off / tick, 2)
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
