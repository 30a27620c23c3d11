"""Per-tick latency of ``FrameStream.push(frames, counts, boxes=)`` on full camera frames against what a caller does without
it: per stream, slice the frame to its box, ``.contiguous()``, and ``FrameStream.push`` of that stream alone.

    python tools/bench_frames_boxes.py [--reps 200] [--rounds 5] [--out profiles/frames_boxes_latency.json]

Settings: S in {1, 32} streams, one tick per call: one 1280 x 720 frame per stream, 48 -> 40 crop, one face box per frame with
sides 150 .. 400 that lies inside the frame (so that the alternative needs no padding) and changes every tick; a pool of
``POOL`` ticks of frames and boxes cycles.  The alternative runs twice: ``warm``, its per-geometry coefficient tables cached
(every (h, w) of the pool has been seen), and ``cold``, the cache emptied before every call, outside the timed region -- a box
size seen for the first time, which is what a tracker produces.  Before timing, the rings of the two sides are compared for
equality over one cycle of the pool.  Each figure is the median over ``rounds * reps`` calls of the time between two HIP events
around ONE call, after warm-up, the methods alternating round by round in the same process; the host-clock median (call +
synchronise) is kept next to it.  Streams are reset between calls (host ints only), outside the timed region.  Also records the
build time and size of the table store.  Prints one JSON line and writes it to ``--out``.  Needs the GPU.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.modules.setdefault("triton", None)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from bench_stream import timed  # noqa: E402

H, W, POOL, LO, HI = 720, 1280, 8, 150, 400


def make_case(streams, g, rng):
    from feature_vs_text_compound_emotion_amd.frames import FrameStream
    video = torch.randint(0, 256, (POOL, streams, H, W, 3), device="cuda", generator=g, dtype=torch.uint8)
    boxes = []
    for _ in range(POOL):
        tick = []
        for _ in range(streams):
            bw, bh = rng.randint(LO, HI), rng.randint(LO, HI)
            x0, y0 = rng.randint(0, W - bw), rng.randint(0, H - bh)
            tick.append((x0, y0, x0 + bw, y0 + bh))
        boxes.append(tick)
    boxed = FrameStream(streams, max_new=1)
    alone = {kind: [FrameStream(1, max_new=1) for _ in range(streams)] for kind in ("warm", "cold")}
    state = {"boxed": 0, "warm": 0, "cold": 0}

    def push_boxed():
        t = state["boxed"] % POOL
        state["boxed"] += 1
        boxed.reset()
        boxed.push(video[t], [1] * streams, boxes[t])

    def by_hand(kind):
        t = state[kind] % POOL
        state[kind] += 1
        for s, fs in enumerate(alone[kind]):
            fs.reset()
            x0, y0, x1, y1 = boxes[t][s]
            fs.push(video[t, s, y0:y1, x0:x1].contiguous()[None], [1])

    def prepare_cold():
        for fs in alone["cold"]:
            fs._xf._tables.clear()

    def rings_equal():
        mine = boxed.take([(s, 0) for s in range(streams)])
        theirs = torch.cat([fs.take([(0, 0)]) for fs in alone["warm"]])
        return torch.equal(mine, theirs)

    return push_boxed, by_hand, prepare_cold, rings_equal


def timed_cold(fn, prepare, reps):
    ev, host = [], []
    for _ in range(reps):
        prepare()
        e, h = timed(fn, 1)
        ev += e
        host += h
    return ev, host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3 * POOL)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_boxes_latency.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frames_boxes.py measures on the GPU; none is visible")
    from feature_vs_text_compound_emotion_amd import frames
    t = time.perf_counter()
    store = frames.box_tables(48, frames.BOX_MAX_SIDE)
    built = time.perf_counter() - t
    g, rng = torch.Generator(device="cuda").manual_seed(5), random.Random(5)
    result = {"frame": [H, W], "size": 48, "crop": 40, "box_sides": [LO, HI], "pool_ticks": POOL, "reps": a.reps, "rounds": a.rounds,
              "table_store": {"size": 48, "max_side": store.max_side, "build_s": round(built, 3),
                              "bytes": int(store.data.nbytes + store.meta.nbytes), "max_band_rows": store.max_rows,
                              "max_ksize": store.max_ks},
              "boxed": {}, "by_hand_warm": {}, "by_hand_cold": {}}
    cases, compared = {}, 0
    for s in (1, 32):
        push_boxed, by_hand, prepare_cold, rings_equal = make_case(s, g, rng)
        for _ in range(max(a.warmup, POOL)):      # every geometry of the pool is seen here, and the two sides are compared
            push_boxed()
            by_hand("warm")
            if not rings_equal():
                raise SystemExit(f"S = {s}: the boxed push and the per-stream slices differ")
            compared += s
        cases[f"boxed_S{s}"] = (push_boxed, None)
        cases[f"by_hand_warm_S{s}"] = (lambda f=by_hand: f("warm"), None)
        cases[f"by_hand_cold_S{s}"] = (lambda f=by_hand: f("cold"), prepare_cold)
    result["frames_compared_equal"] = compared
    samples = {name: ([], []) for name in cases}
    for _ in range(a.rounds):           # alternate the methods: a drift of the machine hits all alike
        for name, (fn, prepare) in cases.items():
            ev, host = timed(fn, a.reps) if prepare is None else timed_cold(fn, prepare, a.reps)
            samples[name][0].extend(ev)
            samples[name][1].extend(host)
    for name in cases:
        kind, s = name.rsplit("_S", 1)
        ev, host = samples[name]
        q = statistics.quantiles(ev, n=10)
        result[kind]["S" + s] = {"event_ms_median": round(statistics.median(ev), 4), "event_ms_p10": round(q[0], 4),
                                 "event_ms_p90": round(q[-1], 4), "host_ms_median": round(statistics.median(host), 4),
                                 "calls": len(ev)}
    for s in ("S1", "S32"):
        for kind in ("by_hand_warm", "by_hand_cold"):
            result[f"{kind}_over_boxed_{s}"] = round(result[kind][s]["event_ms_median"] / result["boxed"][s]["event_ms_median"], 3)
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
