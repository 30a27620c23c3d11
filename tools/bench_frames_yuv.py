"""Per-tick latency of a boxed ``FrameStream.push`` of NV12 camera frames against the same pictures pushed as RGB, and against
what a caller had to do before the 4:2:0 pixel formats: convert every full frame to RGB with torch ops, then push.

    python tools/bench_frames_yuv.py [--reps 200] [--rounds 5] [--out profiles/frames_yuv_latency.json]

Settings: S in {1, 32} streams, one tick per call: one 1280 x 720 frame per stream already on the device, 48 -> 40 crop, one
face box per frame with sides 150 .. 400 inside the frame, new every tick; a pool of ``POOL`` ticks cycles.  Three methods:
``nv12`` -- ``FrameStream(pixel_format="nv12").push(frames, counts, boxes)``; ``rgb`` -- the same pictures, converted
beforehand (outside the timed region), through the RGB boxed push; ``torch_then_rgb`` -- the conversion written with torch ops
(the integers of ``yuv_coefficients``, nearest chroma) inside the timed region, followed by the RGB boxed push.  Before timing,
the rings of ``nv12`` and ``rgb`` are compared for equality over the pool (the RGB frames come from the torch conversion, so
this also holds the kernel's conversion equal to it).  Each figure is the median over ``rounds * reps`` calls of the time between
two HIP events around ONE call, after warm-up, the methods alternating round by round in the same process; p10, p90 and the
host-clock median (call + synchronise) are kept next to it.  Streams are reset between calls (host ints only).  The gate:
``nv12`` at most 1.25 x ``rgb`` at both S.  Prints one JSON line and writes it to ``--out``.  Needs the GPU.
"""
import argparse
import json
import os
import random
import statistics
import sys

sys.modules.setdefault("triton", None)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from bench_stream import timed  # noqa: E402

H, W, POOL, LO, HI, GATE = 720, 1280, 8, 150, 400, 1.25


def nv12_to_rgb(nv12, coef):
    """uint8 [n, H * 3 / 2, W] -> uint8 [n, H, W, 3] with torch ops: what a caller writes today."""
    cy, crv, cgu, cgv, cbu, yoff = coef
    n, rows, w = nv12.shape
    h = rows // 3 * 2
    c = (nv12[:, :h].to(torch.int32) - yoff) * cy + (1 << 13)
    uv = nv12[:, h:].reshape(n, h // 2, w // 2, 2).to(torch.int32) - 128
    uv = uv.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    u, v = uv[..., 0], uv[..., 1]
    rgb = torch.stack([c + crv * v, c + cgu * u + cgv * v, c + cbu * u], dim=-1) >> 14
    return rgb.clamp_(0, 255).to(torch.uint8)


def make_case(streams, g, rng):
    from feature_vs_text_compound_emotion_amd.frames import FrameStream, yuv_coefficients
    coef = yuv_coefficients()
    nv12 = torch.randint(0, 256, (POOL, streams, H * 3 // 2, W), device="cuda", generator=g, dtype=torch.uint8)
    rgb = torch.stack([nv12_to_rgb(tick, coef) for tick in nv12])
    boxes = []
    for _ in range(POOL):
        tick = []
        for _ in range(streams):
            bw, bh = rng.randint(LO, HI), rng.randint(LO, HI)
            x0, y0 = rng.randint(0, W - bw), rng.randint(0, H - bh)
            tick.append((x0, y0, x0 + bw, y0 + bh))
        boxes.append(tick)
    fs = {"nv12": FrameStream(streams, max_new=1, pixel_format="nv12"), "rgb": FrameStream(streams, max_new=1),
          "torch_then_rgb": FrameStream(streams, max_new=1)}
    state = dict.fromkeys(fs, 0)

    def push(kind):
        t = state[kind] % POOL
        state[kind] += 1
        fs[kind].reset()
        if kind == "nv12":
            fs[kind].push(nv12[t], [1] * streams, boxes[t])
        else:
            fs[kind].push(rgb[t] if kind == "rgb" else nv12_to_rgb(nv12[t], coef), [1] * streams, boxes[t])

    def rings_equal():
        pairs = [(s, 0) for s in range(streams)]
        a, b, c = (fs[k].take(pairs) for k in ("nv12", "rgb", "torch_then_rgb"))
        return torch.equal(a, b) and torch.equal(a, c)

    return push, rings_equal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3 * POOL)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_yuv_latency.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frames_yuv.py measures on the GPU; none is visible")
    g, rng = torch.Generator(device="cuda").manual_seed(5), random.Random(5)
    kinds = ("nv12", "rgb", "torch_then_rgb")
    result = {"frame": [H, W], "size": 48, "crop": 40, "box_sides": [LO, HI], "pool_ticks": POOL, "reps": a.reps, "rounds": a.rounds,
              "matrix": "bt601", "range": "limited", "gate": GATE, **{k: {} for k in kinds}}
    cases, compared = {}, 0
    for s in (1, 32):
        push, rings_equal = make_case(s, g, rng)
        for _ in range(max(a.warmup, POOL)):      # every tick of the pool is seen here, and the rings are compared
            for k in kinds:
                push(k)
            if not rings_equal():
                raise SystemExit(f"S = {s}: the NV12 push and the RGB push of the converted frames differ")
            compared += s
        for k in kinds:
            cases[f"{k}_S{s}"] = lambda f=push, k=k: f(k)
    result["frames_compared_equal"] = compared
    samples = {name: ([], []) for name in cases}
    for _ in range(a.rounds):           # alternate the methods: a drift of the machine hits all alike
        for name, fn in cases.items():
            ev, host = timed(fn, a.reps)
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
        med = {k: result[k][s]["event_ms_median"] for k in kinds}
        result[f"nv12_over_rgb_{s}"] = round(med["nv12"] / med["rgb"], 3)
        result[f"torch_then_rgb_over_nv12_{s}"] = round(med["torch_then_rgb"] / med["nv12"], 3)
    result["gate_met"] = all(result[f"nv12_over_rgb_{s}"] <= GATE for s in ("S1", "S32"))
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
