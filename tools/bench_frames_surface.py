"""Per-tick latency of ``FrameStream.push`` on frames read in place -- BGR, a pitched NV12 decoder surface, YUYV -- against
what a caller had to do before those were pixel formats and layouts: a full-frame torch pass, then the push that existed.

    python tools/bench_frames_surface.py [--reps 50] [--rounds 4] [--out profiles/frames_surface_latency.json]

Settings: S in {1, 32} streams, one tick per call: one frame per stream already on the device, 48 -> 40 crop; a pool of ``POOL``
ticks cycles.  (a) - (c) are boxed pushes of 1280 x 720 pictures, one face box per frame with sides 150 .. 400 inside the frame,
new every tick; (d) is the unboxed push of 256 x 256 pictures.
  (a) ``bgr``          ``FrameStream(pixel_format="bgr24").push(frames, counts, boxes)``
      ``flip_rgb``     ``frames.flip(-1).contiguous()``, then the boxed ``rgb24`` push
  (b) ``nv12_pitch``   the boxed ``nv12`` push of surfaces [M, 1080, 1536] with ``layout=`` (row pitch 1536)
      ``repack_nv12``  ``surfaces[:, :, :1280].contiguous()``, then the boxed ``nv12`` push of the tight frames
  (c) ``yuyv``         the boxed ``yuyv422`` push
      ``torch_rgb``    YUYV -> RGB with torch ops (the integers of ``yuv_coefficients``), then the boxed ``rgb24`` push
  (d) ``bgr_256``      the unboxed ``bgr24`` push: the per-pixel staging branch of ``frames_transform_kernel``
      ``rgb_256``      the unboxed ``rgb24`` push of the same pictures: the 16-byte staging branch
Before timing, the rings of the two sides of every pair are compared for equality over the pool.  Each figure is the median
over ``rounds * reps`` (200) single calls of the time between two HIP events around ONE call, after warm-up, all cases
alternating round by round in the same process; p10, p90 and the host-clock median (call + synchronise) are kept next to it.
Streams are reset between calls (host ints only).  No gate: the new calls have no counterpart to be held to; the ratios are
reported.  Prints one JSON line and writes it to ``--out``.  Needs the GPU.
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

H, W, PITCH, SMALL, POOL, LO, HI = 720, 1280, 1536, 256, 8, 150, 400
PAIRS = (("bgr", "flip_rgb"), ("nv12_pitch", "repack_nv12"), ("yuyv", "torch_rgb"), ("bgr_256", "rgb_256"))


def yuyv_to_rgb(yuyv, coef):
    """uint8 [n, H, W, 2] -> uint8 [n, H, W, 3] with torch ops: what a caller writes without the format."""
    cy, crv, cgu, cgv, cbu, yoff = coef
    n, h, w, _ = yuyv.shape
    c = (yuyv[..., 0].to(torch.int32) - yoff) * cy + (1 << 13)
    uv = yuyv.view(n, h, w // 2, 4)[..., 1::2].to(torch.int32) - 128
    uv = uv.repeat_interleave(2, dim=2)
    u, v = uv[..., 0], uv[..., 1]
    rgb = torch.stack([c + crv * v, c + cgu * u + cgv * v, c + cbu * u], dim=-1) >> 14
    return rgb.clamp_(0, 255).to(torch.uint8)


def make_case(streams, g, rng):
    from feature_vs_text_compound_emotion_amd.frames import FrameStream, surface_layout, yuv_coefficients
    coef = yuv_coefficients()
    rand = lambda *shape: torch.randint(0, 256, (POOL, streams, *shape), device="cuda", generator=g, dtype=torch.uint8)  # noqa: E731
    bgr, surf, yuyv, small = rand(H, W, 3), rand(H * 3 // 2, PITCH), rand(H, W, 2), rand(SMALL, SMALL, 3)
    small_rgb = small.flip(-1).contiguous()
    layout = surface_layout("nv12", H, W, pitch=PITCH)
    assert layout.frame_stride == H * 3 // 2 * PITCH
    boxes = []
    for _ in range(POOL):
        tick = []
        for _ in range(streams):
            bw, bh = rng.randint(LO, HI), rng.randint(LO, HI)
            x0, y0 = rng.randint(0, W - bw), rng.randint(0, H - bh)
            tick.append((x0, y0, x0 + bw, y0 + bh))
        boxes.append(tick)
    fmt = {"bgr": "bgr24", "flip_rgb": "rgb24", "nv12_pitch": "nv12", "repack_nv12": "nv12", "yuyv": "yuyv422", "torch_rgb": "rgb24",
           "bgr_256": "bgr24", "rgb_256": "rgb24"}
    fs = {k: FrameStream(streams, max_new=1, pixel_format=f) for k, f in fmt.items()}
    state = dict.fromkeys(fs, 0)
    counts = [1] * streams

    def push(kind):
        t = state[kind] % POOL
        state[kind] += 1
        s = fs[kind]
        s.reset()
        if kind == "bgr":
            s.push(bgr[t], counts, boxes[t])
        elif kind == "flip_rgb":
            s.push(bgr[t].flip(-1).contiguous(), counts, boxes[t])
        elif kind == "nv12_pitch":
            s.push(surf[t], counts, boxes[t], layout=layout)
        elif kind == "repack_nv12":
            s.push(surf[t][:, :, :W].contiguous(), counts, boxes[t])
        elif kind == "yuyv":
            s.push(yuyv[t], counts, boxes[t])
        elif kind == "torch_rgb":
            s.push(yuyv_to_rgb(yuyv[t], coef), counts, boxes[t])
        elif kind == "bgr_256":
            s.push(small[t], counts)
        else:
            s.push(small_rgb[t], counts)

    def rings_equal():
        pairs = [(s, 0) for s in range(streams)]
        return all(torch.equal(fs[a].take(pairs), fs[b].take(pairs)) for a, b in PAIRS)

    return push, rings_equal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2 * POOL)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_surface_latency.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frames_surface.py measures on the GPU; none is visible")
    g, rng = torch.Generator(device="cuda").manual_seed(5), random.Random(5)
    kinds = [k for pair in PAIRS for k in pair]
    result = {"frame": [H, W], "nv12_pitch": PITCH, "unboxed_frame": [SMALL, SMALL], "size": 48, "crop": 40, "box_sides": [LO, HI],
              "pool_ticks": POOL, "reps": a.reps, "rounds": a.rounds, "matrix": "bt601", "range": "limited", "cases": {k: {} for k in kinds}}
    cases, compared = {}, 0
    for s in (1, 32):
        push, rings_equal = make_case(s, g, rng)
        for _ in range(max(a.warmup, POOL)):      # every tick of the pool is seen here, and the rings are compared
            for k in kinds:
                push(k)
            if not rings_equal():
                raise SystemExit(f"S = {s}: a push of frames read in place and its comparison path differ")
            compared += s
        for k in kinds:
            cases[f"{k}_S{s}"] = lambda f=push, k=k: f(k)
    result["frames_compared_equal"] = compared
    samples = {name: ([], []) for name in cases}
    for _ in range(a.rounds):           # alternate the cases: a drift of the machine hits all alike
        for name, fn in cases.items():
            ev, host = timed(fn, a.reps)
            samples[name][0].extend(ev)
            samples[name][1].extend(host)
    for name in cases:
        kind, s = name.rsplit("_S", 1)
        ev, host = samples[name]
        q = statistics.quantiles(ev, n=10)
        result["cases"][kind]["S" + s] = {"event_ms_median": round(statistics.median(ev), 4), "event_ms_p10": round(q[0], 4),
                                          "event_ms_p90": round(q[-1], 4), "host_ms_median": round(statistics.median(host), 4),
                                          "calls": len(ev)}
    for new, old in PAIRS:
        for s in ("S1", "S32"):
            result[f"{old}_over_{new}_{s}"] = round(result["cases"][old][s]["event_ms_median"] / result["cases"][new][s]["event_ms_median"], 3)
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
