"""Per-tick latency of ``FrameStream.push_aligned(frames, counts, affines)`` on full camera frames against the closest existing
kernel and against what a caller does without it.

    python tools/bench_frames_align.py [--reps 200] [--rounds 5] [--out profiles/frames_align.json]

Settings: S in {1, 32} streams, one tick per call: one 1280 x 720 frame per stream, ``align_size`` 256 -> 48 -> 40 crop, five
landmarks per frame of a face 150 .. 400 pixels wide, turned by up to 20 degrees, that changes every tick; a pool of ``POOL``
ticks cycles.  Three methods:

  aligned   ``push_aligned`` with ``similarity_from_landmarks`` of the landmarks (the fit is inside the timed region);
  boxed     ``push(..., boxes=)`` of the same frames with the axis-aligned box of the same face: the closest existing kernel;
  pillow    the alternative without the kernel: ``PIL.Image.transform`` warps every frame on the host (the frames are host
            arrays there, as a capture hands them out), one upload of the faces, and a plain ``push``.

Before timing, the rings of ``aligned`` and ``pillow`` are compared for equality over one cycle of the pool.  Each figure is the
median over ``rounds * reps`` calls of the time between two HIP events around ONE call, after warm-up, the methods alternating
round by round in the same process; the host-clock median (call + synchronise) is kept next to it.  Streams are reset between
calls (host ints only), inside the call.  Also records VGPRs, SGPRs, LDS and scratch of the four kernel instances from the
compiler's ``-Rpass-analysis=kernel-resource-usage`` and the LDS bytes one block asks for.  Prints one JSON line and writes it
to ``--out``.  Needs the GPU.
"""
import argparse
import json
import math
import os
import random
import re
import statistics
import subprocess
import sys
import tempfile

sys.modules.setdefault("triton", None)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_stream import timed  # noqa: E402

H, W, POOL, LO, HI, ALIGN = 720, 1280, 8, 150, 400, 256


def make_case(streams, g, rng):
    from PIL import Image
    from feature_vs_text_compound_emotion_amd.frames import ARCFACE_TEMPLATE, FrameStream, similarity_from_landmarks
    video = torch.randint(0, 256, (POOL, streams, H, W, 3), device="cuda", generator=g, dtype=torch.uint8)
    host = video.cpu().numpy()
    template = np.array(ARCFACE_TEMPLATE) * ALIGN / 112.0 - ALIGN / 2
    landmarks, boxes = [], []
    for _ in range(POOL):
        lm, bx = [], []
        for _ in range(streams):
            side, angle = rng.randint(LO, HI), math.radians(rng.uniform(-20, 20))
            cx, cy = rng.uniform(side / 2, W - side / 2), rng.uniform(side / 2, H - side / 2)
            c, s = math.cos(angle) * side / ALIGN, math.sin(angle) * side / ALIGN
            lm.append(np.stack([cx + c * template[:, 0] - s * template[:, 1], cy + s * template[:, 0] + c * template[:, 1]], axis=1))
            x0, y0 = int(cx - side / 2), int(cy - side / 2)
            bx.append((x0, y0, x0 + side, y0 + side))
        landmarks.append(np.stack(lm))
        boxes.append(bx)
    fs = {kind: FrameStream(streams, max_new=1) for kind in ("aligned", "boxed", "pillow")}
    state = dict.fromkeys(fs, 0)

    def tick(kind):
        t = state[kind] % POOL
        state[kind] += 1
        fs[kind].reset()
        return t

    def push_aligned():
        t = tick("aligned")
        fs["aligned"].push_aligned(video[t], [1] * streams, similarity_from_landmarks(landmarks[t], ALIGN), ALIGN)

    def push_boxed():
        t = tick("boxed")
        fs["boxed"].push(video[t], [1] * streams, boxes[t])

    def push_pillow():
        t = tick("pillow")
        a = similarity_from_landmarks(landmarks[t], ALIGN)
        faces = np.stack([np.asarray(Image.fromarray(host[t, s]).transform((ALIGN, ALIGN), Image.AFFINE, tuple(a[s]),
                                                                            resample=Image.BILINEAR)) for s in range(streams)])
        fs["pillow"].push(torch.from_numpy(faces).cuda(), [1] * streams)

    def rings_equal():
        pairs = [(s, 0) for s in range(streams)]
        return torch.equal(fs["aligned"].take(pairs), fs["pillow"].take(pairs))

    return {"aligned": push_aligned, "boxed": push_boxed, "pillow": push_pillow}, rings_equal


def kernel_resources():
    """{kernel instance: {vgprs, sgprs, scratch_bytes_per_lane, static_lds_bytes, occupancy}} of csrc/frames_affine.hip."""
    from feature_vs_text_compound_emotion_amd import build
    src = os.path.join(build.CSRC, "frames_affine.hip")
    with tempfile.TemporaryDirectory() as tmp:
        done = subprocess.run([build.HIPCC, *build.FLAGS, "-c", src, "-o", os.path.join(tmp, "frames_affine.o"),
                               "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    if done.returncode != 0:
        return {"error": done.stderr[-500:]}
    out, name = {}, None
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "LDS Size [bytes/block]": "static_lds_bytes", "Occupancy [waves/SIMD]": "occupancy"}
    for line in done.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            place = "ring" if "AffineRingPlace" in m.group(1) else "clip"
            name = f"{place}_{'yuv420' if 'px_yuv420' in m.group(1) else 'rgb24'}"
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+)", line)
        if m and name and m.group(1) in keys:
            out[name][keys[m.group(1)]] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2 * POOL)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_align.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frames_align.py measures on the GPU; none is visible")
    from feature_vs_text_compound_emotion_amd import frames
    geom = frames.affine_geometry(ALIGN, 48)
    g, rng = torch.Generator(device="cuda").manual_seed(5), random.Random(5)
    result = {"frame": [H, W], "align_size": ALIGN, "size": 48, "crop": 40, "face_sides": [LO, HI], "pool_ticks": POOL,
              "reps": a.reps, "rounds": a.rounds,
              "geometry": {"ksize": geom.ks, "max_band_rows": geom.span, "dynamic_lds_bytes": geom.lds_bytes(40)},
              "kernel_resources": kernel_resources(), "aligned": {}, "boxed": {}, "pillow": {}}
    cases, compared = {}, 0
    for s in (1, 32):
        methods, rings_equal = make_case(s, g, rng)
        for _ in range(max(a.warmup, POOL)):      # every tick of the pool is seen here, and the kernel is held to Pillow
            for fn in methods.values():
                fn()
            if not rings_equal():
                raise SystemExit(f"S = {s}: push_aligned and the faces Pillow warped differ")
            compared += s
        for kind, fn in methods.items():
            cases[f"{kind}_S{s}"] = fn
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
        for kind in ("boxed", "pillow"):
            result[f"aligned_over_{kind}_{s}"] = round(result["aligned"][s]["event_ms_median"] / result[kind][s]["event_ms_median"], 3)
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
