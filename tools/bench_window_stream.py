"""Latency of one ``WindowStream.push`` tick under the reference's window rule (W = 300, H = 200), and the encoder work it saves.

    python tools/bench_window_stream.py [--reps 20] [--rounds 5] [--out profiles/window_stream_latency.json]

A tick brings one 40 x 40 frame (through IR-50), one VGGish row and, for the LFAN, one BERT row per stream, for S = 1 and S = 32
streams in lockstep, to a tri-modal LFAN and to a JMT (random weights, fp32, ``encoder_batch`` = 8, ``max_new`` = 32).

  idle      the streams stand at frame 450: the tick completes no window.  It encodes the frame, appends the embedding rows
            and emits frame 150 of every stream (one stitch launch).
  complete  the streams stand at frame 499: the tick completes window 1 ([200, 500)) of EVERY stream at once, the worst case of
            lockstep streams: S windows of 300 rows go through the model (one per call for the JMT and for the LFAN at
            ``window_batch`` = 1; the LFAN at S = 32 is also timed at ``window_batch`` = 8), then frame 199 is emitted.

Before each call the stream's host ints are set back (the rings keep their rows), so every call is the same tick.  Each figure
is the median over ``rounds * reps`` single calls between two HIP events, after warm-up, with p10 - p90, the cases alternating
round by round in the same process; the host-clock median (call + synchronise) stands next to it.  Launches are counted as
C-ABI calls through ``ops``.

``encoder_frames`` are counts, not timings: the frames IR-50 sees for an n-frame video, n here (each frame once) against
W x len(windowing(range(n), W, H)) in the offline evaluator.  Prints one JSON line and writes it to ``--out``.  Needs the GPU.
"""
import argparse
import json
import os
import statistics
import sys

sys.modules.setdefault("triton", None)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from bench_live import build_model, count_calls  # noqa: E402
from bench_stream import timed  # noqa: E402

W, H, HW = 300, 200, 40
IDLE, COMPLETE = 450, 499            # frames a stream has seen before the tick


def encoder_frames(lengths=(300, 900, 1800, 9000)):
    import numpy as np

    from feature_vs_text_compound_emotion_amd.trainer import windowing
    return {str(n): {"live": n, "offline": W * len(windowing(np.arange(n), W, H))} for n in lengths}


def build_jmt():
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.fusion_heads import JMT
    mods = ["video", "vggish"]
    spec, alias = synth.jmt_spec(mods, "JMT")
    m = JMT(task="CLASSIFICATION", modalities=mods, tcn_settings=synth.TCN_SETTINGS, backbone_settings={}, output_dim=7,
            root_dir="", device="cuda", model_name="JMT", load_backbone=False)
    m.load_state_dict(synth.make_state_dict(spec, alias, seed=3), strict=True)
    return m.cuda().eval()


def make_case(model, streams, seen, window_batch, g):
    from feature_vs_text_compound_emotion_amd.window_stream import WindowStream
    stream = WindowStream(model, streams, W, H, max_new=32, encoder_batch=8, window_batch=window_batch)
    for ring in stream.rings.values():
        ring.normal_(generator=g)
    X = {}
    for m in stream.modalities:
        X[m] = (torch.randn((streams, 1, 3, HW, HW), device="cuda", generator=g) if m == "video" else
                torch.randn((streams, 1, 1, stream.dims[m]), device="cuda", generator=g))
    done = (seen - W) // H + 1

    def call():
        stream.frames_seen, stream.emitted = [seen] * streams, [seen - W] * streams
        stream.windows_done = [done] * streams
        logits, counts = stream.push(X)
        assert counts == [1] * streams and stream.windows_done == [(seen + 1 - W) // H + 1] * streams
        return logits
    return call, stream


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_stream_latency.json"))
    a = ap.parse_args()
    result = {"window_length": W, "hop_length": H, "frame": [HW, HW], "max_new": 32, "encoder_batch": 8, "reps": a.reps,
              "rounds": a.rounds, "encoder_frames": encoder_frames()}
    if not torch.cuda.is_available():
        raise SystemExit("bench_window_stream.py measures on the GPU; none is visible")
    g = torch.Generator(device="cuda").manual_seed(11)
    models = {"lfan": build_model()[0], "jmt": build_jmt()}
    cases = {}
    for name, model in models.items():
        for s in (1, 32):
            for kind, seen in (("idle", IDLE), ("complete", COMPLETE)):
                cases[f"{name}_S{s}_{kind}"], stream = make_case(model, s, seen, 1, g)
            result[f"{name}_S{s}_state"] = {"ring_frames": stream.ring_frames, "ring_windows": stream.ring_windows,
                                            "wring_bytes": stream.wring.numel() * 4,
                                            "embedding_ring_bytes": sum(r.numel() * 4 for r in stream.rings.values())}
    cases["lfan_S32_complete_window_batch8"], _ = make_case(models["lfan"], 32, COMPLETE, 8, g)
    for fn in cases.values():
        for _ in range(a.warmup):
            fn()
    samples = {name: ([], []) for name in cases}
    for _ in range(a.rounds):           # alternate the cases: a drift of the machine hits all alike
        for name, fn in cases.items():
            ev, host = timed(fn, a.reps)
            samples[name][0].extend(ev)
            samples[name][1].extend(host)
    for name, fn in cases.items():
        made = count_calls(fn)[0]
        ev, host = samples[name]
        q = statistics.quantiles(ev, n=10)
        result[name] = {"event_ms_median": round(statistics.median(ev), 4), "event_ms_p10": round(q[0], 4),
                        "event_ms_p90": round(q[-1], 4), "host_ms_median": round(statistics.median(host), 4),
                        "launches": len(made), "entries": {m[len("cer_"):]: made.count(m) for m in dict.fromkeys(made)}}
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
