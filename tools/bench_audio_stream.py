"""Per-tick latency of the streaming audio front end (``LogMelStream.push``) against what a caller could do before it: re-run
the offline log-mel over each stream's last 0.975 s of audio (15 600 samples, 96 STFT rows) for every video frame and frame
the one newest example.

    python tools/bench_audio_stream.py [--reps 200] [--rounds 5] [--out profiles/audio_stream_latency.json]

Settings: S in {1, 32} streams, one tick of 30 fps video per call: 533 or 534 new samples per stream (16 000 / 30), which
completes 3 or 4 STFT rows and one example per stream.  Streamed: one ``LogMelStream.push`` (one table upload, three launches).
Alternative: ``ops.logmel`` with pad 0 over a contiguous copy of the last 15 600 samples of every stream, then
``ops.frame_examples`` for the example at row 0 (one start upload, one copy, two launches).  The PCM of both sides is already on
the device, so neither pays for moving samples.  Before timing, every example the stream emits over the first two seconds is
compared for equality with the alternative run over that example's own 15 600 samples.  Each figure is the median over
``rounds * reps`` calls of the time between two HIP events around ONE call, after warm-up, the two methods alternating round by
round in the same process; the host-clock median (call + synchronise) is kept next to it.  Launches are counted as C-ABI calls
(each is one kernel launch).  Prints one JSON line and writes it to ``--out``.  Needs the GPU.
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

from bench_stream import timed  # noqa: E402

FPS, WINDOW_SAMPLES, WIN = 30, 15600, 96
HOP_SEC = 1.0 / FPS


def tick_sizes(n):
    """Samples per video frame at 30 fps: 16 000 t / 30 rounded down, differenced: 533, 533, 534, ..."""
    return [16000 * (t + 1) // FPS - 16000 * t // FPS for t in range(n)]


def count_calls(fn):
    from feature_vs_text_compound_emotion_amd import ops
    calls, real = [], ops.check

    def counting(rc, what):
        calls.append(what)
        return real(rc, what)
    ops.check = counting
    try:
        fn()
        torch.cuda.synchronize()
        return calls
    finally:
        ops.check = real


def check_equal(mel):
    """Two seconds of two streams, tick by tick: each streamed example equals the offline log-mel of its own window."""
    from feature_vs_text_compound_emotion_amd import ops, synth
    from feature_vs_text_compound_emotion_amd.audio_stream import LogMelStream
    pcm = torch.stack([synth.make_audio_int16(2.0, seed=s) for s in (1, 2)]).cuda()
    stream, at, seen, compared = LogMelStream(2, HOP_SEC, max_samples=1024), 0, [0, 0], 0
    for n in tick_sizes(2 * FPS):
        ex, counts = stream.push(torch.cat([pcm[0, at:at + n], pcm[1, at:at + n]]), [n, n])
        at += n
        row = 0
        for s, c in enumerate(counts):
            for _ in range(c):
                start = round(stream.hop_frames * seen[s])
                window = pcm[s:s + 1, 160 * start:160 * start + WINDOW_SAMPLES].contiguous()
                want = ops.frame_examples(ops.logmel(window, 0, mel, 0.01), [0], WIN)[0, 0]
                if not torch.equal(ex[row], want):
                    raise SystemExit(f"streamed example {seen[s]} of stream {s} differs from the offline log-mel of its window")
                seen[s], row, compared = seen[s] + 1, row + 1, compared + 1
    return compared


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_stream_latency.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_audio_stream.py measures on the GPU; none is visible")
    from feature_vs_text_compound_emotion_amd import ops
    from feature_vs_text_compound_emotion_amd.audio_backbone import mel_matrix
    from feature_vs_text_compound_emotion_amd.audio_stream import LogMelStream
    mel = torch.from_numpy(mel_matrix()).cuda().contiguous()
    result = {"fps": FPS, "window_samples": WINDOW_SAMPLES, "reps": a.reps, "rounds": a.rounds,
              "examples_compared_equal": check_equal(mel), "stream": {}, "recompute": {}}
    calls = a.warmup + a.reps * a.rounds + 1
    sizes = tick_sizes(calls)
    g = torch.Generator(device="cuda").manual_seed(3)
    cases, state = {}, {}
    for s in (1, 32):
        pcm = (torch.randn(s, WINDOW_SAMPLES + sum(sizes), device="cuda", generator=g) * 3000.0).round().clamp(-32768, 32767)
        pcm = pcm.to(torch.int16)
        ends, at = [], WINDOW_SAMPLES
        for n in sizes:
            at += n
            ends.append(at)
        ticks = [pcm[:, e - n:e].reshape(-1).contiguous() for e, n in zip(ends, sizes)]      # stream-major packed chunks
        stream = LogMelStream(s, HOP_SEC, max_samples=1024)
        state[s] = {"stream_tick": 0, "recompute_tick": 0}

        def push(s=s, stream=stream, ticks=ticks):
            t = state[s]["stream_tick"]
            state[s]["stream_tick"] = t + 1
            return stream.push(ticks[t], [sizes[t]] * s)

        def recompute(s=s, pcm=pcm, ends=ends):
            t = state[s]["recompute_tick"]
            state[s]["recompute_tick"] = t + 1
            window = pcm[:, ends[t] - WINDOW_SAMPLES:ends[t]].contiguous()
            return ops.frame_examples(ops.logmel(window, 0, mel, 0.01), [0], WIN)

        cases[f"stream_S{s}"], cases[f"recompute_S{s}"] = push, recompute
    samples = {name: ([], []) for name in cases}
    for fn in cases.values():
        for _ in range(a.warmup):       # the streams also fill their first 0.975 s here: every timed push emits an example
            fn()
    for _ in range(a.rounds):           # alternate the methods: a drift of the machine hits both alike
        for name, fn in cases.items():
            ev, host = timed(fn, a.reps)
            samples[name][0].extend(ev)
            samples[name][1].extend(host)
    for name, fn in cases.items():
        made = count_calls(fn)
        ev, host = samples[name]
        q = statistics.quantiles(ev, n=10)
        kind, s = name.split("_S")
        result[kind]["S" + s] = {"event_ms_median": round(statistics.median(ev), 4), "event_ms_p10": round(q[0], 4),
                                 "event_ms_p90": round(q[-1], 4), "host_ms_median": round(statistics.median(host), 4),
                                 "launches": len(made), "entries": [m[len("cer_"):] for m in made],
                                 "extra": "one int32 table upload" if kind == "stream" else
                                          "one int32 start upload, one copy of the windows"}
    for s in ("S1", "S32"):
        st, re = result["stream"][s], result["recompute"][s]
        result[f"recompute_over_stream_{s}"] = round(re["event_ms_median"] / st["event_ms_median"], 2)
        result[f"stream_faster_{s}"] = st["event_ms_median"] < re["event_ms_median"]
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
