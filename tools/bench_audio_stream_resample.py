"""Per-tick latency of the streaming audio front end on 48 kHz stereo PCM (``LogMelStream(resample=...).push``) against what a
caller could do before it: resample and log-mel each stream's last 0.975 s of audio plus the filter's reach again for every
video frame and frame the one newest example.

    python tools/bench_audio_stream_resample.py [--rate 48000] [--channels 2] [--filter kaiser_best] [--reps 200] [--rounds 5]
                                                [--out profiles/audio_stream_resample_latency.json]

Settings: S in {1, 32} streams, one tick of 30 fps video per call: rate / 30 input frames per stream (1600 at 48 kHz), which
completes 533 or 534 samples at 16 kHz, 3 or 4 STFT rows and one example per stream.  Streamed: one ``LogMelStream.push`` (one
table upload, four launches).  Alternative: the launches ``VGGish.wav_int16_to_examples(resample=...)`` is made of, without
its second of padding, over a contiguous copy of the window of every stream: ``ops.resample_pcm`` (160 samples of lead-in at
16 kHz so that the filter's reach before the window is real signal, the 15 600 samples of the example, and the J + 1 input
frames after them), ``ops.logmel_f64`` and ``ops.frame_examples`` for the example at row 1 (one start upload, one copy, three
launches).  The PCM of both sides is already on the device.  Before timing, every example the stream emits over the first two
seconds is compared for equality with the alternative run over that example's own window.  Each figure is the median over
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

from bench_audio_stream import count_calls  # noqa: E402
from bench_stream import timed  # noqa: E402

FPS, WINDOW_SAMPLES, WIN, LEAD = 30, 15600, 96, 160
HOP_SEC = 1.0 / FPS


class Recompute:
    """The alternative: the newest example of every stream from a window of its PCM, with the offline launches."""

    def __init__(self, rate, filter, mel):
        from feature_vs_text_compound_emotion_amd.audio_backbone import resample_taps
        taps, self.L, self.M = resample_taps(rate, filter)
        self.taps, self.T, self.mel = torch.from_numpy(taps).cuda().contiguous(), taps.shape[1], mel
        if (LEAD * self.M) % self.L or LEAD * self.M // self.L < (self.T - 2) // 2:
            raise SystemExit(f"the {LEAD}-sample lead-in is no whole number of input frames at this rate, or shorter than the "
                             "filter's reach")
        self.n_out = LEAD + WINDOW_SAMPLES
        self.frames = ((self.n_out - 1) * self.M) // self.L + self.T // 2 + 1      # up to the last output's input q + J + 1

    def first_frame(self, start_row):
        """Input frame at which the window of the example that starts at STFT row ``start_row`` (>= 1) begins."""
        return (160 * start_row - LEAD) * self.M // self.L

    def __call__(self, window):
        from feature_vs_text_compound_emotion_amd import ops
        samples = ops.resample_pcm(window, window.dim() == 3, 0, self.taps, self.L, self.M, self.n_out)
        return ops.frame_examples(ops.logmel_f64(samples, self.mel, 0.01), [1], WIN)


def check_equal(rate, channels, filter, alt):
    """Two seconds of two streams, tick by tick: each streamed example equals the alternative over its own window."""
    from feature_vs_text_compound_emotion_amd.audio_stream import LogMelStream
    tick = rate // FPS
    g = torch.Generator(device="cuda").manual_seed(1)
    pcm = (torch.randn(2, 2 * rate, channels, device="cuda", generator=g) * 3000.0).round().clamp(-32768, 32767).to(torch.int16)
    pcm = pcm if channels > 1 else pcm[:, :, 0].contiguous()
    stream = LogMelStream(2, HOP_SEC, max_samples=tick, sample_rate=rate, channels=channels, resample=filter)
    at, seen, compared = 0, [0, 0], 0
    for _ in range(2 * FPS):
        ex, counts = stream.push(torch.cat([pcm[0, at:at + tick], pcm[1, at:at + tick]]), [tick, tick])
        at += tick
        row = 0
        for s, c in enumerate(counts):
            for _ in range(c):
                start = round(stream.hop_frames * seen[s])
                if start >= 1:      # example 0 has no lead-in: zeros stand before the signal
                    first = alt.first_frame(start)
                    want = alt(pcm[s:s + 1, first:first + alt.frames].contiguous())[0, 0]
                    if not torch.equal(ex[row], want):
                        raise SystemExit(f"streamed example {seen[s]} of stream {s} differs from the alternative over its window")
                    compared += 1
                seen[s], row = seen[s] + 1, row + 1
    return compared


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--filter", default="kaiser_best")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_stream_resample_latency.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_audio_stream_resample.py measures on the GPU; none is visible")
    if a.rate % FPS:
        raise SystemExit(f"--rate must be a multiple of {FPS}: one tick is rate / {FPS} frames")
    from feature_vs_text_compound_emotion_amd.audio_backbone import mel_matrix
    from feature_vs_text_compound_emotion_amd.audio_stream import LogMelStream
    mel = torch.from_numpy(mel_matrix()).cuda().contiguous()
    alt = Recompute(a.rate, a.filter, mel)
    tick = a.rate // FPS
    result = {"fps": FPS, "rate": a.rate, "channels": a.channels, "filter": a.filter, "frames_per_tick": tick,
              "window_frames": alt.frames, "reps": a.reps, "rounds": a.rounds,
              "examples_compared_equal": check_equal(a.rate, a.channels, a.filter, alt), "stream": {}, "recompute": {}}
    calls = a.warmup + a.reps * a.rounds + 1
    g = torch.Generator(device="cuda").manual_seed(3)
    cases, state = {}, {}
    for s in (1, 32):
        # a circular second and a half of noise per stream: the timing does not depend on the values
        period = alt.frames + 8 * tick
        pcm = (torch.randn(s, period, a.channels, device="cuda", generator=g) * 3000.0).round().clamp(-32768, 32767)
        pcm = pcm.to(torch.int16)
        pcm = pcm if a.channels > 1 else pcm[:, :, 0].contiguous()
        ticks = [pcm[:, k * tick:(k + 1) * tick].reshape((-1,) + tuple(pcm.shape[2:])).contiguous() for k in range(8)]
        stream = LogMelStream(s, HOP_SEC, max_samples=tick, sample_rate=a.rate, channels=a.channels, resample=a.filter)
        state[s] = {"stream_tick": 0, "recompute_tick": 0}

        def push(s=s, stream=stream, ticks=ticks):
            t = state[s]["stream_tick"]
            state[s]["stream_tick"] = t + 1
            return stream.push(ticks[t % 8], [tick] * s)

        def recompute(s=s, pcm=pcm):
            t = state[s]["recompute_tick"]
            state[s]["recompute_tick"] = t + 1
            first = (t % 8) * tick
            return alt(pcm[:, first:first + alt.frames].contiguous())

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
