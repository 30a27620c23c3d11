"""Time of the VGGish front end (PCM -> log-mel examples, ``VGGish.wav_int16_to_examples``) for a batch of clips: 16 kHz mono
(the int16 log-mel alone) beside other rates and channel counts (mixdown + resampling + the float64 log-mel).  Timed with
device events around ``--iters`` calls after ``--warmup`` calls of the same shape; prints one JSON line per configuration.

    python tools/bench_audio_frontend.py [--clips 32 --seconds 1.0 --iters 50 --warmup 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.modules.setdefault("triton", None)

import torch  # noqa: E402

CONFIGS = [(16000, 1, None), (16000, 2, "kaiser_best"), (48000, 2, "kaiser_best"), (48000, 2, "kaiser_fast"),
           (44100, 2, "kaiser_best"), (8000, 1, "kaiser_best")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_audio_frontend.py needs the GPU: a CPU run measures nothing")
    from feature_vs_text_compound_emotion_amd.audio_backbone import VGGish
    net = VGGish().cuda()
    g = torch.Generator().manual_seed(0)
    for sr, ch, filt in CONFIGS:
        shape = (args.clips, int(args.seconds * sr)) + ((ch,) if ch > 1 else ())
        pcm = torch.clamp(torch.round(torch.randn(shape, generator=g) * 3000.0), -32768, 32767).to(torch.int16).cuda()
        for _ in range(args.warmup):
            ex = net.wav_int16_to_examples(pcm, sr, 0.96, 1.0 / 32, resample=filt)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.iters):
            ex = net.wav_int16_to_examples(pcm, sr, 0.96, 1.0 / 32, resample=filt)
        stop.record()
        stop.synchronize()
        print(json.dumps({"sample_rate": sr, "channels": ch, "resample": filt, "clips": args.clips, "seconds": args.seconds,
                          "examples": list(ex.shape), "iters": args.iters,
                          "ms_per_call": round(start.elapsed_time(stop) / args.iters, 4)}), flush=True)


if __name__ == "__main__":
    main()
