"""What the standardisation of the ``vggish`` / ``bert`` rows costs: on a live tick, and as a statistics pass behind the encoders.

    python tools/bench_feature_norm.py [--reps 100] [--rounds 3] [--out profiles/feature_norm_latency.json]

1. The tick.  S in {1, 32} streams, one tick of 30 fps video per call (one raw 256 x 256 frame and 533 or 534 samples of 16 kHz
   PCM per stream, 48 -> 40 crop, the tri-modal LFAN of tools/bench_live.py, synthetic weights), four sessions side by side:
     extra            ``bert`` rows handed over with the frames, no ``mean_std``: the tick as it was before ``mean_std`` existed
                      (with the argument left out the session runs the same launches on the same bits)
     extra_ms         the same with ``mean_std`` for ``vggish``: one ``cer_standardize_rows`` more per model call
     text             a ``TextStream`` leg (2-layer encoder; sentences of 16 frames are pushed ahead of the frames, outside
                      the timed call), no ``mean_std``
     text_ms          the same with ``mean_std`` for ``vggish`` and ``bert``: two launches more
   Before timing, each ``_ms`` session's logits over the warm-up are compared for equality with a twin built with statistics of
   (0, 1), whose logits in turn equal the plain session's.  Each figure is the median over ``rounds * reps`` ticks of the time
   between two HIP events around ONE ``push``, after warm-up, in the same process on the same card; the host-clock median
   (call + synchronise) is kept next to it.  Every session runs its tick t before any runs tick t + 1, in rotating order.  A
   tick pairs 0, 1 or 2 frames per stream, so tick times are bimodal and a difference of medians can land on either mode:
   the cost added by ``mean_std`` is the median of the per-tick differences (tick t pairs the same frames in both sessions).
2. The statistics pass.  ``feature_moments_update`` and ``standardize_rows`` on [9600, 768] and [9600, 128] rows (five minutes
   of 32 fps video), next to the encoder calls that make such rows: the 12-layer BERT on [150, 64] token ids, and VGGish on
   9600 examples (timed as one call of 960 examples, times ten).  Median of ``rounds * reps`` calls between two HIP events.

Prints one JSON line and writes it to ``--out``.  Needs the GPU.
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
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_audio_stream import tick_sizes  # noqa: E402
from bench_live import FPS, HW, POOL, build_model, count_calls  # noqa: E402
from bench_stream import timed  # noqa: E402

SPAN, TOKENS, MAX_TOKENS = 16, 12, 16      # a sentence: 10 words over 16 frames
ROWS = 9600


def stats(dims, unit=False, seed=9):
    rng = np.random.default_rng(seed)
    return {f: {"mean": np.zeros(c, np.float32) if unit else (rng.standard_normal(c) * 0.3).astype(np.float32),
                "std": np.ones(c, np.float32) if unit else rng.uniform(0.5, 2.0, c).astype(np.float32)} for f, c in dims.items()}


def make_session(model, audio, encoder, streams, sizes, g, text, mean_std):
    from feature_vs_text_compound_emotion_amd.live import AVStream
    from feature_vs_text_compound_emotion_amd.text_stream import TextStream
    video = torch.randint(0, 256, (POOL, streams, HW, HW, 3), device="cuda", generator=g, dtype=torch.uint8)
    bert = torch.randn((POOL, streams, 768), device="cuda", generator=g)
    pcm = (torch.randn(streams, sum(sizes), device="cuda", generator=g) * 3000.0).round().clamp(-32768, 32767).to(torch.int16)
    chunks, at = [], 0
    for n in sizes:
        chunks.append(pcm[:, at:at + n].reshape(-1).contiguous())
        at += n
    leg = TextStream(encoder, streams, max_tokens=MAX_TOKENS, sentence_batch=4) if text else None
    sess = AVStream(model, streams, FPS, max_samples=1024, audio_backbone=audio, text=leg, mean_std=mean_std)
    gs = torch.Generator().manual_seed(4)
    sentence = [101] + torch.randint(1000, 30000, (TOKENS - 2,), generator=gs).tolist() + [102]
    state = {"t": 0}

    def prepare():      # outside the timed call: keep the text a few frames ahead of the video
        if text and sess.text_seen[0] < sess.frames_seen[0] + 2:
            sess.push_text([(s, sentence, sess.text_seen[s], SPAN) for s in range(streams)])

    def tick():
        t = state["t"]
        state["t"] = t + 1
        extra = None if text else {"bert": bert[t % POOL]}
        return sess.push(video[t % POOL], [1] * streams, chunks[t], [sizes[t]] * streams, extra=extra)[0]

    return prepare, tick, sess


def timed_ticks(prepare, tick, reps):
    ev, host = [], []
    for _ in range(reps):
        prepare()
        e, h = timed(tick, 1)
        ev += e
        host += h
    return ev, host


def summary(ev, host):
    q = statistics.quantiles(ev, n=10)
    return {"event_ms_median": round(statistics.median(ev), 4), "event_ms_p10": round(q[0], 4), "event_ms_p90": round(q[-1], 4),
            "host_ms_median": round(statistics.median(host), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_norm_latency.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_feature_norm.py measures on the GPU; none is visible")
    from feature_vs_text_compound_emotion_amd import ops
    from feature_vs_text_compound_emotion_amd.text_encoder import BertEncoderHIP
    model, audio = build_model()
    torch.manual_seed(5)
    small = BertEncoderHIP(num_hidden_layers=2).cuda().eval()
    total = a.warmup + a.reps * a.rounds + 64
    sizes = tick_sizes(total)
    result = {"fps": FPS, "frame": [HW, HW], "crop": 40, "reps": a.reps, "rounds": a.rounds, "tick": {}, "passes": {}}
    cases = {}
    for s in (1, 32):
        for text in (False, True):
            dims = {"vggish": 128, "bert": 768} if text else {"vggish": 128}
            kind = "text" if text else "extra"
            made = {}
            for name, ms in ((kind, None), (kind + "_ms", stats(dims)), ("unit", stats(dims, unit=True))):
                g = torch.Generator(device="cuda").manual_seed(3)      # the same inputs for the three
                made[name] = make_session(model, audio, small, s, sizes, g, text, ms)
            # warm-up; statistics of (0, 1) leave the plain session's bits, and real ones do not
            same = other = 0
            for _ in range(a.warmup):
                out = {}
                for name, (prepare, tick, _) in made.items():
                    prepare()
                    out[name] = tick()
                if not torch.equal(out["unit"], out[kind]):
                    raise SystemExit(f"S = {s}, {kind}: statistics of (0, 1) changed the logits")
                same += out[kind].shape[0]
                other += int(out[kind].shape[0] > 0 and not torch.equal(out[kind + "_ms"], out[kind]))
            if not other:
                raise SystemExit(f"S = {s}, {kind}: mean_std changed nothing")
            result["tick"].setdefault("logit_rows_compared", 0)
            result["tick"]["logit_rows_compared"] += same
            for name in (kind, kind + "_ms"):
                cases[f"{name}_S{s}"] = made[name]
    samples = {name: ([], []) for name in cases}
    names = list(cases)
    for t in range(a.rounds * a.reps):      # every session runs its tick t before any runs t + 1, in rotating order
        for name in names[t % len(names):] + names[:t % len(names)]:
            prepare, tick, _ = cases[name]
            ev, host = timed_ticks(prepare, tick, 1)
            samples[name][0].extend(ev)
            samples[name][1].extend(host)
    for name, (prepare, tick, _) in cases.items():
        s = int(name.rsplit("_S", 1)[1])
        for _ in range(32):             # a tick that pairs exactly one frame per stream
            prepare()
            calls, out = count_calls(tick)
            if out.shape[0] == s:
                break
        result["tick"][name] = {**summary(*samples[name]), "launches": len(calls),
                                "standardize_rows": calls.count("cer_standardize_rows")}
    for s in ("S1", "S32"):
        for kind in ("extra", "text"):
            base, with_ms = result["tick"][f"{kind}_{s}"], result["tick"][f"{kind}_ms_{s}"]
            # tick t pairs the same frames in both sessions (0, 1 or 2 per stream, which makes the tick times bimodal):
            # the cost added is the median of the per-tick differences, not the difference of the medians
            diffs = [y - x for x, y in zip(samples[f"{kind}_{s}"][0], samples[f"{kind}_ms_{s}"][0])]
            q = statistics.quantiles(diffs, n=10)
            added = statistics.median(diffs)
            result["tick"][f"{kind}_added_ms_{s}"] = {"paired_median": round(added, 4), "paired_p10": round(q[0], 4),
                                                      "paired_p90": round(q[-1], 4),
                                                      "of_medians": round(with_ms["event_ms_median"] - base["event_ms_median"], 4)}
            result["tick"][f"{kind}_added_percent_{s}"] = round(100.0 * added / base["event_ms_median"], 3)

    # ---- the passes next to the encoders
    torch.manual_seed(6)
    bert = BertEncoderHIP().cuda().eval()
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(1000, 30000, (ROWS // 64, 64), generator=g).cuda()
    mask = torch.ones_like(ids)
    examples = torch.randn((960, 96, 64), device="cuda")
    passes = {}
    for c in (768, 128):
        rows = torch.randn((ROWS, c), device="cuda")
        acc = torch.zeros((2, c), dtype=torch.float64, device="cuda")
        ms = stats({"f": c})["f"]
        mean, std, out = torch.from_numpy(ms["mean"]).cuda(), torch.from_numpy(ms["std"]).cuda(), torch.empty_like(rows)
        passes[f"moments_{ROWS}x{c}"] = (lambda rows=rows, acc=acc: ops.feature_moments_update(rows, acc), rows.numel() * 4)
        passes[f"standardize_{ROWS}x{c}"] = (lambda rows=rows, mean=mean, std=std, out=out: ops.standardize_rows(rows, mean, std, out=out),
                                            rows.numel() * 8)
    for c in (768, 128):
        rows = torch.randn((32, c), device="cuda")
        one = torch.ones(c, device="cuda")
        passes[f"standardize_32x{c}"] = (lambda rows=rows, one=one: ops.standardize_rows(rows, one, one, out=rows), rows.numel() * 8)
    with torch.no_grad():
        passes["bert_150x64"] = (lambda: bert(ids, mask), 0)
        passes["vggish_960"] = (lambda: audio(examples), 0)
        for fn, _ in passes.values():
            for _ in range(5):
                fn()
        for name, (fn, nbytes) in passes.items():
            reps = 5 if name.startswith(("bert", "vggish")) else a.reps
            ev = []
            for _ in range(a.rounds):
                ev += timed(fn, reps)[0]
            med = statistics.median(ev)
            result["passes"][name] = {"event_ms_median": round(med, 4)}
            if nbytes:
                result["passes"][name]["gb_per_s"] = round(nbytes / med / 1e6, 1)
    p = result["passes"]
    p["vggish_9600_ms"] = round(10 * p["vggish_960"]["event_ms_median"], 3)
    p["moments_over_bert"] = round(p[f"moments_{ROWS}x768"]["event_ms_median"] / p["bert_150x64"]["event_ms_median"], 4)
    p["moments_over_vggish"] = round(p[f"moments_{ROWS}x128"]["event_ms_median"] / p["vggish_9600_ms"], 5)
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
