"""Latency of one ``AVStream.push_text`` call next to the BERT call inside it.

    python tools/bench_live_text.py [--reps 40] [--rounds 5] [--out profiles/live_text_latency.json]

One call is one finished sentence of 24 token ids spoken over 90 frames (3 s at 30 fps), handed to a tri-modal session of
S = 1 and of S = 32 streams (``hold`` = 512, ``max_tokens`` = 64, ``sentence_batch`` = 4, the full 12-layer encoder with random
weights, fp32).  The call checks the sentence on the host, uploads the padded ids, runs BERT on [4, 64], spreads the 22 words
over the 90 frame rows (``cer_text_spread_rows``) and appends them to the text ring; no frame is waiting, so no model launch
follows.  The stream's text is reset between calls (host ints only), so the ring never fills.  ``bert_alone`` is the encoder on
a device-resident [4, 64] batch of the same sentence: the difference is the share of the host checks, the two uploads, the
spread kernel and the ring append.  Each figure is the median over ``rounds * reps`` calls of the time between two HIP events
around ONE call, after warm-up, the cases alternating round by round in the same process; the host-clock median (call +
synchronise) is kept next to it.  Launches are counted as C-ABI calls through ``ops``.  Prints one JSON line and writes it to
``--out``.  Needs the GPU.
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

FPS, TOKENS, FRAMES, MAX_TOKENS, BATCH, HOLD = 30, 24, 90, 64, 4, 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live_text_latency.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_live_text.py measures on the GPU; none is visible")
    from feature_vs_text_compound_emotion_amd.live import AVStream
    from feature_vs_text_compound_emotion_amd.text_encoder import BertEncoderHIP
    from feature_vs_text_compound_emotion_amd.text_stream import TextStream
    model, audio = build_model()
    torch.manual_seed(5)
    encoder = BertEncoderHIP().cuda().eval()
    g = torch.Generator().manual_seed(6)
    sentence = [101] + torch.randint(1000, 30000, (TOKENS - 2,), generator=g).tolist() + [102]
    ids = torch.zeros((BATCH, MAX_TOKENS), dtype=torch.int64)
    ids[:, :TOKENS] = torch.tensor(sentence)
    mask = (torch.arange(MAX_TOKENS) < TOKENS).long().expand(BATCH, MAX_TOKENS).contiguous()
    ids, mask = ids.cuda(), mask.cuda()
    cases, result = {}, {"fps": FPS, "tokens": TOKENS, "frames": FRAMES, "max_tokens": MAX_TOKENS, "sentence_batch": BATCH,
                         "hold": HOLD, "encoder_layers": len(encoder.encoder.layer), "precision": encoder.precision,
                         "reps": a.reps, "rounds": a.rounds}

    def session_case(streams):
        text = TextStream(encoder, streams, max_tokens=MAX_TOKENS, sentence_batch=BATCH)
        sess = AVStream(model, streams, FPS, hold=HOLD, audio_backbone=audio, text=text)
        state = {"t": 0}

        def call():
            s = state["t"] % streams
            state["t"] += 1
            text.reset([s])
            return sess.push_text([(s, sentence, 0, FRAMES)])[0]
        return call, sess

    for s in (1, 32):
        cases[f"push_text_S{s}"], sess = session_case(s)
        result[f"rings_S{s}"] = {"frames": sess.ring_frames, "examples": sess.ring_examples}
    cases["bert_alone"] = lambda: encoder(ids, mask)
    # the session's rows against the encoder's, before timing
    sess_rows = TextStream(encoder, 1, max_tokens=MAX_TOKENS, sentence_batch=BATCH).push([(0, sentence, 0, FRAMES)])[0]
    from feature_vs_text_compound_emotion_amd.text_stream import spread_index
    want = encoder(ids, mask)[0][[1 + j for j in spread_index(TOKENS - 2, FRAMES)]]
    if not torch.equal(sess_rows, want):
        raise SystemExit("the TextStream's rows differ from the encoder's token rows under the host index plan")
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
    for s in ("S1", "S32"):
        result[f"outside_bert_ms_{s}"] = round(result[f"push_text_{s}"]["event_ms_median"] - result["bert_alone"]["event_ms_median"], 4)
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
