"""Per-tick latency of a live audio-visual session (``AVStream.push``) against what a caller can do without it: the offline
``FrameTransform`` on the new frames, a Python list of held tensors and ``torch.cat`` for the ones that fall due,
``LogMelStream.push``, the audio backbone, ``LFANStream.push_ragged``.

    python tools/bench_live.py [--reps 200] [--rounds 5] [--out profiles/live_latency.json]

Settings: S in {1, 32} streams, one tick of 30 fps video per call: one raw 256 x 256 frame and 533 or 534 samples of 16 kHz PCM
per stream, 48 -> 40 crop, a tri-modal LFAN (video, vggish, bert; synthetic weights) with the ``bert`` row of each frame handed
over next to it.  After the first 0.975 s a tick pairs one frame per stream on average (0, 1 or 2), about 29 frames behind the
newest.  Both sides take the same device-resident inputs and run the same encoders, ``encoder_batch`` = 8 frames per call.
Before timing, the logits of both sides are compared for equality over the first two seconds.  Each figure is the median over
``rounds * reps`` calls of the time between two HIP events around ONE call, after warm-up, the two methods alternating round
by round in the same process; the host-clock median (call + synchronise) is kept next to it.  Launches are counted as C-ABI
calls through ``ops`` and ``frames`` (each is one kernel launch) on one steady-state tick that pairs one frame per stream; the
torch copies of the hand-written side (``torch.stack`` / ``torch.cat`` of held tensors) are not in that count.  Prints one JSON
line and writes it to ``--out``.  Needs the GPU.
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

from bench_audio_stream import tick_sizes  # noqa: E402
from bench_stream import timed  # noqa: E402

FPS, HW, POOL, MODS = 30, 256, 8, ["video", "vggish", "bert"]


def count_calls(fn):
    from feature_vs_text_compound_emotion_amd import frames, ops
    calls, real = [], ops.check

    def counting(rc, what):
        calls.append(what)
        return real(rc, what)
    ops.check = frames.check = counting
    try:
        out = fn()
        torch.cuda.synchronize()
        return calls, out
    finally:
        ops.check = frames.check = real


def build_model():
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.audio_backbone import AudioBackbone
    from feature_vs_text_compound_emotion_amd.lfan import LFAN
    model = LFAN(backbone_settings={}, output_dim=7, task="CLASSIFICATION", modality=MODS, example_length=32, kernel_size=5,
                 tcn_channel=synth.TCN_CHANNELS, root_dir="", device="cuda", head_hw=5)
    model.init(load_backbone=False)
    model.load_state_dict(synth.lfan_state_dict(MODS, n_cls=7, head_hw=5, seed=0), strict=True)
    audio = AudioBackbone()
    audio.backbone.load_state_dict(synth.make_state_dict(synth.vggish_spec(""), seed=41))
    return model.cuda().eval(), audio.cuda().eval()


class ByHand:
    """The same session with the parts a caller had before ``AVStream``: host lists hold the transformed frames and the extra
    rows, the pairing ints live in the caller."""

    def __init__(self, model, audio, streams):
        from feature_vs_text_compound_emotion_amd.audio_stream import LogMelStream
        from feature_vs_text_compound_emotion_amd.frames import FrameTransform
        from feature_vs_text_compound_emotion_amd.streaming import LFANStream
        self.s, self.audio = streams, audio
        self.xf = FrameTransform(48, 40, train=False)
        self.crop = self.xf.draw(streams)
        self.logmel = LogMelStream(streams, 1.0 / FPS, max_samples=1024)
        self.lfan = LFANStream(model, streams)
        self.frames, self.rows, self.examples = [], [], []      # held per tick / per example, all streams in lockstep
        self.first_frame = self.first_example = self.paired = 0

    def push(self, video, pcm, n, bert):
        self.frames.append(self.xf(video.view(self.s, 1, HW, HW, 3), crop_xyf=self.crop)[:, 0])
        self.rows.append(bert)
        ex, counts = self.logmel.push(pcm, [n] * self.s)
        k = counts[0]
        if k:
            ex = ex.view(self.s, k, 96, 64)
            self.examples += [ex[:, i] for i in range(k)]
        have_f, have_e = self.first_frame + len(self.frames), self.first_example + len(self.examples)
        due = min(have_f, have_e) - self.paired
        if due <= 0:
            return None
        f0, e0 = self.paired - self.first_frame, self.paired - self.first_example
        video_due = torch.stack(self.frames[f0:f0 + due], dim=1).reshape(self.s * due, 3, 40, 40)     # stream-major
        bert_due = torch.stack(self.rows[f0:f0 + due], dim=1).reshape(self.s * due, 768)
        ex_due = torch.stack(self.examples[e0:e0 + due], dim=1).reshape(self.s * due, 96, 64)
        del self.frames[:f0 + due], self.rows[:f0 + due], self.examples[:e0 + due]
        self.first_frame += f0 + due
        self.first_example += e0 + due
        self.paired += due
        vggish = self.lfan._in_groups(self.audio, ex_due)
        return self.lfan.push_ragged({"video": video_due, "vggish": vggish, "bert": bert_due}, [due] * self.s)


def make_case(model, audio, streams, ticks, sizes, g):
    from feature_vs_text_compound_emotion_amd.live import AVStream
    video = torch.randint(0, 256, (POOL, streams, HW, HW, 3), device="cuda", generator=g, dtype=torch.uint8)
    bert = torch.randn((POOL, streams, 768), device="cuda", generator=g)
    pcm = (torch.randn(streams, sum(sizes), device="cuda", generator=g) * 3000.0).round().clamp(-32768, 32767).to(torch.int16)
    chunks, at = [], 0
    for n in sizes:
        chunks.append(pcm[:, at:at + n].reshape(-1).contiguous())      # stream-major packed
        at += n
    sess, hand = AVStream(model, streams, FPS, max_samples=1024, audio_backbone=audio), ByHand(model, audio, streams)
    state = {"live": 0, "hand": 0}

    def live():
        t = state["live"]
        state["live"] = t + 1
        return sess.push(video[t % POOL], [1] * streams, chunks[t], [sizes[t]] * streams, extra={"bert": bert[t % POOL]})[0]

    def by_hand():
        t = state["hand"]
        state["hand"] = t + 1
        return hand.push(video[t % POOL], chunks[t], sizes[t], bert[t % POOL])

    return live, by_hand, sess


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live_latency.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_live.py measures on the GPU; none is visible")
    model, audio = build_model()
    total = a.warmup + a.reps * a.rounds + 64
    sizes = tick_sizes(total)
    g = torch.Generator(device="cuda").manual_seed(3)
    result = {"fps": FPS, "frame": [HW, HW], "crop": 40, "modalities": MODS, "reps": a.reps, "rounds": a.rounds, "session": {},
              "by_hand": {}}
    cases, compared = {}, 0
    for s in (1, 32):
        live, by_hand, sess = make_case(model, audio, s, total, sizes, g)
        for _ in range(a.warmup):      # the first 0.975 s fill here, and the two sides are compared
            x, y = live(), by_hand()
            if (y is None) != (x.shape[0] == 0) or (y is not None and not torch.equal(x, y)):
                raise SystemExit(f"S = {s}: the session's logits differ from the hand-written pipeline's")
            compared += x.shape[0]
        cases[f"session_S{s}"], cases[f"by_hand_S{s}"] = live, by_hand
        result[f"rings_S{s}"] = {"frames": sess.ring_frames, "examples": sess.ring_examples}
    result["logit_rows_compared_equal"] = compared
    samples = {name: ([], []) for name in cases}
    for _ in range(a.rounds):           # alternate the methods: a drift of the machine hits both alike
        for name, fn in cases.items():
            ev, host = timed(fn, a.reps)
            samples[name][0].extend(ev)
            samples[name][1].extend(host)
    for name, fn in cases.items():
        kind, s = name.rsplit("_S", 1)
        for _ in range(32):             # a tick that pairs exactly one frame per stream
            made, out = count_calls(fn)
            if out is not None and out.shape[0] == int(s):
                break
        ev, host = samples[name]
        q = statistics.quantiles(ev, n=10)
        result[kind]["S" + s] = {"event_ms_median": round(statistics.median(ev), 4), "event_ms_p10": round(q[0], 4),
                                 "event_ms_p90": round(q[-1], 4), "host_ms_median": round(statistics.median(host), 4),
                                 "launches": len(made),
                                 "entries": {m[len("cer_"):]: made.count(m) for m in dict.fromkeys(made)}}
    for s in ("S1", "S32"):
        se, bh = result["session"][s], result["by_hand"][s]
        result[f"by_hand_over_session_{s}"] = round(bh["event_ms_median"] / se["event_ms_median"], 3)
        result[f"session_faster_{s}"] = se["event_ms_median"] < bh["event_ms_median"]
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
