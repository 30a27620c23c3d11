"""The host rules of the live text leg, no GPU: the closed form of the token -> frame spreading that ``cer_text_spread_rows``
evaluates, the pairing of frames with examples and text rows, the text ring's refusal and the refusals of ``TextStream``."""
import random

import pytest
import torch


def _pkg():
    from feature_vs_text_compound_emotion_amd import live, text_stream
    return live, text_stream


# ---------------------------------------------------------------------------------------------- 1. j(i)
def test_closed_form_equals_align_tokens_to_frames():
    from feature_vs_text_compound_emotion_amd.feature_extractor import align_tokens_to_frames
    _, ts = _pkg()
    for n_tokens in range(70):
        for n_frames in range(1, 70):
            assert ts.spread_index(n_tokens, n_frames) == align_tokens_to_frames(n_tokens, n_frames), (n_tokens, n_frames)


def test_frames_of_seconds():
    _, ts = _pkg()
    assert ts.frames_of_seconds(0.0, 1.0, 30) == (0, 30)
    assert ts.frames_of_seconds(0.51, 0.9, 10) == (6, 3)      # frames at 0.6, 0.7, 0.8 s


# ---------------------------------------------------------------------------------------------- 2. pairing
def _simulate(ticks, final):
    """Brute force, frame by frame: after each tick (frames, examples, text are totals) frame i is emitted, with example i,
    when it is the next one and all three of it exist.  At the end (``final`` examples in all) text is taken as complete and
    every remaining frame i goes with example min(i, final - 1); ``final`` = 0 drops them."""
    emitted, per_tick = [], []
    for f, e, t in ticks:
        new = []
        while len(emitted) < f and len(emitted) < e and len(emitted) < t:
            new.append((len(emitted), len(emitted)))
            emitted.append(new[-1])
        per_tick.append(new)
    f = ticks[-1][0] if ticks else 0
    last = []
    if final:
        while len(emitted) < f:
            last.append((len(emitted), min(len(emitted), final - 1)))
            emitted.append(last[-1])
    return per_tick, last


def _schedule(seed, frames, text_lag, audio_lag, text_short=0):
    """Totals (F, E, T) per tick: ``text_lag`` / ``audio_lag`` > 0: that side runs behind the frames by up to that many;
    < 0: ahead of them.  ``text_short``: the text never reaches the last that-many frames."""
    rng, f, e, t, ticks = random.Random(seed), 0, 0, 0, []
    while f < frames:
        f = min(frames, f + rng.randint(0, 3))
        want_e = f - rng.randint(0, audio_lag) if audio_lag >= 0 else f + rng.randint(0, -audio_lag)
        want_t = f - rng.randint(0, text_lag) if text_lag >= 0 else f + rng.randint(0, -text_lag)
        e, t = max(e, want_e), max(t, min(want_t, frames - text_short) if text_short else want_t)
        ticks.append((f, e, t))
    return ticks


@pytest.mark.parametrize("case", ["text late", "text ahead", "audio late", "text short at the end", "both late"])
@pytest.mark.parametrize("seed", range(6))
def test_pair_schedule_text_equals_the_brute_force(case, seed):
    live, _ = _pkg()
    text_lag, audio_lag, short = {"text late": (9, 0, 0), "text ahead": (-7, 2, 0), "audio late": (0, 9, 0),
                                  "text short at the end": (5, 3, 4), "both late": (8, 8, 0)}[case]
    ticks = _schedule(seed, 40, text_lag, audio_lag, short)
    frames, examples, text = ticks[-1]
    for final in (max(examples, 1) + 2, max(frames - 3, 1), 0):      # examples past the frames, fewer than them, no audio at all
        if final and final < examples:
            continue
        want_ticks, want_last = _simulate(ticks, final)
        paired = 0
        for (f, e, t), want in zip(ticks, want_ticks):
            got = live.pair_schedule_text(f, e, t, paired)
            assert got == want, (case, seed, f, e, t, paired)
            paired += len(got)
        assert paired == min(frames, examples, text)
        assert live.pair_schedule_text(frames, final, text, paired, final=final) == want_last
    if case == "text short at the end":
        assert text < frames


@pytest.mark.parametrize("seed", range(6))
def test_with_text_never_behind_the_frames_it_is_pair_schedule(seed):
    live, _ = _pkg()
    ticks, paired = _schedule(seed, 40, -5, 6), 0
    for f, e, t in ticks:
        assert t >= f
        got = live.pair_schedule_text(f, e, t, paired)
        assert got == live.pair_schedule(f, e, paired)
        paired += len(got)
    f, e, t = ticks[-1]
    for final in (e + 2, 0):
        assert live.pair_schedule_text(f, final, t, paired, final=final) == live.pair_schedule(f, final, paired, final=final)


def test_check_text_waiting_at_its_boundary():
    live, _ = _pkg()
    assert live.check_text_waiting(10, 6, 8, 8) == 8           # rows 8 .. 15 fill the ring of 8: equal passes
    with pytest.raises(ValueError, match="ring of 8"):
        live.check_text_waiting(10, 7, 8, 8)                   # one more refuses
    assert live.check_text_waiting(0, 0, 0, 8) == 0
    assert live.check_text_waiting(5, 128, 5, 128) == 128
    with pytest.raises(ValueError):
        live.check_text_waiting(5, 129, 5, 128)


# ---------------------------------------------------------------------------------------------- 3. TextStream refusals
def _stream(streams=2, **kw):
    from feature_vs_text_compound_emotion_amd.text_encoder import BertEncoderHIP
    _, ts = _pkg()
    enc = BertEncoderHIP(vocab_size=50, hidden_size=128, num_hidden_layers=1, num_attention_heads=4, intermediate_size=256,
                         max_position_embeddings=16).eval()
    return ts.TextStream(enc, streams, max_tokens=16, sentence_batch=4, **kw)


SENT = [1, 7, 9, 2]


@pytest.mark.parametrize("sentences,upto,match", [
    ([(0, SENT, 3, 5), (0, SENT, 7, 3)], None, "spans ascend and do not overlap"),        # overlap inside one call
    ([(0, SENT, 2, 5)], None, "before frame 3"),                                           # a span before covered
    ([(0, [1], 3, 5)], None, "1 token ids"),                                               # length 1
    ([(0, list(range(16)), 3, 5)], None, "16 token ids"),                                  # length max_tokens
    ([(2, SENT, 3, 5)], None, "stream 2 of 2"),                                            # stream out of range
    ([(-1, SENT, 3, 5)], None, "stream -1 of 2"),
    ([(0, [1, 50, 2], 3, 5)], None, "token id 50"),                                        # outside the vocabulary
    ([(0, [1, -1, 2], 3, 5)], None, "token id -1"),
    ([(0, SENT, 3, 0)], None, "num >= 1"),
    ([(0, SENT, 3.0, 2)], None, "ints"),
    ([(0, SENT, 3, 5)], [7, None], r"upto\[0\] = 7 lies below frame 8"),
    ([], [2, None], r"upto\[0\] = 2 lies below frame 3"),
    ([], [4], "one entry per stream"),
    ([], {2: 4}, "stream 2 of 2"),
    ([(0, SENT, 3)], None, "expected \\(stream, token_ids"),
])
def test_check_push_refusals_need_no_gpu(sentences, upto, match):
    ts = _stream()
    ts.covered[0] = 3
    with pytest.raises(ValueError, match=match):
        ts.check_push(sentences, upto)
    with pytest.raises(ValueError, match=match):
        ts.push(sentences, upto)
    assert ts.covered == [3, 0]


def test_a_good_call_is_refused_only_for_the_cpu_encoder_and_train_mode():
    ts = _stream()
    good = [(0, SENT, 3, 5), (1, SENT, 0, 2), (0, [1, 2], 9, 1)]
    with pytest.raises(ValueError, match="on the CPU"):
        ts.check_push(good, {1: 6})
    ts.encoder.train()
    with pytest.raises(ValueError, match="train mode"):
        ts.push(good)
    assert ts.covered == [0, 0]


def test_constructor_refusals():
    for kw, match in ((dict(last_n_sum=0), "last_n_sum"), (dict(streams=0), "streams")):
        with pytest.raises(ValueError, match=match):
            _stream(**kw)
    from feature_vs_text_compound_emotion_amd.text_encoder import BertEncoderHIP
    _, ts = _pkg()
    enc = BertEncoderHIP(vocab_size=50, hidden_size=128, num_hidden_layers=1, num_attention_heads=4, intermediate_size=256,
                         max_position_embeddings=16).eval()
    with pytest.raises(ValueError, match="16 positions"):
        ts.TextStream(enc, 1, max_tokens=17)


def test_text_spread_tables_refusals_need_no_gpu():
    from feature_vs_text_compound_emotion_amd import ops
    table, index = ops.text_spread_tables([(4, 3, [5, 5, 1]), (0, 2, []), (2, 2, [9])], 7, 10)
    assert table == [(4, 3, 3, 0), (0, 2, 0, 3), (2, 2, 1, 3)] and index == [5, 5, 1, 9]
    for segments, match in (([(0, 3, [0]), (2, 2, [0])], "overlap"), ([(5, 3, [0])], "outside"), ([(-1, 2, [0])], "outside"),
                            ([(0, 0, [0])], "empty"), ([(0, 2, [10])], "token row 10"), ([(0, 2, [-1])], "token row -1"),
                            ([(0, 2.0, [1])], "not an int"), ([(0, 2, [True])], "not an int"), ([], "no segment"),
                            ([(0, 2)], "expected")):
        with pytest.raises(ValueError, match=match):
            ops.text_spread_tables(segments, 7, 10)
    with pytest.raises(ValueError):
        ops.text_spread_rows(torch.zeros(2, 4), [(0, 1, [0])], 1)      # a CPU tensor
