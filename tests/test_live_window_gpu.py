"""``AVStream(window=(W, H))``: a live audio-visual session under the evaluator's window rule.  Raw frames and raw PCM of a JMT
and of an LFAN session give, bit for bit, what a ``WindowStream`` gives the offline-prepared rows the session paired (frame i
with example min(i, n - 1)); ``decisions=`` receives every emitted row; without ``window=`` nothing changes."""
import functools
import random

import pytest
import torch

from test_live_gpu import (FPS, NCLS, _backbone, _cut_and_repeat, _drive, _examples, _model, _offline_video, _pcm, _raw,
                           _vggish_rows)

pytestmark = pytest.mark.gpu

W, H, L, SECONDS = 8, 3, 16, 1.2      # 16 frames: windows at 0, 3 and 6, the tail at 8; 13 examples


@functools.lru_cache(maxsize=None)
def _jmt():
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.fusion_heads import JMT
    mods = ["video", "vggish"]
    spec, alias = synth.jmt_spec(mods, "JMT", n_cls=NCLS)
    m = JMT(task="CLASSIFICATION", modalities=mods, tcn_settings=synth.TCN_SETTINGS, backbone_settings={}, output_dim=NCLS,
            root_dir="", device="cuda", model_name="JMT", load_backbone=False)
    m.load_state_dict(synth.make_state_dict(spec, alias, seed=8), strict=True)
    return m.cuda().eval()


def _schedule(frames, samples, seed):
    """Audio late (the first ticks bring frames only), a silent gap (a tick that brings nothing), then both sides at random."""
    rng, fv, fa, ticks = random.Random(seed), list(frames), list(samples), []
    for _ in range(2):
        vc = [min(n, rng.randint(1, 2)) for n in fv]
        fv = [n - c for n, c in zip(fv, vc)]
        ticks.append((vc, [0] * len(fa)))
    while any(fv) or any(fa):
        if len(ticks) == 5:
            ticks.append(([0] * len(fv), [0] * len(fa)))
        vc = [min(n, rng.randint(0, 2)) for n in fv]
        ac = [min(n, rng.randint(0, 2048)) for n in fa]
        fv, fa = [n - c for n, c in zip(fv, vc)], [n - c for n, c in zip(fa, ac)]
        ticks.append((vc, ac))
    return ticks


@pytest.mark.parametrize("kind", ["jmt", "logmel"])
def test_a_windowed_session_equals_a_window_stream_on_the_rows_it_paired(kind):
    from feature_vs_text_compound_emotion_amd import live, window_stream
    model = _jmt() if kind == "jmt" else _model("logmel")
    raws, pcms = [_raw(L, 21), _raw(L, 22)], [_pcm(SECONDS, 91), _pcm(SECONDS, 92)]
    ex = _examples(pcms)
    assert 1 < ex.shape[1] < L                        # the last frames repeat the last example
    if kind == "jmt":
        X = {"video": _offline_video(raws), "vggish": _vggish_rows(ex, L)[:, None]}
    else:
        X = {"video": _offline_video(raws), "logmel": _cut_and_repeat(ex, L).permute(0, 3, 1, 2).contiguous()}
    with torch.no_grad():
        want = window_stream.window_forward(model, X, W, H, chunk=2)
    assert want.shape == (2, L, NCLS)
    sess = live.AVStream(model, 2, FPS, hold=16, lead=8, max_new=2, max_samples=2048, window=(W, H), decisions={},
                         audio_backbone=_backbone() if kind == "jmt" else None)
    assert isinstance(sess.model_stream, window_stream.WindowStream) and sess.window == (W, H)
    fed, to_decisions, push = [[], []], sess.decisions.push_ragged, sess.push

    def spy(rows, counts, track=False):
        assert max(counts) <= sess.decisions.max_new
        at = 0
        for s, c in enumerate(counts):
            fed[s].append(rows[at:at + c].clone())
            at += c
        return to_decisions(rows, counts, track)

    def checked_push(*args, **kw):
        logits, counts = push(*args, **kw)
        # ``paired`` counts the frames handed to the model, ``emitted`` the rows that came out: a frame waits for W more
        assert sess.emitted == [max(p - W, 0) for p in sess.paired] == sess.model_stream.emitted
        return logits, counts

    sess.decisions.push_ragged, sess.push = spy, checked_push
    ticks = _schedule([L, L], [p.shape[0] for p in pcms], seed=7)
    assert ticks[5] == ([0, 0], [0, 0]) and not any(sum(ac) for _, ac in ticks[:2])
    got = _drive(sess, raws, pcms, ticks, [[1], [0]])
    assert torch.equal(torch.stack(got), want)
    for s in range(2):                                 # the decisions saw every emitted row, in order, and no other
        assert torch.equal(torch.cat(fed[s]), got[s])
    assert sess.frames_seen == sess.paired == sess.emitted == [0, 0]


def test_a_session_without_window_is_unchanged():
    from feature_vs_text_compound_emotion_amd import live
    with pytest.raises(TypeError, match="JMT / MT attend over time and are not causal"):
        live.AVStream(_jmt(), 2, FPS, audio_backbone=_backbone())
    sess = live.AVStream(_model("logmel"), 2, FPS)
    assert sess.window is None and type(sess.model_stream).__name__ == "LFANStream" and sess.emitted == [0, 0]
    with pytest.raises(ValueError, match="window"):
        live.AVStream(_model("logmel"), 2, FPS, window=8)
    with pytest.raises(ValueError, match="hop_length"):
        live.AVStream(_model("logmel"), 2, FPS, window=(8, 9))
