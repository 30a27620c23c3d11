"""The live audio-visual session on the GPU: raw frames and raw PCM pushed through ``AVStream`` in any chunking give, bit for bit,
the logits ``stream_forward`` gives the offline-prepared clip (``FrameTransform`` of the frames; ``wav_int16_to_examples`` cut to
``min(n, L)`` with the last example repeated).  Every stage is bit-identical to its offline counterpart and the holds copy
bits, so every comparison of logits is for equality."""
import functools
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

FPS, NCLS, H, W = 10, 7, 64, 56      # hop 0.1 s


def _pkg():
    from feature_vs_text_compound_emotion_amd import live, streaming, synth
    return live, streaming, synth


@functools.lru_cache(maxsize=None)
def _model(kind):
    from test_tail_gpu import _build_lfan
    _, _, synth = _pkg()
    if kind == "can":
        from feature_vs_text_compound_emotion_amd.fusion_heads import CAN
        mods = ("video", "vggish")
        spec, alias = synth.can_spec(mods)
        m = CAN(task="CLASSIFICATION", modalities=mods, tcn_settings=synth.TCN_SETTINGS, backbone_settings={}, output_dim=NCLS,
                root_dir="", device="cuda", load_backbone=False)
        m.load_state_dict(synth.make_state_dict(spec, alias, seed=6), strict=True)
        return m.cuda().eval()
    mods = {"logmel": ["video", "logmel"], "tri": ["video", "vggish", "bert"]}[kind]
    spec, alias = synth.lfan_spec(mods, n_cls=NCLS)
    return _build_lfan(mods, synth.make_state_dict(spec, alias, seed=5), 4, n_cls=NCLS).eval()


@functools.lru_cache(maxsize=None)
def _backbone():
    from feature_vs_text_compound_emotion_amd.audio_backbone import AudioBackbone
    ab = AudioBackbone()
    ab.backbone.load_state_dict(_pkg()[2].make_state_dict(_pkg()[2].vggish_spec(""), seed=41))
    return ab.cuda().eval()


@functools.lru_cache(maxsize=None)
def _pcm(seconds, seed, rate=16000):
    return _pkg()[2].make_audio_int16(seconds, rate, seed=seed).cuda()


@functools.lru_cache(maxsize=None)
def _raw(frames, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (frames, H, W, 3), generator=g, dtype=torch.uint8).cuda()


@functools.lru_cache(maxsize=None)
def _bert(frames, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((frames, 768), generator=g).cuda()


def _offline_video(raws):
    from feature_vs_text_compound_emotion_amd.frames import FrameTransform
    return FrameTransform(48, 40, train=False)(torch.stack(raws))


def _cut_and_repeat(x, L):
    """x [B, n, ...] -> [B, L, ...]: the first min(n, L) rows, the last of them repeated (``audio_features``)."""
    use = min(x.shape[1], L)
    x = x[:, :use]
    return x if use == L else torch.cat([x, x[:, -1:].expand(-1, L - use, *x.shape[2:])], dim=1)


def _examples(pcms, rate=16000, resample=None):
    from feature_vs_text_compound_emotion_amd.audio_backbone import VGGish
    return VGGish().cuda().wav_int16_to_examples(torch.stack(pcms), rate, 0.96, 1.0 / FPS, resample=resample)


def _ticks(frames, samples, seed, max_frames=2, max_samples=1024, audio_first=False, late=None):
    """(video counts, audio counts) per push until every stream has brought everything.  ``audio_first``: no frame before
    the last sample; ``late``: (stream, tick) joins then."""
    rng, fv, fa, ticks = random.Random(seed), list(frames), list(samples), []
    while any(fv) or any(fa):
        on = [not (late and s == late[0] and len(ticks) < late[1]) for s in range(len(fv))]
        ac = [min(fa[s], rng.randint(0, max_samples)) if on[s] else 0 for s in range(len(fa))]
        fa = [n - c for n, c in zip(fa, ac)]
        vc = [min(fv[s], rng.randint(0, max_frames)) if on[s] and not (audio_first and any(fa)) else 0 for s in range(len(fv))]
        fv = [n - c for n, c in zip(fv, vc)]
        ticks.append((vc, ac))
    return ticks


def _cat(parts, like):
    parts = [p for p in parts if p.shape[0]]
    return torch.cat(parts) if parts else like[:0]


def _drive(sess, raws, pcms, ticks, finish_groups, extra=None):
    """Feed the ticks (input i is stream i), then finish the groups in turn.  Returns one logits tensor per stream."""
    out = [[] for _ in raws]
    fv, fa = [0] * len(raws), [0] * len(raws)

    def collect(logits, counts):
        assert logits.shape == (sum(counts), NCLS) and len(counts) == sess.streams
        at = 0
        for s, c in enumerate(counts):
            if c:
                out[s].append(logits[at:at + c])
            at += c

    for vc, ac in ticks:
        video = _cat([r[f:f + c] for r, f, c in zip(raws, fv, vc)], raws[0]) if sum(vc) else None
        audio = _cat([p[f:f + c] for p, f, c in zip(pcms, fa, ac)], pcms[0]) if sum(ac) else None
        ex = {m: _cat([r[f:f + c] for r, f, c in zip(rows, fv, vc)], rows[0]) for m, rows in (extra or {}).items()} if sum(vc) else None
        collect(*sess.push(video, vc if sum(vc) else None, audio, ac if sum(ac) else None, extra=ex))     # a side may be absent
        fv, fa = [a + b for a, b in zip(fv, vc)], [a + b for a, b in zip(fa, ac)]
    for group in finish_groups:
        collect(*sess.finish(group))
    return [torch.cat(o) if o else torch.empty((0, NCLS), device="cuda") for o in out]


# ---------------------------------------------------------------------------------------------- 4. session equals offline
@functools.lru_cache(maxsize=None)
def _reference(kind, L):
    """Offline logits [2, L, n_cls] of the two 0.3 s clips, and the offline examples."""
    _, streaming, _ = _pkg()
    model = _model(kind)
    ex = _examples([_pcm(0.3, 81), _pcm(0.3, 82)])
    assert ex.shape[1] == 4
    video = _offline_video([_raw(L, 1), _raw(L, 2)])
    if kind == "logmel":
        X = {"video": video, "logmel": _cut_and_repeat(ex, L).permute(0, 3, 1, 2).contiguous()}
    else:
        X = {"video": video, "vggish": _vggish_rows(ex, L)[:, None]}
    with torch.no_grad():
        return streaming.stream_forward(model, X)


def _vggish_rows(ex, L, encoder_batch=8):
    """The audio backbone on the offline examples [B, n, 96, 64], in calls of exactly ``encoder_batch`` examples (the last one
    filled up with zeros, its surplus rows dropped), cut to min(n, L) and the last row repeated -> [B, L, 128]."""
    rows = []
    for b in range(ex.shape[0]):
        use, outs = min(ex.shape[1], L), []
        for i in range(0, use, encoder_batch):
            part = ex[b, i:min(use, i + encoder_batch)]
            full = torch.zeros((encoder_batch, 96, 64), device=ex.device)
            full[:part.shape[0]] = part
            with torch.no_grad():
                outs.append(_backbone()(full)[:part.shape[0]])
        rows.append(torch.cat(outs))
    return _cut_and_repeat(torch.stack(rows), L)


@pytest.mark.parametrize("L", [3, 4, 6])      # examples dropped, exact, the last example repeated
@pytest.mark.parametrize("kind", ["logmel", "can"])
def test_frames_and_pcm_to_logits_equal_the_offline_forward(kind, L):
    live, _, _ = _pkg()
    ref = _reference(kind, L)
    raws, pcms = [_raw(L, 1), _raw(L, 2)], [_pcm(0.3, 81), _pcm(0.3, 82)]
    total = pcms[0].shape[0]
    runs = ((_ticks([L, L], [total] * 2, seed=1), [None]),
            (_ticks([L, L], [total] * 2, seed=2, audio_first=True), [[1], [0]]))
    for ticks, groups in runs:
        sess = live.AVStream(_model(kind), 2, FPS, hold=6, lead=4, max_new=2, max_samples=1024,
                             audio_backbone=_backbone() if kind == "can" else None)
        assert sess.ring_frames == 8
        got = torch.stack(_drive(sess, raws, pcms, ticks, groups))
        assert got.shape == ref.shape and torch.equal(got, ref)
        assert sess.frames_seen == sess.examples_seen == sess.paired == [0, 0]      # finished streams are reset


def test_examples_wait_for_late_frames():
    """1.3 s of audio completes four examples before the stream ends and fourteen in all: pushed entirely before the video,
    they wait in the example ring (``lead`` = 4), and the last two of sixteen frames repeat the last example."""
    live, streaming, _ = _pkg()
    model, L = _model("logmel"), 16
    pcms, raws = [_pcm(1.3, 83)], [_raw(L, 3)]
    ex = _examples(pcms)
    assert ex.shape[1] == 14
    with torch.no_grad():
        ref = streaming.stream_forward(model, {"video": _offline_video(raws),
                                               "logmel": _cut_and_repeat(ex, L).permute(0, 3, 1, 2).contiguous()})
    sess = live.AVStream(model, 1, FPS, hold=12, lead=4, max_new=4)
    assert sess.ring_examples == 8
    at, waited = 0, 0
    while at < pcms[0].shape[0]:
        c = min(4096, pcms[0].shape[0] - at)
        logits, counts = sess.push(audio=pcms[0][at:at + c], audio_counts=[c])
        assert counts == [0] and logits.shape == (0, NCLS)
        at, waited = at + c, max(waited, sess.examples_seen[0])
    assert waited == 4 and sess.paired == [0]      # four examples are held, none is paired yet
    parts = [sess.push(video=raws[0][i:i + 4], video_counts=[4])[0] for i in range(0, L, 4)]
    assert [p.shape[0] for p in parts] == [4, 0, 0, 0]
    parts.append(sess.finish()[0])
    assert torch.equal(torch.cat(parts)[None], ref)


def test_resampled_stereo_session():
    live, streaming, _ = _pkg()
    model, L = _model("logmel"), 4
    pcms = [torch.stack([_pcm(0.3, 90 + 2 * s, 48000), _pcm(0.3, 91 + 2 * s, 48000)], dim=1).contiguous() for s in range(2)]
    raws = [_raw(L, 1), _raw(L, 2)]
    ex = _examples(pcms, 48000, "kaiser_fast")
    with torch.no_grad():
        ref = streaming.stream_forward(model, {"video": _offline_video(raws),
                                               "logmel": _cut_and_repeat(ex, L).permute(0, 3, 1, 2).contiguous()})
    sess = live.AVStream(model, 2, FPS, sample_rate=48000, channels=2, resample="kaiser_fast", hold=4, lead=4, max_new=4)
    got = torch.stack(_drive(sess, raws, pcms, _ticks([L, L], [pcms[0].shape[0]] * 2, seed=4, max_samples=4096), [None]))
    assert torch.equal(got, ref)


# ---------------------------------------------------------------------------------------------- 5. vggish-keyed, tri-modal
def test_trimodal_session_runs_the_audio_backbone_itself():
    from feature_vs_text_compound_emotion_amd.feature_extractor import MultimodalFeatureExtractor
    live, streaming, _ = _pkg()
    model, L = _model("tri"), 6
    raws, pcms, bert = [_raw(L, 1), _raw(L, 2)], [_pcm(0.3, 81), _pcm(0.3, 82)], [_bert(L, 1), _bert(L, 2)]
    ex = _examples(pcms)
    rows = _vggish_rows(ex, L)
    with torch.no_grad():
        ref = streaming.stream_forward(model, {"video": _offline_video(raws), "vggish": rows[:, None],
                                               "bert": torch.stack(bert)[:, None]})
    sess = live.AVStream(model, 2, FPS, hold=6, lead=4, max_new=2, max_samples=1024, audio_backbone=_backbone())
    seen, push_ragged = [], sess.model_stream.push_ragged

    def spy(X, counts):
        seen.append((X["vggish"].clone(), list(counts)))
        return push_ragged(X, counts)

    sess.model_stream.push_ragged = spy
    # refused before any launch, and the session goes on as if the call had never been made
    with pytest.raises(ValueError, match="extra"):
        sess.push(raws[0][:2], [2, 0], extra={"bert": bert[0][:3]})
    with pytest.raises(ValueError, match="extra"):
        sess.push(raws[0][:2], [2, 0])
    assert sess.frames_seen == [0, 0] and sess.frame_stream.frames_seen == [0, 0] and sess.frame_stream.ring is None
    got = torch.stack(_drive(sess, raws, pcms, _ticks([L, L], [pcms[0].shape[0]] * 2, seed=5), [None], extra={"bert": bert}))
    assert torch.equal(got, ref)
    # the rows the session handed the model, against audio_features on the same PCM, at the bar tests/test_encoders_gpu.py
    # holds VGGish to
    per = [[], []]
    for x, counts in seen:
        at = 0
        for s, c in enumerate(counts):
            per[s].append(x[at:at + c])
            at += c
    mine = torch.stack([torch.cat(p) for p in per])
    assert torch.equal(mine, rows)
    fx = MultimodalFeatureExtractor(audio=_backbone(), text=torch.nn.Identity(), fps=FPS)
    with torch.no_grad():
        want = fx.audio_features(torch.stack(pcms), L)[:, 0]
    assert (mine - want).abs().max().item() < 1e-4 * max(1.0, want.abs().max().item())


# ---------------------------------------------------------------------------------------------- 6. ragged session
def test_ragged_session_equals_each_stream_alone():
    live, _, _ = _pkg()
    model = _model("logmel")
    Ls, secs = [5, 3, 4], [0.3, 0.45, 0.3]
    raws, pcms = [_raw(n, 10 + i) for i, n in enumerate(Ls)], [_pcm(t, 84 + i) for i, t in enumerate(secs)]
    ticks = _ticks(Ls, [p.shape[0] for p in pcms], seed=6, late=(1, 3))
    kw = dict(hold=6, lead=4, max_new=4, max_samples=1024)
    sess = live.AVStream(model, 3, FPS, **kw)
    # stream 2 is used and reset before its real run
    sess.push(_raw(3, 99), [0, 0, 3], _pcm(0.3, 98)[:900], [0, 0, 900])
    sess.reset([2])
    assert sess.frames_seen == [0, 0, 0] and sess.frame_stream.frames_seen == [0, 0, 0]
    got = _drive(sess, raws, pcms, ticks, [[0], [2, 1]])
    for s in range(3):
        alone = _drive(live.AVStream(model, 1, FPS, **kw), [raws[s]], [pcms[s]], [([vc[s]], [ac[s]]) for vc, ac in ticks], [None])
        assert got[s].shape == (Ls[s], NCLS) and torch.equal(got[s], alone[0]), s


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refused_calls_change_nothing():
    live, _, _ = _pkg()
    model = _model("logmel")
    pcm, raw = _pcm(1.2, 85), _raw(5, 20)
    cuts = [0, 4096, 8192, 12288, 16384]

    def run(with_refusals):
        sess = live.AVStream(model, 1, FPS, hold=4, lead=1, max_new=8)
        parts = [sess.push(audio=pcm[a:a + 4096], audio_counts=[4096])[0] for a in cuts[:4]]
        assert sess.examples_seen == [1]
        if with_refusals:
            state = (list(sess.audio_stream.samples_seen), list(sess.audio_stream.examples_emitted), list(sess.examples_seen))
            with pytest.raises(ValueError, match="lead = 1"):      # two more examples would wait
                sess.push(audio=pcm[16384:], audio_counts=[pcm.shape[0] - 16384])
            with pytest.raises(ValueError, match="hold = 4"):
                sess.push(video=raw, video_counts=[5])
            with pytest.raises(ValueError):                        # the audio side is bad: the good video side is not pushed
                sess.push(video=raw[:3], video_counts=[3], audio=pcm[16384:].float(), audio_counts=[pcm.shape[0] - 16384])
            assert state == (sess.audio_stream.samples_seen, sess.audio_stream.examples_emitted, sess.examples_seen)
            assert sess.frames_seen == [0] and sess.frame_stream.frames_seen == [0] and sess.frame_stream.ring is None
        parts.append(sess.push(video=raw[:3], video_counts=[3])[0])
        parts.append(sess.push(audio=pcm[16384:], audio_counts=[pcm.shape[0] - 16384])[0])
        assert sess.paired == [3]
        parts.append(sess.finish()[0])
        return torch.cat(parts)

    a, b = run(True), run(False)
    assert a.shape == (3, NCLS) and torch.equal(a, b)


def test_models_that_cannot_stream_are_refused():
    from feature_vs_text_compound_emotion_amd.fusion_heads import JMT
    live, _, synth = _pkg()
    jmt = JMT(task="CLASSIFICATION", modalities=("video", "vggish"), tcn_settings=synth.TCN_SETTINGS, backbone_settings={},
              output_dim=NCLS, root_dir="", device="cuda", model_name="JMT", load_backbone=False).cuda().eval()
    with pytest.raises(TypeError, match="not causal"):
        live.AVStream(jmt, 1, FPS)
    model = _model("logmel")
    try:
        with pytest.raises(RuntimeError, match="train mode"):
            live.AVStream(model.train(), 1, FPS)
    finally:
        model.eval()
    with pytest.raises(ValueError, match="audio_backbone"):
        live.AVStream(_model("can"), 1, FPS)
