"""``WindowStream``: the evaluator's window rule on live streams.  An LFAN's live logits are the bits of the offline evaluator
(``Trainer.inference_forward_windows`` with one window per forward) under any chunking and among any neighbours; JMT, MT, CAN
and a tri-modal LFAN with the encoders in front stay within the offline forwards' bar of float64 windows stitched in numpy."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

W, H, NCLS = 8, 3, 7
BIMODAL = ["vggish", "bert"]
CHUNKINGS = {"ones": [1], "max_new": [4], "cycle": [3, 1, 4, 2]}
TOL = 1e-4          # tests/test_heads_gpu.py:40 and LFAN_TOL of tests/test_stream_gpu.py: the offline forwards' bar
_TIME = {"video": 1}


def _pkg():
    from feature_vs_text_compound_emotion_amd import window_stream
    return window_stream


def _lfan(mods, sd, task="CLASSIFICATION", n_cls=NCLS):
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.lfan import LFAN
    m = LFAN(backbone_settings={}, output_dim=n_cls, task=task, modality=mods, example_length=W, kernel_size=5,
             tcn_channel=synth.TCN_CHANNELS, modal_dim=32, num_heads=2, root_dir="", device="cuda", head_hw=5)
    m.init(load_backbone=False)
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


@functools.lru_cache(maxsize=None)
def _bimodal(seed=9, task="CLASSIFICATION"):
    from feature_vs_text_compound_emotion_amd import synth
    return _lfan(BIMODAL, synth.lfan_state_dict(BIMODAL, n_cls=NCLS, seed=seed), task=task)


@functools.lru_cache(maxsize=None)
def _data(streams=3, total=19, seed=10):
    from feature_vs_text_compound_emotion_amd import synth
    x, _ = synth.make_clip_batch(BIMODAL, streams, total, seed=seed)
    return {m: v.cuda() for m, v in x.items()}


def _frames(x, t0, c, streams=None):
    return {m: (v if streams is None else v[streams]).narrow(_TIME.get(m, 2), t0, c).contiguous() for m, v in x.items()}


def _split(per, logits, counts):
    assert logits.shape == (sum(counts), logits.shape[1]) and len(counts) == len(per)
    at = 0
    for s, c in enumerate(counts):
        per[s].append(logits[at:at + c])
        at += c


def _push_all(stream, x, n, cycle):
    """Push the first n frames of every stream in chunks of ``cycle``, then finish -> one [n, n_out] per stream."""
    per, pos, i = [[] for _ in range(stream.streams)], 0, 0
    while pos < n:
        c = min(cycle[i % len(cycle)], n - pos)
        _split(per, *stream.push(_frames(x, pos, c)))
        pos, i = pos + c, i + 1
        assert stream.frames_seen == [pos] * stream.streams and stream.emitted == [max(pos - W, 0)] * stream.streams
    _split(per, *stream.finish())
    assert stream.frames_seen == stream.emitted == stream.windows_done == [0] * stream.streams
    return [torch.cat(p) for p in per]


@functools.lru_cache(maxsize=None)
def _offline(n):
    """The offline evaluator on the first n frames of stream 0, one window per forward."""
    from feature_vs_text_compound_emotion_amd.trainer import Trainer
    model = _bimodal()
    tr = Trainer(model, device="cuda", window_length=W, hop_length=H, number_classes=NCLS)
    tr.eval_frame_budget = W
    model.example_length = min(n, W)          # the offline forward insists on it; a video below W frames is one short window
    try:
        with torch.no_grad():
            return tr.inference_forward_windows(_frames(_data(), 0, n, slice(0, 1)), aggregate="device")[0]
    finally:
        model.example_length = W


# ---------------------------------------------------------------------------------------------- 1. the offline evaluator's bits
@pytest.mark.parametrize("n", [5, 8, 14, 19])
def test_live_logits_are_the_offline_evaluators_bits(n):
    ws = _pkg()
    want = _offline(n)
    assert want.shape == (n, NCLS)
    x = _frames(_data(), 0, n, slice(0, 1))
    for name, cycle in CHUNKINGS.items():
        got = _push_all(ws.WindowStream(_bimodal(), 1, W, H, max_new=4, window_batch=1), x, n, cycle)[0]
        assert torch.equal(got, want), (n, name)
    # one push of everything: several windows of the stream complete in one call and run in successive rounds
    assert torch.equal(_push_all(ws.WindowStream(_bimodal(), 1, W, H, max_new=32), x, n, [n])[0], want)
    # max_new below the push: the stream cuts it itself
    assert torch.equal(_push_all(ws.WindowStream(_bimodal(), 1, W, H, max_new=2), x, n, [5])[0], want)


# ---------------------------------------------------------------------------------------------- 2. chunking, neighbours, reset
def test_a_stream_among_ragged_neighbours_equals_itself_alone():
    ws = _pkg()
    x, model = _data(), _bimodal()
    lengths, rates = [19, 14, 11], [[3, 1, 4, 2], [1], [4, 0, 2]]
    for batch in (1, 2):
        alone = [_push_all(ws.WindowStream(model, 1, W, H, max_new=4, window_batch=batch), _frames(x, 0, n, slice(s, s + 1)), n,
                           [4])[0] for s, n in enumerate(lengths)]
        stream = ws.WindowStream(model, 3, W, H, max_new=4, window_batch=batch)
        per, pos, i = [[], [], []], [0, 0, 0], 0
        while pos != lengths:
            counts = [min(r[i % len(r)], n - p) for r, n, p in zip(rates, lengths, pos)]
            X = {m: torch.cat([x[m][s, 0, p:p + c] for s, (p, c) in enumerate(zip(pos, counts))]) for m in BIMODAL}
            _split(per, *stream.push_features_ragged(X, counts))
            pos, i = [p + c for p, c in zip(pos, counts)], i + 1
            if pos[2] == lengths[2] and stream.frames_seen[2]:      # stream 2 ends while the others run on
                _split(per, *stream.finish([2]))
        _split(per, *stream.finish([0, 1]))
        for s in range(3):
            assert torch.equal(torch.cat(per[s]), alone[s]), (batch, s)
        if batch == 1:
            assert torch.equal(alone[0], _offline(19))


def test_reset_of_one_stream_leaves_the_others_bits_alone():
    ws = _pkg()
    x, model = _data(), _bimodal()
    calm = _push_all(ws.WindowStream(model, 2, W, H, max_new=4), _frames(x, 0, 19, slice(0, 2)), 19, [3, 1])
    stream = ws.WindowStream(model, 2, W, H, max_new=4)
    per = [[], []]
    for t0 in range(0, 12, 4):
        _split(per, *stream.push(_frames(x, t0, 4, slice(0, 2))))
    stream.reset([1])
    assert stream.frames_seen == [12, 0] and stream.emitted == [4, 0] and stream.windows_done == [2, 0]
    late = [[], []]
    for t0 in range(12, 19):        # stream 0 goes on; stream 1 starts over with stream 2's frames
        feats = {m: torch.stack([x[m][0, 0, t0:t0 + 1], x[m][2, 0, t0 - 12:t0 - 11]]) for m in BIMODAL}
        _split(late, *stream.push_features(feats))
    _split(late, *stream.finish())
    assert torch.equal(torch.cat(per[0] + late[0]), calm[0])
    fresh = _push_all(ws.WindowStream(model, 1, W, H, max_new=4), _frames(x, 0, 7, slice(2, 3)), 7, [1])[0]
    assert torch.equal(torch.cat(late[1]), fresh)


def test_a_later_load_state_dict_is_honoured():
    from feature_vs_text_compound_emotion_amd import synth
    ws = _pkg()
    model = _lfan(BIMODAL, synth.lfan_state_dict(BIMODAL, n_cls=NCLS, seed=9))
    x = _frames(_data(), 0, 14, slice(0, 1))
    stream = ws.WindowStream(model, 1, W, H, max_new=4)
    first = _push_all(stream, x, 14, [4])[0]
    model.load_state_dict(synth.lfan_state_dict(BIMODAL, n_cls=NCLS, seed=77), strict=True)
    again = _push_all(stream, x, 14, [4])[0]
    assert torch.equal(again, _push_all(ws.WindowStream(model, 1, W, H, max_new=4), x, 14, [4])[0])
    assert not torch.equal(again, first)
    model.train()
    with pytest.raises(RuntimeError, match="train mode"):
        stream.push(_frames(x, 0, 1))
    assert stream.frames_seen == [0]


def test_regression_is_the_mean_of_the_windows_tanh_and_window_forward_is_push_and_finish():
    from feature_vs_text_compound_emotion_amd.trainer import windowing
    ws = _pkg()
    n, x = 19, _frames(_data(), 0, 19, slice(0, 2))
    cls, reg = _bimodal(), _bimodal(task="REGRESSION")
    got = ws.window_forward(reg, x, W, H, chunk=4)
    assert got.shape == (2, n, NCLS)
    assert torch.equal(got, torch.stack(_push_all(ws.WindowStream(reg, 2, W, H, max_new=4), x, n, [4])))
    assert torch.equal(ws.window_forward(cls, _frames(x, 0, n, slice(0, 1)), W, H, chunk=4)[0], _offline(n))
    acc, cnt = np.zeros((n, NCLS), np.float32), np.zeros(n, np.float32)
    for wd in windowing(np.arange(n), W, H):
        with torch.no_grad():
            logits = cls(_frames(x, int(wd[0]), W, slice(0, 1)))[0]
        acc[wd] = acc[wd] + torch.tanh(logits.cpu().double()).float().numpy()      # ops.tanh_fwd: double tanh, rounded once
        cnt[wd] += 1
    assert torch.equal(got[0].cpu(), torch.from_numpy(acc / cnt[:, None]))


# ---------------------------------------------------------------------------------------------- 3. the float64 oracle
def _build_head(name, sd):
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.fusion_heads import CAN, JMT
    mods = ["video", "vggish"]
    if name == "CAN":
        m = CAN(task="CLASSIFICATION", modalities=mods, tcn_settings=synth.TCN_SETTINGS, backbone_settings={}, output_dim=NCLS,
                root_dir="", device="cuda", load_backbone=False)
    else:
        m = JMT(task="CLASSIFICATION", modalities=mods, tcn_settings=synth.TCN_SETTINGS, backbone_settings={}, output_dim=NCLS,
                root_dir="", device="cuda", model_name=name, load_backbone=False)
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


@pytest.mark.parametrize("name", ["JMT", "MT", "CAN", "LFAN"])
def test_windowed_live_logits_against_float64_windows_of_the_oracle(name):
    """W = 8, H = 3, n = 19 in chunks of 4, 40 x 40 frames through IR-50: every window through the float64 oracle forward,
    stitched in numpy.  A stitch is a convex combination of window outputs, so it adds nothing to the offline forwards' bar."""
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.trainer import windowing
    from oracle.jmt import can_forward, jmt_forward
    from oracle.lfan import lfan_forward
    ws = _pkg()
    n = 19
    if name == "LFAN":
        mods = ["video", "vggish", "bert"]
        sd = synth.lfan_state_dict(mods, n_cls=NCLS, seed=31)
        model, oracle = _lfan(mods, sd), lambda xs, sdd: lfan_forward(xs, sdd, mods)
    else:
        mods = ["video", "vggish"]
        spec, alias = synth.can_spec(mods) if name == "CAN" else synth.jmt_spec(mods, name)
        sd = synth.make_state_dict(spec, alias, seed=32)
        model = _build_head(name, sd)
        oracle = (lambda xs, sdd: can_forward(xs, sdd, mods)) if name == "CAN" else \
            (lambda xs, sdd: jmt_forward(xs, sdd, mods, model_name=name))
    x, _ = synth.make_clip_batch(mods, 1, n, hw=40, seed=33)
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    acc, cnt = np.zeros((n, NCLS)), np.zeros(n)
    for wd in windowing(np.arange(n), W, H):
        with torch.no_grad():
            o = oracle({m: v.narrow(_TIME.get(m, 2), int(wd[0]), W).double() for m, v in x.items()}, sd64)
        acc[wd] += o[0].numpy()
        cnt[wd] += 1
    want = acc / cnt[:, None]
    got = _push_all(ws.WindowStream(model, 1, W, H, max_new=4), {m: v.cuda() for m, v in x.items()}, n, [4])[0]
    err = np.abs(got.cpu().double().numpy() - want).max()
    print(f"{name} windowed live logits, n = {n}, against float64 oracle windows: {err:.3e} (bar {TOL:.0e})")
    assert got.shape == (n, NCLS) and err < TOL, err
