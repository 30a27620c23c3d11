"""The live audio-visual session without a GPU: the pairing rule of ``AVStream`` against the offline rule of
``MultimodalFeatureExtractor.audio_features`` (``use = min(n, L)``, repeat the last row), the row tables, the ring bounds the
session derives, and every refusal that must come before a launch."""
import ctypes
import random

import pytest
import torch

FRAMES = (0, 1, 3, 4, 6, 40)
EXAMPLES = (0, 1, 4, 5, 41)
HOLD = LEAD = 41      # the longest side: the reference schedule (one side entirely before the other) stays inside


def _live():
    from feature_vs_text_compound_emotion_amd import live
    return live


def _feeds(L, n_pre, seed):
    """Interleavings of L frames and n_pre examples as ('v' | 'a', count) events."""
    rng = random.Random(seed)
    feeds = {"video first": [("v", L), ("a", n_pre)], "audio first": [("a", n_pre), ("v", L)],
             "one at a time": [e for i in range(max(L, n_pre)) for e in ((("v", 1),) if i < L else ()) + ((("a", 1),) if i < n_pre else ())]}
    for k in range(20):
        v, a, ev = L, n_pre, []
        while v or a:
            side = rng.choice([s for s, left in (("v", v), ("a", a)) if left])
            c = rng.randint(1, min(5, v if side == "v" else a))
            ev.append((side, c))
            v, a = (v - c, a) if side == "v" else (v, a - c)
        feeds[f"random {k}"] = ev
    return feeds


def _run(L, n, n_pre, events, hold=HOLD, lead=LEAD):
    """The session's bookkeeping on ints: check, advance, pair -- the order of ``AVStream.push`` and ``finish``."""
    live = _live()
    F = E = P = 0
    pairs = []
    for side, c in events:
        nf, ne = (c, E) if side == "v" else (0, E + c)
        wf, we = live.check_waiting(F, E, P, nf, ne, hold, lead)
        assert wf <= hold and we <= lead
        F, E = F + nf, ne
        new = live.pair_schedule(F, E, P)
        P += len(new)
        pairs += new
        assert F - P <= hold and max(E - F, 0) <= lead and P == min(F, E)
    assert (F, E) == (L, n_pre)
    pairs += live.pair_schedule(F, n, P, final=n)
    return pairs


@pytest.mark.parametrize("L", FRAMES)
@pytest.mark.parametrize("n", EXAMPLES)
def test_pairs_equal_the_offline_rule_under_any_interleaving(L, n):
    want = [(i, min(i, n - 1)) for i in range(L)] if n > 0 else []
    for n_pre in sorted({0, n // 2, max(n - 1, 0), n}):     # how many examples are complete before the stream ends
        feeds = _feeds(L, n_pre, seed=1000 * L + n)
        assert len(feeds) >= 23
        for name, events in feeds.items():
            assert _run(L, n, n_pre, events) == want, (name, n_pre)


def test_exceeding_hold_or_lead_is_refused_with_the_ints_unchanged():
    live = _live()
    with pytest.raises(ValueError, match="hold = 4"):
        _run(5, 0, 0, [("v", 3), ("v", 2)], hold=4)
    with pytest.raises(ValueError, match="lead = 2"):
        _run(0, 3, 3, [("a", 2), ("a", 1)], lead=2)
    # frames that arrive with the examples they pair with still count as waiting until the call has paired them
    with pytest.raises(ValueError, match="hold = 4"):
        live.check_waiting(10, 10, 10, 5, 15, 4, 8)
    assert live.check_waiting(10, 10, 10, 4, 14, 4, 8) == (4, 0)
    assert live.check_waiting(10, 12, 10, 0, 18, 4, 8) == (0, 8)
    state = (3, 7, 3)
    with pytest.raises(ValueError):
        live.check_waiting(*state, 0, 7 + 9, 4, 8)
    assert live.pair_schedule(*state) == [] and live.pair_schedule(5, 7, 3) == [(3, 3), (4, 4)]
    assert live.pair_schedule(6, 4, 4, final=4) == [(4, 3), (5, 3)] and live.pair_schedule(3, 0, 0, final=0) == []


def test_row_tables():
    from feature_vs_text_compound_emotion_amd import ops
    rs, rp = ops.stream_row_table([(1 << 30) - 2, 7, 0, (1 << 31) + 5], [3, 0, 2, 1], "cpu")
    assert rs.tolist() == [0, 0, 0, 2, 2, 3]                      # stream-major, a zero count has no row
    assert rp.tolist() == [(1 << 30) - 2, (1 << 30) - 1, 0, 0, 1, 5]   # time order, modulo 2^30
    assert rs.dtype == rp.dtype == torch.int32
    with pytest.raises(ValueError):
        ops.stream_row_table([0, 0], [1, -1], "cpu")
    ps, pp = ops.stream_pair_table([(2, (1 << 30) + 3), (0, 5), (2, 1)], "cpu")
    assert ps.tolist() == [2, 0, 2] and pp.tolist() == [3, 5, 1] and pp.dtype == torch.int32   # the caller's order
    with pytest.raises(ValueError):
        ops.stream_pair_table([(0, -1)], "cpu")


@pytest.mark.parametrize("hop_sec", [1 / 30, 1 / 25, 0.1])
@pytest.mark.parametrize("max_samples", [160, 1024, 4096])
def test_no_step_completes_more_examples_than_the_example_ring_allows(hop_sec, max_samples):
    from feature_vs_text_compound_emotion_amd import audio_stream as a
    from feature_vs_text_compound_emotion_amd.frames import hold_ring
    live = _live()
    hop = hop_sec * 100.0
    bound = live.examples_per_step(max_samples, hop)
    for lead in (1, 8):
        re = hold_ring(lead, bound)
        assert re >= lead + bound and re & (re - 1) == 0 and re < 2 * (lead + bound)
    rng = random.Random(int(hop * 1000) + max_samples)
    worst = 0
    for feed in ("full", "random"):
        state, total = (0, 0, 0), 40000
        while state[0] < total:
            c = max_samples if feed == "full" else rng.randint(1, max_samples)
            state, _, starts = a.schedule(*state, c, 96, hop)
            worst = max(worst, len(starts))
        limit = a.num_examples(a.num_rows(state[0] + a.PAD_SAMPLES), 96, hop)
        for c in a.pad_chunks(max_samples):
            state, _, starts = a.schedule(*state, c, 96, hop, limit)
            worst = max(worst, len(starts))
        assert state[2] == limit
    assert 1 <= worst <= bound
    assert bound <= worst + 2            # and the formula is not loose


def test_frame_ring_length():
    from feature_vs_text_compound_emotion_amd.frames import FrameStream, hold_ring
    assert [hold_ring(h, m) for h, m in ((64, 32), (4, 4), (5, 4), (1, 1), (3, 5))] == [128, 8, 16, 2, 8]
    fs = FrameStream(3, hold=5, max_new=3)
    assert fs.ring_frames == 8 and fs.ring is None and fs.held == [0, 0, 0]
    assert fs.crop_xyf.tolist() == [[4, 4, 0]] * 3          # GroupCenterCrop(40) of 48


def test_frame_stream_refuses_before_any_launch():
    from feature_vs_text_compound_emotion_amd.frames import FrameStream
    for kw in ({"streams": 0}, {"crop": 50}, {"hold": 0}, {"max_new": 0}, {"device": "cpu"}, {"std": 0.0},
               {"crop_xyf": [[9, 0, 0], [0, 0, 0]]}, {"crop_xyf": [[0, 0, 0]]}):
        with pytest.raises(ValueError):
            FrameStream(**{"streams": 2, **kw})
    fs = FrameStream(2, hold=4, max_new=3)
    u8 = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    bad = [(u8, [1, 1]),                                   # a CPU tensor
           (u8, [1]), (u8, [1, -1]), (u8, [4, 0]), (u8, 3), (u8, [1, 2]),      # counts
           (torch.zeros((2, 8, 8, 3)), [1, 1]),            # not uint8
           (torch.zeros((2, 8, 8, 4), dtype=torch.uint8), [1, 1]), (torch.zeros((2, 8, 8), dtype=torch.uint8), [1, 1])]
    for frames, counts in bad:
        with pytest.raises(ValueError):
            fs.push(frames, counts)
    fs.frames_seen = [3, 0]                                # three frames wait in stream 0
    with pytest.raises(ValueError, match="hold = 4"):
        fs.push(u8, [2, 0])
    with pytest.raises(ValueError, match="not held"):
        fs.take([(0, 3)])
    with pytest.raises(ValueError):
        fs.take([(2, 0)])
    assert fs.frames_seen == [3, 0] and fs.frames_taken == [0, 0] and fs.ring is None


def test_wrappers_refuse_cpu_and_wrong_dtype_tensors():
    from feature_vs_text_compound_emotion_amd import ops
    ring = torch.zeros((1, 8, 4, 4, 3), dtype=torch.uint8)
    i32 = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="u8ring"):
        ops.frames_stream_gather(ring, i32, i32)
    with pytest.raises(ValueError, match="u8ring"):
        ops.frames_stream_gather(ring.float(), i32, i32)
    tables = tuple(torch.zeros((6, 2), dtype=torch.int32) for _ in range(4))
    with pytest.raises(ValueError, match="u8ring"):
        ops.frames_stream_append(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), tables, 3, 6, torch.zeros((1, 3), dtype=torch.int32),
                                 i32, i32, 1, ring)


class _OnGpu(torch.Tensor):
    """A CPU tensor that says it is on the GPU: the wrappers ask ``is_cuda`` and compare devices, and every check runs before
    the library is loaded, so the refusals after the first can be reached without a GPU."""
    is_cuda = True


def test_clip_wrapper_refuses_by_argument_name_before_the_library_is_loaded():
    from feature_vs_text_compound_emotion_amd import ops
    gpu = lambda t: t.as_subclass(_OnGpu)      # noqa: E731
    frames = gpu(torch.zeros((2, 8, 8, 3), dtype=torch.uint8))      # two 8 x 8 frames, size 6, crop 4
    tables = tuple(gpu(torch.zeros((6, k), dtype=torch.int32)) for k in (2, 3, 2, 3))
    cx, out, u8 = gpu(torch.zeros((2, 3), dtype=torch.int32)), gpu(torch.zeros((2, 3, 4, 4))), gpu(torch.zeros((2, 4, 4, 3), dtype=torch.uint8))

    def call(frames=frames, tables=tables, cx=cx, group=1, out=out, u8=u8, **kw):
        ops.frames_transform(frames, tables, 8, 6, cx, group, 0.5, 0.5, out, u8, **kw)
    bad_table = lambda i, t: tables[:i] + (t,) + tables[i + 1:]      # noqa: E731
    for match, kw in (("frames: ", {"frames": torch.zeros((2, 8, 8, 3), dtype=torch.uint8)}),      # a CPU tensor
                      ("frames: ", {"frames": gpu(torch.zeros((2, 8, 8, 4), dtype=torch.uint8))}),
                      ("frames: ", {"frames": frames[:1]}),                                      # one frame for two rows of out
                      ("out: ", {"out": torch.zeros((2, 3, 4, 4))}),                             # a CPU float tensor
                      ("out: ", {"out": gpu(torch.zeros((2, 3, 4, 4), dtype=torch.float64))}),
                      ("out: ", {"out": gpu(torch.zeros((2, 4, 4, 3)))}),
                      ("out_u8: ", {"u8": gpu(torch.zeros((2, 4, 4, 3)))}),
                      ("out_u8: ", {"u8": u8[:1]}),
                      ("crop_xyf: ", {"cx": cx[:1]}),                                            # one entry for two groups
                      ("crop_xyf: ", {"group": 2}),                                              # two entries for one group
                      ("crop_xyf: ", {"cx": gpu(torch.zeros((2, 3), dtype=torch.int64))}),
                      ("frames_per_group", {"group": 0}),
                      ("hcoef: ", {"tables": bad_table(1, gpu(torch.zeros((6, 3), dtype=torch.int64)))}),
                      ("vbounds: ", {"tables": bad_table(2, gpu(torch.zeros((6, 2))))}),
                      ("hbounds: ", {"tables": bad_table(0, gpu(torch.zeros((5, 2), dtype=torch.int32)))}),
                      ("vcoef: ", {"tables": bad_table(3, torch.zeros((6, 3), dtype=torch.int32))}),
                      ("yuv: ", {"yuv": object()})):
        with pytest.raises(ValueError, match="^" + match):
            call(**kw)


def test_c_entries_refuse_before_any_launch():
    from feature_vs_text_compound_emotion_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))      # never dereferenced: every case below is refused first

    def append(frames=p, n=1, h=8, w=8, hks=3, vks=3, size=6, crop=4, span=3, rows=1, max_count=1, ring=p, s=1, rf=8):
        return lib.cer_frames_stream_append(frames, n, h, w, p, p, hks, p, p, vks, size, crop, p, span, p, p, rows, max_count, ring,
                                            s, rf, None)

    def gather(ring=p, s=1, rf=8, crop=4, rows=1, std=0.5, out=p):
        return lib.cer_frames_stream_gather(ring, s, rf, crop, p, p, rows, 0.5, std, out, None)

    for kw, text in (({"frames": None}, b"null"), ({"ring": None}, b"null"), ({"rf": 6}, b"power of two"), ({"rf": 0}, b"power of two"),
                     ({"crop": 7}, b"exceeds size"), ({"max_count": 9}, b"exceed Rf"), ({"rows": 65536}, b"65535"),
                     ({"n": 65536}, b"65535"), ({"h": 4096, "w": 4096, "span": 64}, b"LDS"), ({"n": 0}, b">= 1"), ({"s": 0}, b">= 1")):
        assert append(**kw) != 0, kw
        msg = lib.cer_last_error()
        assert msg.startswith(b"frames_stream_append:") and text in msg, (kw, msg)
    for kw, text in (({"ring": None}, b"null"), ({"out": None}, b"null"), ({"rf": 12}, b"power of two"), ({"rows": 65536}, b"65535"),
                     ({"rows": 0}, b">= 1"), ({"std": 0.0}, b"std")):
        assert gather(**kw) != 0, kw
        msg = lib.cer_last_error()
        assert msg.startswith(b"frames_stream_gather:") and text in msg, (kw, msg)


def _lfan(mods):
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.lfan import LFAN
    m = LFAN(backbone_settings={}, output_dim=7, task="CLASSIFICATION", modality=mods, example_length=4,
             tcn_channel=synth.TCN_CHANNELS, root_dir="", device="cpu")
    m.init(load_backbone=False)
    return m


def test_session_refuses_models_it_cannot_stream():
    live = _live()
    with pytest.raises(TypeError, match="LFAN or a CAN"):
        live.AVStream(torch.nn.Linear(2, 2), 1, 30)
    with pytest.raises(RuntimeError, match="train mode"):
        live.AVStream(_lfan(["vggish"]).train(), 1, 30)
    with pytest.raises(ValueError, match="'video'"):
        live.AVStream(_lfan(["vggish"]).eval(), 1, 30)
    with pytest.raises(ValueError, match="exactly one"):
        live.AVStream(_lfan(["vggish", "logmel"]).eval(), 1, 30)
