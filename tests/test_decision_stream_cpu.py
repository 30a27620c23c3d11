"""``DecisionStream`` without a GPU: the entries are declared, exported and bound and refuse bad descriptors before any launch;
the host class refuses what it cannot run with no state changed; the segment table has its documented layout; the mirror
(``decision_ref``) agrees with ``collections.Counter`` and numpy on hand-written rows; and the seeded inputs of
``tests/test_decision_stream_gpu.py`` keep the share of rows whose mean-probability decision is too close to compare under
its cap, by the mirror alone."""
import ctypes
from collections import Counter

import numpy as np
import pytest
import torch

import decision_ref as ref

ENTRIES = ("cer_decision_stream_push", "cer_decision_stream_read")


def _lib():
    from feature_vs_text_compound_emotion_amd import _lib
    from feature_vs_text_compound_emotion_amd.build import build
    build(verbose=False)
    return _lib, _lib.load()


def test_entries_are_declared_exported_and_bound():
    import test_abi_cpu
    mod, lib = _lib()
    for name in ENTRIES:
        assert name in mod.exported_symbols() and name in test_abi_cpu._header_functions()
        assert getattr(ctypes.CDLL(mod.LIB_PATH), name) is not None
        assert getattr(lib, name).argtypes[0]._type_ is mod.DecisionStreamDesc


def test_public_name_is_exported_from_the_package():
    import feature_vs_text_compound_emotion_amd as pkg
    from feature_vs_text_compound_emotion_amd import decisions
    assert pkg.DecisionStream is decisions.DecisionStream


# a non-null pointer the library must never dereference on these paths: a host buffer
_BUF = (ctypes.c_double * 64)()
_P = ctypes.c_void_p(ctypes.addressof(_BUF))


def _desc(mod, **kw):
    base = dict(S=2, C=7, M=5, max_count=3, W=0, R=0, drop_last=0, classify=1)
    base.update(kw)
    return mod.DecisionStreamDesc(**base)


def _push(lib, d, **nulls):
    a = {n: _P for n in ("rows", "segments", "votes", "first", "slog", "sprob", "zring", "track", "track_means")}
    a.update(nulls)
    return lib.cer_decision_stream_push(ctypes.byref(d) if d is not None else None, a["rows"], a["segments"], 2, a["votes"],
                                        a["first"], a["slog"], a["sprob"], a["zring"], a["track"], a["track_means"], None)


def _read(lib, d, **nulls):
    a = {n: _P for n in ("table", "votes", "first", "slog", "sprob", "zring", "decisions", "means")}
    a.update(nulls)
    return lib.cer_decision_stream_read(ctypes.byref(d) if d is not None else None, a["table"], a["votes"], a["first"], a["slog"],
                                        a["sprob"], a["zring"], a["decisions"], a["means"], None)


REFUSED = [
    ("C = 1", dict(C=1)),
    ("C = 17", dict(C=17)),
    ("S = 0", dict(S=0)),
    ("M = 0", dict(M=0)),
    ("max_count = 0", dict(max_count=0)),
    ("max_count < 0", dict(max_count=-2)),
    ("R = 12 is no power of two", dict(W=5, R=12)),
    ("R = 0 under a window", dict(W=5, R=0)),
    ("W + max_count = 9 > R = 8", dict(W=6, R=8)),
    ("W + max_count overflows an int", dict(W=2 ** 31 - 1, R=2 ** 30)),
    ("W < 0", dict(W=-1, R=8)),
    ("drop_last with C = 2", dict(C=2, drop_last=1)),
    ("drop_last without classify", dict(drop_last=1, classify=0)),
]


@pytest.mark.parametrize("what,kw", REFUSED, ids=[r[0] for r in REFUSED])
def test_both_entries_refuse_bad_descriptors_without_a_gpu(what, kw):
    mod, lib = _lib()
    assert _push(lib, _desc(mod, **kw)) == -1 and b"decision_stream_push" in lib.cer_last_error(), what
    assert _read(lib, _desc(mod, **kw)) == -1 and b"decision_stream_read" in lib.cer_last_error(), what


@pytest.mark.parametrize("window", [0, 5])
def test_both_entries_refuse_null_pointers_without_a_gpu(window):
    mod, lib = _lib()
    d = _desc(mod, W=window, R=8 if window else 0)
    state = ("zring",) if window else ("votes", "first", "slog", "sprob")
    assert _push(lib, None) == -1 and b"decision_stream_push" in lib.cer_last_error()
    assert _read(lib, None) == -1 and b"decision_stream_read" in lib.cer_last_error()
    for name in ("rows", "segments") + state:
        assert _push(lib, d, **{name: None}) == -1 and b"decision_stream_push: null" in lib.cer_last_error(), name
    for name in ("table", "decisions", "means") + state:
        assert _read(lib, d, **{name: None}) == -1 and b"decision_stream_read: null" in lib.cer_last_error(), name
    # a regression stream has no votes, no probabilities and no decisions; a track of decisions is refused for it
    r = _desc(mod, W=window, R=8 if window else 0, C=2, classify=0)
    assert _push(lib, r, track=_P) == -1 and b"decision_stream_push" in lib.cer_last_error()


def test_host_class_refuses_bad_arguments_with_no_state_changed():
    from feature_vs_text_compound_emotion_amd import DecisionStream
    for kw in (dict(n_out=1), dict(n_out=17), dict(streams=0), dict(max_new=0), dict(window=0), dict(window=2.5),
               dict(n_out=2, drop_last=True), dict(task="REGRESSION", drop_last=True), dict(task="JMT")):
        with pytest.raises(ValueError):
            DecisionStream(**{"n_out": 7, "streams": 2, **kw})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DecisionStream(7, 2, device="cpu")
    for window in (None, 4):
        ds = DecisionStream(7, 3, window=window, max_new=4)
        rows = torch.zeros(5, 7)
        with pytest.raises(ValueError, match="GPU"):
            ds.push_ragged(rows, [2, 0, 3])
        with pytest.raises(ValueError, match="GPU"):
            ds.push_rows(torch.zeros(6, 7))
        for counts in ([2, 3], [2, 0, 5], [2, -1, 4], 5):
            with pytest.raises(ValueError, match="counts"):
                ds.push_ragged(rows, counts)
        assert ds.frames_seen == [0, 0, 0] and ds._pos == [0, 0, 0] and ds.state is None
        with pytest.raises(IndexError):
            ds.reset([3])


def test_segment_table_layout():
    from feature_vs_text_compound_emotion_amd import ops
    big = (5 << 32) + 0x9abcdef0                      # low word has its top bit set, high word 5
    segs = [(0, 3, 0, 7, 0), (2, 1, 3, 2 ** 30 - 1, 2 ** 31 - 3), (4, 8, 4, 2 ** 30 + 6, big), (1, 0, 12, 3 * 2 ** 30, 2 ** 32)]
    t = ops.decision_segment_table(segs, "cpu")
    assert t.dtype == torch.int32 and tuple(t.shape) == (ops.DECISION_FIELDS, 4) == (6, 4) and t.is_contiguous()
    assert t[0].tolist() == [0, 2, 4, 1] and t[1].tolist() == [3, 1, 8, 0] and t[2].tolist() == [0, 3, 4, 12]
    assert t[3].tolist() == [7, 2 ** 30 - 1, 6, 0]                                # positions modulo 2^30
    lo, hi = t[4].to(torch.int64) & 0xffffffff, t[5].to(torch.int64) & 0xffffffff
    assert ((hi << 32) | lo).tolist() == [0, 2 ** 31 - 3, big, 2 ** 32]           # the split 64-bit counts
    assert t[4].tolist()[2] < 0                                                    # stored as the int32 with those bits
    for bad in ((0, -1, 0, 0, 0), (0, 1, -1, 0, 0), (0, 1, 0, -1, 0), (0, 1, 0, 0, -1), (0, 1, 0, 0, 2 ** 63), (0, 1, 2 ** 31, 0, 0)):
        with pytest.raises(ValueError):
            ops.decision_segment_table([bad], "cpu")
    with pytest.raises(ValueError):
        ops.decision_segment_table([], "cpu")


def test_wrappers_reject_cpu_state_and_rows():
    from feature_vs_text_compound_emotion_amd import ops
    state = ops.decision_stream_state(2, 7, device="cpu")
    assert sorted(state) == ["first", "slog", "sprob", "votes"] and state["first"].unique().tolist() == [2 ** 63 - 1]
    assert tuple(ops.decision_stream_state(2, 7, window=37, max_new=8, device="cpu")["zring"].shape) == (2, 64, 7)
    assert tuple(ops.decision_stream_state(2, 7, window=1, max_new=3, device="cpu")["zring"].shape) == (2, 4, 7)
    table = ops.decision_segment_table([(0, 1, 0, 0, 0)], "cpu")
    with pytest.raises(ValueError, match="GPU"):
        ops.decision_stream_push(torch.zeros(1, 7), table, 1, state)
    with pytest.raises(ValueError, match="GPU"):
        ops.decision_stream_read(table, 1, state)


# ------------------------------------------------------------------------------------------------ the mirror's own rules
def test_mirror_vote_ties_follow_counter_most_common():
    c = 4
    frames = [2, 0, 2, 0, 3, 3, 1]                     # 2, 0 and 3 tie at two votes; 2 was seen first
    z = np.eye(c, dtype=np.float32)[frames] * 5
    assert Counter(frames).most_common(1)[0][0] == 2
    t = ref.track(z)
    want = [Counter(frames[:i + 1]).most_common(1)[0][0] for i in range(len(frames))]
    assert t["decisions"][:, 0].tolist() == want == [2, 2, 2, 2, 2, 2, 2]
    assert ref.track(z[1:])["decisions"][:, 0].tolist() == [0, 0, 0, 0, 0, 0]      # without the first frame, 0 leads the tie
    # inside a window the first occurrence counts from the window's oldest row: rows 3 .. 6 are 0, 3, 3, 1 -> 3; rows 1 .. 4
    # are 0, 2, 0, 3 -> 0
    w = ref.track(z, window=4)
    assert w["decisions"][6, 0] == 3 and w["decisions"][4, 0] == 0
    assert np.array_equal(w["decisions"][:4], t["decisions"][:4])
    for i in range(len(frames)):
        lo = max(0, i + 1 - 4)
        assert w["decisions"][i, 0] == Counter(frames[lo:i + 1]).most_common(1)[0][0]
        assert np.array_equal(ref.decide(z[lo:i + 1])[0], w["decisions"][i])


def test_mirror_equal_maxima_and_non_finite_rows_follow_numpy():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    z = np.array([[1, 3, 3, 0], [0, 2, nan, nan], [inf, 1, 1, 1], [0, 0, 0, 0]], dtype=np.float32)
    assert ref.track(z)["decisions"][:, 0].tolist() == [1, 1, 1, 0] and np.argmax(z, axis=1).tolist() == [1, 2, 0, 0]
    t = ref.track(z)
    # the first NaN wins: column 2 of the mean logits; a NaN logit makes every probability of its row NaN, so column 0
    assert t["decisions"][1].tolist() == [1, 2, 0]
    assert np.isnan(t["mean_outputs"][3, 2:]).all() and np.isposinf(t["mean_outputs"][3, 0])
    assert ref.track(z, window=2)["decisions"][3].tolist() == [0, 0, 0]      # rows 2, 3: +inf mean logit; inf / inf = NaN in column 0
    assert ref.track(z, window=1)["decisions"][3].tolist() == [0, 0, 0] and not np.isnan(ref.track(z, window=1)["mean_probs"][3]).any()
    # a logit of 100 overflows float32's exp: NaN in that column only; rows of -200 underflow: NaN everywhere
    over = np.array([[0, 100, 0]], dtype=np.float32)
    p = ref.frame_probs(over)
    assert np.isnan(p[0, 1]) and p[0, 0] == 0 and p[0, 2] == 0 and ref.decide(over)[0].tolist() == [1, 1, 1]
    assert np.isnan(ref.frame_probs(np.full((1, 3), -200, dtype=np.float32))).all()
    plain = np.array([[0.5, -1.0, 2.0]], dtype=np.float32)
    e = np.exp(plain.astype(np.float64))
    assert np.array_equal(ref.frame_probs(plain), e / e.sum())
    assert ref.top_two_gap(np.array([0.2, np.nan, 0.1])) == np.inf and abs(ref.top_two_gap(np.array([0.2, 0.5, 0.1])) - 0.3) < 1e-15
    d = ref.decide(np.array([[0, 1, 9], [0, 1, 9]], dtype=np.float32), drop_last=True)
    assert d[0].tolist() == [1, 1, 1] and d[1].shape == (2,)


def test_mirror_cumsum_is_the_time_ordered_chain():
    z = ref.random_logits(1, 300, 7)
    chain = np.zeros(7)
    for t in range(300):
        chain = chain + z[t].astype(np.float64)
    assert np.array_equal(ref.track(z)["mean_outputs"][-1], chain / 300)
    assert np.array_equal(ref.means_only(z[:, :2])[-1], chain[:2] / 300)
    assert np.array_equal(ref.means_only(z[:, :2], window=5)[-1], ref.track(z, window=5)["mean_outputs"][-1][:2])
    assert np.array_equal(ref.track(z, start=10)["mean_outputs"][-1], chain / 310)


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
def test_seeded_inputs_keep_the_skipped_share_under_its_cap():
    gaps = []
    for name, c, frames in ref.PREFIX_SEQUENCES:
        z = ref.prefix_sequence(name)
        assert z.shape == (frames, c) and z.dtype == np.float32
        g = ref.track(z)["gap"]
        assert ref.skipped_share(g) <= ref.SKIP_CAP, (name, ref.skipped_share(g))
        gaps.append(g)
    assert {c for _, c, _ in ref.PREFIX_SEQUENCES} == {2, 7, 8, 16}
    for s, z in enumerate(ref.stream_sequences()):
        for window in (None,) + ref.WINDOWS:
            g =ref.track(z, window=window)["gap"]
            assert ref.skipped_share(g) <= ref.SKIP_CAP, (s, window, ref.skipped_share(g))
    # the running decisions do move along these sequences: the test is about every prefix, not about one answer
    d = ref.track(ref.prefix_sequence("c7"))["decisions"]
    assert len(set(d[:, 0].tolist())) > 1 and len(set(d[:, 2].tolist())) > 1


def test_offline_comparison_videos_keep_the_skipped_share_under_its_cap():
    import eval_ref
    for name in ref.OFFLINE_CASES:
        data, n_cls, ic = ref.offline_videos(name)
        drop = ic is not None
        gaps = [ref.decide(e["logits"], drop_last=drop)[3] for e in data.values()]
        assert ref.skipped_share(gaps) <= ref.SKIP_CAP, (name, ref.skipped_share(gaps))
        assert all(eval_ref.is_exact(e["logits"]) for e in data.values()) == (name != "ignore_class")
        if name == "random_exact":
            continue
        case = eval_ref.get_case(name)
        # the mirror is the reference's own function on these videos
        ic = case.n_cls - 1 if drop else None
        mine = np.array([ref.decide(e["logits"], drop_last=drop)[0] for i, e in enumerate(case.data.values()) if i in case.kept[ic]])
        assert np.array_equal(mine[:, 0], case.video_preds[ic][:, 0])


def test_ragged_schedule_has_what_the_issue_lists():
    ticks = ref.ragged_schedule([ref.STREAM_FRAMES] * 5, 8, seed=3)
    flat = [c for t in ticks for c in t]
    assert set(flat) == set(range(9)) and [sum(t[s] for t in ticks) for s in range(5)] == [ref.STREAM_FRAMES] * 5
    assert all(t[1] == 0 for t in ticks[:4]) and any(sum(t) == 1 and max(t) == 1 for t in ticks)
    for w in ref.WINDOWS:
        for m in ref.MAX_NEWS:
            r = 1
            while r < w + m:
                r *= 2
            assert ref.STREAM_FRAMES >= 3 * r, (w, m, r)      # the ring wraps at least three times
