"""The four kernels of ``csrc/eval_metrics.hip`` behind every score the project reports, at the inputs where such kernels go
wrong without crashing: vote ties decided in different strides of the block, several equal maxima in a frame, the maximum
in the column ``ignore_class`` drops, C = 2 and C = 16, classes absent from targets and predictions, 5000-frame and 300-video
calls, NaN / inf / overflowing logits, and windows that overlap three and more deep.

Every expected value comes from the host mirror of the reference (``metrics.py``) or from the reference's stitch sequence
written out in ``eval_ref.stitch_ref``; the case tables and the conditions that make an exact comparison meaningful live in
``eval_ref.py`` and are checked without a GPU by ``test_eval_scores_cpu.py``.  The only device-against-device comparisons
are the multi-video stitch against the one-video stitch and batched ``add`` against per-video ``add``; both are pinned to the
host as well."""
import numpy as np
import pytest
import torch

import eval_ref as er

pytestmark = pytest.mark.gpu


def _same(a, b):
    if isinstance(a, dict):
        assert set(a) == set(b)
        for k in a:
            _same(a[k], b[k])
    elif a is None:
        assert b is None
    else:
        assert np.allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), atol=1e-12), (a, b)


def _accumulate(case, groups, label_dtype=torch.float32):
    """One ``add`` per group of videos (a group of one: without offsets).  -> (accumulator, {ignore: counts [4, C, C]},
    {ignore: per-video (vote, mean logits, mean probabilities) [V, 3]})."""
    from feature_vs_text_compound_emotion_amd.eval_device import DeviceEvalAccumulator
    acc = DeviceEvalAccumulator(case.n_cls, case.ignore, keep_video_predictions=True)
    for keys in groups:
        logits, labels, off = er.concat(case, keys)
        acc.add(torch.tensor(logits).cuda(), torch.tensor(labels).to(label_dtype).cuda(),
                video_offsets=None if len(keys) == 1 else off)
    counts = {ic: cm.cpu().numpy() for ic, cm in acc.cm.items()}
    triples = {ic: torch.cat([p for i, p in acc.video_predictions if i == ic]).cpu().numpy() for ic in case.ignore}
    return acc, counts, triples


def _assert_equals_host(case, acc, counts, triples):
    for ic in case.ignore:
        assert counts[ic].shape == (4, case.n_cls, case.n_cls) and counts[ic].dtype == np.int64
        wrong = [(k, got.tolist(), want.tolist()) for k, got, want in
                 zip(np.array(list(case.data))[case.kept[ic]], triples[ic][case.kept[ic]], case.video_preds[ic])
                 if not np.array_equal(got, want)]
        assert not wrong, f"{case.name} ignore={ic}: (video, device, host) {wrong[:8]}"
        assert np.array_equal(counts[ic], case.counts[ic]), (case.name, ic, np.argwhere(counts[ic] != case.counts[ic])[:8])
    _same(acc.compute(), case.perf)


# ---------------------------------------------------------------------------------------------------- the accumulator
@pytest.mark.parametrize("mode", ["one_call", "per_video"])
@pytest.mark.parametrize("name", list(er.ACCUMULATOR_CASES))
def test_counts_decisions_and_scores_equal_the_host(name, mode):
    case = er.get_case(name)
    keys = list(case.data)
    groups = [keys] if mode == "one_call" else [[k] for k in keys]
    _assert_equals_host(case, *_accumulate(case, groups))


def test_long_and_many_three_paths_give_identical_counts():
    """The 5000-frame video and 300 short ones: all in one call, one by one, and the long one alone followed by the 300 in
    one call -- the same counts and decisions in the three paths (and, by the test above, the host's)."""
    case = er.get_case("long_and_many")
    keys = list(case.data)
    assert len(case.data[keys[0]]["labels"]) == 5000 and len(keys) == 301
    runs = [_accumulate(case, g) for g in ([keys], [[k] for k in keys], [keys[:1], keys[1:]])]
    for acc, counts, triples in runs:
        assert np.array_equal(counts[None], runs[0][1][None]) and np.array_equal(triples[None], runs[0][2][None])
    _assert_equals_host(case, *runs[2])


@pytest.mark.parametrize("c", [1, 17])
def test_class_counts_outside_2_to_16_are_refused(c):
    from feature_vs_text_compound_emotion_amd.eval_device import DeviceEvalAccumulator
    acc = DeviceEvalAccumulator(c)
    with pytest.raises(RuntimeError, match="2 <= C <= 16"):
        acc.add(torch.zeros(6, c).cuda(), torch.zeros(6).cuda())
    assert int(acc.cm[None].sum()) == 0 and int(acc.bad.item()) == 0


@pytest.mark.parametrize("name", ["label_batch", "ignore_class"])
def test_int64_labels_count_like_float32_labels(name):
    case = er.get_case(name)
    keys = list(case.data)
    _, as_float, vp_float = _accumulate(case, [keys], torch.float32)
    acc, as_long, vp_long = _accumulate(case, [keys[:2], keys[2:3], keys[3:]], torch.int64)
    for ic in case.ignore:
        assert np.array_equal(as_float[ic], as_long[ic]) and np.array_equal(vp_float[ic], vp_long[ic])
    _assert_equals_host(case, acc, as_long, vp_long)


@pytest.mark.parametrize("how", ["mixed", "range"])
def test_a_bad_video_inside_a_batch_makes_compute_raise(how):
    from feature_vs_text_compound_emotion_amd.eval_device import DeviceEvalAccumulator
    case = er.get_case("label_batch")
    logits, labels, off = er.bad_labels(case, how)
    assert len(off) == 6
    acc = DeviceEvalAccumulator(case.n_cls)
    acc.add(torch.tensor(logits).cuda(), torch.tensor(labels).cuda(), video_offsets=off)
    with pytest.raises(AssertionError, match="labels outside"):
        acc.compute()
    good = DeviceEvalAccumulator(case.n_cls)                      # the same call with the labels it should have had
    good.add(torch.tensor(logits).cuda(), torch.tensor(er.concat(case)[1]).cuda(), video_offsets=off)
    _same(good.compute(), case.perf)


# ---------------------------------------------------------------------------------------------------- window stitching
@pytest.mark.parametrize("win,hop,n", er.STITCH_GEOMETRIES)
def test_stitch_adds_overlapping_windows_in_the_reference_order(win, hop, n):
    from feature_vs_text_compound_emotion_amd.eval_device import stitch_windows
    _, _, starts, outs = er.window_set(n, win, hop, seed=win * 1000 + n)
    want = er.stitch_ref(outs, starts, n)
    got = stitch_windows(outs.cuda(), starts, n).cpu()
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} elements differ"


def _multi(videos):
    from feature_vs_text_compound_emotion_amd.eval_device import stitch_windows_multi
    starts, woff, foff = [], [0], [0]
    for n, _, st, _ in videos:
        starts += st
        woff.append(woff[-1] + len(st))
        foff.append(foff[-1] + n)
    return stitch_windows_multi(torch.cat([v[3] for v in videos]).cuda(), starts, woff, foff).cpu(), foff


@pytest.fixture(scope="module")
def multi_videos():
    """257 window sets of window length 8, what the host sequence gives for each, and what one launch per video gives."""
    from feature_vs_text_compound_emotion_amd.eval_device import stitch_windows
    videos = er.multi_videos(max(er.MULTI_V))
    host = [er.stitch_ref(o, st, n) for n, _, st, o in videos]
    alone = [stitch_windows(o.cuda(), st, n).cpu() for n, _, st, o in videos]
    return videos, host, alone


@pytest.mark.parametrize("v", er.MULTI_V)
def test_multi_video_stitch_equals_the_host_and_one_launch_per_video(multi_videos, v):
    videos, host, alone = multi_videos
    got, foff = _multi(videos[:v])
    assert tuple(got.shape) == (foff[-1], er.STITCH_CLASSES)
    for k in range(v):                                  # video by video: a wrong binary search shows as a whole video off
        rows = got[foff[k]:foff[k + 1]]
        assert torch.equal(rows, host[k]), (v, k)
        assert torch.equal(rows, alone[k]), (v, k)


@pytest.mark.parametrize("geometries", [((300, 70, 650), (300, 200, 301), (300, 200, 300)), ((1, 1, 5), (1, 1, 1), (1, 1, 3))])
def test_multi_video_stitch_at_the_long_window_and_at_window_length_one(geometries):
    from feature_vs_text_compound_emotion_amd.eval_device import stitch_windows
    videos = [er.window_set(n, win, hop, seed=70 + i) for i, (win, hop, n) in enumerate(geometries)]
    for order in ([0, 1, 2], [2, 0, 1], [1], [0, 2]):
        got, foff = _multi([videos[i] for i in order])
        for k, i in enumerate(order):
            n, _, st, o = videos[i]
            assert torch.equal(got[foff[k]:foff[k + 1]], er.stitch_ref(o, st, n)), (order, i)
            assert torch.equal(got[foff[k]:foff[k + 1]], stitch_windows(o.cuda(), st, n).cpu()), (order, i)


def test_a_nan_and_an_inf_stay_in_the_frame_and_class_of_their_window_element():
    from feature_vs_text_compound_emotion_amd.eval_device import stitch_windows
    n, win, starts, outs = er.window_set(30, 8, 2, seed=9)
    outs = outs.clone()
    (wa, ra, ca), (wb, rb, cb) = (4, 3, 2), (9, 7, 6)
    outs[wa, ra, ca], outs[wb, rb, cb] = float("nan"), float("inf")
    fa, fb = starts[wa] + ra, starts[wb] + rb
    assert fa != fb and er.overlap_depth(starts, win, n)[[fa, fb]].min() >= 3      # other windows add to the same frames
    want = er.stitch_ref(outs, starts, n)
    other = er.window_set(20, 8, 1, seed=10)
    multi, foff = _multi([other, (n, win, starts, outs), other])
    for got in (stitch_windows(outs.cuda(), starts, n).cpu(), multi[foff[1]:foff[2]]):
        assert torch.isnan(got).nonzero().tolist() == [[fa, ca]] and torch.isinf(got).nonzero().tolist() == [[fb, cb]]
        assert got[fb, cb] == float("inf")
        ok = torch.isfinite(want)
        assert int((~ok).sum()) == 2 and torch.equal(got[ok], want[ok])
    clean = er.stitch_ref(other[3], other[2], other[0])                # the neighbouring videos of the launch are untouched
    assert torch.equal(multi[:foff[1]], clean) and torch.equal(multi[foff[2]:], clean)


# ---------------------------------------------------------------------------------------------------- refusals
@pytest.fixture
def launches(monkeypatch):
    """Call counters around the three library entry points; the calls still go through."""
    from feature_vs_text_compound_emotion_amd import _lib
    lib = _lib.load()
    calls = {}
    for name in ("cer_eval_accumulate", "cer_window_stitch", "cer_window_stitch_multi"):
        fn = getattr(lib, name)
        calls[name] = 0

        def counted(*a, _fn=fn, _name=name):
            calls[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, counted)
    return calls


def test_bad_video_offsets_are_refused_before_any_launch(launches):
    from feature_vs_text_compound_emotion_amd.eval_device import DeviceEvalAccumulator
    acc = DeviceEvalAccumulator(7, (None, 6))
    logits, labels = torch.zeros(10, 7).cuda(), torch.zeros(10).cuda()
    for off in ([1, 10], [2, 5, 10],                                   # not starting at 0
                [0, 5, 5, 10], [0, 7, 3, 10],                          # not strictly rising
                [0, 5, 9], [0, 5, 12], [0, 11],                        # not ending at R
                [0], [10], [],                                         # shorter than two entries
                torch.tensor([0, 5, 12]), torch.tensor([0, 5, 5, 10]).cuda(), np.array([3, 10])):      # from a tensor or an array
        with pytest.raises(ValueError, match="video_offsets"):
            acc.add(logits, labels, video_offsets=off)
    assert launches == {"cer_eval_accumulate": 0, "cer_window_stitch": 0, "cer_window_stitch_multi": 0}
    assert all(int(cm.sum()) == 0 for cm in acc.cm.values()) and int(acc.bad.item()) == 0
    acc.add(logits, labels, video_offsets=torch.tensor([0, 4, 10]))    # a good call is counted: one launch per ignore setting
    assert launches["cer_eval_accumulate"] == 2
    assert [int(cm[0].sum()) for cm in acc.cm.values()] == [10, 10] and int(acc.bad.item()) == 0


UNCOVERED = [([0, 9], 17, "a gap between two starts larger than the window"),
             ([1, 5], 13, "the first window starts above 0"),
             ([0, 5], 14, "the last window ends before the video does")]


@pytest.mark.parametrize("starts,total,why", UNCOVERED)
def test_window_sets_that_leave_a_frame_uncovered_are_refused_before_any_launch(launches, starts, total, why):
    from feature_vs_text_compound_emotion_amd.eval_device import stitch_windows, stitch_windows_multi
    win = torch.ones(2, 8, 7).cuda()
    for st in (starts, starts[::-1]):
        with pytest.raises(ValueError, match="uncovered"):
            stitch_windows(win, st, total)
    three = torch.ones(3, 8, 7).cuda()
    with pytest.raises(ValueError, match="uncovered"):                 # the bad video after a good one, and before it
        stitch_windows_multi(three, [0] + starts, [0, 1, 3], [0, 8, 8 + total])
    with pytest.raises(ValueError, match="uncovered"):
        stitch_windows_multi(three, starts + [0], [0, 2, 3], [0, total, total + 8])
    assert launches == {"cer_eval_accumulate": 0, "cer_window_stitch": 0, "cer_window_stitch_multi": 0}, why
    # the nearest covered sets go through, are counted, and average to the ones they were given
    assert torch.equal(stitch_windows(win, [0, 8], 16).cpu(), torch.ones(16, 7))
    assert torch.equal(stitch_windows_multi(three, [0, 0, 5], [0, 1, 3], [0, 8, 21]).cpu(), torch.ones(21, 7))
    assert launches == {"cer_eval_accumulate": 0, "cer_window_stitch": 1, "cer_window_stitch_multi": 1}
