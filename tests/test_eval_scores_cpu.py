"""``eval_device.scores_from_confusion`` against the host mirror of the reference's sklearn flow (``metrics.per_class_f1``,
``compute_f1_score``, ``compute_class_acc``, ``compute_confusion_matrix``) on label lists expanded from the same counts, and
the self-checks of the case tables in ``eval_ref.py`` (what ``test_eval_edges_gpu.py`` runs on the kernels)."""
import numpy as np
import pytest
import torch

import eval_ref as er
from feature_vs_text_compound_emotion_amd import metrics
from feature_vs_text_compound_emotion_amd.eval_device import _check_coverage, _offsets, scores_from_confusion


def _lists(cm):
    """Counts [C, C] (rows = targets, columns = predictions) -> (targets, predictions), one entry per count."""
    t, p = np.nonzero(cm)
    reps = cm[t, p]
    return np.repeat(t, reps).tolist(), np.repeat(p, reps).tolist()


def _assert_scores_match(cm):
    trgs, preds = _lists(cm)
    assert len(trgs) == cm.sum() > 0
    got = scores_from_confusion(cm)
    f1s, _, classes = metrics.per_class_f1(trgs, preds)
    assert classes.tolist() == np.flatnonzero((cm.sum(0) + cm.sum(1)) > 0).tolist()      # absent classes are skipped
    for g, w in ((got["f1_per_class"], f1s),
                 (got["macro_f1"], metrics.compute_f1_score(trgs, preds, metrics.MACRO_F1)[1]),
                 (got["weighted_f1"], metrics.compute_f1_score(trgs, preds, metrics.W_F1)[1]),
                 (got["accuracy"], metrics.compute_class_acc(trgs, preds)),
                 (got["confusion"], metrics.compute_confusion_matrix(trgs, preds))):
        g, w = np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64)
        assert g.shape == w.shape and np.allclose(g, w, rtol=0.0, atol=1e-12), (cm, g, w)


@pytest.mark.parametrize("c", [2, 7, 8, 16])
def test_scores_from_random_counts_equal_the_host_scores(c):
    rng = np.random.default_rng(c)
    for i in range(200):
        cm = rng.integers(0, 40, (c, c))
        if i % 2:                                         # sparse: most cells empty
            cm *= rng.random((c, c)) < 0.3
        if i % 3 == 0:                                    # zero rows and columns: classes absent from both
            gone = rng.random(c) < 0.4
            gone[int(rng.integers(0, c))] = False
            cm[gone, :] = 0
            cm[:, gone] = 0
        if i % 5 == 0:
            cm[int(rng.integers(0, c)), :] = 0            # predicted, never a target
        if i % 7 == 0:
            cm[:, int(rng.integers(0, c))] = 0            # a target, never predicted
        if cm.sum() == 0:
            cm[0, c - 1] = 1
        _assert_scores_match(cm)


@pytest.mark.parametrize("c", [2, 7, 8, 16])
def test_scores_with_support_but_no_predictions_and_the_reverse(c):
    cm = np.zeros((c, c), dtype=np.int64)
    if c == 2:
        a = 0
        cm[:] = [[0, 7], [0, 3]]                          # class 0: support 7, never predicted
    else:
        a = c - 1
        cm[0, 0], cm[0, 1], cm[1, 1], cm[a, 0] = 5, 2, 3, 4   # class a: support 4, never predicted
    for m in (cm, cm.T.copy()):                           # transposed: class a is predicted and has no support
        _assert_scores_match(m)
        present = np.flatnonzero((m.sum(0) + m.sum(1)) > 0).tolist()
        assert (m[a].sum() == 0) != (m[:, a].sum() == 0)
        assert scores_from_confusion(m)["f1_per_class"][present.index(a)] == 0.0


@pytest.mark.parametrize("c", [2, 7, 8, 16])
def test_scores_of_a_single_class_matrix(c):
    for k in (0, c - 1):
        cm = np.zeros((c, c), dtype=np.int64)
        cm[k, k] = 11
        _assert_scores_match(cm)
        got = scores_from_confusion(cm)
        assert got["f1_per_class"].tolist() == [1.0] and got["macro_f1"] == got["weighted_f1"] == 1.0
        assert got["accuracy"] == 100.0 and got["confusion"].tolist() == [[1.0]]


# ---------------------------------------------------------------------------------------------------- the case tables
@pytest.mark.parametrize("name", list(er.ACCUMULATOR_CASES))
def test_case_builds_and_meets_its_conditions(name):
    """``build`` asserts the exact-sum / margin conditions for every video (none is dropped) and the case functions assert
    what each case is for; here the host results are also cross-checked: counts rebuilt from the prediction lists give the
    host's own scores through ``scores_from_confusion``."""
    case = er.get_case(name)
    assert case.offsets[-1] == sum(len(e["labels"]) for e in case.data.values()) and len(case.offsets) == len(case.data) + 1
    for ic in case.ignore:
        cm = case.counts[ic]
        assert cm[0].sum() == len(case.frame_trgs[ic]) and all(m.sum() == len(case.kept[ic]) for m in cm[1:])
        for level, m in zip([None, *er.KEYS], cm):
            got = scores_from_confusion(m)
            for metric, key in ((metrics.MACRO_F1, "macro_f1"), (metrics.W_F1, "weighted_f1"), (metrics.CL_ACC, "accuracy"),
                                (metrics.CFUSE_MATRIX, "confusion")):
                entry = case.perf[ic][metric]
                want = entry[metrics.FRAME_LEVEL] if level is None else entry[metrics.VIDEO_LEVEL][level]
                assert np.allclose(np.asarray(got[key]), np.asarray(want["master"]), rtol=0.0, atol=1e-12), (name, ic, level, key)


def test_case_sizes_stay_within_what_the_gpu_tests_promise():
    rows = {name: er.get_case(name).offsets[-1] for name in er.ACCUMULATOR_CASES}
    assert max(len(e["labels"]) for e in er.get_case("long_and_many").data.values()) == er.MAX_FRAMES
    assert max(rows.values()) < 16000 and max(len(er.get_case(n).data) for n in rows) == 301


def test_conditions_reject_what_they_are_there_to_reject():
    rng = np.random.default_rng(0)
    z = er.exact_logits(rng, 50, 7)
    assert er.is_exact(z) and not er.is_exact(z + np.float32(2.0 ** -9)) and not er.is_exact(z * 2)
    assert not er.is_exact(np.zeros((2 ** 13, 2), dtype=np.float32))
    # column means 1.0 and 1.00005, neither separated nor identical; every frame is decided (gaps 3 and 1) and the
    # probability means are far apart (0.56 / 0.44), so only the logits condition can refuse it
    close = np.tile(np.array([[1.0, 0.0, -3.0]], dtype=np.float32), (40, 1))
    close[::4, 1] = np.float32(4.0002)
    m64 = close.astype(np.float64).mean(axis=0)
    assert 4e-5 < m64[1] - m64[0] < 6e-5
    with pytest.raises(AssertionError, match="mean-logits margin"):
        er.check_video("close", close, "float", 0)
    apart = close.copy()
    apart[::4, 1] = np.float32(4.02)                      # 5e-3 apart: the same video passes
    er.check_video("apart", apart, "float", 0)
    # the mirror image: logits means 0.52 and 2.5, probability means 0.75 s(ln 2) + 0.25 s(-10) and 0.75 s(-ln 2) + 0.25 s(10)
    # (s = logistic), both 0.5 to within 2e-5
    even = np.tile(np.array([[np.log(2.0), 0.0, -12.0]], dtype=np.float32), (40, 1))
    even[::4, :2] = np.float32([0.0, 10.0])
    with pytest.raises(AssertionError, match="mean-probability margin"):
        er.check_video("even", even, "float", 0)
    with pytest.raises(AssertionError, match="frame top-two gap"):
        er.check_video("frame", np.array([[0.0, 2.0, 2.00001]], dtype=np.float32), "float", 0)
    with pytest.raises(AssertionError, match="not exact-sum"):
        er.check_video("inexact", close, "exact", 0)
    # one-hot x 5 with equal counts: the probability means tie in real arithmetic only
    tie = er.one_hot_logits([0, 1] * 30, 4)
    with pytest.raises(AssertionError, match="mean-probability margin"):
        er.check_video("tie", tie, "exact", 0)
    er.check_video("identical", np.tile(np.float32([[1.5, 1.5, 1.5]]), (9, 1)), "exact", 0)       # tied by construction


def test_stitch_tables_and_reference_sequence():
    er.check_stitch_tables()
    # the written-out sequence on a case small enough to do by hand: windows [0, 1] and [1, 2] of a 3-frame video
    outs = torch.tensor([[[1.0], [2.0]], [[4.0], [8.0]]])
    assert er.stitch_ref(outs, [0, 1], 3).flatten().tolist() == [1.0, 3.0, 8.0]


def test_offset_and_coverage_validators():
    """The host checks behind ``DeviceEvalAccumulator.add`` and the stitch wrappers (their GPU tests count the launches)."""
    assert _offsets("x", [0, 3, 9], 9) == [0, 3, 9] and _offsets("x", np.array([0, 2]), None) == [0, 2]
    assert _offsets("x", torch.tensor([0, 3, 9]), 9) == [0, 3, 9]
    assert _offsets("x", torch.tensor([[0, 9]], dtype=torch.int32), 9) == [0, 9]
    for bad in ([1, 3, 9], [0, 3, 3, 9], [0, 5, 3, 9], [0, 3, 8], [0, 3, 10], [9], [], [0], torch.tensor(0),
                torch.tensor([0, 3, 8])):
        with pytest.raises(ValueError):
            _offsets("x", bad, 9)
    _check_coverage("x", [0, 5, 13], 8, 21)
    _check_coverage("x", [5, 0], 8, 13)                   # any order
    _check_coverage("x", [0, 8], 8, 16)                   # abutting windows
    for starts, lw, total in (([0, 9], 8, 17), ([1, 5], 8, 13), ([0, 5], 8, 14), ([], 8, 8)):
        with pytest.raises(ValueError, match="uncovered"):
            _check_coverage("x", starts, lw, total)
