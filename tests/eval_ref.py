"""The case tables of the device-evaluation edge tests, with what the host mirror of the reference gives for each.

Nothing here needs a GPU: ``tests/test_eval_scores_cpu.py`` builds every case on any machine, ``tests/test_eval_edges_gpu.py``
runs them through ``DeviceEvalAccumulator`` and the stitch kernels of ``csrc/eval_metrics.hip``.  Every expected value is
``metrics.compute_perf`` / ``metrics.format_trg_pred_video`` / ``metrics.format_trg_pred_frames`` on the same data, or the
reference's stitch sequence written out in ``stitch_ref``.

A device result can only be compared with the host's when the answer does not hang on the last bits of a float32 sum, whose
order differs (numpy adds row after row, the kernel adds 256 strided partial sums in a tree).  ``build`` asserts, for every
video and every ``ignore_class`` setting of its case, that each of the three decisions is one of

* exact -- multiples of 2^-8 with |z| <= 5 (``exact_logits`` draws |z| <= 4; one-hot x 5 rows reach 5) and
  ``frames * 5 * 256 < 2^24``, so every float32 column sum, partial sums included, is an integer number of 2^-8 steps below
  2^24 of them and exact in ANY order; an exact tie goes to the first index on both sides.  The host divides the sum by n,
  the kernel does not: two different sums differ by >= 2^-8, their quotients by >= 2^-8 / n > 2^-21 (n < 2^13), one ulp
  below 8, so the division cannot merge them;
* tied by construction -- the leading columns are bitwise identical in every row, so their sums (and their softmax terms)
  go through the same operations on the same numbers and come out bitwise equal, whatever the order;
* non-finite in a way no order changes -- a NaN among the column means (the first NaN wins), or +inf as their maximum;
* separated -- the top two column means (float64) differ by >= ``MARGIN`` = 1e-3 of the larger.  A float32 sum of n <= 5000
  terms is off by at most (n - 1) 2^-24 < 3e-4 of the sum of their magnitudes, in any order; softmax terms are positive,
  so two such sums cannot swap across a 1e-3 gap.  Logits have both signs, so their gap is measured against the larger mean
  MAGNITUDE (sum |z| / n), which is never smaller than what the bare means would ask for.  This is a condition on the
  inputs, not a tolerance on the outputs: the comparison itself is exact.

The frame decision compares the same float32 numbers on both sides and needs no margin; random float logits still keep
their top two at least ``FRAME_MARGIN`` = 1e-4 apart (non-finite rows aside) so that no frame sits on an accidental tie.
No video is ever dropped to meet a condition: the seeds below were chosen so that all of them pass.
"""
from collections import namedtuple

import numpy as np
import torch

from feature_vs_text_compound_emotion_amd import metrics

MARGIN, FRAME_MARGIN = 1e-3, 1e-4
MAX_FRAMES = 5000
EXACT_LIMIT = 5.0
KEYS = (metrics.FRM_VOTE, metrics.FRM_AVG_LOGITS, metrics.FRM_AVG_PROBS)

# data: {video: {"labels" [n] int64, "logits" [n, C] float32}} in insertion order; kinds: {video: "exact" | "float"};
# frame_preds / frame_trgs / video_trgs: {ignore: list}; video_preds: {ignore: [V', 3] int (vote, mean logits, mean probs)};
# kept: {ignore: positions of the videos the host keeps (not labelled `ignore`)}; counts: {ignore: [4, C, C] int64}
Case = namedtuple("Case", "name n_cls ignore data kinds offsets perf frame_preds frame_trgs video_preds video_trgs kept counts")


# ------------------------------------------------------------------------------------------------ inputs
def exact_logits(rng, n, c, lim=4.0):
    """[n, c] float32 multiples of 2^-8 in [-lim, lim]."""
    k = int(lim * 256)
    return (rng.integers(-k, k + 1, (n, c)) / 256.0).astype(np.float32)


def one_hot_logits(frames, c, scale=5.0):
    """one-hot x ``scale`` rows; argmax of row i is frames[i]."""
    return np.eye(c, dtype=np.float32)[np.asarray(frames)] * np.float32(scale)


def _video(label, logits):
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    return {"labels": np.full(len(logits), int(label), dtype=np.int64), "logits": logits}


# ------------------------------------------------------------------------------------------------ conditions
def is_exact(logits):
    z = logits.astype(np.float64)
    return bool(np.isfinite(z).all() and (z * 256 == np.round(z * 256)).all() and np.abs(z).max() <= EXACT_LIMIT
                and len(z) * EXACT_LIMIT * 256 < 2 ** 24 and len(z) < 2 ** 13)


def _decided(z, means, scale):
    """Every column of ``z`` is either separated from the top one -- its mean lies >= MARGIN x the larger of the two
    ``scale`` entries below the top mean -- or tied with it by construction: bitwise the same column.  Columns with a -inf
    mean drop out; at least one finite mean must remain."""
    keep = np.flatnonzero(np.isfinite(means))
    if len(keep) == 0:
        return False
    a = keep[np.argmax(means[keep])]
    near = [j for j in keep if j != a and means[a] - means[j] < MARGIN * max(scale[a], scale[j])]
    return all(np.array_equal(z[:, a], z[:, j]) for j in near)


def check_video(name, logits, kind, n_drop):
    """The conditions of the module docstring for one video with the last ``n_drop`` columns dropped (0 or 1)."""
    z32 = logits[:, :logits.shape[1] - n_drop] if n_drop else logits
    assert 1 <= len(z32) <= MAX_FRAMES, (name, len(z32))
    assert kind in ("exact", "float"), kind
    with np.errstate(all="ignore"):
        z = z32.astype(np.float64)
        finite_rows = np.isfinite(z).all(axis=1)
        if kind == "exact":
            assert is_exact(logits), f"{name}: not exact-sum logits"
        else:
            srt = np.sort(z[finite_rows], axis=1)
            # a row of one repeated value (the all--200 rows of the underflow case) is a tie on purpose
            gap = np.where(srt[:, -1] == srt[:, 0], np.inf, srt[:, -1] - srt[:, -2])
            assert gap.size == 0 or gap.min() >= FRAME_MARGIN, f"{name}: frame top-two gap {gap.min():.3g}"
        # mean logits, as float32 would classify them: NaN / +inf / -inf are order-independent (finite parts are < 2^21)
        lsum = z.sum(axis=0) / len(z)
        if not (np.isnan(lsum).any() or np.isposinf(lsum).any()):
            if kind == "exact" and finite_rows.all():
                pass                                  # exact in any order; ties go to the first index on both sides
            else:
                mag = np.where(np.isfinite(z), np.abs(z), 0.0).sum(axis=0) / len(z)
                assert _decided(z32, lsum, mag), f"{name}: mean-logits margin"
        # mean probabilities: the float32 softmax decides which entries are NaN / 0 (exp overflows above 88.7 and
        # underflows below -104; the inputs stay far from both: |z| <= 4 or one of nan, +-inf, 100, -200)
        odd = z32[~np.isin(z32, (np.inf, -np.inf, 100.0, -200.0)) & ~np.isnan(z32)]
        assert odd.size == 0 or np.abs(odd).max() <= (EXACT_LIMIT if kind == "exact" else 16.0), f"{name}: logit magnitude"
        p = metrics.softmax(z32).astype(np.float64)
        if finite_rows.all() and np.abs(z).max() <= 16.0:
            p64 = np.exp(z)
            p64 /= p64.sum(axis=1, keepdims=True)
            assert np.abs(p - p64).max() < 1e-6                 # float32 softmax = float64 softmax to rounding
            p = p64
        pm = p.mean(axis=0)
        if not np.isnan(pm).any():
            assert _decided(z32, pm, pm), f"{name}: mean-probability margin"


# ------------------------------------------------------------------------------------------------ host results
def counts_from_lists(n_cls, frame_trgs, frame_preds, video_trgs, video_preds):
    cm = np.zeros((4, n_cls, n_cls), dtype=np.int64)
    for t, p in zip(frame_trgs, frame_preds):
        cm[0, int(t), int(p)] += 1
    for t, triple in zip(video_trgs, video_preds):
        for i, p in enumerate(triple):
            cm[1 + i, int(t), int(p)] += 1
    return cm


def build(name, n_cls, ignore, data, kinds):
    """Check the conditions and run the host mirror.  ``kinds``: "exact" / "float" for every video, or one for all."""
    kinds = {k: kinds for k in data} if isinstance(kinds, str) else dict(kinds)
    assert list(kinds) == list(data) and 2 <= n_cls <= 16
    lengths = []
    for k, e in data.items():
        assert e["logits"].dtype == np.float32 and e["logits"].shape == (len(e["labels"]), n_cls), k
        assert e["labels"].dtype == np.int64 and len(np.unique(e["labels"])) == 1 and 0 <= e["labels"][0] < n_cls, k
        lengths.append(len(e["labels"]))
        for ic in ignore:
            assert ic is None or ic == n_cls - 1          # the reference drops the LAST column, whatever ignore_class is
            check_video(f"{name}/{k}/ignore={ic}", e["logits"], kinds[k], 0 if ic is None else 1)
    offsets = np.cumsum([0] + lengths).tolist()
    fp, ft, vp, vt, kept, counts = {}, {}, {}, {}, {}, {}
    with np.errstate(all="ignore"):
        perf = metrics.compute_perf(data, ignore)
        for ic in ignore:
            fp[ic], ft[ic] = metrics.format_trg_pred_frames(data, ic)
            preds, vt[ic] = metrics.format_trg_pred_video(data, ic)
            vp[ic] = np.array([[p[k] for k in KEYS] for p in preds], dtype=np.int64).reshape(-1, 3)
            kept[ic] = [i for i, e in enumerate(data.values()) if ic is None or int(e["labels"][0]) != ic]
            assert len(kept[ic]) == len(preds) > 0 and len(fp[ic]) > 0      # "every frame ignored" is out of scope
            counts[ic] = counts_from_lists(n_cls, ft[ic], fp[ic], vt[ic], vp[ic])
    return Case(name, n_cls, tuple(ignore), data, kinds, offsets, perf, fp, ft, vp, vt, kept, counts)


def concat(case, keys=None):
    """(logits [R, C], labels [R] int64, offsets [V+1]) of the videos ``keys`` (default: all, in order)."""
    keys = list(case.data) if keys is None else list(keys)
    off = np.cumsum([0] + [len(case.data[k]["labels"]) for k in keys]).tolist()
    return (np.concatenate([case.data[k]["logits"] for k in keys]), np.concatenate([case.data[k]["labels"] for k in keys]), off)


# ------------------------------------------------------------------------------------------------ 1: vote ties across strides
TIE_FRAMES, TIE_COUNT, TIE_ROWS = 750, 110, (5, 300, 601)


def _tie_video(classes, firsts, boosted, fillers, c=7):
    """TIE_FRAMES one-hot x 5 frames.  ``classes`` get TIE_COUNT votes each, class i from row firsts[i] on (one row in each
    256-row stride of the block: 5, 300, 601); every other row votes for one of ``fillers`` in turn, fewer than TIE_COUNT
    each, and carries 3.0 in column ``boosted``.  The fillers settle the two mean decisions on ``boosted``: three equal
    vote counts are an exact tie of the probability means in real arithmetic, which no float32 summation order keeps."""
    votes = np.full(TIE_FRAMES, -1)
    for cls, row in sorted(zip(classes, firsts), key=lambda t: t[1]):
        free = np.flatnonzero(votes[row:] < 0)[:TIE_COUNT] + row
        assert len(free) == TIE_COUNT and free[0] == row
        votes[free] = cls
    rest = np.flatnonzero(votes < 0)
    votes[rest] = [fillers[i % len(fillers)] for i in range(len(rest))]
    logits = one_hot_logits(votes, c)
    logits[rest, boosted] = 3.0
    return votes, logits


def case_vote_ties():
    """Three classes tied on votes, first seen at rows 5, 300 and 601 (one in each 256-row stride), C = 7: why 750 frames.
    The class first seen at row 601 of an n-frame video has at most n - 601 votes, so the three tied classes take
    3 (n - 601) rows at the most and the four classes left share the rest, each below the tied count:
    n - 3 (n - 601) < 4 (n - 601) gives n > 7 x 601 / 6 = 701.2.  750 frames leave room: 110 votes for each tied class,
    105 for each of the four fillers."""
    data = {}
    # rows 5, 300, 601 -> classes 4, 1, 5: class 4 wins the vote; the lowest tied index is 1; both means pick 5
    votes, logits = _tie_video((4, 1, 5), TIE_ROWS, boosted=5, fillers=(0, 2, 3, 6))
    first = {int(c): int(np.flatnonzero(votes == c)[0]) for c in (4, 1, 5)}
    assert first == {4: 5, 1: 300, 5: 601} and all((votes == c).sum() == TIE_COUNT for c in (4, 1, 5))
    assert max((votes == c).sum() for c in (0, 2, 3, 6)) < TIE_COUNT
    assert {first[c] // 256 for c in first} == {0, 1, 2}
    data["tie_5_300_601"] = _video(4, logits)
    # the same counts, first appearances permuted: class 4 from row 300, class 5 from row 5, class 1 from row 601
    votes, logits = _tie_video((4, 5, 1), (300, 5, 601), boosted=4, fillers=(0, 2, 3, 6))
    assert [int(np.flatnonzero(votes == c)[0]) for c in (4, 5, 1)] == [300, 5, 601]
    data["tie_300_5_601"] = _video(2, logits)
    # a strict majority whose class appears last: rows 0..339 go round the other six classes, class 3 takes 340..699
    votes = np.array([(0, 1, 2, 4, 5, 6)[i % 6] for i in range(340)] + [3] * 360)
    data["majority_last"] = _video(3, one_hot_logits(votes, 7))
    case = build("vote_ties", 7, (None,), data, "exact")
    assert case.video_preds[None].tolist() == [[4, 5, 5], [5, 4, 4], [3, 3, 3]], case.video_preds[None]
    return case


# ------------------------------------------------------------------------------------------------ 2: equal maxima in a frame
def _tied_rows(rng, n, c, n_tied, top=3.0, last=None):
    """Exact base in [-2, 2]; in every row ``n_tied`` random columns of the first ``c - (last is not None)`` hold ``top``;
    ``last``: the value of the final column (above ``top``: the overall maximum sits in the column ignore_class drops)."""
    z = exact_logits(rng, n, c, lim=2.0)
    width = c if last is None else c - 1
    for r in range(n):
        z[r, rng.choice(width, size=n_tied, replace=False)] = top
    if last is not None:
        z[:, -1] = last
    return z


def _equal_maxima(name, c, ignore, seed):
    rng = np.random.default_rng(seed)
    last = None if ignore == (None,) else 3.5
    width = c if last is None else c - 1
    data = {"two": _video(1, _tied_rows(rng, 300, c, 2, last=last)),
            "three": _video(0, _tied_rows(rng, 300, c, 3, last=last)),
            "all": _video(2, _tied_rows(rng, 40, c, width, last=last)),
            "mixed": _video(1, np.concatenate([_tied_rows(rng, 120, c, k, last=last) for k in (2, 3, width, 2)]))}
    # every column of "all" is the same column: all three decisions are exact ties, the answer is index 0
    case = build(name, c, ignore, data, "exact")
    for ic in ignore:
        nc = c if ic is None else c - 1
        for k, n_tied in (("two", 2), ("three", 3), ("all", width)):
            z = data[k]["logits"][:, :nc]
            n_max = (z == z.max(axis=1, keepdims=True)).sum(axis=1)
            assert (n_max == (1 if (ic is None and last is not None) else n_tied)).all(), (name, k, ic)
    if last is not None:
        assert all((e["logits"].argmax(axis=1) == c - 1).all() for e in data.values())
        assert case.video_preds[None][:, 0].tolist() == [c - 1] * 4 and (case.video_preds[c - 1] < c - 1).all()
    assert case.video_preds[ignore[-1]][2].tolist() == [0, 0, 0]
    return case


def case_equal_maxima():
    return _equal_maxima("equal_maxima", 7, (None,), seed=21)


def case_equal_maxima_ignored_column():
    return _equal_maxima("equal_maxima_ignored_column", 8, (None, 7), seed=22)


# ------------------------------------------------------------------------------------------------ 3: class-count limits
def _random_exact_videos(rng, n_videos, c, lengths, boost=2.0):
    data = {}
    for v in range(n_videos):
        n = lengths[v] if v < len(lengths) else int(rng.integers(1, 601))
        label = int(rng.integers(0, c))
        z = exact_logits(rng, n, c, lim=2.0)
        z[:, int(rng.integers(0, c))] += np.float32(rng.integers(64, int(boost * 256)) / 256.0)   # right or wrong class
        data[f"v{v}"] = _video(label, z)
    return data


def case_class_limits(c):
    assert c in (2, 16)
    rng = np.random.default_rng({2: 302, 16: 316}[c])
    data = _random_exact_videos(rng, 40, c, lengths=(1, 257, 600, 256, 2))
    assert {1, 257} <= {len(e["labels"]) for e in data.values()} and max(len(e["labels"]) for e in data.values()) <= 600
    return build(f"class_limits_c{c}", c, (None,), data, "exact")


# ------------------------------------------------------------------------------------------------ 4: absent classes
def case_absent_classes():
    """C = 16, six videos; targets {1, 4}, predictions {4, 9} at both levels: class 9 is predicted and never a target,
    class 1 is a target and never predicted, thirteen classes are absent from both and must not count in macro F1."""
    rng = np.random.default_rng(41)
    data = {}
    for v, (label, major, n) in enumerate([(1, 4, 90), (1, 9, 300), (4, 4, 41), (4, 9, 130), (4, 4, 7), (1, 4, 260)]):
        z = exact_logits(rng, n, 16, lim=1.0)
        minor = 9 if major == 4 else 4
        cols = np.where(rng.random(n) < 0.7, major, minor)
        z[np.arange(n), cols] = 3.0
        z[:, major] += 0.5
        data[f"v{v}"] = _video(label, z)
    case = build("absent_classes", 16, (None,), data, "exact")
    assert set(case.frame_trgs[None]) == {1, 4} and set(case.frame_preds[None]) == {4, 9}
    assert set(case.video_trgs[None]) == {1, 4}
    for i in range(3):
        assert set(case.video_preds[None][:, i].tolist()) == {4, 9}
    for cm in case.counts[None]:
        present = (cm.sum(0) + cm.sum(1)) > 0
        assert np.flatnonzero(present).tolist() == [1, 4, 9]
        assert cm[:, 1].sum() == 0 and cm[1].sum() > 0 and cm[9].sum() == 0 and cm[:, 9].sum() > 0
    return case


# ------------------------------------------------------------------------------------------------ 5, 6: random float logits
def _random_float_videos(rng, lengths, c, labels=None, sharp=3.0):
    """Standard-normal logits plus a per-video offset on every column (so the column means are O(1) and apart) and a
    boost on one column that is the label's for about half of the videos."""
    data = {}
    for v, n in enumerate(lengths):
        label = int(rng.integers(0, c)) if labels is None else labels[v]
        z = rng.standard_normal((n, c)) + rng.uniform(-1.0, 1.0, c)
        z[:, label if rng.random() < 0.5 else int(rng.integers(0, c))] += 0.5 + rng.random() * sharp
        data[f"v{v}"] = _video(label, z.astype(np.float32))
    return data


def case_ignore_class(seed=3):
    """C = 8 scored with ignore = (None, 7): videos labelled 7 count under None and are skipped at both levels under 7;
    frames (and videos) whose full-width argmax is column 7 fall to their best of the first seven columns."""
    rng = np.random.default_rng(seed)
    lengths = [int(n) for n in rng.integers(1, 400, 30)]
    labels = [int(x) for x in rng.integers(0, 8, 30)]
    labels[3] = labels[11] = labels[29] = 7
    data = _random_float_videos(rng, lengths, 8, labels)
    for k in ("v5", "v11", "v20"):                      # column 7 wins most frames of these, labelled 7 or not
        data[k]["logits"][:, 7] += np.float32(4.0)
    case = build("ignore_class", 8, (None, 7), data, "float")
    assert case.video_trgs[None].count(7) >= 3 and 7 not in case.video_trgs[7] and 7 not in case.frame_trgs[7]
    assert len(case.kept[7]) == len(case.kept[None]) - case.video_trgs[None].count(7)
    assert 7 in case.frame_preds[None] and 7 in case.video_preds[None] and 7 not in case.frame_preds[7]
    assert case.counts[7][:, 7].sum() == 0 and case.counts[7][:, :, 7].sum() == 0
    return case


def case_long_and_many(seed=6):
    """One 5000-frame video and 300 short ones, C = 16 (the largest input of the suite: 5000 x 16 logits)."""
    rng = np.random.default_rng(seed)
    lengths = [5000] + [int(n) for n in rng.integers(1, 48, 300)]
    case = build("long_and_many", 16, (None,), _random_float_videos(rng, lengths, 16), "float")
    assert len(case.data) == 301 and case.offsets[1] == 5000
    return case


# ------------------------------------------------------------------------------------------------ 7: non-finite logits
def _ordinary(rng, n, c, col):
    z = rng.standard_normal((n, c))
    z[:, col] += 2.0
    return z.astype(np.float32)


def case_non_finite(seed=2):
    """Ordinary videos (column 5 leads) with a few odd frames each.  What the host mirror gives, and why:

    nan_col0     NaN in column 0: the frames vote 0; mean logits [NaN, ...] -> 0; every softmax term of such a row is NaN -> 0
    nan_middle   NaN in column 3: the frames vote 3; mean logits -> 3; all probability means NaN -> 0
    pos_inf      +inf in column 2: mean logits +inf -> 2; softmax inf / inf = NaN in column 2 only -> 2
    neg_inf      -inf in all columns but 4: those frames vote 4; columns != 4 have mean -inf -> 4; probabilities are finite
    overflow     a logit of 100 in column 3: finite mean logits; exp overflows, inf / inf = NaN in column 3 -> 3
    underflow    rows of -200: every exp is 0, 0 / 0 = NaN in every column -> 0; the frames vote 0 (seven equal maxima)
    both_inf     +inf and -inf in column 1 of different frames: mean logits NaN -> 1; probabilities NaN in column 1 -> 1
    plain        no odd frame: the control
    """
    rng = np.random.default_rng(seed)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    data = {}

    def video(name, label, n, rows, edit):
        z = _ordinary(rng, n, 7, 5)
        for r in rows:
            edit(z, r)
        data[name] = _video(label, z)

    video("nan_col0", 5, 300, (2, 270), lambda z, r: z.__setitem__((r, 0), nan))
    video("nan_middle", 5, 300, (7, 290), lambda z, r: z.__setitem__((r, 3), nan))
    video("pos_inf", 2, 90, (40,), lambda z, r: z.__setitem__((r, 2), inf))

    def all_but_4(z, r):
        z[r, [0, 1, 2, 3, 5, 6]] = -inf
    video("neg_inf", 4, 200, range(0, 200, 5), all_but_4)
    video("overflow", 5, 280, (0, 279), lambda z, r: z.__setitem__((r, 3), np.float32(100.0)))
    video("underflow", 0, 60, (10, 11, 59), lambda z, r: z.__setitem__((r, slice(None)), np.float32(-200.0)))

    def both(z, r):
        z[r, 1] = inf if r == 20 else -inf
    video("both_inf", 1, 300, (20, 280), both)
    video("plain", 5, 257, (), None)
    case = build("non_finite", 7, (None,), data, "float")
    want = {"nan_col0": [5, 0, 0], "nan_middle": [5, 3, 0], "pos_inf": [5, 2, 2], "neg_inf": [5, 4, 5], "overflow": [5, 5, 3],
            "underflow": [5, 5, 0], "both_inf": [5, 1, 1], "plain": [5, 5, 5]}
    got = dict(zip(data, case.video_preds[None].tolist()))
    assert got == want, got
    fp = np.array(case.frame_preds[None])
    off = case.offsets
    assert fp[off[0] + 2] == 0 and fp[off[1] + 7] == 3 and fp[off[2] + 40] == 2 and fp[off[3]] == 4 and fp[off[4]] == 3
    assert fp[off[5] + 10] == 0 and fp[off[6] + 20] == 1
    return case


def case_non_finite_ignored_column(seed=2):
    """C = 8, ignore = (None, 7), NaN in column 7 of some frames: it decides under None and is never read under 7."""
    rng = np.random.default_rng(seed)
    data = {}
    for v, label in enumerate((5, 7, 2)):
        z = _ordinary(rng, 270, 8, 5)
        z[[3, 260], 7] = np.nan
        data[f"v{v}"] = _video(label, z)
    case = build("non_finite_ignored_column", 8, (None, 7), data, "float")
    assert case.video_preds[None].tolist() == [[5, 7, 0]] * 3 and case.video_preds[7].tolist() == [[5, 5, 5]] * 2
    return case


# ------------------------------------------------------------------------------------------------ 8: labels
def case_label_batch(seed=2):
    """Five ordinary videos (C = 7) for the label tests; ``bad_labels`` spoils the middle one."""
    rng = np.random.default_rng(seed)
    return build("label_batch", 7, (None,), _random_float_videos(rng, [40, 300, 17, 1, 258], 7), "float")


def bad_labels(case, how):
    """The concatenated labels of ``case`` with video 2 spoilt: "mixed" (one frame of another class, which the host
    mirror refuses with its ``len(unique) == 1`` assertion) or "range" (a label >= n_cls)."""
    logits, labels, off = concat(case)
    labels = labels.copy()
    a, b = off[2], off[3]
    if how == "mixed":
        labels[a + (b - a) // 2] = (labels[a] + 1) % case.n_cls
        data = {k: dict(e) for k, e in case.data.items()}
        data["v2"]["labels"] = labels[a:b]
        try:
            metrics.format_trg_pred_video(data, None)
        except AssertionError:
            pass
        else:
            raise AssertionError("the host mirror accepts a video with two labels")
    else:
        assert how == "range"
        labels[a:b] = case.n_cls + 2
    return logits, labels, off


ACCUMULATOR_CASES = {
    "vote_ties": case_vote_ties,
    "equal_maxima": case_equal_maxima,
    "equal_maxima_ignored_column": case_equal_maxima_ignored_column,
    "class_limits_c2": lambda: case_class_limits(2),
    "class_limits_c16": lambda: case_class_limits(16),
    "absent_classes": case_absent_classes,
    "ignore_class": case_ignore_class,
    "long_and_many": case_long_and_many,
    "non_finite": case_non_finite,
    "non_finite_ignored_column": case_non_finite_ignored_column,
    "label_batch": case_label_batch,
}
_BUILT = {}


def get_case(name):
    """Built once per process and shared; nobody writes to a case."""
    if name not in _BUILT:
        case = ACCUMULATOR_CASES[name]()
        assert case.name == name
        for e in case.data.values():
            e["logits"].setflags(write=False)
            e["labels"].setflags(write=False)
        _BUILT[name] = case
    return _BUILT[name]


# ------------------------------------------------------------------------------------------------ window stitching
# (window length, hop, frames): three and more windows deep, window length 1, and the two-deep geometries of the trainer
STITCH_GEOMETRIES = ((8, 2, 30), (8, 1, 20), (300, 70, 650), (1, 1, 5), (1, 1, 1))
STITCH_CLASSES = 7
MULTI_V = (1, 2, 3, 255, 256, 257)
MULTI_GEOMETRIES = ((8, 2, 30), (8, 1, 20), (8, 5, 21), (8, 5, 8), (8, 3, 13), (8, 2, 9))     # one window length per launch


def window_starts(n, win, hop):
    from feature_vs_text_compound_emotion_amd.trainer import windowing
    return [int(w[0]) for w in windowing(np.arange(n), win, hop)]


def overlap_depth(starts, win, n):
    cnt = np.zeros(n, dtype=np.int64)
    for s in starts:
        cnt[s:s + win] += 1
    return cnt


def window_set(n, win, hop, seed, c=STITCH_CLASSES):
    """(n, win, starts, window outputs [nw, win, c] random float32): with three and more terms per frame the sum depends
    on the order in which they are added."""
    starts = window_starts(n, win, hop)
    g = torch.Generator().manual_seed(seed)
    return n, win, starts, torch.randn(len(starts), win, c, generator=g)


def stitch_ref(outs, starts, n):
    """The reference's sequence (trainer.py:861-880): add window after window into zeros, divide by the overlap count."""
    win = outs.shape[1]
    final = torch.zeros(n, outs.shape[2])
    cnt = torch.zeros(n)
    for o, s in zip(outs, starts):
        final[s:s + win] = final[s:s + win] + o
        cnt[s:s + win] += 1
    return final / cnt[:, None]


def multi_videos(count, seed=5):
    """``count`` window sets of window length 8 and mixed lengths, the same prefix for every count."""
    vids = []
    for i in range(count):
        win, hop, n = MULTI_GEOMETRIES[(i * 5 + i // 6) % len(MULTI_GEOMETRIES)]
        vids.append(window_set(n, win, hop, seed=seed * 1000 + i))
    return vids


def check_stitch_tables():
    for win, hop, n in STITCH_GEOMETRIES[:3]:
        starts = window_starts(n, win, hop)
        depth = overlap_depth(starts, win, n)
        assert depth.min() >= 1 and depth.max() >= 3, (win, hop, n, depth.max())
        assert starts == sorted(starts)
        # the order matters at these depths: adding the windows backwards changes bits of the reference itself
        _, _, _, outs = window_set(n, win, hop, seed=1)
        fwd = stitch_ref(outs, starts, n)
        bwd = stitch_ref(outs.flip(0), starts[::-1], n)
        assert not torch.equal(fwd, bwd) and (fwd - bwd).abs().max().item() < 1e-5
    for win, hop, n in STITCH_GEOMETRIES[3:]:
        assert win == 1 and overlap_depth(window_starts(n, win, hop), win, n).tolist() == [1] * n
    vids = multi_videos(max(MULTI_V))
    assert {v[1] for v in vids} == {8} and len({v[0] for v in vids[:3]}) == 3 and len({v[0] for v in vids}) == len(MULTI_GEOMETRIES)
    assert max(overlap_depth(v[2], 8, v[0]).max() for v in vids[:2]) >= 3
    assert sum(v[0] for v in vids) < 2 ** 13
