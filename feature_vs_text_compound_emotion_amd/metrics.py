"""Frame- and video-level scores (host side, numpy).

Mirror of the parts of the reference's metrics.py the hot path feeds (metrics.py:43-193):
prediction formatting (frame level; video level by majority vote / mean logits / mean
probabilities, with the C-EXPR-DB 'Other' class option), per-class / macro / weighted F1 (the
definitions sklearn.metrics.f1_score uses, restated so the GPU box needs no sklearn), accuracy and
the row-normalised confusion matrix.
"""
from collections import Counter

import numpy as np

FRM_VOTE, FRM_AVG_LOGITS, FRM_AVG_PROBS = "FRAMES_MAJORITY_VOTING", "FRAMES_AVERAGE_LOGITS", "FRAMES_AVERAGE_PROBS"
MACRO_F1, W_F1, CL_ACC, CFUSE_MATRIX = "MACRO_F1", "W_F1", "CL_ACC", "CONFUSION_MATRIX"
FRAME_LEVEL, VIDEO_LEVEL = "FRAME_LEVEL", "VIDEO_LEVEL"


def softmax(x):
    assert x.ndim == 2, x.ndim
    e = np.exp(x)  # like the reference: no max subtraction
    return e / e.sum(axis=1, keepdims=True)


def format_trg_pred_frames(data, ignore_class=None):
    limited = isinstance(ignore_class, int)
    preds, trgs = [], []
    for vid in data:
        labels, logits = data[vid]["labels"].tolist(), data[vid]["logits"]
        if limited:
            logits = logits[:, :-1]
        p = np.argmax(logits, axis=1).flatten().tolist()
        assert len(p) == len(labels), f"{len(p)} | {len(labels)}"
        for i, l in enumerate(labels):
            if limited and l == ignore_class:
                continue
            trgs.append(l)
            preds.append(p[i])
    return preds, trgs


def format_trg_pred_video(data, ignore_class=None):
    limited = isinstance(ignore_class, int)
    preds, trgs = [], []
    for vid in data:
        labels = data[vid]["labels"]
        uniq = np.unique(labels).tolist()
        assert len(uniq) == 1, len(uniq)
        if limited and uniq[0] == ignore_class:
            continue
        logits = data[vid]["logits"]
        if limited:
            logits = logits[:, :-1]
        frame_preds = np.argmax(logits, axis=1).flatten().tolist()
        preds.append({FRM_VOTE: Counter(frame_preds).most_common(1)[0][0],
                      FRM_AVG_LOGITS: int(np.argmax(logits.mean(axis=0))),
                      FRM_AVG_PROBS: int(np.argmax(softmax(logits).mean(axis=0)))})
        trgs.append(uniq[0])
    return preds, trgs


def per_class_f1(trgs, preds):
    """F1 per class over the sorted union of labels present in trgs or preds (sklearn's default)."""
    t, p = np.asarray(trgs).astype(np.int64), np.asarray(preds).astype(np.int64)
    classes = np.unique(np.concatenate([t, p]))
    f1, support = [], []
    for c in classes:
        tp = float(np.sum((t == c) & (p == c)))
        fp = float(np.sum((t != c) & (p == c)))
        fn = float(np.sum((t == c) & (p != c)))
        den = 2 * tp + fp + fn
        f1.append(2 * tp / den if den > 0 else 0.0)
        support.append(float(np.sum(t == c)))
    return np.array(f1), np.array(support), classes


def compute_f1_score(trgs, preds, f1_type):
    f1s, support, _ = per_class_f1(trgs, preds)
    if f1_type == MACRO_F1:
        return f1s, float(np.mean(f1s))
    if f1_type == W_F1:
        return f1s, float(np.sum(f1s * support) / max(np.sum(support), 1.0))
    raise NotImplementedError(f1_type)


def compute_class_acc(trgs, preds):
    return float((np.asarray(trgs, dtype=np.float32) == np.asarray(preds, dtype=np.float32)).mean() * 100.0)


def compute_confusion_matrix(trgs, preds):
    t, p = np.asarray(trgs).astype(np.int64), np.asarray(preds).astype(np.int64)
    classes = np.unique(np.concatenate([t, p]))
    idx = {c: i for i, c in enumerate(classes)}
    m = np.zeros((len(classes), len(classes)))
    for a, b in zip(t, p):
        m[idx[a], idx[b]] += 1
    rows = m.sum(axis=1, keepdims=True)
    return np.divide(m, rows, out=np.zeros_like(m), where=rows > 0)


def compute_perf(data, ignore_classes=(None,)):
    """{ignore_class: {metric: {FRAME_LEVEL: {...}, VIDEO_LEVEL: {agg: {...}}}}} like Trainer.compute_perf
    (trainer.py:525-605)."""
    out = {}
    for ic in ignore_classes:
        perf = {m: {FRAME_LEVEL: None, VIDEO_LEVEL: {}} for m in (MACRO_F1, W_F1, CL_ACC, CFUSE_MATRIX)}
        preds, trgs = format_trg_pred_frames(data, ic)
        f1s, macro = compute_f1_score(trgs, preds, MACRO_F1)
        perf[MACRO_F1][FRAME_LEVEL] = {"master": macro, "per_cl": f1s}
        perf[W_F1][FRAME_LEVEL] = {"master": compute_f1_score(trgs, preds, W_F1)[1], "per_cl": f1s}
        acc = compute_class_acc(trgs, preds)
        perf[CL_ACC][FRAME_LEVEL] = {"master": acc, "per_cl": acc}
        cm = compute_confusion_matrix(trgs, preds)
        perf[CFUSE_MATRIX][FRAME_LEVEL] = {"master": cm, "per_cl": cm}
        vpreds, vtrgs = format_trg_pred_video(data, ic)
        for k in (FRM_VOTE, FRM_AVG_LOGITS, FRM_AVG_PROBS):
            pk = [item[k] for item in vpreds]
            f1s, macro = compute_f1_score(vtrgs, pk, MACRO_F1)
            perf[MACRO_F1][VIDEO_LEVEL][k] = {"master": macro, "per_cl": f1s}
            perf[W_F1][VIDEO_LEVEL][k] = {"master": compute_f1_score(vtrgs, pk, W_F1)[1], "per_cl": f1s}
            acc = compute_class_acc(vtrgs, pk)
            perf[CL_ACC][VIDEO_LEVEL][k] = {"master": acc, "per_cl": acc}
            cm = compute_confusion_matrix(vtrgs, pk)
            perf[CFUSE_MATRIX][VIDEO_LEVEL][k] = {"master": cm, "per_cl": cm}
        out[ic] = perf
    return out


# ------------------------------------------------------------------ the regression task (base/logger.py:213-246,274-351)
OVERALL = "overall"
RMSE, PCC, CCC = "rmse", "pcc", "ccc"


def _pearson_p_value(r, n):
    """Two-sided p-value of Pearson's r on n points (what ``scipy.stats.pearsonr`` reports: r is Beta(n/2 - 1, n/2 - 1) on
    [-1, 1] under the null hypothesis); NaN when scipy is absent."""
    try:
        from scipy import stats
    except ImportError:
        return float("nan")
    if n < 3 or not np.isfinite(r):
        return 1.0 if n == 2 and np.isfinite(r) else float("nan")
    ab = n / 2.0 - 1.0
    return float(2.0 * stats.beta(ab, ab, loc=-1.0, scale=2.0).cdf(-abs(min(max(r, -1.0), 1.0))))


def regression_scores(pred, label):
    """``ContinuousMetricsCalculator.calculator`` for its three metrics on one pair of 1-D arrays, in float64:
    ``{"rmse": sqrt(mean((p - l)^2)), "pcc": (r, p_value), "ccc": calculate_ccc(p, l)}`` -- Lin's CCC exactly as
    base/logger.py:213-246 (biased covariance, variances over n - 1, ``+ 1e-100`` in the denominator).  ``p_value`` comes
    from ``scipy.stats.pearsonr`` when scipy imports and is NaN otherwise."""
    p, l = np.asarray(pred, dtype=np.float64).reshape(-1), np.asarray(label, dtype=np.float64).reshape(-1)
    assert p.shape == l.shape and p.size >= 2, (p.shape, l.shape)
    n = p.size
    dp, dl = p - p.mean(), l - l.mean()
    with np.errstate(divide="ignore", invalid="ignore"):
        r = float(np.sum(dp * dl) / np.sqrt(np.sum(dp * dp) * np.sum(dl * dl)))
    try:
        from scipy.stats import pearsonr
        p_value = float(pearsonr(p, l)[1])
    except ImportError:
        p_value = float("nan")
    ccc = 2.0 * np.mean(dp * dl) / (np.sum(dp * dp) / (n - 1) + np.sum(dl * dl) / (n - 1) + (p.mean() - l.mean()) ** 2 + 1e-100)
    return {RMSE: float(np.sqrt(np.mean((p - l) ** 2))), PCC: (r, p_value), CCC: float(ccc)}


def compute_regression_perf(per_video):
    """``{trial: {"labels", "outputs"}}`` -> ``{trial: {"rmse", "pcc", "ccc"}, ..., "overall": {...}}`` like
    ``ContinuousMetricsCalculator.calculate_metrics`` (base/logger.py:325-351): every trial on its own, then the trials'
    arrays concatenated in the dictionary's (loader) order."""
    out = {trial: regression_scores(v["outputs"], v["labels"]) for trial, v in per_video.items()}
    def cat(key):
        return np.concatenate([np.asarray(v[key], dtype=np.float64).reshape(-1) for v in per_video.values()])
    out[OVERALL] = regression_scores(cat("outputs"), cat("labels"))
    return out


def fold_moments(rows):
    """Rows ``{n, mean_p, mean_l, M2_p, M2_l, C_pl, SSE, 0}`` of consecutive segments -> the row of their concatenation, folded
    in order with the pairwise centred update (Chan et al.): ``M2 += M2_b + delta^2 n_a n_b / n`` and likewise for C."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 8)
    acc = rows[0].copy()
    for b in rows[1:]:
        na, nb = acc[0], b[0]
        n = na + nb
        dp, dl = b[1] - acc[1], b[2] - acc[2]
        acc[3] += b[3] + dp * dp * na * nb / n
        acc[4] += b[4] + dl * dl * na * nb / n
        acc[5] += b[5] + dp * dl * na * nb / n
        acc[1] += dp * nb / n
        acc[2] += dl * nb / n
        acc[6] += b[6]
        acc[0] = n
    return acc


def scores_from_moments(row):
    """One moment row -> the ``regression_scores`` dictionary of the frames it summarises."""
    n, mp, ml, m2p, m2l, c, sse = (float(x) for x in np.asarray(row, dtype=np.float64)[:7])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = float(np.float64(c) / np.sqrt(np.float64(m2p) * np.float64(m2l)))
    ccc = 2.0 * (c / n) / (m2p / (n - 1) + m2l / (n - 1) + (mp - ml) ** 2 + 1e-100)
    return {RMSE: float(np.sqrt(sse / n)), PCC: (r, _pearson_p_value(r, int(n))), CCC: float(ccc)}
