"""Evaluation scores from confusion counts gathered ON THE DEVICE.

``DeviceEvalAccumulator`` receives each video's logits and labels as GPU tensors (nothing is copied to the host per
video), accumulates the frame-level and the three video-level confusion count matrices with ``cer_eval_accumulate`` and
turns them into the reference's score dictionary (trainer.py:525-605 / metrics.py:148-193: macro / weighted F1 with
sklearn's "classes present in targets or predictions" convention, accuracy, row-normalised confusion matrix) after ONE
[4, C, C] device-to-host copy per evaluation and ignore-class setting.  ``DeviceRegressionAccumulator`` does the same for the
regression task from per-video moment rows.  Both answer to the three calls ``Trainer.inference`` makes:
``add(values, labels, video_offsets=None, keys=None)``, ``merge_ranks(group=None)`` and ``compute()``.
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, current_stream, ptr
from .metrics import (CFUSE_MATRIX, CL_ACC, FRAME_LEVEL, FRM_AVG_LOGITS, FRM_AVG_PROBS, FRM_VOTE, MACRO_F1, VIDEO_LEVEL, W_F1)


def _check_coverage(what, starts, lw, total):
    """Every frame of a ``total``-frame video lies in one of the ``lw``-frame windows at ``starts`` (all inside the video).  The
    reference divides by the overlap count, so an uncovered frame is 0 / 0 = NaN there; the kernels would write 0."""
    s = sorted(starts)
    if not s or s[0] > 0 or s[-1] + lw < total or any(b - a > lw for a, b in zip(s, s[1:])):
        raise ValueError(f"{what}: the {lw}-frame windows starting at {s} leave frames of the {total}-frame video uncovered")


def stitch_windows(win_out, starts, total):
    """win_out [nw, Lw, C] (GPU), starts: list of window start frames -> [total, C]; trainer.py:832-892 in one launch.
    The windows must lie inside the video and cover every frame of it (checked here, before the launch)."""
    if not (isinstance(win_out, torch.Tensor) and win_out.is_cuda and win_out.dtype == torch.float32 and win_out.dim() == 3):
        raise ValueError("stitch_windows: expected a [n_windows, window_length, n_classes] float32 GPU tensor")
    nw, lw, c = win_out.shape
    starts = [int(s) for s in starts]
    if len(starts) != nw:
        raise ValueError(f"stitch_windows: {nw} windows but {len(starts)} start frames (one video per call)")
    if nw and (min(starts) < 0 or max(starts) + lw > total):
        raise ValueError(f"stitch_windows: a window of {lw} frames starting at {max(starts)} leaves the {total}-frame video")
    _check_coverage("stitch_windows", starts, lw, total)
    st = torch.tensor(list(starts), dtype=torch.int32, device=win_out.device)
    out = torch.empty((total, c), device=win_out.device, dtype=torch.float32)
    check(_lib.load().cer_window_stitch(ptr(win_out.contiguous()), ptr(st), nw, lw, c, total, ptr(out), current_stream()),
          "cer_window_stitch")
    return out


def _offsets(name, offsets, end):
    """A list (or tensor / array, brought to the host in one copy) of at least two offsets that start at 0, rise strictly
    and, with ``end``, stop there."""
    if isinstance(offsets, (torch.Tensor, np.ndarray)):
        offsets = offsets.reshape(-1).tolist()
    offsets = [int(o) for o in offsets]
    if len(offsets) < 2 or offsets[0] != 0 or any(b <= a for a, b in zip(offsets, offsets[1:])) or \
            (end is not None and offsets[-1] != end):
        raise ValueError(f"{name} must rise strictly from 0"
                         + ("" if end is None else f" to {end}") + f", got {offsets}")
    return offsets


def stitch_windows_multi(win_out, starts, win_offsets, frame_offsets):
    """``stitch_windows`` for V videos in ONE launch.  win_out [nw, Lw, C] (GPU) holds the videos' windows, video after video;
    video v owns windows ``win_offsets[v]:win_offsets[v+1]``, whose start frames ``starts`` are relative to the video, and rows
    ``frame_offsets[v]:frame_offsets[v+1]`` of the result [R = frame_offsets[-1], C] -- the concatenation
    ``DeviceEvalAccumulator.add(..., video_offsets=frame_offsets)`` takes.  Every row is bit-identical to ``stitch_windows`` on
    its video alone.  All arguments are checked here, before the launch: the offsets, that every window lies inside its video
    and that every frame of every video lies in a window."""
    if not (isinstance(win_out, torch.Tensor) and win_out.is_cuda and win_out.dtype == torch.float32 and win_out.dim() == 3):
        raise ValueError("stitch_windows_multi: expected a [n_windows, window_length, n_classes] float32 GPU tensor")
    nw, lw, c = win_out.shape
    starts = [int(s) for s in starts]
    if len(starts) != nw:
        raise ValueError(f"stitch_windows_multi: {nw} windows but {len(starts)} start frames")
    woff = _offsets("stitch_windows_multi: win_offsets", win_offsets, nw)
    foff = _offsets("stitch_windows_multi: frame_offsets", frame_offsets, None)
    if len(woff) != len(foff):
        raise ValueError(f"stitch_windows_multi: {len(woff) - 1} videos in win_offsets, {len(foff) - 1} in frame_offsets")
    for v in range(len(woff) - 1):
        total = foff[v + 1] - foff[v]
        for w in range(woff[v], woff[v + 1]):
            if starts[w] < 0 or starts[w] + lw > total:
                raise ValueError(f"stitch_windows_multi: window {w} ({lw} frames from {starts[w]}) leaves video {v} "
                                 f"({total} frames)")
        _check_coverage(f"stitch_windows_multi: video {v}", starts[woff[v]:woff[v + 1]], lw, total)
    dev = win_out.device
    st = torch.tensor(starts, dtype=torch.int32, device=dev)
    wo = torch.tensor(woff, dtype=torch.int32, device=dev)
    fo = torch.tensor(foff, dtype=torch.int32, device=dev)
    r = foff[-1]
    out = torch.empty((r, c), device=dev, dtype=torch.float32)
    check(_lib.load().cer_window_stitch_multi(ptr(win_out.contiguous()), ptr(st), ptr(wo), ptr(fo), len(woff) - 1, nw, lw, c,
                                              r, ptr(out), current_stream()), "cer_window_stitch_multi")
    return out


def scores_from_confusion(cm):
    """Counts [C, C] (rows = targets, columns = predictions) -> the four entries the reference derives with sklearn."""
    cm = np.asarray(cm, dtype=np.float64)
    present = (cm.sum(0) + cm.sum(1)) > 0            # sklearn: labels = sorted union of targets and predictions
    sub = cm[np.ix_(present, present)]
    tp = np.diag(sub)
    fp, fn = sub.sum(0) - tp, sub.sum(1) - tp
    den = 2 * tp + fp + fn
    f1 = np.divide(2 * tp, den, out=np.zeros_like(tp), where=den > 0)
    support = sub.sum(1)
    total = sub.sum()
    rows = sub.sum(1, keepdims=True)
    return {"f1_per_class": f1, "macro_f1": float(f1.mean()) if f1.size else 0.0,
            "weighted_f1": float((f1 * support).sum() / max(support.sum(), 1.0)),
            "accuracy": float(tp.sum() / total * 100.0) if total > 0 else 0.0,
            "confusion": np.divide(sub, rows, out=np.zeros_like(sub), where=rows > 0)}


class DeviceEvalAccumulator:
    def __init__(self, n_classes, ignore_classes=(None,), device="cuda", keep_video_predictions=False):
        self.c, self.ignore_classes, self.device = n_classes, tuple(ignore_classes), device
        self.cm = {ic: torch.zeros((4, n_classes, n_classes), dtype=torch.int64, device=device) for ic in self.ignore_classes}
        self.bad = torch.zeros((1,), dtype=torch.int32, device=device)
        self.keep = keep_video_predictions
        self.video_predictions = []

    def add(self, values, labels, video_offsets=None, keys=None):
        """values: logits [R, C] float32 GPU, labels [R] (float or long) GPU; ``video_offsets`` = row offsets [V+1] when several
        videos are concatenated (default: one video): a list, or a tensor read in one copy, that starts at 0, rises strictly
        and ends at R.  The kernel reads rows ``video_offsets[v]:video_offsets[v+1]`` unchecked, so anything else is refused here.
        ``keys`` (the videos' names, which ``DeviceRegressionAccumulator.add`` keeps) are ignored: counts carry no names."""
        if not (values.is_cuda and values.dtype == torch.float32 and values.dim() == 2 and values.shape[1] == self.c):
            raise ValueError("logits: expected a [R, n_classes] float32 GPU tensor")
        if not (isinstance(labels, torch.Tensor) and labels.is_cuda):
            raise ValueError("labels: expected a GPU tensor (one label per logits row)")
        values = values.contiguous()
        labels = labels.reshape(-1).float().contiguous()
        r = values.shape[0]
        if labels.numel() != r:
            raise ValueError("one label per logits row")
        offsets = [0, r] if video_offsets is None else _offsets("DeviceEvalAccumulator.add: video_offsets", video_offsets, r)
        off = torch.tensor(offsets, dtype=torch.int32, device=values.device)
        v = off.numel() - 1
        lib = _lib.load()
        for ic, cm in self.cm.items():
            vp = torch.empty((v, 3), dtype=torch.int32, device=values.device) if self.keep else None
            check(lib.cer_eval_accumulate(ptr(values), ptr(labels), ptr(off), v, r, self.c, -1 if ic is None else int(ic),
                                          ptr(cm[0]), ptr(cm[1:]), ptr(vp), ptr(self.bad), current_stream()), "cer_eval_accumulate")
            if self.keep:
                self.video_predictions.append((ic, vp))

    def merge_ranks(self, group=None):
        """Sum the counts of every rank (sharded evaluation): every ignore-class's [4, C, C] counts and the ``bad`` counter go
        in ONE int64 buffer through ONE ``all_reduce(SUM)``.  Afterwards every rank holds the global counts, so ``compute``
        gives the same scores everywhere -- and raises on every rank if any rank saw a bad label."""
        import torch.distributed as dist
        cms = list(self.cm.values())
        flat = torch.cat([cm.reshape(-1) for cm in cms] + [self.bad.to(torch.int64)])
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
        n = 4 * self.c * self.c
        for i, cm in enumerate(cms):
            cm.copy_(flat[i * n:(i + 1) * n].view_as(cm))
        self.bad.copy_(flat[-1:])

    def compute(self):
        """One device -> host copy per ignore-class setting; the reference's nested score dictionary."""
        if int(self.bad.item()) != 0:
            raise AssertionError(f"{int(self.bad.item())} frame(s) / video(s) with labels outside [0, n_classes) or mixed labels "
                                 "inside one video (the reference asserts len(unique) == 1, metrics.py:104-105)")
        out = {}
        for ic, cm in self.cm.items():
            counts = cm.cpu().numpy()
            perf = {m: {FRAME_LEVEL: None, VIDEO_LEVEL: {}} for m in (MACRO_F1, W_F1, CL_ACC, CFUSE_MATRIX)}

            def put(level, key, s):
                entries = {MACRO_F1: {"master": s["macro_f1"], "per_cl": s["f1_per_class"]},
                           W_F1: {"master": s["weighted_f1"], "per_cl": s["f1_per_class"]},
                           CL_ACC: {"master": s["accuracy"], "per_cl": s["accuracy"]},
                           CFUSE_MATRIX: {"master": s["confusion"], "per_cl": s["confusion"]}}
                for m, e in entries.items():
                    if level == FRAME_LEVEL:
                        perf[m][FRAME_LEVEL] = e
                    else:
                        perf[m][VIDEO_LEVEL][key] = e
            put(FRAME_LEVEL, None, scores_from_confusion(counts[0]))
            for i, k in enumerate((FRM_VOTE, FRM_AVG_LOGITS, FRM_AVG_PROBS)):
                put(VIDEO_LEVEL, k, scores_from_confusion(counts[1 + i]))
            out[ic] = perf
        return out


class DeviceRegressionAccumulator:
    """The regression task's scores (base/logger.py:274-351: RMSE, Pearson's r, Lin's CCC, per trial and over the concatenated
    partition) from per-video moments gathered ON THE DEVICE.  Each ``add`` leaves one ``{n, mean_p, mean_l, M2_p, M2_l, C_pl,
    SSE, 0}`` float64 row per video on the card (``cer_regression_moments``); ``compute`` brings all rows to the host in ONE
    copy, scores every video from its row and folds the rows, in loader order, into the ``"overall"`` scores."""

    def __init__(self, device="cuda"):
        self.device = device
        self.rows, self.keys = [], []        # [V, 8] float64 tensors; one (loader position, trial) per row

    def add(self, values, labels, video_offsets=None, keys=None):
        """values: outputs [R, 1] or [R] float32 GPU, labels [R] or [R, 1] GPU; ``video_offsets`` as ``DeviceEvalAccumulator.add``
        takes them (default: one video).  ``keys``: one ``(loader position, trial)`` per video (default: the running video
        count for both).  Everything is checked here, before the launch: the kernel reads rows unchecked, and a video of fewer
        than two frames has no variance (the reference divides by ``len - 1``)."""
        if not (isinstance(values, torch.Tensor) and values.is_cuda and values.dtype == torch.float32 and values.dim() in (1, 2)):
            raise ValueError("outputs: expected a [R, 1] or [R] float32 GPU tensor")
        if values.dim() == 2 and values.shape[1] != 1:
            raise ValueError(f"outputs: output_dim = {values.shape[1]}, but the regression scores cover ONE output column "
                             "(the reference scores column 0 only, base/logger.py:105-108)")
        if not (isinstance(labels, torch.Tensor) and labels.is_cuda):
            raise ValueError("labels: expected a GPU tensor (one label per output row)")
        r = values.shape[0]
        if labels.numel() != r:
            raise ValueError("one label per output row")
        offsets = [0, r] if video_offsets is None else _offsets("DeviceRegressionAccumulator.add: video_offsets", video_offsets, r)
        short = [v for v, (a, b) in enumerate(zip(offsets, offsets[1:])) if b - a < 2]
        if short:
            raise ValueError(f"DeviceRegressionAccumulator.add: video(s) {short} have fewer than 2 frames (no variance)")
        v = len(offsets) - 1
        if keys is None:
            keys = [(len(self.keys) + i,) * 2 for i in range(v)]
        if len(keys) != v:
            raise ValueError(f"DeviceRegressionAccumulator.add: {len(keys)} keys for {v} videos")
        from . import ops
        self.rows.append(ops.regression_moments(values.reshape(-1).contiguous(), labels.reshape(-1).float().contiguous(), offsets))
        self.keys.extend((int(pos), trial) for pos, trial in keys)

    def _host_rows(self):
        if not self.rows:
            return np.zeros((0, 8))
        rows = [r if isinstance(r, torch.Tensor) else torch.as_tensor(r) for r in self.rows]
        return (rows[0] if len(rows) == 1 else torch.cat(rows)).cpu().numpy().reshape(-1, 8)

    def merge_ranks(self, group=None):
        """Sharded evaluation: every rank receives every rank's moment rows with their loader positions; ``compute`` orders
        them by position, so every rank folds the same rows in the same order and reports identical scores."""
        import torch.distributed as dist
        parts = [None] * dist.get_world_size(group)
        dist.all_gather_object(parts, (list(self.keys), self._host_rows()), group=group)
        self.keys = [k for keys, _ in parts for k in keys]
        self.rows = [np.concatenate([rows for _, rows in parts])]

    def compute(self):
        """``{trial: {"rmse", "pcc", "ccc"}, ..., "overall": {...}}``.  Videos in loader order; a trial id that comes back
        replaces the earlier video of that name, as in the per-video dictionary ``inference`` returns."""
        from .metrics import OVERALL, fold_moments, scores_from_moments
        rows = self._host_rows()
        assert len(rows) == len(self.keys) and len(rows) > 0, (len(rows), len(self.keys))
        by_trial = {}
        for i in sorted(range(len(rows)), key=lambda i: self.keys[i][0]):
            by_trial[self.keys[i][1]] = rows[i]
        out = {trial: scores_from_moments(row) for trial, row in by_trial.items()}
        out[OVERALL] = scores_from_moments(fold_moments(list(by_trial.values())))
        return out
