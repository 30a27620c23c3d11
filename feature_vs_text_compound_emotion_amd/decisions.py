"""Running video-level decisions of live streams: per-frame logits in, the reference's three decisions out.

The reference never reports a frame's argmax: for every video it reports the majority vote over the frame predictions, the
argmax of the mean logits and the argmax of the mean softmax probabilities (``metrics.format_trg_pred_video``), on C-EXPR-DB
without the last column.  ``DecisionStream`` keeps that answer up to date for ``streams`` independent live streams as their
logit rows arrive, over everything since a stream's reset (``window=None``, the reference's rule) or over its last ``window``
frames.

State (csrc/decision_stream.hip).  Whole-stream: four accumulators per (stream, class) on the device -- ``votes`` and
``first`` int64, ``slog`` and ``sprob`` float64.  Window: a ring of the logits themselves, [S, R, C] float32 with R the power of
two >= window + max_new, and no accumulators: a decision is recomputed from the window's rows.  The host keeps two ints per
stream: the frames since its reset and its ring position.

Every column sum is one chain of ``acc += (double)value`` in time order, continued by each push (whole-stream) or walked from
the window's oldest row (window), so a result is the same bits however the rows were cut into pushes, whatever ``max_new``,
the number of streams or what the other streams do.
"""
import torch

from . import ops
from .lfan import REGRESSION
from .streaming import _check_counts, _check_packed, _check_tensor

CLASSIFICATION = "CLASSIFICATION"


class DecisionStream:
    """``n_out`` outputs per frame (2 .. 16) of ``streams`` live streams.

      push_ragged(rows [M, n_out], counts, track=False)   stream s brings ``counts[s]`` (0 .. max_new) rows, packed stream-major
            in ascending stream order, each stream's rows in time order (what ``LFANStream.push_ragged`` returns).
      push_rows(rows [S * c, n_out], track=False)          every stream brings c rows (any c >= 1; what ``push`` returns, viewed
            as rows).
            Both return None, or with ``track=True`` (decisions [M, 3] int32, mean_outputs [M, n_out], mean_probs [M, n_out]):
            the answer of ``decide`` as it stands after each new row, in the row order of the input.
      decide()   -> (decisions [S, 3] int32: vote, mean logits, mean probabilities, -1 for a stream without a frame;
            mean_outputs [S, n_out]; mean_probs [S, n_out]); the means of a stream without a frame are NaN.
      reset(streams=None)   forget those streams (indices; None = all).
      frames_seen           host list: frames since reset, per stream.

    ``drop_last``: decide over the first n_out - 1 columns (C-EXPR-DB's 'Other'); the dropped column keeps its mean logit
    and has mean probability 0.  ``task="REGRESSION"``: the rows are the model's tanh outputs, only their running mean is
    defined: ``decisions`` and ``mean_probs`` are None.  Bad counts, shapes, dtypes or CPU tensors raise ValueError before
    any launch, with no state changed."""

    def __init__(self, n_out, streams, *, window=None, max_new=32, drop_last=False, task=CLASSIFICATION, device="cuda"):
        n_out, streams, max_new = int(n_out), int(streams), int(max_new)
        if task not in (CLASSIFICATION, REGRESSION):
            raise ValueError(f"task = {task!r}: {CLASSIFICATION!r} or {REGRESSION!r}")
        if not 2 <= n_out <= 16:
            raise ValueError(f"n_out = {n_out}: the kernel takes 2 .. 16 outputs per frame")
        if streams < 1 or max_new < 1:
            raise ValueError(f"streams = {streams}, max_new = {max_new}: both must be >= 1")
        if window is not None and (isinstance(window, bool) or int(window) != window or window < 1):
            raise ValueError(f"window = {window!r}: an integer >= 1, or None for the whole stream")
        self.classify = task == CLASSIFICATION
        if drop_last and (not self.classify or n_out < 3):
            raise ValueError("drop_last needs a classification task with at least 3 outputs")
        if torch.device(device).type != "cuda":
            raise RuntimeError("DecisionStream runs on the HIP kernels only: give it a GPU device (no CPU fallback)")
        self.n_out, self.streams, self.max_new, self.task = n_out, streams, max_new, task
        self.window = None if window is None else int(window)
        self.drop_last, self.device = bool(drop_last), torch.device(device)
        self.state = None           # allocated by the first push or decide
        self.frames_seen = [0] * streams
        self._pos = [0] * streams   # rows pushed per stream since construction: the ring slot is _pos[s] & (R - 1)
        self._mode = dict(window=self.window, drop_last=self.drop_last, classify=self.classify)

    def _alloc(self):
        if self.state is None:
            self.state = ops.decision_stream_state(self.streams, self.n_out, window=self.window, max_new=self.max_new,
                                                   classify=self.classify, device=self.device)

    def reset(self, streams=None):
        idx = list(range(self.streams)) if streams is None else [int(s) for s in streams]
        for s in idx:
            if not 0 <= s < self.streams:
                raise IndexError(f"stream {s} of {self.streams}")
        for s in idx:
            self.frames_seen[s] = 0
        if not idx or self.state is None:
            return
        sel = torch.tensor(idx, device=self.device)
        for name, t in self.state.items():   # a window needs no zeroing: rows before the reset are never in a window again
            if name != "zring":
                t.index_fill_(0, sel, ops.DECISION_NEVER if name == "first" else 0)

    def _push(self, rows, counts, track):
        self._alloc()
        segments, off = [], 0
        for s, c in enumerate(counts):
            if c:
                segments.append((s, c, off, self._pos[s], self.frames_seen[s]))
            off += c
        out = ops.decision_stream_push(rows, ops.decision_segment_table(segments, self.device), max(counts), self.state,
                                       track=track, **self._mode)
        self._pos = [p + c for p, c in zip(self._pos, counts)]
        self.frames_seen = [f + c for f, c in zip(self.frames_seen, counts)]
        return out

    def _track(self, parts):
        dec = torch.cat([p[0] for p in parts]) if self.classify else None
        means = torch.cat([p[1] for p in parts])
        return dec, means[:, 0], means[:, 1] if self.classify else None

    @torch.no_grad()
    def push_ragged(self, rows, counts, track=False):
        counts = _check_counts(counts, self.streams, self.max_new)
        _check_packed(rows, "rows", sum(counts), (self.n_out,))
        if not rows.shape[0]:
            empty = torch.empty((0, self.n_out), device=self.device)
            return (torch.empty((0, 3), dtype=torch.int32, device=self.device) if self.classify else None, empty,
                    empty if self.classify else None) if track else None
        out = self._push(rows.contiguous(), counts, track)
        return self._track([out]) if track else None

    @torch.no_grad()
    def push_rows(self, rows, track=False):
        _check_tensor(rows, "rows")
        if rows.dim() != 2 or rows.shape[1] != self.n_out or rows.shape[0] < 1 or rows.shape[0] % self.streams:
            raise ValueError(f"rows: expected [{self.streams} streams * c >= 1 rows, {self.n_out}], got {tuple(rows.shape)}")
        rows, c = rows.contiguous(), rows.shape[0] // self.streams
        x = rows.view(self.streams, c, self.n_out)
        parts = []
        for c0 in range(0, c, self.max_new):
            n = min(self.max_new, c - c0)
            chunk = rows if n == c else x[:, c0:c0 + n].reshape(self.streams * n, self.n_out)
            parts.append(self._push(chunk.contiguous(), [n] * self.streams, track))
        if not track:
            return None
        if len(parts) == 1:
            return self._track(parts)
        # back into the input's row order: stream-major over all c rows
        dec, mo, mp = self._track(parts)
        sizes = [min(self.max_new, c - c0) for c0 in range(0, c, self.max_new)]

        def order(t):
            if t is None:
                return None
            per = t.split([self.streams * n for n in sizes])
            return torch.cat([p.view(self.streams, n, -1) for p, n in zip(per, sizes)], dim=1).reshape(self.streams * c, -1)
        return order(dec), order(mo), order(mp)

    @torch.no_grad()
    def decide(self):
        self._alloc()
        w = self.window
        table = ops.decision_segment_table([(s, 0 if w is None else min(f, w), 0, p, f)
                                            for s, (p, f) in enumerate(zip(self._pos, self.frames_seen))], self.device)
        dec, means = ops.decision_stream_read(table, self.max_new, self.state, **self._mode)
        return dec, means[:, 0], means[:, 1] if self.classify else None
